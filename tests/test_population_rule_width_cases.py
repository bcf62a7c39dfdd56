"""The inputs of tests/test_gpu_population_rule_widths.py keep enough runs to test something: properties of the NumPy
models alone, checked without a device.

A case on tables with NaN, +inf and -inf cells that loses most of its runs to ``IndexError`` compares nothing.  Each such
case is built here by the very functions the GPU module calls (``nan_case``, ``tie_case``, ``eval_nan_case``,
``dyna_host_models``) and must satisfy:

* the model completes at least half of its runs;
* at least one run is flagged (the cases at the 10 / 11 threshold);
* at least one completed run ends with a non-finite cell;
* the -inf-row cases: at least one completed run has written into its -inf row.

Every test prints the figures it asserts on (``pytest -s``).
"""
import numpy as np
import pytest

import test_gpu_population_rule_widths as cases

HALF = (cases.M_ODD + 1) // 2


def _non_finite(done):
    return sum(not all(np.isfinite(t).all() for t in cases.tables_of(run)) for run, _, _ in done.values())


@pytest.mark.parametrize(("family", "A", "masked"), cases.NAN_CASES)
def test_the_threshold_cases_keep_half_their_runs_flag_some_and_keep_special_cells(family, A, masked):
    c = cases.nan_case(family, A, masked)
    kept = _non_finite(c["done"])
    print(f"{c['fam']} A={A} masked={masked}: completed {len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, "
          f"completed with a non-finite cell {kept}")
    assert len(c["done"]) + len(c["flagged"]) == cases.M_ODD
    assert len(c["done"]) >= HALF
    assert c["flagged"]
    assert kept >= 1


@pytest.mark.parametrize(("fam", "A"), cases.TIE_CASES)
def test_the_minus_infinity_row_cases_keep_half_their_runs_and_write_into_the_row(fam, A):
    c = cases.tie_case(fam, A)
    wrote = [r for r in c["rows"] if r in c["done"] and cases.wrote_into_its_row(c, r)]
    kept = _non_finite(c["done"])
    print(f"{fam} A={A}: completed {len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, completed with a "
          f"non-finite cell {kept}, completed and wrote into the -inf row {len(wrote)} of {len(c['rows'])}")
    assert sorted(c["rows"]) == list(range(0, cases.M_ODD, 3))
    for r, s in c["rows"].items():  # one whole row of -inf in an otherwise finite table
        for t in (c["q0"], c["qb0"]) if c["qb0"] is not None else (c["q0"],):
            assert np.isneginf(t[r, s]).all() and np.isfinite(np.delete(t[r], s, axis=0)).all()
    eps = [s.get_value() for s in c["sched"][0]]
    assert eps[0::2] == [0.0] * len(eps[0::2]) and eps[1::2] == [0.3] * len(eps[1::2])
    assert len(c["done"]) >= HALF
    assert kept >= 1
    assert wrote


@pytest.mark.parametrize("double", [False, True], ids=["single", "double"])
@pytest.mark.parametrize(("A", "masked"), cases.EVAL_NAN_CASES)
def test_the_evaluation_cases_keep_half_their_runs(A, masked, double):
    c = cases.eval_nan_case(A, masked, double)
    tables = (c["q0"],) if c["qb0"] is None else (c["q0"], c["qb0"])
    kept = sum(not all(np.isfinite(t[r]).all() for t in tables) for r in c["done"])
    print(f"evaluation A={A} masked={masked} double={double}: completed {len(c['done'])} of {cases.M_ODD}, "
          f"flagged {len(c['flagged'])}, completed on a table with a non-finite cell {kept}")
    assert len(c["done"]) >= HALF
    assert kept >= 1
    if A > 10:  # the NumPy-style selection: a NaN maximum has no candidate
        assert c["flagged"]


@pytest.mark.parametrize(("S", "A"), [(4, 3), (6, 5)])
def test_most_dyna_runs_see_every_cell_before_the_model_goes_through_the_host(S, A):
    done = cases.dyna_host_models(S, A)
    full = sum(run.planning_model[4] == S * A for run, _, _ in done.values())
    print(f"Dyna-Q S={S} A={A}: {full} of {len(done)} runs have seen all {S * A} cells")
    assert len(done) >= 10 and 2 * full >= len(done)


def test_every_family_meets_every_dtype_and_learn_mode_in_the_width_sweep():
    met = {}
    for p in cases.WIDTH_CASES:
        fam, _, _, dt, mode = p.values
        met.setdefault(fam, set()).add((dt, mode))
    assert sorted(met) == sorted(cases.FAMILIES)
    assert all(len(v) == 4 for v in met.values()), met
