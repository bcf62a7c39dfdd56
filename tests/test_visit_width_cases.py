"""The inputs of tests/test_gpu_visit_widths.py keep enough runs to test something: properties of the NumPy model of
the visit counts alone (visit_model.py), checked without a device.

A case on tables with NaN, +inf and -inf cells that loses most of its runs to ``IndexError`` compares nothing, and with
visit counts an untried cell at -inf scores ``-inf + inf = NaN`` on top of that.  Each such case is built here by the
very functions the GPU module calls (``nan_case``, ``tie_case``) and must satisfy:

* the model completes at least half of its runs;
* at least one run is flagged (the cases at the 10 / 11 threshold);
* at least one completed run ends with a non-finite cell;
* the -inf-row cases with starting counts: at least one completed run has written into its -inf row.

Every test prints the figures it asserts on (``pytest -s``).
"""
import numpy as np
import pytest

import test_gpu_visit_widths as cases

HALF = (cases.M_ODD + 1) // 2


def _non_finite(done):
    return sum(not np.isfinite(run.q).all() for run, _, _ in done.values())


@pytest.mark.parametrize(("A", "masked"), cases.NAN_CASES)
def test_the_threshold_cases_keep_half_their_runs_flag_some_and_keep_special_cells(A, masked):
    c = cases.nan_case(A, masked)
    kept = _non_finite(c["done"])
    print(f"visit counts A={A} masked={masked} {np.dtype(c['dt']).name} {c['mode']} visit_lr={c['visit_lr']}: completed "
          f"{len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, completed with a non-finite cell {kept}")
    assert len(c["done"]) + len(c["flagged"]) == cases.M_ODD
    assert len(c["done"]) >= HALF
    assert c["flagged"]
    assert kept >= 1


@pytest.mark.parametrize(("A", "tried"), cases.TIE_CASES)
def test_the_minus_infinity_row_cases_keep_half_their_runs_and_write_into_the_row(A, tried):
    c = cases.tie_case(A, tried)
    wrote = [r for r in c["rows"] if r in c["done"] and cases.wrote_into_its_row(c, r)]
    print(f"visit counts A={A} {'with' if tried else 'without'} starting counts, {np.dtype(c['dt']).name} {c['mode']} "
          f"visit_lr={c['visit_lr']}: completed {len(c['done'])} of {cases.M_ODD}, flagged {len(c['flagged'])}, completed and "
          f"wrote into the -inf row {len(wrote)} of {len(c['rows'])}")
    assert sorted(c["rows"]) == list(range(0, cases.M_ODD, 3))
    for r, s in c["rows"].items():  # one whole row of -inf in an otherwise finite table
        assert np.isneginf(c["q0"][r, s]).all() and np.isfinite(np.delete(c["q0"][r], s, axis=0)).all()
    eps = [s.get_value() for s in c["sched"][0]]
    assert eps[0::2] == [0.0] * len(eps[0::2]) and eps[1::2] == [0.3] * len(eps[1::2])
    assert len(c["done"]) + len(c["flagged"]) == cases.M_ODD
    assert len(c["done"]) >= HALF
    if not tried:
        assert c["n0"] is None
        return
    n0 = c["n0"]
    assert n0.dtype == np.uint32 and n0.max() <= 4
    for r, s in c["rows"].items():  # every cell of the -inf row is tried: it scores -inf exactly, never NaN
        assert n0[r, s].min() >= 1 and np.delete(n0[r], s, axis=0).max() <= 3
    assert (n0 == 0).any()
    assert wrote


def test_the_width_sweep_meets_every_dtype_learn_mode_and_rate_masked_and_plain():
    met = {}
    for p in cases.WIDTH_CASES:
        _, masked, dt, mode, visit_lr = p.values
        met.setdefault((dt, mode, visit_lr), set()).add(masked)
    assert len(met) == 8 and all(v == {False, True} for v in met.values()), met
    assert sorted({p.values[0] for p in cases.WIDTH_CASES}) == [1, 2, 3, 5, 9, 17, 33, 63]
