"""Golden anchor of the wide-row cases (tests/wide_row_cases.py), generated from the REAL reference (run where the
reference is installed only; no test imports this file):

    PYTHONPATH=/root/reference/src PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wide_rows.py

For every width of ``GOLDEN_WIDTHS`` every selection case and every learn case of the width runs on the reference's own
``OptimalQLearningBase`` with the draws injected (oracle/draws.py).  Stored per selection case: what the reference did
(0 actions, 1 IndexError, 2 no record: the shim cannot observe the call, 3 another exception, with its name) and the
actions; per learn case the cells that changed and their new values.  Tables are not stored: the builder's arguments are
the case, and ``fp_<A>_<dtype>`` holds the fingerprint of what the builder returned here."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from dist_classicrl.algorithms.base_algorithms.q_learning_optimal import OptimalQLearningBase  # noqa: E402

import wide_row_cases as W  # noqa: E402

out, counts = {}, {0: 0, 1: 0, 2: 0, 3: 0}
for A in W.GOLDEN_WIDTHS:
    for dt in W.DTYPES:
        out[f"fp_{A}_{dt}"] = np.array(W.table_fingerprint(W.wide_table(A, dt)), dtype=np.uint32)
    for k, c in enumerate(W.select_cases(A)):
        q, states, masks = W.select_inputs(c)
        status, actions, name = 2, None, ""
        if not W.shim_cannot_observe(c):
            algo = OptimalQLearningBase(W.S_ROWS, A, 0.9, seed=0)
            algo.q_table = q.copy()
            try:
                res, actions = W.call_select(algo, c, states, masks, W.shimmed(algo, c))
                status = 0 if res == "ok" else 1
            except Exception as exc:  # noqa: BLE001 -- what the reference did is the record
                status, name = 3, type(exc).__name__
        counts[status] += 1
        out[f"s{A}_{k}_status"] = np.array(status, dtype=np.int8)
        out[f"s{A}_{k}_actions"] = np.zeros(0, dtype=np.int16) if actions is None else actions.astype(np.int16)
        if name:
            out[f"s{A}_{k}_exception"] = np.array(name)
    for k, c in enumerate(W.learn_cases(A)):
        q0, batch = W.learn_inputs(c)
        algo = OptimalQLearningBase(W.S_ROWS, A, W.LEARN_GAMMA, seed=0)
        algo.q_table = q0.copy()
        W.call_learn(algo, c, batch)
        q = np.asarray(algo.q_table)
        assert q.dtype == q0.dtype
        idx = W.changed_cells(q, q0)
        out[f"l{A}_{k}_idx"] = idx.astype(np.int32)
        out[f"l{A}_{k}_val"] = q.ravel()[idx]
np.savez_compressed(Path(__file__).resolve().parent / "wide_rows.npz", **out)
print("selection cases by status", counts, "| learn cases", sum(len(W.learn_cases(A)) for A in W.GOLDEN_WIDTHS))
