"""CPU: the replay-ring oracle against the fixture generated from the real reference class."""

import numpy as np
import pytest

from conftest import GOLDEN
from oracle.replay_oracle import OracleReplay


def replay_script(make):
    """Replays tests/golden/replay.npz against `make(capacity, seed)`; yields nothing, asserts everything."""
    g = np.load(GOLDEN / "replay.npz")
    capacity, seed = (int(v) for v in g["meta"])
    rb = make(capacity, seed)
    pushed = iter(g["pushed"])
    for op, pos, full, length, s, a, r, n, d in g["log"]:
        if op == 0:
            e = next(pushed)
            rb.push((int(e[0]), int(e[1]), float(e[2]), int(e[3]), bool(e[4])))
        else:
            got = rb.sample(1)
            assert got == (int(s), int(a), float(r), int(n), bool(d))
            assert [type(v) for v in got] == [int, int, float, int, bool]
        assert (rb.position, int(rb.full), len(rb)) == (int(pos), int(full), int(length))
    valid = len(rb)
    assert np.array_equal(rb.state_buffer[:valid], g["final_state"])
    assert np.array_equal(rb.action_buffer[:valid], g["final_action"])
    assert np.array_equal(rb.reward_buffer[:valid], g["final_reward"])
    assert np.array_equal(rb.next_state_buffer[:valid], g["final_next"])
    assert np.array_equal(rb.done_buffer[:valid], g["final_done"])
    with pytest.raises(TypeError):  # int(array of two) -- upstream's sample only works for one experience
        rb.sample(2)
    return rb


def test_oracle_replay_matches_reference_fixture():
    replay_script(OracleReplay)


# ---------------------------------------------------------------------------- helpers of the GPU ring tests
@pytest.mark.parametrize("capacity", [1, 2, 7, 36, 37, 38, 100])
@pytest.mark.parametrize(("position0", "full0"), [(0, False), (3, False), (5, True)])
def test_ring_after_equals_push_entry_by_entry(capacity, position0, full0):
    """37 pushes into rings smaller than, as large as and larger than that, from a ring that stands somewhere."""
    from helpers import ring_after

    position0 %= capacity
    rng = np.random.default_rng(capacity)
    k = 37
    tr = (rng.integers(1 << 40, size=k), rng.integers(100, size=k), rng.standard_normal(k).astype(np.float32),
          rng.integers(1 << 40, size=k), rng.random(k) < 0.3)
    ref = OracleReplay(capacity, 0)
    ref.position, ref.full = position0, full0
    written = np.zeros(capacity, dtype=bool)
    for e in zip(*tr):
        written[ref.position] = True
        ref.push(e)
    got = ring_after(tr, capacity, position0, full0)
    assert (got["position"], got["full"], got["len"]) == (ref.position, ref.full, len(ref))
    assert np.array_equal(got["written"], written) and written.sum() == min(k, capacity)
    for name in ("state", "action", "reward", "next_state", "done"):
        buf = getattr(ref, name + "_buffer")
        assert got[name].dtype == buf.dtype
        assert np.array_equal(got[name][written], buf[written]), name
    # nothing pushed: the ring stays where it stands
    none = ring_after(tuple(x[:0] for x in tr), capacity, position0, full0)
    assert (none["position"], none["full"]) == (position0, full0) and not none["written"].any()


@pytest.mark.parametrize(("spec", "dt", "mode"), [
    (("hash", 24, 50, 6, False), "f4", "iter"),
    (("hash", 24, 50, 6, False), "f8", "vec"),
    (("hash", 16, 40, 12, True), "f8", "iter"),
])
def test_recorded_transitions_reproduce_the_closed_loop(spec, dt, mode):
    """The recorded transitions ARE what the closed loop learned from: fed to ``learn`` step by step, with the learning
    rate of each step, they rebuild ``run_oracle_trace``'s table (unmasked), and the chunked loop ends where the
    unchunked one does."""
    from helpers import make_oracle_env, run_oracle_trace, run_oracle_transitions, transitions_of
    from oracle.qlearn_oracle import OracleQLearning

    steps, n = 30, spec[1]
    whole = run_oracle_trace(spec, steps, dt, "bench", mode)
    want = run_oracle_transitions(make_oracle_env(spec), [11, 1, 18], dt, "bench", mode)
    assert [c["steps"] for c in want["chunks"]] == [11, 12, 30] and want["n"] == n
    last = want["chunks"][-1]
    for k in ("q", "history", "final_obs", "agent_rewards"):
        assert np.array_equal(last[k], whole[k]), k
    s, a, r, s2, d = transitions_of(want)
    assert len(s) == steps * n and r.dtype == np.float32 and d.dtype == bool
    assert np.array_equal(a.reshape(steps, n), whole["actions"])
    assert np.array_equal(s2.reshape(steps, n)[-1], whole["final_obs"])
    assert np.array_equal(s.reshape(steps, n)[1:], s2.reshape(steps, n)[:-1])  # SAME_STEP autoreset: s' is the next s
    assert d.any()
    if spec[4]:
        return  # (a masked loop maximises over the valid actions of s': not what the ring's five fields determine)
    algo = OracleQLearning(spec[2], spec[3], 0.99, seed=0, dtype=np.dtype(dt))
    fn = algo.learn if mode == "iter" else algo.learn_vec
    for t in range(steps):
        ts, ta, tr, ts2, td = transitions_of(want, t, t + 1)
        fn(ts, ta, tr, ts2, td, float(whole["lr"][t]))  # (a Python float, as the schedule hands it to `_learn`)
    assert np.array_equal(algo.q_table, whole["q"])
