"""The one statement of a configs[4] closed loop, on the CPU: workload.make_streams against the block it replaced, and the named reads of
the stream records (boundmpc_amd.stream) against unpack_traj and the raw words over a CPU mirror loop (tests/closed_loop.py)."""
import numpy as np
import pytest

from boundmpc_amd import stream as bstream, workload
from tests.closed_loop import Oracle, cpu_mirror_loop


@pytest.mark.parametrize("B,seed,N,take", [(3, 3, 10, None), (2, 11, 36, None), (256, 3, 10, 3)])
def test_make_streams_equals_the_inline_construction(B, seed, N, take):
    mpcs, recs = workload.make_streams(B, seed=seed, N=N, take=take)
    q0s = workload.random_q0(B, seed=seed)[:take]
    assert len(mpcs) == len(q0s) and recs.shape == (len(q0s), bstream.RB["LEN"])
    for b, q0 in enumerate(q0s):
        m, p0fk = workload.make_mpc(q0, N=N)
        rec = bstream.robot_record(q0, np.zeros(7), np.zeros(7), p0fk, np.zeros(6), np.array([m.phi_max[0], 0.0, 0.0]), np.zeros(7))
        assert np.array_equal(recs[b], rec)
        assert np.array_equal(bstream.path_table(mpcs[b].ref_path)[0], bstream.path_table(m.ref_path)[0])
        assert np.array_equal(bstream.initial_state(mpcs[b], N), bstream.initial_state(m, N))


@pytest.mark.parametrize("N", [10, 12])
def test_record_reads_equal_unpack_traj_over_a_loop_that_loses_its_plan(N):
    """One stream, the solver failing at ticks 3, 4 (rejected, then recovered) and from tick 6 on (the plan runs out): on every tick the named reads
    equal what unpack_traj and the raw words say, and has_plan flips exactly when the error count reaches N."""
    fails = (3, 4) + tuple(range(6, 6 + N))
    (mpc,), (rec,) = (a[2:] for a in workload.make_streams(3, seed=5, N=N))
    seen = []
    for c in cpu_mirror_loop(mpc, rec, 6 + N, N=N, solve=Oracle(fails, N=N, nthreads=4).solve):
        ss, tr = c["ss"], c["traj"]
        _, fl = bstream.unpack_traj(tr, N)
        assert bool(bstream.applied(tr)) == fl["success"] == (c["t"] not in fails)
        assert float(bstream.g_viol(tr)) == fl["g_viol"]
        ec = int(ss[bstream.SS["ERRCNT"]])
        assert bool(bstream.has_plan(ss, N)) == (ec < N) == bool(bstream.valid(ss))
        assert float(bstream.phi(ss)) == ss[bstream.SS["PHI"]] <= ss[bstream.SS["PHIMAX"]]
        if c["t"] == 0:
            assert c["phi"] == float(mpc.phi_current[0])      # (before the first pack: the host object's own path parameter)
        # the batched forms read the same words
        assert bstream.applied(tr[None])[0] == bstream.applied(tr) and bstream.has_plan(ss[None], N)[0] == bstream.has_plan(ss, N)
        seen.append((ec, bool(bstream.has_plan(ss, N))))
    assert [ec for ec, _ in seen] == [0, 0, 0, 1, 2, 0] + list(range(1, N + 1))
    assert [hp for _, hp in seen] == [True] * (5 + N) + [False]      # lost on the tick the count reaches N (N = 12: still held at 10 and 11)


@pytest.mark.parametrize("N", [10, 12])
def test_level_reads_the_word_the_pack_wrote_under_a_level_rule(N):
    rule = (0.02, 0.01, 0.1)
    (mpc,), (rec,) = (a[1:] for a in workload.make_streams(2, seed=3, N=N))
    kw = dict(tol=1e-3, mu_init=0.1, mu_warm=0.01, mu_min_fac=10.0, hold_mu=1)
    levels = []
    for c in cpu_mirror_loop(mpc, rec, 4, N=N, cap=5, accept_capped=True, rt_tol=1e-2, level_rule=rule, opts_kw=kw):
        if c["t"]:      # (tick 0 packs a cold dual state: the rule leaves it alone)
            want = min(max(rule[0] * (float(mpc.phi_max[0]) - c["phi"]), rule[1]), rule[2])
            assert abs(c["level"] - want) < 1e-15, (c["t"], c["level"], want)
        levels.append(c["level"])
    assert levels[0] == 0.0 and all(rule[1] <= v <= rule[2] for v in levels[1:])


def test_set_continue_rejected_writes_the_word_stream_pack_reads():
    N = 10
    ss = np.zeros((2, bstream.ss_len(N)))
    bstream.set_continue_rejected(ss, N)
    assert (ss[:, bstream.ss_updated(N) + 1] == 1.0).all() and ss.sum() == 2.0
    bstream.set_continue_rejected(ss, N, False)
    assert not ss.any()
