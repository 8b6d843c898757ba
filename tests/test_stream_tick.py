"""The fused tick -- {pack, solve, post} of a stream in one launch -- as device code: the kernel entry text csrc/bmpc_tick_kernel.inl compiled for the CPU
(tests/emu/bmpc_emu.cpp, emu.stream_tick), one wave per stream and the team of 4, against the three separate entries the three-kernel tick runs, written
out here.  Bit for bit on every tick array; the skip of a stream that has lost its plan, lane and wave orders, several streams per launch, the arguments
the entry refuses."""
import ctypes

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu
from tests.emu import emu_rollout as er

SS = bstream.SS
H = 0.1


def _opts(N):
    return emu.opts_for(N, start_rollout=0)


def _stream(N, S, which=2):
    _, rec, T, ss = er.small_stream(N, S, which=which)
    return np.ascontiguousarray(T, dtype=np.float64), er.fresh_arrays(N, S, ss, rec)


def _separate_entries_tick(N, S, T, A, warm_dual=True):
    """one tick as the three-kernel tick runs it: emu.stream_pack -> the in-kernel solve on what it packed -> the post entry on the stream's persisting record"""
    dual = A["dual"] if warm_dual else None
    p, x0 = emu.stream_pack(N, S, T, A["ss"], A["rb"], dual=dual)
    A["p"][:], A["x0"][:] = p, x0
    r = emu.solve(p, x0, N, S, H, opts=_opts(N), state=dual[None] if dual is not None else None, in_kernel=True)
    A["x"][:], A["g"][:], A["iters"][0], A["status"][0], A["kkt"][0] = r["x"][0], r["g"][0], r["iters"][0], r["status"][0], r["kkt"][0]
    # (the emulator's own entry, not emu.stream_post: that one hands out a fresh record per call, while a stream's record persists -- a shortened
    # trajectory leaves the columns behind it as the tick before wrote them)
    c = ctypes
    emu.lib().bmpc_emu_stream_post(c.c_int(N), c.c_int(S), c.c_double(H), emu._p(T), emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["x"]), emu._p(A["g"]),
                                   c.c_int(int(A["status"][0])), emu._p(A["traj"]), c.c_int(1), c.c_double(1e-4), c.c_double(0.0))


def _four_ticks_against_the_separate_entries(N, S, warm_dual):
    T, A = _stream(N, S)
    B = er.copy_arrays(A)
    for t in range(4):
        _separate_entries_tick(N, S, T, A, warm_dual)
        emu.stream_tick(N, S, H, T, B, warm_dual=warm_dual, opts=_opts(N))
        er.assert_arrays_equal(A, B, f"N {N} S {S} tick {t}")
        assert A["status"][0] == 0 and A["iters"][0] > 0
    if not warm_dual:
        assert (B["dual"] == 0.0).all()


@pytest.mark.parametrize("N,S", [(2, 2), (1, 2), (3, 5), (12, 2)])
def test_tick_entry_equals_the_separate_entries_bit_for_bit(N, S):
    """4 ticks from the cold start, dual state carried: both iterate placements ((2, 2), (1, 2): LDS; (3, 5): S beyond the LDS window; (12, 2): N beyond
    the short horizons), the smallest horizon."""
    _four_ticks_against_the_separate_entries(N, S, True)


def test_tick_entry_equals_the_separate_entries_without_the_dual_state():
    _four_ticks_against_the_separate_entries(2, 2, False)


def _assert_lost_plan_is_skipped(N, S, **kw):
    T, A = _stream(N, S)
    A["ss"][SS["ERRCNT"]] = N
    A["status"][0], A["iters"][0], A["kkt"][0] = 7, 7, 7.0
    B = er.copy_arrays(A)
    emu.stream_tick(N, S, H, T, B, opts=_opts(N), **kw)
    assert (B["status"][0], B["iters"][0], B["kkt"][0]) == (3, 0, 0.0)
    for k in er.TICK_ARRAYS:
        if k not in ("status", "iters", "kkt"):
            assert np.array_equal(A[k], B[k], equal_nan=True), k


def test_a_stream_that_has_lost_its_plan_is_not_ticked():
    """ERRCNT = N before the tick: status 3, iters 0, kkt 0, every other array bit-unchanged"""
    _assert_lost_plan_is_skipped(2, 2)


def test_tick_entry_in_any_lane_order():
    N, S = 2, 2
    T, A0 = _stream(N, S)
    ref = er.copy_arrays(A0)
    for _ in range(2):
        emu.stream_tick(N, S, H, T, ref, opts=_opts(N))
    for order in (1, 2):
        C = er.copy_arrays(A0)
        for _ in range(2):
            emu.stream_tick(N, S, H, T, C, opts=_opts(N), lane_order=order)
        er.assert_arrays_equal(ref, C, f"lane order {order}")


def test_several_streams_in_one_call_equal_one_call_each():
    """B = 3 distinct streams.  The arrays hold a fourth row of a sentinel behind the three: the entry's extra block (b = B, the kernel's own guard) writes nothing."""
    N, S, B = 2, 2, 3
    streams = [_stream(N, S, which=w) for w in range(B)]
    assert not np.array_equal(streams[0][1]["rb"], streams[1][1]["rb"]) and not np.array_equal(streams[1][1]["rb"], streams[2][1]["rb"])
    T = np.stack([s[0] for s in streams])
    sentinel = {k: (-12345 if streams[0][1][k].dtype == np.int32 else -12345.5) for k in er.TICK_ARRAYS}
    full = {k: np.ascontiguousarray(np.stack([s[1][k] for s in streams] + [np.full_like(streams[0][1][k], sentinel[k])])) for k in er.TICK_ARRAYS}
    for k in ("iters", "status", "kkt"):
        full[k] = np.ascontiguousarray(full[k].reshape(B + 1))
    batch = {k: v[:B] for k, v in full.items()}
    for t in range(2):
        emu.stream_tick(N, S, H, T, batch, opts=_opts(N))
        for b, (Tb, Ab) in enumerate(streams):
            emu.stream_tick(N, S, H, Tb, Ab, opts=_opts(N))
            for k in er.TICK_ARRAYS:
                assert np.array_equal(np.ravel(batch[k][b]), np.ravel(Ab[k]), equal_nan=True), (t, b, k)
    for k in er.TICK_ARRAYS:
        assert (full[k][B] == sentinel[k]).all(), k


def test_team_tick_is_order_invariant_and_follows_the_one_wave_tick():
    """The team of 4 (bmpc_team_tick_kernel, wave 0 packs and posts, the team solves) at (2, 2), 4 ticks: bit for bit the same under the (lane, wave) orders
    (1, 1), (2, 2), (0, 2); against the one-wave tick equal status, equal iterations and |dx| <= 1e-9 (the bound tests/test_emu.py holds teams to against
    one wave).  Measured worst |dx| over the 4 ticks: 0.0."""
    N, S = 2, 2
    T, A0 = _stream(N, S)
    one, team = er.copy_arrays(A0), er.copy_arrays(A0)
    others = {o: er.copy_arrays(A0) for o in ((1, 1), (2, 2), (0, 2))}
    worst = 0.0
    for t in range(4):
        emu.stream_tick(N, S, H, T, one, opts=_opts(N))
        emu.stream_tick(N, S, H, T, team, opts=_opts(N), nw=4)
        for (lo, wo), C in others.items():
            emu.stream_tick(N, S, H, T, C, opts=_opts(N), nw=4, lane_order=lo, wave_order=wo)
            er.assert_arrays_equal(team, C, f"tick {t}, lane order {lo}, wave order {wo}")
        worst = max(worst, np.abs(team["x"] - one["x"]).max())
        print(f"tick {t}: team against one wave, status {team['status'][0]} / {one['status'][0]}, iters {team['iters'][0]} / {one['iters'][0]}, worst |dx| so far {worst:.3e}")
        assert team["status"][0] == one["status"][0] == 0 and team["iters"][0] == one["iters"][0] > 0
        assert np.abs(team["x"] - one["x"]).max() <= 1e-9


def test_team_tick_skips_a_stream_that_has_lost_its_plan():
    _assert_lost_plan_is_skipped(2, 2, nw=4)


@pytest.mark.parametrize("nw", [1, 4])
def test_tick_entry_refuses_what_the_library_refuses(nw):
    """tick_args_ok of the C ABI: a path table shorter than S + 1 entries, x = NULL, a negative iteration cap"""
    N, S = 2, 2
    T, A = _stream(N, S)
    B = er.copy_arrays(A)
    assert emu.stream_tick(N, S, H, T[:S], B, opts=_opts(N), nw=nw, want_rc=True) == 1
    assert emu.stream_tick(N, S, H, T, dict(B, x=None), opts=_opts(N), nw=nw, want_rc=True) == 1
    assert emu.stream_tick(N, S, H, T, B, opts=_opts(N), nw=nw, max_iter=-1, want_rc=True) == 1
    er.assert_arrays_equal(A, B, "refused calls")
    assert emu.stream_tick(N, S, H, T, B, opts=_opts(N), nw=nw, want_rc=True) == 0 and B["status"][0] == 0
