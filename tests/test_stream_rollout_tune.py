"""Sweeps inside a rollout -- a table of controller settings per stream, validated and resolved on the device -- as device code compiled for the CPU
(csrc/bmpc_rollout_kernel.inl with TU; tests/emu/bmpc_emu_rollout.cpp, once for one wave per stream and once for teams of four).  The checker is
the contract: stream b of a tuned rollout against the ONE-STREAM run of the queue entry's CPU build with the resolved row as its settings, bit for bit
(emu_rollout.assert_equals_one_stream_runs).  (2, 2), B = 4 streams of emu_rollout.small_stream behind a solved-out tick 0, T = 6; the table of
emu_rollout.table: all NaN / a low cap and a loose tol / the held mode as slots / margin, slack push, stall window, final level."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er

TUNE, CROSS, ROLL, RP = bstream.TUNE, bstream.TUNE_CROSS, bstream.ROLL, bstream.RP
N, S, T, B = 2, 2, 6, 4
H = er.H
NAN = float("nan")
_copy = er.copy_arrays


def _queue(K=2):
    """[B][K][len]: a leg back, then a leg back with a detour, per stream"""
    kinds = [er.small_batch(N, S, B)[3], er.small_batch(N, S, B, detour=0.05)[3]]
    return np.ascontiguousarray(np.stack([kinds[k % 2] for k in range(K)], axis=1))


def _events():
    """a two-record queue (record 0 behind tick 1 or 2, record 1 behind tick 4) and disturbances on ticks 1 and 4"""
    lt = np.array([[1, 4], [2, 4], [1, 4], [2, 4]], dtype=np.int32)
    return dict(leg_tick=lt, leg_on=np.zeros((B, 2), dtype=np.int32), disturb=er.disturbances(T, B, on=(1, 4)))


# ---- 1. the contract ----
@pytest.mark.parametrize("nw,wave_order,lane_order", [(1, 0, 0), (1, 0, 2), (4, 0, 0), (4, 1, 1)])
def test_a_tuned_rollout_equals_one_stream_runs_with_the_resolved_rows(nw, wave_order, lane_order):
    """events, audit, log, tracking record and a two-record queue on, real-time acceptance on (the held row's acceptance words are read): every tick
    array, history array, record and queue output of every stream; under other lane and wave orders the same bits"""
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, tab = _queue(), er.table()
    r, A, Tb, R = er.assert_equals_one_stream_runs(N, S, A0, Tab, Q, T, tab, f"nw {nw} orders {wave_order} {lane_order}", nw=nw, wave_order=wave_order, lane_order=lane_order,
                                                   accept_capped=True, log_stages=N, **_events())
    assert r["tune_info"].tolist() == [0] * B and r["ticks_run"].tolist() == [T] * B and r["legs_done"].tolist() == [2] * B
    assert np.array_equal(r["tune_used"][:, 14:], np.zeros((B, 2))) and not np.isnan(r["tune_used"]).any()
    # an ignored table cannot pass: every row that sets something changes the iterations or the iterate of its stream against the untuned run
    C, Tc = _copy(A0), Tab.copy()
    plain = er.rollout(N, S, H, Tc, C, T, entry=5, tune=None, nw=nw, wave_order=wave_order, lane_order=lane_order, replan=Q.copy(), accept_capped=True, log_stages=N, **_events())
    assert plain["ran"] == 4
    er.assert_streams_equal(er.stream_of(r, 0), er.stream_of(plain, 0), "the all-NaN row")
    assert np.array_equal(A["x"][0], C["x"][0])
    for b in (1, 2, 3):
        assert not np.array_equal(r["hist"][:, b, ROLL["ITERS"]], plain["hist"][:, b, ROLL["ITERS"]]) or not np.array_equal(A["x"][b], C["x"][b]), f"row {b} changed nothing"
    assert (r["hist"][:, 1, ROLL["ITERS"]] <= 3).all() and (r["hist"][:, 2, ROLL["ITERS"]] == 30).all() and (r["hist"][:, 2, ROLL["STATUS"]] == 1).all()
    if (nw, wave_order, lane_order) != (nw, 0, 0):      # the orders change no bit
        D, Td = _copy(A0), Tab.copy()
        fwd = er.rollout(N, S, H, Td, D, T, entry=5, tune=tab, nw=nw, replan=Q.copy(), accept_capped=True, log_stages=N, **_events())
        for b in range(B):
            er.assert_arrays_equal(er.unstack(A, b), er.unstack(D, b), f"orders, stream {b}")
            er.assert_streams_equal(er.stream_of(r, b), er.stream_of(fwd, b), f"orders, stream {b}")


def test_a_sweep_without_a_queue_and_on_a_held_launch():
    """replan NULL (the Python layer's call without legs), and NaN slots that resolve to a launch in held mode with an iteration cap argument"""
    from tests.rollout_contract import HELD
    A0, Tab, _ = er.start(N, S, 1, B)
    base = dict(opts=er.emu.opts_for(N, start_rollout=0, tol=HELD["tol"], mu_init=0.1, mu_warm=0.01, mu_min_fac=10.0, bound_margin=HELD["bound_margin"], hold_mu=1),
                max_iter=5, rt_tol=1e-2, rt_row_cap=1e-5, level_rule=(0.02, 0.01, 0.1))
    r, _, _, _ = er.assert_equals_one_stream_runs(N, S, A0, Tab, None, T, er.table(), "held launch", base=base, accept_capped=True, disturb=er.disturbances(T, B, on=(1, 4)))
    assert r["legs_done"] is None and r["tune_info"].tolist() == [0] * B
    want0 = [5, 1e-3, 0.1, 0.01, 10.0, 0.01, 2e-3, 1, 0.02, 0.01, 0.1, 1e-2, 1e-5, 40, 0, 0]
    assert r["tune_used"][0].tolist() == want0 and r["tune_used"][1, :2].tolist() == [3.0, 1e-3] and r["tune_used"][1, 2:].tolist() == want0[2:]
    assert (r["hist"][:, 0, ROLL["ITERS"]] == 5).all() and (r["hist"][:, 1, ROLL["ITERS"]] <= 3).all() and (r["hist"][:, 2, ROLL["ITERS"]] == 30).all()


# ---- 2. no table, a table of NaN ----
@pytest.mark.parametrize("nw", [1, 4])
def test_no_table_and_a_table_of_nan_are_the_queue_entry(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev = _queue(), _events()
    A, Tb, R = _copy(A0), Tab.copy(), Q.copy()
    want = er.rollout(N, S, H, Tb, A, T, entry=4, nw=nw, replan=R, log_stages=N, **ev)
    assert want["ran"] == 4
    for tab, ran in ((None, 4), (np.full((B, TUNE["LEN"]), NAN), 5)):
        C, Tc, Rc = _copy(A0), Tab.copy(), Q.copy()
        r = er.rollout(N, S, H, Tc, C, T, entry=5, tune=tab, nw=nw, replan=Rc, log_stages=N, **ev)
        assert r["ran"] == ran
        for k in er.TICK_ARRAYS:
            assert np.array_equal(A[k], C[k], equal_nan=True), k
        assert np.array_equal(Tb, Tc) and np.array_equal(R, Rc)
        for k in er.OUTPUTS + ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why"):
            assert np.array_equal(want[k], r[k], equal_nan=True), k
        # without a table its outputs are not looked at; with one every row resolves to the launch's settings
        assert (r["tune_info"] == (-7 if tab is None else 0)).all()
        assert (r["tune_used"] == -7.0).all() if tab is None else np.array_equal(r["tune_used"], np.tile(er.tune_check(np.full(16, NAN), N)[1], (B, 1)))


# ---- 3. the validity rule ----
EDGE = [NAN, np.inf, -np.inf, -0.0, 0.0, 0.5, 1.0, 0.3, 2.5, 3.0, 16.0, 17.0, -1.0, 100000.0, 100001.0, 1e-300, 0.5000001, 2147483646.0, 2147483648.0, 1e308]


def test_the_python_rule_is_the_compiled_rule():
    """every slot on the edge values, one slot at a time; then the cross-slot test on the row as resolved, against launches with and without a level rule"""
    names = [n for n in TUNE if n != "LEN"]
    for name in names:
        for v in EDGE:
            row = np.full(TUNE["LEN"], NAN); row[TUNE[name]] = v
            bad, used = er.tune_check(row, N)
            ok = np.isnan(v) or bstream.tune_slot_ok(name, v)
            assert bool(bad & 1 << TUNE[name]) == (not ok), (name, v, bad)
            assert bad & ~(1 << TUNE[name] | 1 << CROSS) == 0
            assert bstream.tune_check(row, used if np.isnan(v) else None) & 1 << TUNE[name] == bad & 1 << TUNE[name]
            assert np.isnan(v) or used[TUNE[name]] == v or (v == 0 and used[TUNE[name]] == 0)      # (a refused value shows as it was given)
    # what each slot accepts, in words
    ok = lambda name: [v for v in EDGE[1:] if bstream.tune_slot_ok(name, v)]
    assert ok("MAX_ITER") == [1.0, 3.0, 16.0, 17.0, 100000.0] and ok("HOLD") == [-0.0, 0.0, 1.0] and ok("BOUND_MARGIN") == [-0.0, 0.0, 0.5, 0.3, 1e-300]
    assert ok("STALL_WINDOW") == [-0.0, 0.0, 16.0, 100000.0, 2147483646.0] and ok("TOL") == [0.5, 1.0, 0.3, 2.5, 3.0, 16.0, 17.0, 100000.0, 100001.0, 1e-300, 0.5000001, 2147483646.0, 2147483648.0, 1e308]
    assert ok("RT_ROW_CAP") == [-0.0, 0.0] + ok("TOL") and ok("LVL_HI") == ok("RT_ROW_CAP")
    # the cross-slot test: (lo, hi) as given, against a launch without a rule (0, 0, 0) and against one with (0.02, 0.01, 0.1)
    rule = (0.02, 0.01, 0.1)
    for lo, hi, plain, ruled in ((0.0, 0.1, True, True), (0.2, 0.1, True, True), (0.05, 0.1, False, False), (0.1, 0.1, False, False), (0.0, 0.0, False, False),
                                 (NAN, 0.005, True, True), (NAN, 0.5, True, False), (0.0, NAN, False, True), (0.2, NAN, False, True), (0.05, NAN, False, False), (NAN, NAN, False, False)):
        row = np.full(TUNE["LEN"], NAN); row[TUNE["LVL_LO"]], row[TUNE["LVL_HI"]] = lo, hi
        for level_rule, want in (((0.0, 0.0, 0.0), plain), (rule, ruled)):
            bad, used = er.tune_check(row, N, level_rule=level_rule)
            assert bad == (1 << CROSS if want else 0), (lo, hi, level_rule, bad)
            defaults = er.tune_check(np.full(16, NAN), N, level_rule=level_rule)[1]
            assert bstream.tune_check(row, defaults) == bad
    # tune_table refuses what the device refuses
    for kw in (dict(max_iter=0), dict(tol=-1.0), dict(hold=2), dict(stall_window=15), dict(bound_margin=0.6), dict(lvl_lo=0.0, lvl_hi=0.1), dict(rt_tol=np.inf), dict(mu_warm=[1.0, 0.0])):
        with pytest.raises(ValueError, match="tune row"):
            bstream.tune_table(2, **kw)


@pytest.mark.parametrize("nw", [1, 4])
def test_invalid_rows_do_not_run_and_their_neighbours_do(nw):
    """rows 0 and 2 invalid (an odd stall window with a zero tol; a level rule that fails as resolved), rows 1 and 3 of the table of the tests"""
    A0, Tab, _ = er.start(N, S, nw, B)
    Q, ev, tab = _queue(), _events(), er.table()
    bad = tab.copy()
    bad[0, TUNE["STALL_WINDOW"]], bad[0, TUNE["TOL"]] = 15.0, 0.0
    bad[2] = NAN; bad[2, TUNE["LVL_HI"]] = 0.1
    A, Tb, R = _copy(A0), Tab.copy(), Q.copy()
    for k in ("x", "g", "kkt", "p", "x0"):
        A[k][[0, 2]] = 7.25      # (what the memory held: it stays)
    A["iters"][[0, 2]], A["status"][[0, 2]] = 77, 9
    before = _copy(A)
    r = er.rollout(N, S, H, Tb, A, T, entry=5, tune=bad, nw=nw, replan=R, accept_capped=True, log_stages=N, **ev)
    assert r["tune_info"].tolist() == [1 << TUNE["STALL_WINDOW"] | 1 << TUNE["TOL"], 0, 1 << CROSS, 0] and r["ticks_run"].tolist() == [0, T, 0, T]
    assert r["tune_used"][0, TUNE["STALL_WINDOW"]] == 15.0 and r["tune_used"][0, TUNE["TOL"]] == 0.0 and r["tune_used"][2, TUNE["LVL_HI"]] == 0.1 and r["tune_used"][2, TUNE["LVL_LO"]] == 0.0
    for b in (0, 2):
        er.assert_arrays_equal(er.unstack(before, b), er.unstack(A, b), f"invalid row, stream {b}")
        assert np.array_equal(Tb[b], Tab[b]) and np.array_equal(R[b], Q[b]) and (R[b, :, RP["FLAG"]] == 1.0).all()
        assert all(np.isnan(r[k][:, b]).all() for k in ("hist", "traj_hist", "tube_hist", "log_hist"))
        assert r["legs_done"][b] == 0 and (r["leg_fired"][b] == -1).all() and (r["leg_why"][b] == 0).all() and (r["replan_info"][b] == -1).all()
    # ... their audit and tracking records are those of a stream lost on entry
    L, Tl = _copy(A0), Tab.copy()
    L["ss"][:, bstream.SS["ERRCNT"]] = N
    lost = er.rollout(N, S, H, Tl, L, T, entry=5, tune=None, nw=nw, replan=Q.copy(), log_stages=N, **ev)
    assert lost["ticks_run"].tolist() == [0] * B
    for b in (0, 2):
        assert np.array_equal(r["audit"][b], lost["audit"][b], equal_nan=True) and np.array_equal(r["track"][b], lost["track"][b], equal_nan=True)
    # the neighbours: what the table of the tests gives them
    C, Tc, Rc = _copy(A0), Tab.copy(), Q.copy()
    good = er.rollout(N, S, H, Tc, C, T, entry=5, tune=tab, nw=nw, replan=Rc, accept_capped=True, log_stages=N, **ev)
    for b in (1, 3):
        er.assert_arrays_equal(er.unstack(C, b), er.unstack(A, b), f"neighbour {b}")
        er.assert_streams_equal(er.stream_of(r, b), er.stream_of(good, b), f"neighbour {b}")
        assert np.array_equal(Tb[b], Tc[b]) and np.array_equal(R[b], Rc[b])


def test_argument_errors_of_the_entry():
    """what the queue entry refuses, with a table; the table's outputs may be NULL"""
    A0, Tab, _ = er.start(N, S, 1, B)
    Q, tab = _queue(), er.table()
    lt, lo = np.ones((B, 2), dtype=np.int32), np.zeros((B, 2), dtype=np.int32)
    ok = dict(replan=Q, leg_tick=lt, leg_on=lo)
    for kw in (dict(ok, leg_tick=None), dict(ok, leg_on=None), dict(ok, update_flags=8), dict(ok, ticks=0), dict(ok, simulate=False), dict(ok, goal_tol=-1.0), dict(goal_tol=NAN),
               dict(ok, audit_tol=-1.0), dict(audit_tol=np.inf), dict(ok, log_stages=N + 1)):
        A, Tb = _copy(A0), Tab.copy()
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else Q.copy()
        assert er.rollout(N, S, H, Tb, A, kw.pop("ticks", 2), entry=5, tune=tab, want_rc=True, **kw) == 1, {k: v for k, v in kw.items() if k != "replan"}
        for b in range(B):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=5, tune=tab, want_rc=True, want_tune_info=False, want_used=False, **dict(ok, replan=Q.copy())) == 0


# ---- 4. the surface ----
def test_the_python_surface():
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "boundmpc_hip.h")).read()
    enum = re.search(r"enum \{ (BMPC_TUNE_MAX_ITER = 0,.*?) \};", header, re.S).group(1)
    names = [w.strip() for w in enum.replace("\n", " ").split(",")]
    assert names[-1] == "BMPC_TUNE_LEN = 16" and names[0] == "BMPC_TUNE_MAX_ITER = 0"
    order = [n.split("=")[0].strip()[len("BMPC_TUNE_"):] for n in names[:-1]]
    assert order == sorted((n for n in TUNE if n != "LEN"), key=TUNE.get) and [TUNE[n] for n in order] == list(range(14)) == er.tune_slots()
    assert TUNE["LEN"] == 16 == bstream.tune_len() and CROSS == 15
    from boundmpc_amd import _lib, solver
    for sym in ("bmpc_stream_tune_len", "bmpc_stream_tune_defaults", "bmpc_stream_rollout_tuned"):
        assert sym in _lib.SIGNATURES and re.search(r"\b%s\(" % sym, header)
    assert len(_lib.SIGNATURES["bmpc_stream_rollout_tuned"][1]) == len(_lib.SIGNATURES["bmpc_stream_rollout_legs"][1]) + 3
    libpath = _lib.LIB_PATH
    if os.path.exists(libpath):      # (a built tree: the three symbols are exported; loading the library needs no GPU)
        L = ctypes.CDLL(libpath)
        assert all(hasattr(L, sym) for sym in ("bmpc_stream_tune_len", "bmpc_stream_tune_defaults", "bmpc_stream_rollout_tuned")) and L.bmpc_stream_tune_len() == 16
    assert {"tune", "want_tune_used"} <= set(inspect.signature(bstream.StreamBatch.rollout).parameters) and hasattr(solver.BatchedOCPSolver, "tune_defaults")
    # tune_table: scalars, arrays, NaN elsewhere; unpack_tune
    t = bstream.tune_table(3, max_iter=[5, NAN, 7], TOL=1e-4)
    assert t.shape == (3, 16) and t[:, 0].tolist()[::2] == [5.0, 7.0] and np.isnan(t[1, 0]) and (t[:, 1] == 1e-4).all() and np.isnan(t[:, 2:]).all()
    u = bstream.unpack_tune(t[0])
    assert u["max_iter"] == 5 and isinstance(u["max_iter"], int) and u["tol"] == 1e-4 and u["hold"] is None and set(u) == {n.lower() for n in TUNE if n != "LEN"}
    with pytest.raises(ValueError, match="no slot"):
        bstream.tune_table(2, cap=3)
    with pytest.raises(ValueError, match="must be a scalar"):
        bstream.tune_table(2, tol=[1e-3] * 3)
    # fixed_barrier= expands as the constructor does: "auto", a pair, a float (the constructor's lines: hold and the level rule for the first two)
    src = inspect.getsource(solver.BatchedOCPSolver.__init__)
    assert "(0.01, 0.1) if fixed_barrier == \"auto\"" in src and "mu_min_fac = lo / float(tol)" in src and "mu_init, mu_warm = hi, lo" in src and "level_c=0.02" in src
    t = bstream.tune_table(4, tol=[1e-3, 1e-3, 1e-2, 1e-3], fixed_barrier=["auto", (0.02, 0.2), 0.05, None], level_c=0.02)
    pick = lambda b: [t[b, TUNE[n]] for n in ("HOLD", "LVL_C", "LVL_LO", "LVL_HI", "MU_INIT", "MU_WARM", "MU_MIN_FAC")]
    assert pick(0) == [1.0, 0.02, 0.01, 0.1, 0.1, 0.01, 0.01 / 1e-3] and pick(1) == [1.0, 0.02, 0.02, 0.2, 0.2, 0.02, 0.02 / 1e-3]
    assert pick(2) == [0.0, 0.0, 0.0, 0.0, 0.05, 0.05, 0.05 / 1e-2] and np.isnan(pick(3)).all()
    assert np.array_equal(bstream.tune_table(2, tol=1e-3, fixed_barrier="auto")[1], t[0], equal_nan=True)
    with pytest.raises(ValueError, match="needs the tol column"):
        bstream.tune_table(2, fixed_barrier="auto")
    with pytest.raises(ValueError, match="sets hold"):
        bstream.tune_table(2, tol=1e-3, fixed_barrier="auto", mu_init=0.3)


# ---- 5. the stand-alone program under the sanitizers ----
def sanitizer_cases(nw):
    A0, Tab, _ = er.start(N, S, nw, B)
    bad = er.table(); bad[0, TUNE["TOL"]] = -1.0
    return [("table", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, tune=er.table(), disturb=er.disturbances(3, B, on=(1,)), flags=3)),
            ("refused", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=3, tune=bad, flags=3))]


@pytest.mark.parametrize("nw", [1, 4])
def test_the_tune_text_is_clean_under_the_sanitizers(nw):
    """the host program with its own main, built with -fsanitize=address,undefined on exact-size buffers and run as a child process (nothing is loaded
    into this interpreter); on teams under both wave orders"""
    out = er.run_sanitized(sanitizer_cases(nw), nw)
    print("\n".join(out))
    assert len(out) == 2 and all("rc 0 ran 5" in line and "DIFFERS" not in line for line in out)
    assert "[stream 0 ticks_run 3 tune_info 0" in out[0] and "[stream 2 ticks_run 3 tune_info 0 iters 30]" in out[0]
    assert "[stream 0 ticks_run 0 tune_info 2 " in out[1] and "[stream 1 ticks_run 3 tune_info 0" in out[1]
