"""TEST-ONLY: the CPU build of the rollout in all its variants and entries (boundmpc_amd/csrc/bmpc_rollout_kernel.inl through tests/emu/bmpc_emu_rollout.cpp,
built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the rollouts share: the one wrapper of the one entry
(rollout; the library's RArgs record goes in as its ctypes mirror), the contract's loop {fused tick's own kernel text, plant step text, tube text, log text,
disturb text, splice + update text of the record due -- the scheduled one or the head of the queue --, stop rules} that is the exact checker of every
variant, the small streams and batches, their new paths and disturbances, the tables of the sweeps' tests, a resolved settings row as arguments.

  python -m tests.emu.emu_rollout --sanitize [4]    builds bmpc_emu_rollout.cpp (with bmpc_emu.cpp beside it: tick 0 of the cases without events runs the
                                                    fused tick's text) as a stand-alone program with -fsanitize=address,undefined and runs it on
                                                    plain_cases and on the cases of the missions', the sweeps' and the plants' tests
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream, workload
from tests.closed_loop import stream_arrays
from tests.emu import emu, emu_stream_log as el, emu_stream_tube as et, emu_stream_update as eup

TICK_ARRAYS = ("ss", "rb", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")
ROLL, SS, TUBE, AUDIT, TRACK = bstream.ROLL, bstream.SS, bstream.TUBE, bstream.AUDIT, bstream.TRACK
TUNE, CROSS, PLANT, PLANT_STATE, PLANT_REC = bstream.TUNE, bstream.TUNE_CROSS, bstream.PLANT, bstream.PLANT_STATE, bstream.PLANT_REC
AT_GOAL, ON_LOST, WHY_GOAL, WHY_LOST, WHY_TICK = 1, 2, 1, 2, 4
H = 0.1
NAN = float("nan")
HISTORIES = ("hist", "traj_hist", "tube_hist", "log_hist")      # per stream [ticks][B][..]
OUTPUTS = HISTORIES + ("audit", "track")                        # ... and [B][..]
_DEPS = ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl", "bmpc_stream_tube.inl", "bmpc_stream_log.inl", "bmpc_stream_plant.inl")


class RArgs(ctypes.Structure):
    """the library's RArgs record (csrc/bmpc_args.h), member by member; tests/test_stream_rollout.py holds it to the offsets of both builds"""
    _fields_ = [("ticks", ctypes.c_int), ("goal_tol", ctypes.c_double), ("hist", ctypes.c_void_p), ("traj_hist", ctypes.c_void_p), ("ticks_run", ctypes.c_void_p),
                ("replan", ctypes.c_void_p), ("replan_tick", ctypes.c_void_p), ("replan_info", ctypes.c_void_p), ("update_flags", ctypes.c_int), ("disturb", ctypes.c_void_p),
                ("tube_hist", ctypes.c_void_p), ("audit", ctypes.c_void_p), ("audit_tol", ctypes.c_double),
                ("log_hist", ctypes.c_void_p), ("log_stages", ctypes.c_int), ("track", ctypes.c_void_p),
                ("legs", ctypes.c_int), ("leg_tick", ctypes.c_void_p), ("leg_on", ctypes.c_void_p), ("leg_tol", ctypes.c_void_p), ("legs_done", ctypes.c_void_p),
                ("leg_fired", ctypes.c_void_p), ("leg_why", ctypes.c_void_p),
                ("tune", ctypes.c_void_p), ("tune_info", ctypes.c_void_p), ("tune_used", ctypes.c_void_p),
                ("plant", ctypes.c_void_p), ("plant_state", ctypes.c_void_p), ("plant_info", ctypes.c_void_p), ("plant_rec", ctypes.c_void_p)]


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout.so" if nw == 1 else f"libbmpc_emu_rollout_team{nw}.so", "bmpc_emu_rollout.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_rollout_waves() == nw and L.bmpc_emu_stream_rollout_len() == bstream.rollout_len() and L.bmpc_emu_stream_track_len() == bstream.track_len()
    assert L.bmpc_emu_rargs_size() == ctypes.sizeof(RArgs), "tests/emu/emu_rollout.py RArgs is not the library's record"
    assert L.bmpc_emu_leg_bits() == AT_GOAL | ON_LOST << 4 | WHY_GOAL << 8 | WHY_LOST << 12 | WHY_TICK << 16
    assert L.bmpc_emu_tune_slot(-1) == TUNE["LEN"] and L.bmpc_emu_tune_slot(-2) == CROSS
    assert [L.bmpc_emu_plant_slot(w, -1) for w in range(3)] == [PLANT["LEN"], PLANT_STATE["LEN"], PLANT_REC["LEN"]]
    return L


def rollout_log_len(N, stages):
    return lib().bmpc_emu_stream_rollout_log_len(ctypes.c_int(N), ctypes.c_int(int(stages)))


def tune_slots():
    """the slots of the kernel text's settings row, by position of the header's enum"""
    return [lib().bmpc_emu_tune_slot(k) for k in range(14)]


def plant_slots():
    """the enums of the kernel text's plant, by position of the header's: (row, state, record)"""
    return tuple([lib().bmpc_emu_plant_slot(w, k) for k in range(n)] for w, n in ((0, 5), (1, 2), (2, 6)))


# ---- streams, batches, events ----
def small_stream(N, S, seed=5, which=2, experiment=1):
    """(mpc, robot record, path table, stream state) of one workload stream at horizon N and window S, at rest in its start configuration"""
    q0 = workload.random_q0(which + 1, seed=seed)[which]
    mpc, p0fk = workload.make_mpc(q0, N=N, S=S, experiment=experiment)
    rec = bstream.robot_record(q0, np.zeros(7), np.zeros(7), p0fk, np.zeros(6), np.array([mpc.phi_max[0], 0.0, 0.0]), np.zeros(7))
    T, ss = stream_arrays(mpc, N)
    return mpc, rec, T, ss


def fresh_arrays(N, S, ss, rb):
    """the tick arrays of one stream as a StreamBatch allocates them (p, x0, x, g: whatever the memory held -- here NaN)"""
    tr = emu.stream_lengths(N)["traj"]
    return dict(ss=np.array(ss, dtype=float), rb=np.array(rb, dtype=float), p=np.full(141 + 91 * S, np.nan), x0=np.full(44 * N, np.nan), dual=np.zeros(57 * N + 2),
                x=np.full(44 * N, np.nan), g=np.full(43 * N, np.nan), iters=np.zeros(1, dtype=np.int32), status=np.zeros(1, dtype=np.int32), kkt=np.zeros(1),
                traj=np.zeros(tr))


def copy_arrays(A):
    return {k: v.copy() for k, v in A.items()}


def stack(arrays):
    """the tick arrays of B streams (fresh_arrays each) with a leading axis of B"""
    return {k: np.ascontiguousarray(np.stack([A[k] for A in arrays])) for k in arrays[0]}


def unstack(A, b):
    return {k: A[k][b].copy() for k in A}


def leg_back(mpc, rec, T, S, tube=1.0, detour=0.0):
    """A new path for a stream of small_stream: from the pose the splice will write (via point 0: a placeholder here) to the via points of the
    stream's own path in reverse order -- a leg back to the start -- with the tube limits scaled by `tube` and its middle via point raised by `detour` metres (a longer leg).  -> the arguments of replan_record after
    (S, entries), n = the stream's own number of via points (<= entries - S + 1)."""
    rp = mpc.ref_path
    n = T.shape[0] - S + 1
    at = lambda lst, j: np.array(lst[min(j, len(lst) - 1)], dtype=float)
    order = list(range(n))[::-1]
    pos = [at(rp.p, j) for j in order]
    rot = [at(rp.r, j) for j in order]
    pos[n // 2][2] += detour
    lim = lambda lst: [tube * at(lst, j) for j in order]
    sc = lambda lst: [float(at(lst, j)) for j in order]
    return [pos, rot, [lim(rp.p_lower), lim(rp.p_upper)], [lim(rp.r_lower), lim(rp.r_upper)], [at(rp.bp1, 0)], [at(rp.br1, 0)], sc(rp.s), sc(rp.e_p_min), sc(rp.e_r_min),
            sc(rp.e_p_max), sc(rp.e_r_max), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), np.array(mpc.weights, dtype=float)]


def small_batch(N, S, B=3, **leg):
    """B small streams (small_stream with `which` = 0..B-1) -> (mpcs, stacked tick arrays, T [B][cap][48], records [B][len] of leg_back(**leg), flags raised)"""
    streams = [small_stream(N, S, which=b) for b in range(B)]
    cap = max(s[2].shape[0] for s in streams)
    assert all(s[2].shape[0] == cap for s in streams)
    A = stack([fresh_arrays(N, S, ss, rec) for _, rec, _, ss in streams])
    T = np.ascontiguousarray(np.stack([s[2] for s in streams]))
    recs = np.ascontiguousarray(np.stack([bstream.replan_record(S, cap, *leg_back(m, rec, Tb, S, **leg)) for m, rec, Tb, _ in streams]))
    return [s[0] for s in streams], A, T, recs


def disturbances(ticks, B, on=(1, 4), seed=3, scale=(2e-3, 5e-3, 1e-2)):
    """[ticks][B][21]: zero but on the ticks `on`, where every stream gets its own small push in q, dq and ddq"""
    rng = np.random.default_rng(seed)
    d = np.zeros((ticks, B, bstream.DIST_LEN))
    for t in on:
        if t < ticks:
            d[t] = rng.normal(size=(B, 21)) * np.repeat(scale, 7)
    return d


def push(ticks=6, B=3):
    """[ticks][B][21]: behind tick 2 of stream 1 a push of 0.01 rad in every joint, alternating signs -- 5 mm outside the position tube"""
    d = np.zeros((ticks, B, bstream.DIST_LEN))
    d[2, 1, :7] = 0.01 * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    return d


def opts(N):
    """the option record of a stream handle: the horizon's defaults without the start rollout"""
    return emu.opts_for(N, start_rollout=0)


def _entry_opts(N, entry):
    """the option record a call without `opts` runs with: the library's defaults of the horizon; from the sweeps' entry on a stream handle's (opts)"""
    return opts(N) if entry >= 5 else emu.opts_for(N)


@functools.lru_cache(maxsize=None)
def start(N, S, nw=1, B=3):
    """small_batch(N, S, B) with tick 0 of every stream solved out (nw = 4: by the team tick): (tick arrays, path tables, re-plan records); copy before use"""
    _, A0, Tab, recs = small_batch(N, S, B)
    for b in range(B):
        Ab = unstack(A0, b)
        tick(N, S, H, Tab[b], Ab, max_iter=100, warm_dual=True, opts=opts(N), nw=nw)
        for k in A0:
            A0[k][b] = Ab[k]
    assert (A0["status"] == 0).all() and (A0["ss"][:, SS["ERRCNT"]] == 0).all()
    return A0, Tab, recs


def args_of_record(rec, S):
    """the arguments of apply_update after (ss, N, S) that a (spliced) record stands for"""
    RP, RV = bstream.RP, bstream.RV
    n, nb = int(rec[RP["N"]]), int(rec[RP["NB"]])
    via = rec[RP["HEAD"]:RP["HEAD"] + n * RV["LEN"]].reshape(n, RV["LEN"])
    col = lambda k, w: [via[j, RV[k]:RV[k] + w].copy() for j in range(n)]
    sc = lambda k: [float(via[j, RV[k]]) for j in range(n)]
    six = lambda k: np.concatenate([rec[RP[k]:RP[k] + 3], np.zeros(3)])
    return [col("P", 3), [via[j, RV["R"]:RV["R"] + 9].reshape(3, 3).copy() for j in range(n)], [col("PLO", 2), col("PUP", 2)], [col("RLO", 2), col("RUP", 2)],
            col("BP1", 3)[:nb], col("BR1", 3)[:nb], sc("S"), sc("EPMIN"), sc("ERMIN"), sc("EPMAX"), sc("ERMAX"), six("P0"), six("V"), six("A"), six("JERK"), six("P0"),
            rec[RP["W"]:RP["W"] + 15].copy()]


TRACK_INT = [TRACK[k] for k in ("SAMPLES", "TICK_EP_ORTH", "TICK_EP_PAR", "TICK_ER", "REPLAYED")] + [11]
TRACK_FLOAT = [i for i in range(12) if i not in TRACK_INT]


def assert_track(got, want, rtol=1e-12, atol=0.0):
    """tracking records [B][12]: the integer slots (samples, ticks, replayed) exactly, the others within the bound"""
    assert np.array_equal(got[:, TRACK_INT], want[:, TRACK_INT]), (got, want)
    np.testing.assert_allclose(got[:, TRACK_FLOAT], want[:, TRACK_FLOAT], rtol=rtol, atol=atol)


def cut(row, N, stages):
    """a whole log row (bmpc_stream_log) cut to its first `stages` stages: the body's prefix and the trailer"""
    row = np.asarray(row)
    assert row.shape[-1] == bstream.log_len(N)
    return np.concatenate([row[..., :stages * bstream.LOG_STAGE], row[..., -4:]], axis=-1)


# ---- the tables of the sweeps' tests, a settings row as arguments, the compiled validity rules, the plant step ----
def table(tol=1e-3):
    """[4][16].  Row 0: all NaN.  Row 1: a low cap and a loose tol.  Row 2: the held mode of tests/rollout_contract.py HELD written as slots, with the
    acceptance words its batches set (1e-2, 1e-5).  Row 3: a joint-limit margin, roomier slacks, a short stall window, a higher final barrier level (converged like row 0, on other iterates)."""
    from tests.rollout_contract import HELD
    T = bstream.tune_table(4, max_iter=[NAN, 3, HELD["max_iter"], NAN], tol=[NAN, tol, HELD["tol"], NAN], fixed_barrier=[None, None, HELD["fixed_barrier"], None],
                           bound_margin=[NAN, NAN, HELD["bound_margin"], 0.05], rt_tol=[NAN, NAN, 1e-2, NAN], rt_row_cap=[NAN, NAN, 1e-5, NAN],
                           slack_push=[NAN, NAN, NAN, 0.1], stall_window=[NAN, NAN, NAN, 16], mu_min_fac=[NAN, NAN, NAN, 0.5])
    assert np.isnan(T[0]).all() and T[2, TUNE["HOLD"]] == 1.0 and T[2, TUNE["MU_MIN_FAC"]] == 0.01 / HELD["tol"]
    return T


def settings(row, N, base=None):
    """A RESOLVED row as the arguments rollout and the contract's loop take per call: dict(opts, max_iter, rt_tol, rt_row_cap, level_rule).  base: the option
    record the words outside the table come from (None: opts(N))."""
    u = bstream.unpack_tune(row)
    assert all(v is not None for v in u.values()), "a resolved row holds no NaN"
    o = emu.Opts.from_buffer_copy(base if base is not None else opts(N))
    o.max_iter, o.tol, o.mu_init, o.mu_warm, o.mu_min_fac, o.slack_push = u["max_iter"], u["tol"], u["mu_init"], u["mu_warm"], u["mu_min_fac"], u["slack_push"]
    o.bound_margin, o.hold_mu, o.stall_window = u["bound_margin"], u["hold"], u["stall_window"]
    return dict(opts=o, max_iter=0, rt_tol=u["rt_tol"], rt_row_cap=u["rt_row_cap"], level_rule=(u["lvl_c"], u["lvl_lo"], u["lvl_hi"]))


def tune_check(row, N, opts=None, max_iter=0, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0)):
    """the COMPILED validity rule (csrc/bmpc_args.h bmpc_tune_check) on one row against a launch's settings -> (mask, the row as resolved)"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    used = np.full(TUNE["LEN"], -7.0)
    c = ctypes
    bad = lib().bmpc_emu_tune_check(c.c_int(N), c.byref(opts if opts is not None else _entry_opts(N, 5)), c.c_int(int(max_iter)), c.c_double(rt_tol), c.c_double(rt_row_cap),
                                    c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]), emu._p(row), emu._p(used))
    return bad, used


def plant_check(row):
    """the COMPILED validity rule (csrc/bmpc_args.h bmpc_plant_check) on one row -> (mask, the row as resolved)"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    assert row.shape == (PLANT["LEN"],)
    used = np.full(PLANT["LEN"], -7.0)
    return lib().bmpc_emu_plant_check(emu._p(row), emu._p(used)), used


def fresh_rec():
    rec = np.full(PLANT_REC["LEN"], -7.0)
    lib().bmpc_emu_stream_plant_init(emu._p(rec))
    return rec


def stream_plant(N, h, rb, ss, row, state, rec=None, tick=0):
    """what bmpc_stream_plant does with one stream, on copies -> (code, rb, state, rec): code 0 behind a step, -1 skipped (no plan), else the mask of an
    invalid row (both: nothing touched); rec None or accumulated"""
    rb, state, row, ss = (np.array(a, dtype=np.float64, order="C") for a in (rb, state, row, ss))
    rec = None if rec is None else np.array(rec, dtype=np.float64, order="C")
    code = lib().bmpc_emu_stream_plant(ctypes.c_int(N), ctypes.c_double(h), emu._p(rb), emu._p(ss), emu._p(row), emu._p(state), emu._p(rec), ctypes.c_int(int(tick)))
    return code, rb, state, rec


# ---- the rollout text ----
def rollout(N, S, h, T, A, ticks, nw=1, entry=0, level=None, replan=None, replan_tick=None, legs=None, leg_tick=None, leg_on=None, leg_tol=None, tune=None, plant=None,
            plant_state=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0,
            level_rule=(0.0, 0.0, 0.0), lane_order=0, wave_order=0, want_rc=False, audit=None, want_tube=None, audit_tol=1e-6, want_log=None, log_stages=1, track=None,
            want_done=None, want_fired=None, want_tune_info=None, want_used=None, want_plant_info=None, want_rec=None):
    """The CPU build of the rollout text (nw = 1: one wave per stream; 4: teams, the waves of a wide phase in `wave_order`) on the tick arrays `A` of B
    streams (fresh_arrays stacked; advanced in place) and the path tables T [B][cap][48], one workgroup striding over the streams.  entry: the C ABI entry
    the call stands for -- 0 bmpc_stream_rollout, 1 _events, 2 _audit, 3 _log, 4 _legs, 5 _tuned, 6 _plant.  The groups an entry has arguments for:
    replan [B][len] with replan_tick [B] (1 to 3: the scheduled record) or replan [B][K][len] with leg_tick, leg_on [B][K] int and leg_tol [B][K] or None
    (4 to 6: the queue; legs: the count the entry is told, K unless given -- the refusals), both written in place where a record is consumed; tune [B][16]
    (5, 6); plant [B][20] with plant_state [B][16], advanced in place (6).  The output arrays of an entry are on unless switched off (audit, want_tube:
    entry >= 2; want_log, track: entry >= 3; want_done: legs_done, want_fired: leg_fired, leg_why and replan_info -- entry 4, or a queue; want_tune_info,
    want_used: tune_info, tune_used -- entry 5, or a table; want_plant_info, want_rec: plant_info, plant_rec -- entry 6); an array switched off is NULL,
    and one the entry has no argument for is refused.  level: None = the instantiation the library's rule picks, else that one on the same arguments.
    opts None: the library's defaults of the horizon, from entry 5 on a stream handle's (opts(N)).
    -> dict(hist [ticks][B][52], traj_hist, ticks_run [B], replan_info [B] or [B][K], tube_hist [ticks][B][16], audit [B][12], log_hist [ticks][B][88
    log_stages + 4], track [B][12], legs_done [B], leg_fired, leg_why [B][K], tune_info [B], tune_used [B][16], plant_info [B], plant_rec [B][8]; None: an
    array not given; ran: the level that ran), or the return code with want_rc (1: what the C ABI refuses).  One stream (T [cap][48], A of fresh_arrays):
    the same without the axis B, ticks_run an int."""
    T = np.ascontiguousarray(T, dtype=np.float64) if T.ndim == 2 else T
    one = T.ndim == 2
    if one:
        assert all(v.flags.c_contiguous for v in A.values())
        T, A = T[None], {k: v[None] for k, v in A.items()}      # (views: the caller's arrays advance)
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n, queue = T.shape[0], max(int(ticks), 0), entry >= 4
    Kb = replan.shape[1] if queue and replan is not None else 1      # what the arrays hold; `legs` is what the entry is told
    on = lambda want, default: bool(default) if want is None else bool(want)
    i32 = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(shape)
    f64 = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
    full = lambda want, shape, fill, dtype=np.float64: np.full(shape, fill, dtype=dtype) if want else None
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    tube = full(on(want_tube, entry >= 2), (n, B, TUBE["LEN"]), 7.0)
    aud = full(on(audit, entry >= 2), (B, AUDIT["LEN"]), 7.0)
    log = full(on(want_log, entry >= 3), (n, B, bstream.LOG_STAGE * max(int(log_stages), 0) + 4), 7.0)
    trk = full(on(track, entry >= 3), (B, TRACK["LEN"]), 7.0)
    if queue:
        info, fired, why = (full(on(want_fired, entry == 4 or replan is not None), (B, Kb), -7, np.int32) for _ in range(3))
        done = full(on(want_done, entry == 4 or replan is not None), B, -7, np.int32)
    else:
        info, fired, why, done = full(entry >= 1, B, -7, np.int32), None, None, None
    tinfo = full(entry >= 5 and on(want_tune_info, entry == 5 or tune is not None), B, -7, np.int32)
    used = full(entry >= 5 and on(want_used, entry == 5 or tune is not None), (B, TUNE["LEN"]), -7.0)
    pinfo = full(on(want_plant_info, entry >= 6), B, -7, np.int32)
    prec = full(on(want_rec, entry >= 6), (B, PLANT_REC["LEN"]), -7.0)
    if replan is not None:
        assert replan.flags.c_contiguous and replan.dtype == np.float64 and replan.shape == ((B, Kb) if queue else (B,)) + (bstream.replan_len(S, T.shape[1]),)
    assert plant_state is None or (plant_state.flags.c_contiguous and plant_state.dtype == np.float64 and plant_state.shape == (B, PLANT_STATE["LEN"]))
    rt, lt, lo, ltol = i32(replan_tick, (B,)), i32(leg_tick, (B, Kb)), i32(leg_on, (B, Kb)), f64(leg_tol, (B, Kb))
    dz, tn, pl = f64(disturb, (n, B, bstream.DIST_LEN)), f64(tune, (B, TUNE["LEN"])), f64(plant, (B, PLANT["LEN"]))
    c, p = ctypes, emu._p
    r = RArgs(ticks=int(ticks), goal_tol=goal_tol, hist=p(hist), traj_hist=p(th), ticks_run=p(run), replan=p(replan), replan_tick=p(rt), replan_info=p(info),
              update_flags=int(update_flags), disturb=p(dz), tube_hist=p(tube), audit=p(aud), audit_tol=audit_tol, log_hist=p(log), log_stages=int(log_stages), track=p(trk),
              legs=(Kb if legs is None else int(legs)) if queue else 0, leg_tick=p(lt), leg_on=p(lo), leg_tol=p(ltol), legs_done=p(done), leg_fired=p(fired), leg_why=p(why),
              tune=p(tn), tune_info=p(tinfo), tune_used=p(used), plant=p(pl), plant_state=p(plant_state), plant_info=p(pinfo), plant_rec=p(prec))
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(opts if opts is not None else _entry_opts(N, entry)), c.c_int(B), p(T), c.c_int(T.shape[1]),
                                         p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), p(A["x"]), p(A["g"]),
                                         p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(rt_tol),
                                         c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]), c.c_int(lane_order),
                                         c.c_int(wave_order), c.c_int(int(entry)), c.c_int(-1 if level is None else int(level)), c.byref(ran), c.byref(r))
    if want_rc:
        return rc
    assert rc == 0
    r = dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk, legs_done=done, leg_fired=fired, leg_why=why,
             tune_info=tinfo, tune_used=used, plant_info=pinfo, plant_rec=prec)
    if one:
        r = {k: None if v is None else (int(v[0]) if k == "ticks_run" else v[0] if v.ndim < 3 else v[:, 0]) for k, v in r.items()}
    r["ran"] = ran.value
    return r


def stream_of(r, b):
    """the outputs of stream b of a batch result"""
    return {k: (None if r[k] is None else r[k][:, b] if k in HISTORIES else r[k][b]) for k in OUTPUTS + ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why")}


def assert_streams_equal(got, want, what):
    for k, v in want.items():
        assert (v is None and got[k] is None) or np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), f"{what}: {k} differs"


# ---- the contract's loop ----
def tick(N, S, h, T, A, **kw):
    """ONE fused tick -- the kernel entry text, emu.stream_tick -- on the tick arrays `A` (advanced in place).  Returns the history row the rollout would
    write behind this tick (None for a stream that has lost its plan, which the tick skips)."""
    lost = A["ss"][bstream.SS["ERRCNT"]] >= N
    emu.stream_tick(N, S, h, T, A, **kw)
    return None if lost else history_row(A)


def history_row(A):
    """what `hist` holds behind a tick, from the tick arrays of one stream"""
    return np.concatenate([A["rb"], [A["ss"][bstream.SS["PHI"]], A["ss"][bstream.SS["ERRCNT"]], float(A["iters"][0]), float(A["status"][0]), float(A["kkt"][0])], A["traj"][-4:]])


def due(N, ss, t, tick_k, on_k, tol_k):
    """the conditions of a head record that hold behind tick t on the state row ss (WHY bits); 0: not due.  A word with an unknown bit is never due."""
    on_k, tick_k = int(on_k), int(tick_k)
    if on_k & ~(AT_GOAL | ON_LOST):
        return 0
    why = 0
    if (on_k & AT_GOAL) and ss[SS["PHIMAX"]] - ss[SS["PHI"]] <= tol_k:
        why |= WHY_GOAL
    if (on_k & ON_LOST) and ss[SS["ERRCNT"]] >= N:
        why |= WHY_LOST
    if tick_k >= 0 and t >= tick_k:
        why |= WHY_TICK
    return why


def contract_loop(N, S, h, T, A, ticks, stages=1, replan=None, replan_tick=None, leg_tick=None, leg_on=None, leg_tol=None, plant_row=None, plant_state=None, with_rec=True,
                  update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], the scheduled record `replan` [len] or the queue `replan` [K][len], plant state
    [16]; all advanced in place), in the order of the kernel (the header comment of csrc/bmpc_rollout_kernel.inl): per tick the fused tick's text (kw: the
    arguments of emu.stream_tick -- the stream's settings; nw=4: the team tick's), then bmpc_stream_plant's text with tick t when a row is given (plant_row
    None: no plant step at all), then the history row, the tube text on the p that tick packed, the log text on what the tick left, cut to `stages`, then --
    for a stream that still runs -- the disturb text on row `disturb[t]`, then the splice + update text: of the scheduled record when replan_tick == t, of
    the HEAD record of a queue when one of its conditions holds (due; leg_tick, leg_on [K]; leg_tol [K] or None: goal_tol), the head advancing whatever the
    record's flag and validity.  The rollout's stop rules decide what "still runs" means: a tick the stream lost its plan ahead of is not run (it writes the
    three words of a skipped stream), nor anything behind it; with goal_tol > 0 nothing runs behind the tick that leaves phi_max - phi <= goal_tol AFTER its
    events.
    -> dict(hist [ticks][52], traj_hist, tube_hist [ticks][16], p_hist: the p of every tick, log_hist [ticks][88 stages + 4], phi, phi_max: the two words
    behind every tick ahead of its events, cmd: the first planned jerk of every tick [ticks][7], ticks_run, replan_info (a queue: [K]), legs_done,
    leg_fired [K], leg_why [K], plant_rec, snaps: copies of the arrays behind every tick, run or not), NaN rows for the ticks not run"""
    queue = replan is not None and replan.ndim == 2
    K = replan.shape[0] if queue else 0
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan), phi=np.full(ticks, np.nan),
             phi_max=np.full(ticks, np.nan), cmd=np.full((ticks, 7), np.nan), ticks_run=0, replan_info=np.full(K, -1, dtype=np.int32) if queue else -1, legs_done=0,
             leg_fired=np.full(K, -1, dtype=np.int32), leg_why=np.zeros(K, dtype=np.int32), plant_rec=fresh_rec() if plant_row is not None and with_rec else None, snaps=[])
    JERK = slice(bstream.RB["JERK"], bstream.RB["JERK"] + 7)
    for t in range(ticks):
        lost = A["ss"][SS["ERRCNT"]] >= N
        emu.stream_tick(N, S, h, T, A, **kw)
        if lost:                                                  # lost its plan: the tick wrote the words of a skipped stream and the stream stops
            break
        r["cmd"][t] = A["rb"][JERK]
        if plant_row is not None:
            code, rb, st, rec = stream_plant(N, h, A["rb"], A["ss"], plant_row, plant_state, r["plant_rec"], t)
            assert code in (0, -1)
            A["rb"][:], plant_state[:], r["plant_rec"] = rb, st, rec
        r["hist"][t], r["traj_hist"][t], r["p_hist"][t], r["ticks_run"] = history_row(A), A["traj"], A["p"], t + 1
        r["tube_hist"][t] = et.stream_tube(N, S, A["p"])[0]
        r["log_hist"][t] = cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        r["phi"][t], r["phi_max"][t] = A["ss"][SS["PHI"]], A["ss"][SS["PHIMAX"]]
        if disturb is not None:
            A["rb"][:] = eup.stream_disturb(A["rb"], disturb[t])
        k = r["legs_done"]
        why = due(N, A["ss"], t, leg_tick[k], leg_on[k], goal_tol if leg_tol is None else leg_tol[k]) if k < K else 0
        if why or (replan is not None and not queue and replan_tick == t):
            rec = replan[k] if queue else replan
            info, rec[:], T[:], A["ss"][:], A["rb"][:] = eup.stream_update_flags(N, S, h, rec, T, A["ss"], A["rb"], update_flags)
            if queue:
                r["replan_info"][k], r["leg_fired"][k], r["leg_why"][k], r["legs_done"] = info, t, why, k + 1
            else:
                r["replan_info"] = info
        r["snaps"].append(copy_arrays(A))
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    r["snaps"] += [copy_arrays(A)] * (ticks - len(r["snaps"]))
    return r


def assert_arrays_equal(A, B, what=""):
    for k in TICK_ARRAYS:
        assert np.array_equal(A[k], B[k], equal_nan=True), f"{what}: {k} differs (largest deviation {np.nanmax(np.abs(A[k].astype(float) - B[k].astype(float)))})"


def et_audit_track(N, loop, audit_tol=1e-6):
    """the audit and tracking records over the loop's own tube and log rows: the audit's exact numpy reduction (emu_stream_tube.audit_of) and the record
    text of the CPU build over the log rows (stream_track_init, stream_track)"""
    rows, up = np.ascontiguousarray(loop["log_hist"]), np.ascontiguousarray(loop["traj_hist"][:, -3])
    trk = np.full(TRACK["LEN"], -7.0)
    lib().bmpc_emu_stream_track_rows(ctypes.c_int(rows.shape[0]), ctypes.c_int(rows.shape[1]), emu._p(rows), emu._p(up), emu._p(trk))
    return et.audit_of(loop["tube_hist"], audit_tol), trk


def assert_equals_the_loop(N, S, A0, Tab, recs, ticks, what, leg_tick=None, leg_on=None, leg_tol=None, plant=None, state0=None, tune=None, nw=1, wave_order=0, lane_order=0,
                           stages=1, disturb=None, **kw):
    """The queue entry -- with a plant table the plants' entry -- on copies of (A0, Tab, recs [B][K][len] or None, state0 [B][16]) with the tables `plant` and
    `tune` against contract_loop, stream by stream, on other copies and with the settings of tune_used[b]: every tick array, the path table, the queue,
    every history array, the audit and tracking records, the queue's outputs, the plant state and the plant record, bit for bit.  kw: update_flags,
    goal_tol, accept_capped, max_iter, warm_dual, opts, audit_tol.  -> (result, arrays, tables, queues, plant state)"""
    entry = 4 if plant is None else 6
    A, Tb, R, st = copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy(), None if state0 is None else state0.copy()
    r = rollout(N, S, H, Tb, A, ticks, nw=nw, entry=entry, wave_order=wave_order, lane_order=lane_order, replan=R, leg_tick=leg_tick, leg_on=leg_on, leg_tol=leg_tol, tune=tune,
                plant=plant, plant_state=st, disturb=disturb, log_stages=stages, **kw)
    assert r["ran"] == entry and (plant is None or not r["plant_info"].any()) and (tune is None or not r["tune_info"].any())
    loop_kw = {k: v for k, v in kw.items() if k not in ("audit_tol", "opts")}
    per = lambda v, b: None if v is None else np.asarray(v)[b]
    for b in range(Tab.shape[0]):
        s = settings(r["tune_used"][b], N) if tune is not None else dict(opts=kw["opts"] if kw.get("opts") is not None else _entry_opts(N, entry))
        Ab, Tl, Rl, sl = unstack(A0, b), Tab[b].copy(), per(recs, b), per(state0, b)
        Rl, sl = (None if v is None else v.copy() for v in (Rl, sl))
        loop = contract_loop(N, S, H, Tl, Ab, ticks, stages, replan=Rl, leg_tick=per(leg_tick, b), leg_on=per(leg_on, b), leg_tol=per(leg_tol, b), plant_row=per(plant, b),
                             plant_state=sl, disturb=None if disturb is None else disturb[:, b], nw=nw, wave_order=wave_order, lane_order=lane_order, **{**loop_kw, **s})
        assert_arrays_equal(Ab, unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl, Tb[b], equal_nan=True) and (recs is None or np.array_equal(Rl, R[b], equal_nan=True)), f"{what}, stream {b}: table / queue"
        for k in HISTORIES:
            assert np.array_equal(loop[k], r[k][:, b], equal_nan=True), f"{what}, stream {b}: {k}"
        one = et_audit_track(N, loop, kw.get("audit_tol", 1e-6))
        assert np.array_equal(one[0], r["audit"][b], equal_nan=True) and np.array_equal(one[1], r["track"][b], equal_nan=True), f"{what}, stream {b}: audit / track"
        assert int(r["ticks_run"][b]) == loop["ticks_run"], f"{what}, stream {b}: ticks_run {r['ticks_run'][b]}, the loop's {loop['ticks_run']}"
        if plant is not None:
            assert np.array_equal(sl, st[b], equal_nan=True), f"{what}, stream {b}: plant_state"
            assert np.array_equal(loop["plant_rec"], r["plant_rec"][b], equal_nan=True), f"{what}, stream {b}: plant_rec {r['plant_rec'][b]}, the loop's {loop['plant_rec']}"
        if recs is not None:
            got = (int(r["legs_done"][b]), r["leg_fired"][b].tolist(), r["leg_why"][b].tolist(), r["replan_info"][b].tolist())
            want = (loop["legs_done"], loop["leg_fired"].tolist(), loop["leg_why"].tolist(), loop["replan_info"].tolist())
            assert got == want, f"{what}, stream {b}: legs_done, leg_fired, leg_why, replan_info {got}, the loop's {want}"
    return r, A, Tb, R, st


def assert_equals_one_stream_runs(N, S, A0, Tab, recs, ticks, tune, what, nw=1, wave_order=0, lane_order=0, rows=None, base=None, **kw):
    """The sweeps' entry on copies of (A0, Tab, recs [B][K][len] or None) with the table `tune` against, stream by stream, the ONE-STREAM run of
    the queue entry with the settings of tune_used[b] (rows: the streams to check; None: those whose row is valid): every tick array, the path
    table, the queue, every history array, record and queue output, bit for bit.  kw: the arguments both take (leg_tick, leg_on, leg_tol, disturb,
    accept_capped, goal_tol, update_flags, log_stages); base: the launch's settings dict(opts, max_iter, rt_tol, rt_row_cap, level_rule).
    -> (result, arrays, tables, queues)"""
    base = dict(base or {})
    A, Tb, R = copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy()
    r = rollout(N, S, H, Tb, A, ticks, nw=nw, entry=5, tune=tune, wave_order=wave_order, lane_order=lane_order, replan=R, **base, **kw)
    assert r["ran"] == 5
    B = Tab.shape[0]
    per = lambda v, b: None if v is None else np.ascontiguousarray(np.asarray(v)[b:b + 1])
    for b in (range(B) if rows is None else rows):
        if rows is None and r["tune_info"][b]:
            continue
        s = settings(r["tune_used"][b], N, base.get("opts"))
        Ab, Tl, Rl = {k: A0[k][b:b + 1].copy() for k in A0}, Tab[b:b + 1].copy(), None if recs is None else recs[b:b + 1].copy()
        one_kw = {k: (v if k in ("accept_capped", "goal_tol", "update_flags", "log_stages") else v[:, b:b + 1] if k == "disturb" else per(v, b)) for k, v in kw.items()}
        one_kw["disturb"] = None if kw.get("disturb") is None else np.ascontiguousarray(kw["disturb"][:, b:b + 1])
        one = rollout(N, S, H, Tl, Ab, ticks, nw=nw, entry=4, wave_order=wave_order, lane_order=lane_order, replan=Rl, want_done=recs is not None, want_fired=recs is not None,
                      **s, **one_kw)
        assert_arrays_equal({k: Ab[k][0] for k in Ab}, unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl[0], Tb[b], equal_nan=True), f"{what}, stream {b}: path table"
        assert recs is None or np.array_equal(Rl[0], R[b], equal_nan=True), f"{what}, stream {b}: queue"
        assert_streams_equal(stream_of(r, b), stream_of(one, 0), f"{what}, stream {b}")
    return r, A, Tb, R


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A=None, ticks=1, levels=None, ss=None, rb=None, rec=None, replan_tick=-1, recs=None, leg_tick=None, leg_on=None, leg_tol=None, tune=None,
               plant=None, plant_state=None, disturb=None, update_flags=3, flags=1, goal_tol=0.0, max_iter=0, tick0_cap=0):
    """the case file of the stand-alone program (bmpc_emu_rollout.cpp with BMPC_EMU_ROLLOUT_MAIN): a header with the mask of the sections, then the sections.
    A batch behind its tick 0 (T [B][cap][48], A: its tick arrays; disturbances of zero unless given; levels: the entry of the highest section unless
    given) with a queue `recs` [B][K][len], leg_tick, leg_on and leg_tol, a settings table, a plant table and state; or one stream from the cold start
    (T [cap][48], ss, rb; levels: the levels to run) with the scheduled record `rec` [len] due behind replan_tick."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    batch = A is not None
    B = T.shape[0] if batch else 1
    if batch and disturb is None:
        disturb = np.zeros((ticks, B, bstream.DIST_LEN))
    if levels is None:
        levels = (6 if plant is not None else 5 if tune is not None else 4,)
    given = lambda *a: all(v is not None for v in a)
    sections = [(1, [A[k] for k in ("p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] if batch else None), (2, rec), (4, recs), (4, leg_tick), (4, leg_on),
                (8, leg_tol), (16, tune), (32, plant), (32, plant_state), (64, disturb)]
    assert given(recs) == given(leg_tick) == given(leg_on) and given(plant) == given(plant_state) and not (given(rec) and given(recs))
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[-2], flags, goal_tol, max_iter, update_flags, sum({bit for bit, a in sections if a is not None}), sum(1 << l for l in levels),
                  tick0_cap, replan_tick, 0 if recs is None else recs.shape[1]], dtype=np.float64).tofile(f)
        for a in [T, A["ss"] if batch else ss, A["rb"] if batch else rb] + [a for _, a in sections if a is not None]:
            for v in (a if isinstance(a, list) else [a]):
                np.ascontiguousarray(v, dtype=np.float64).tofile(f)


# (N, S, ticks, max_iter, goal_tol), tick 0 solved out by the tick text first: a converged loop, the reference's shape capped at two iterations (runs into
# the lost-plan stop, NaN rows behind it), converged, a goal that is reached inside the ticks, the smallest horizon
PLAIN_CASES = ((2, 2, 6, 0, 0.0), (10, 4, 13, 2, 0.0), (10, 4, 3, 0, 0.0), (2, 2, 6, 0, 6.9242), (1, 2, 4, 0, 0.0))
# (N, S, ticks, max_iter, replan_tick, update_flags, levels) from the cold start, each with disturbances on ticks 1 and 4: a re-plan with splice and the
# poor-bounds rule, the smallest horizon with a re-plan behind the last tick, one iteration per tick (a re-plan, then the lost-plan stop), a record never
# consumed (events alone), the reference's shape
EVENT_CASES = ((2, 2, 6, 0, 2, 7, (1, 2, 3)), (1, 2, 6, 0, 5, 3, (1, 2, 3)), (2, 2, 6, 1, 1, 3, (1, 2, 3)), (2, 2, 4, 0, -1, 3, (1,)), (10, 4, 3, 0, 1, 3, (1, 2, 3)))


def plain_cases(nw=1, only=None):
    """The cases of one stream, levels 0 to 3, as [(what, the arguments of write_case)].  nw = 1: PLAIN_CASES on the plain text, then EVENT_CASES on the
    texts with events, with events and audit and with the log on top (twice: rows of all N stages with the record, then the record alone).  nw = 4:
    PLAIN_CASES on the plain and on the fully-featured kernel under wave orders 0 and 1.  only: the levels to run (a case none of whose levels is among
    them is left out): the test suite runs nw = 1 with only=(3,) and nw = 4 whole, so levels 0 to 2 on one wave run under the sanitizers by hand only
    (--sanitize), as they always did."""
    cases = []
    for plain, ev in [(c, None) for c in PLAIN_CASES] + ([(None, c) for c in EVENT_CASES] if nw == 1 else []):
        levels = [l for l in (ev[6] if ev else (0,) if nw == 1 else (0, 3)) if only is None or l in only]
        if not levels:
            continue
        if plain:
            N, S, ticks, max_iter, goal_tol = plain
            _, rb, T, ss = small_stream(N, S)
            cases.append((f"N {N} S {S} ticks {ticks} max_iter {max_iter}",
                          dict(N=N, S=S, h=H, T=T, ss=ss, rb=rb, ticks=ticks, levels=levels, max_iter=max_iter, goal_tol=goal_tol, tick0_cap=100, update_flags=0)))
        else:
            N, S, ticks, max_iter, rtick, uflags, _ = ev
            mpc, rb, T, ss = small_stream(N, S)
            record = bstream.replan_record(S, T.shape[0], *leg_back(mpc, rb, T, S))
            cases.append((f"N {N} S {S} ticks {ticks} max_iter {max_iter} replan_tick {rtick} update_flags {uflags}",
                          dict(N=N, S=S, h=H, T=T, ss=ss, rb=rb, ticks=ticks, levels=levels, rec=record, disturb=disturbances(ticks, 1)[:, 0], replan_tick=rtick,
                               update_flags=uflags, max_iter=max_iter)))
    return cases


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout.cpp with its own main (and bmpc_emu.cpp, both with BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on
    exact-size buffers, a child process per case.  cases: [(what, dict of write_case's arguments after the path)].  The runs of a case must agree.
    Returns the program's output, a line per case; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_san{nw}")
        cc = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
              "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_ROLLOUT_MAIN"]
        objs = [os.path.join(tmp, name + ".o") for name in ("bmpc_emu_rollout", "bmpc_emu")]      # the two sources side by side
        compiles = [subprocess.Popen(cc + ["-c", "-o", o, os.path.join(here, os.path.basename(o)[:-2] + ".cpp")]) for o in objs]
        if any([p.wait() for p in compiles]):
            raise RuntimeError(f"sanitized rollout, nw {nw}: the build failed")
        subprocess.check_call(["g++", "-fsanitize=address,undefined", "-o", exe] + objs)
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_legs, test_stream_rollout_tune, test_stream_rollout_plant
        nw = 4 if "4" in sys.argv else 1
        cases = plain_cases(nw) + [c for m in (test_stream_rollout_legs, test_stream_rollout_tune, test_stream_rollout_plant) for c in m.sanitizer_cases(nw)]
        print("\n".join(run_sanitized(cases, nw)))
