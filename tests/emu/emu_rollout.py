"""TEST-ONLY: the CPU build of the rollout in all its variants (boundmpc_amd/csrc/bmpc_rollout_kernel.inl through tests/emu/bmpc_emu_rollout.cpp, built once
for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the rollouts share: the contract's loop {fused tick's own kernel
text, tube text, log text, disturb text, splice + update text of the record due, stop rules} that is the exact checker of every variant, the small
streams and batches, their new paths and disturbances.

  python -m tests.emu.emu_rollout --sanitize [4]    builds bmpc_emu_rollout.cpp (with bmpc_emu.cpp beside it: tick 0 of the cases without events runs the
                                                    fused tick's text) as a stand-alone program with -fsanitize=address,undefined and runs it
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
H = 0.1
_DEPS = ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl", "bmpc_stream_tube.inl", "bmpc_stream_log.inl")


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout.so" if nw == 1 else f"libbmpc_emu_rollout_team{nw}.so", "bmpc_emu_rollout.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_rollout_waves() == nw and L.bmpc_emu_stream_rollout_len() == bstream.rollout_len() and L.bmpc_emu_stream_track_len() == bstream.track_len()
    return L


def rollout_log_len(N, stages):
    return lib().bmpc_emu_stream_rollout_log_len(ctypes.c_int(N), ctypes.c_int(int(stages)))


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


@functools.lru_cache(maxsize=None)
def start(N, S, nw=1):
    """small_batch(N, S) with tick 0 of every stream solved out (nw = 4: by the team tick): (tick arrays, path tables, re-plan records); copy before use"""
    _, A0, Tab, recs = small_batch(N, S)
    for b in range(A0["ss"].shape[0]):
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


# ---- the rollout text ----
def rollout(N, S, h, T, A, ticks, nw=1, entry=0, level=None, replan=None, replan_tick=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False,
            simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0), lane_order=0, wave_order=0, want_rc=False, audit=None,
            want_tube=None, audit_tol=1e-6, want_log=None, log_stages=1, track=None):
    """The CPU build of the rollout text (nw = 1: one wave per stream; 4: teams, the waves of a wide phase in `wave_order`) on the tick arrays `A` of B
    streams (fresh_arrays stacked; advanced in place), the path tables T [B][cap][48] and the records `replan` [B][len] (both written in place where a
    record is consumed), one workgroup striding over the streams.  entry: the C ABI entry the call stands for -- 0 bmpc_stream_rollout, 1 _events, 2 _audit,
    3 _log; the output arrays of an entry are on unless switched off (audit, want_tube: entry >= 2; want_log, track: entry 3), an array switched off is NULL,
    and one the entry has no argument for is refused.  level: None = the instantiation the library's rule picks, else that one on the same arguments.
    -> dict(hist [ticks][B][52], traj_hist, ticks_run [B], replan_info [B], tube_hist [ticks][B][16], audit [B][12], log_hist [ticks][B][88 log_stages + 4],
    track [B][12], ran: the level that ran), or the return code with want_rc (1: what the C ABI refuses).  One stream (T [cap][48], A of fresh_arrays):
    the same without the axis B, ticks_run an int."""
    T = np.ascontiguousarray(T, dtype=np.float64) if T.ndim == 2 else T
    one = T.ndim == 2
    if one:
        assert all(v.flags.c_contiguous for v in A.values())
        T, A = T[None], {k: v[None] for k, v in A.items()}      # (views: the caller's arrays advance)
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    on = lambda want, first: entry >= first if want is None else bool(want)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    info = np.full(B, -7, dtype=np.int32) if entry >= 1 else None
    tube = np.full((n, B, TUBE["LEN"]), 7.0) if on(want_tube, 2) else None
    aud = np.full((B, AUDIT["LEN"]), 7.0) if on(audit, 2) else None
    log = np.full((n, B, bstream.LOG_STAGE * max(int(log_stages), 0) + 4), 7.0) if on(want_log, 3) else None
    trk = np.full((B, TRACK["LEN"]), 7.0) if on(track, 3) else None
    if replan is not None:
        assert replan.flags.c_contiguous and replan.shape == (B, bstream.replan_len(S, T.shape[1]))
    rt = None if replan_tick is None else np.ascontiguousarray(replan_tick, dtype=np.int32)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    c, p = ctypes, emu._p
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), p(T), c.c_int(T.shape[1]),
                                         p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), p(A["x"]), p(A["g"]),
                                         p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                         c.c_double(goal_tol), p(hist), p(th), p(run), p(replan), p(rt), p(info), c.c_int(int(update_flags)), p(dz), p(tube), p(aud),
                                         c.c_double(audit_tol), p(log), c.c_int(int(log_stages)), p(trk), c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]),
                                         c.c_double(level_rule[1]), c.c_double(level_rule[2]), c.c_int(lane_order), c.c_int(wave_order), c.c_int(int(entry)),
                                         c.c_int(-1 if level is None else int(level)), c.byref(ran))
    if want_rc:
        return rc
    assert rc == 0
    r = dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk)
    if one:
        r = {k: None if v is None else (int(v[0]) if k == "ticks_run" else v[0] if v.ndim < 3 else v[:, 0]) for k, v in r.items()}
    r["ran"] = ran.value
    return r


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


def contract_loop(N, S, h, T, A, ticks, stages=1, replan=None, replan_tick=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], record `replan` [len]; all advanced in place): per tick the fused tick's text
    (kw: the arguments of emu.stream_tick; nw=4: the team tick's), the tube text on the p that tick packed, the log text on what the tick left, cut to
    `stages`, then -- for a stream that still runs -- the disturb text on row `disturb[t]`, then the splice + update text when replan_tick == t.  The
    rollout's stop rules decide what "still runs" means: a tick the stream lost its plan ahead of is not run (it writes the three words of a skipped
    stream), nor anything behind it; with goal_tol > 0 nothing runs behind the tick that leaves phi_max - phi <= goal_tol AFTER its events.
    -> dict(hist [ticks][52], traj_hist, tube_hist [ticks][16], p_hist: the p of every tick, log_hist [ticks][88 stages + 4], ticks_run, replan_info,
    snaps: copies of the arrays behind every tick, run or not), NaN rows for the ticks not run"""
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan), ticks_run=0, replan_info=-1, snaps=[])
    for t in range(ticks):
        row = tick(N, S, h, T, A, **kw)
        if row is None:                                           # lost its plan: the tick wrote status 3 and the stream stops
            break
        r["hist"][t], r["traj_hist"][t], r["p_hist"][t], r["ticks_run"] = row, A["traj"], A["p"], t + 1
        r["tube_hist"][t] = et.stream_tube(N, S, A["p"])[0]
        r["log_hist"][t] = cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        if disturb is not None:
            A["rb"][:] = eup.stream_disturb(A["rb"], disturb[t])
        if replan is not None and replan_tick == t:
            r["replan_info"], rec, Tn, ss, rb = eup.stream_update_flags(N, S, h, replan, T, A["ss"], A["rb"], update_flags)
            replan[:], T[:], A["ss"][:], A["rb"][:] = rec, Tn, ss, rb
        r["snaps"].append(copy_arrays(A))
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    r["snaps"] += [copy_arrays(A)] * (ticks - len(r["snaps"]))
    return r


def assert_arrays_equal(A, B, what=""):
    for k in TICK_ARRAYS:
        assert np.array_equal(A[k], B[k], equal_nan=True), f"{what}: {k} differs (largest deviation {np.nanmax(np.abs(A[k].astype(float) - B[k].astype(float)))})"


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, ss, rb, ticks, levels, rec=None, dist=None, replan_tick=-1, update_flags=0, flags=1, goal_tol=0.0, max_iter=0, tick0_cap=0):
    """the case file of the stand-alone program (bmpc_emu_rollout.cpp with BMPC_EMU_ROLLOUT_MAIN); levels: the levels to run; rec, dist: the record and
    the disturbances of the one stream, both or neither"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    mask = sum(1 << l for l in levels) | (16 if rec is not None else 0)
    with open(path, "wb") as f:
        np.array([N, S, h, ticks, T.shape[0], flags, goal_tol, max_iter, tick0_cap, replan_tick, update_flags, mask], dtype=np.float64).tofile(f)
        for a in (T, ss, rb) + ((rec, dist) if rec is not None else ()):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


# (N, S, ticks, max_iter, goal_tol), tick 0 solved out by the tick text first: a converged loop, the reference's shape capped at two iterations (runs into
# the lost-plan stop, NaN rows behind it), converged, a goal that is reached inside the ticks, the smallest horizon
PLAIN_CASES = ((2, 2, 6, 0, 0.0), (10, 4, 13, 2, 0.0), (10, 4, 3, 0, 0.0), (2, 2, 6, 0, 6.9242), (1, 2, 4, 0, 0.0))
# (N, S, ticks, max_iter, replan_tick, update_flags, levels) from the cold start, each with disturbances on ticks 1 and 4: a re-plan with splice and the
# poor-bounds rule, the smallest horizon with a re-plan behind the last tick, one iteration per tick (a re-plan, then the lost-plan stop), a record never
# consumed (events alone), the reference's shape
EVENT_CASES = ((2, 2, 6, 0, 2, 7, (1, 2, 3)), (1, 2, 6, 0, 5, 3, (1, 2, 3)), (2, 2, 6, 1, 1, 3, (1, 2, 3)), (2, 2, 4, 0, -1, 3, (1,)), (10, 4, 3, 0, 1, 3, (1, 2, 3)))


def run_sanitized(nw=1, only=None, keep=None):
    """bmpc_emu_rollout.cpp with its own main (and bmpc_emu.cpp, both with BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on
    exact-size buffers.  nw = 1: PLAIN_CASES on the plain text, then EVENT_CASES on the texts with events, with events and audit and with the log on top
    (twice: rows of all N stages with the record, then the record alone).  nw = 4: PLAIN_CASES on the plain and on the fully-featured kernel under wave
    orders 0 and 1.  The runs of a case must agree.  only: the levels to run (a case none of whose levels is among them is left out): the test suite
    runs nw = 1 with only=(3,) and nw = 4 whole, so levels 0 to 2 on one wave run under the sanitizers by hand only (--sanitize), as they always did.  Returns the program's output, a line per case; raises when the build fails, a run returns non-zero
    or a sanitizer reports."""
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
        cases = [(c, None) for c in PLAIN_CASES] + ([(None, c) for c in EVENT_CASES] if nw == 1 else [])
        for i, (plain, ev) in enumerate(cases):
            levels = [l for l in (ev[6] if ev else (0,) if nw == 1 else (0, 3)) if only is None or l in only]
            if not levels:
                continue
            case = os.path.join(tmp, f"case{i}.bin")
            if plain:
                N, S, ticks, max_iter, goal_tol = plain
                _, rec, T, ss = small_stream(N, S)
                write_case(case, N, S, H, T, ss, rec, ticks, levels, max_iter=max_iter, goal_tol=goal_tol, tick0_cap=100)
                what = f"N {N} S {S} ticks {ticks} max_iter {max_iter}"
            else:
                N, S, ticks, max_iter, rtick, uflags, _ = ev
                mpc, rec, T, ss = small_stream(N, S)
                record = bstream.replan_record(S, T.shape[0], *leg_back(mpc, rec, T, S))
                write_case(case, N, S, H, T, ss, rec, ticks, levels, record, disturbances(ticks, 1)[:, 0], rtick, uflags, max_iter=max_iter)
                what = f"N {N} S {S} ticks {ticks} max_iter {max_iter} replan_tick {rtick} update_flags {uflags}"
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout, nw {nw}, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized(4 if "4" in sys.argv else 1)))
