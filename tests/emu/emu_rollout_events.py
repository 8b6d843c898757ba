"""TEST-ONLY: the CPU build of the rollout with events (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with EV, through tests/emu/bmpc_emu_rollout_events.cpp) and
of the two event functions (csrc/bmpc_stream_events.inl), and what the CPU and the GPU tests of them share: the per-tick loop that is the exact
checker -- the fused tick's own kernel text, then the disturb text, then splice + update text at the scheduled tick --, the streams and their new paths.

  python -m tests.emu.emu_rollout_events --sanitize    builds bmpc_emu_rollout_events.cpp as a stand-alone program with -fsanitize=address,undefined
                                                       and runs it
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er

ROLL, SS, RB, RP, RV = bstream.ROLL, bstream.SS, bstream.RB, bstream.RP, bstream.RV
H = 0.1


def lib():
    L = emu._build("libbmpc_emu_rollout_events.so", "bmpc_emu_rollout_events.cpp", (),
                   ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl"))
    assert L.bmpc_emu_stream_disturb_len() == bstream.DIST_LEN
    return L


def stream_splice(h, S, rec, rb, poor_bounds=False, flags=None):
    """the CPU build of stream_splice on a copy of the record -> the record after it"""
    rec, rb = np.array(rec, dtype=np.float64, order="C"), np.array(rb, dtype=np.float64, order="C")
    cap = (rec.shape[0] - RP["HEAD"]) // RV["LEN"] + S - 1
    lib().bmpc_emu_stream_splice(ctypes.c_double(h), ctypes.c_int(S), ctypes.c_int(cap), emu._p(rec), emu._p(rb), ctypes.c_int(2 | (4 if poor_bounds else 0) if flags is None else flags))
    return rec


def stream_disturb(rb, d):
    """the CPU build of stream_disturb on a copy of the robot record -> the record after it"""
    rb, d = np.array(rb, dtype=np.float64, order="C"), np.array(d, dtype=np.float64, order="C")
    assert d.shape == (bstream.DIST_LEN,)
    lib().bmpc_emu_stream_disturb(emu._p(rb), emu._p(d))
    return rb


def stream_update_flags(N, S, h, rec, path, ss, rb, flags):
    """what bmpc_stream_update(flags) does with one stream, on copies -> (info, rec, path, ss, rb); info -2: the C ABI's BMPC_ERR_ARG"""
    rec, path, ss = (np.array(a, dtype=np.float64, order="C") for a in (rec, path, ss))
    rb = None if rb is None else np.array(rb, dtype=np.float64, order="C")
    info = lib().bmpc_emu_stream_update_flags(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), emu._p(rec), emu._p(path), ctypes.c_int(path.shape[0]), emu._p(ss), emu._p(rb),
                                              ctypes.c_int(int(flags)))
    return info, rec, path, ss, rb


def stack(arrays):
    """the tick arrays of B streams (er.fresh_arrays each) with a leading axis of B"""
    return {k: np.ascontiguousarray(np.stack([A[k] for A in arrays])) for k in arrays[0]}


def unstack(A, b):
    return {k: A[k][b].copy() for k in A}


def rollout_events(N, S, h, T, A, ticks, replan=None, replan_tick=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True,
                   goal_tol=0.0, opts=None, rt_tol=1e-4, lane_order=0, want_rc=False, events=True):
    """The CPU build of the rollout with events on the tick arrays `A` of B streams (er.fresh_arrays stacked; advanced in place), the path tables
    T [B][cap][48] and the records `replan` [B][len] (both written in place where a record is consumed), one workgroup striding over the streams ->
    dict(hist [ticks][B][52], traj_hist, ticks_run [B], replan_info [B]), or the return code with want_rc.  events=False: the instantiation without the
    event code on the same arguments."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run, info = np.full(B, -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    if replan is not None:
        assert replan.flags.c_contiguous and replan.shape == (B, bstream.replan_len(S, T.shape[1]))
    rt = None if replan_tick is None else np.ascontiguousarray(replan_tick, dtype=np.int32)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    c = ctypes
    rc = lib().bmpc_emu_stream_rollout_events(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), emu._p(T), c.c_int(T.shape[1]),
                                              emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["p"]), emu._p(A["x0"]), emu._p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                              emu._p(A["x"]), emu._p(A["g"]), emu._p(A["iters"]), emu._p(A["status"]), emu._p(A["kkt"]), emu._p(A["traj"]),
                                              c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(goal_tol), emu._p(hist), emu._p(th), emu._p(run),
                                              emu._p(replan), emu._p(rt), emu._p(info), c.c_int(int(update_flags)), emu._p(dz), c.c_double(rt_tol), c.c_double(0.0),
                                              c.c_double(0.0), c.c_double(0.0), c.c_double(0.0), c.c_int(lane_order), c.c_int(int(bool(events))))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info)


def per_tick_loop_events(N, S, h, T, A, ticks, replan=None, replan_tick=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], record `replan` [len]; all advanced in place): per tick the fused tick's text,
    then -- for a stream that still runs -- the disturb text on row `disturb[t]`, then the splice + update text when replan_tick == t.  The rollout's
    stop rules decide what "still runs" means: a tick the stream lost its plan ahead of is not run, nor anything behind it; with goal_tol > 0 nothing
    runs behind the tick that leaves phi_max - phi <= goal_tol AFTER its events.
    -> (rows [ticks][52], traj rows, ticks_run, replan_info)"""
    rows, trajs = np.full((ticks, ROLL["LEN"]), np.nan), np.full((ticks, A["traj"].shape[0]), np.nan)
    run, info = 0, -1
    for t in range(ticks):
        row = er.tick(N, S, h, T, A, **kw)
        if row is None:                                           # lost its plan: the tick wrote status 3 and the stream stops
            break
        rows[t], trajs[t], run = row, A["traj"], t + 1
        if disturb is not None:
            A["rb"][:] = stream_disturb(A["rb"], disturb[t])
        if replan is not None and replan_tick == t:
            info, rec, Tn, ss, rb = stream_update_flags(N, S, h, replan, T, A["ss"], A["rb"], update_flags)
            replan[:], T[:], A["ss"][:], A["rb"][:] = rec, Tn, ss, rb
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return rows, trajs, run, info


def leg_back(mpc, rec, T, S, tube=1.0, detour=0.0):
    """A new path for a stream of er.small_stream: from the pose the splice will write (via point 0: a placeholder here) to the via points of the
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
    """B small streams (er.small_stream with `which` = 0..B-1) -> (mpcs, stacked tick arrays, T [B][cap][48], records [B][len] of leg_back(**leg), flags raised)"""
    streams = [er.small_stream(N, S, which=b) for b in range(B)]
    cap = max(s[2].shape[0] for s in streams)
    assert all(s[2].shape[0] == cap for s in streams)
    A = stack([er.fresh_arrays(N, S, ss, rec) for _, rec, _, ss in streams])
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


def write_case(path, N, S, h, T, ss, rb, ticks, rec, dist, replan_tick, update_flags=3, flags=1, goal_tol=0.0, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_events.cpp with BMPC_EMU_ROLLOUT_EVENTS_MAIN)"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    with open(path, "wb") as f:
        np.array([N, S, h, ticks, T.shape[0], flags, goal_tol, max_iter, replan_tick, update_flags], dtype=np.float64).tofile(f)
        for a in (T, ss, rb, rec, dist):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases=((2, 2, 6, 0, 2, 7), (1, 2, 6, 0, 5, 3), (2, 2, 6, 1, 1, 3), (2, 2, 4, 0, -1, 3), (10, 4, 3, 0, 1, 3)), keep=None):
    """bmpc_emu_rollout_events.cpp with its own main under AddressSanitizer and UndefinedBehaviorSanitizer, on (N, S, ticks, max_iter, replan_tick,
    update_flags) cases, each with disturbances on ticks 1 and 4: a re-plan with splice and the poor-bounds rule, the smallest horizon with a re-plan
    behind the last tick, one iteration per tick from the cold start (a re-plan, then the lost-plan stop), a record never consumed, the reference's shape.
    Returns the program's output lines; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_rollout_events_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", "-DBMPC_EMU_ROLLOUT_EVENTS_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_events.cpp")])
        for i, (N, S, ticks, max_iter, rtick, uflags) in enumerate(cases):
            mpc, rec, T, ss = er.small_stream(N, S)
            record = bstream.replan_record(S, T.shape[0], *leg_back(mpc, rec, T, S))
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, N, S, H, T, ss, rec, ticks, record, disturbances(ticks, 1)[:, 0], rtick, uflags, max_iter=max_iter)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} ticks {ticks} max_iter {max_iter} replan_tick {rtick} update_flags {uflags}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout with events, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
