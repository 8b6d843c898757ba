"""TEST-ONLY: the CPU build of the TEAM rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with BMPC_NW = 4 waves per stream, namespace bmpct, through
tests/emu/bmpc_emu_team_rollout.cpp: the plain instantiation and the one with events, audit and log, as boundmpc_amd/csrc/bmpc_team_rollout.hip holds
them) and its exact checker: the per-tick loop {team tick text (emu.stream_tick(nw=4)), tube text, log text, disturb text, update text of the record
due}, assembled from the existing emulator functions.

  python -m tests.emu.emu_team_rollout --sanitize    builds bmpc_emu_team_rollout.cpp (with bmpc_emu.cpp as the team's beside it: tick 0 of every case
                                                     runs the team tick's text) as a stand-alone program with -fsanitize=address,undefined and runs it
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_events as ee, emu_rollout_log as elg, emu_stream_log as el, emu_stream_tube as et

NW = 4
ROLL, SS, TUBE, AUDIT, TRACK = bstream.ROLL, bstream.SS, bstream.TUBE, bstream.AUDIT, bstream.TRACK


def lib():
    L = emu._build("libbmpc_emu_team_rollout.so", "bmpc_emu_team_rollout.cpp", (f"-DBMPC_NW={NW}",),
                   ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl", "bmpc_stream_tube.inl", "bmpc_stream_log.inl"))
    assert L.bmpc_emu_team_rollout_waves() == NW and L.bmpc_emu_team_rollout_len() == bstream.rollout_len()
    return L


def rollout(N, S, h, T, A, ticks, full=False, replan=None, replan_tick=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True,
            goal_tol=0.0, opts=None, rt_tol=1e-4, lane_order=0, wave_order=0, want_rc=False, audit=False, want_tube=False, audit_tol=1e-6, want_log=False, log_stages=1,
            track=False):
    """The CPU build of the team rollout on the tick arrays `A` of B streams (ee.stack; advanced in place), the path tables T [B][cap][48] and the records
    `replan` [B][len] (both written in place where a record is consumed), one workgroup striding over the streams, the waves of a wide phase in
    `wave_order` -> dict(hist [ticks][B][52], traj_hist, ticks_run [B], replan_info, tube_hist, audit, log_hist, track), or the return code with want_rc.
    full=False: the plain kernel (no event, audit or log array may be given); True: the kernel with EV, AU and LG, arrays switched off are NULL."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    info = np.full(B, -7, dtype=np.int32) if full else None
    tube = np.full((n, B, TUBE["LEN"]), 7.0) if want_tube else None
    aud = np.full((B, AUDIT["LEN"]), 7.0) if audit else None
    log = np.full((n, B, bstream.LOG_STAGE * max(int(log_stages), 0) + 4), 7.0) if want_log else None
    trk = np.full((B, TRACK["LEN"]), 7.0) if track else None
    if replan is not None:
        assert replan.flags.c_contiguous and replan.shape == (B, bstream.replan_len(S, T.shape[1]))
    rt = None if replan_tick is None else np.ascontiguousarray(replan_tick, dtype=np.int32)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    c = ctypes
    rc = lib().bmpc_emu_team_stream_rollout(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), emu._p(T), c.c_int(T.shape[1]),
                                            emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["p"]), emu._p(A["x0"]), emu._p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                            emu._p(A["x"]), emu._p(A["g"]), emu._p(A["iters"]), emu._p(A["status"]), emu._p(A["kkt"]), emu._p(A["traj"]),
                                            c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(goal_tol), emu._p(hist), emu._p(th), emu._p(run),
                                            emu._p(replan), emu._p(rt), emu._p(info), c.c_int(int(update_flags)), emu._p(dz), emu._p(tube), emu._p(aud), c.c_double(audit_tol),
                                            emu._p(log), c.c_int(int(log_stages)), emu._p(trk), c.c_double(rt_tol), c.c_double(0.0), c.c_double(0.0), c.c_double(0.0),
                                            c.c_double(0.0), c.c_int(lane_order), c.c_int(wave_order), c.c_int(int(bool(full))))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk)


def per_tick_loop(N, S, h, T, A, ticks, stages=1, replan=None, replan_tick=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], record `replan` [len]; all advanced in place): per tick the TEAM tick's text,
    the tube text on the p that tick packed, the log text on what the tick left, cut to `stages`, then the disturb text on row `disturb[t]`, then the
    splice + update text when replan_tick == t; the rollout's stop rules.
    -> dict(hist [ticks][52], traj_hist, tube_hist [ticks][16], log_hist [ticks][88 stages + 4], ticks_run, replan_info), NaN for the ticks not run"""
    hist, trajs = np.full((ticks, ROLL["LEN"]), np.nan), np.full((ticks, A["traj"].shape[0]), np.nan)
    tube, log = np.full((ticks, TUBE["LEN"]), np.nan), np.full((ticks, bstream.rollout_log_len(stages)), np.nan)
    run, info = 0, -1
    for t in range(ticks):
        row = er.tick(N, S, h, T, A, nw=NW, **kw)
        if row is None:                                           # lost its plan: the tick wrote status 3 and the stream stops
            break
        hist[t], trajs[t], run = row, A["traj"], t + 1
        tube[t] = et.stream_tube(N, S, A["p"])[0]
        log[t] = elg.cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        if disturb is not None:
            A["rb"][:] = ee.stream_disturb(A["rb"], disturb[t])
        if replan is not None and replan_tick == t:
            info, rec, Tn, ss, rb = ee.stream_update_flags(N, S, h, replan, T, A["ss"], A["rb"], update_flags)
            replan[:], T[:], A["ss"][:], A["rb"][:] = rec, Tn, ss, rb
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return dict(hist=hist, traj_hist=trajs, tube_hist=tube, log_hist=log, ticks_run=run, replan_info=info)


def run_sanitized(cases=((2, 2, 6, 0, 0.0), (10, 4, 13, 2, 0.0), (10, 4, 3, 0, 0.0), (2, 2, 6, 0, 6.9242), (1, 2, 4, 0, 0.0)), keep=None):
    """bmpc_emu_team_rollout.cpp with its own main (and bmpc_emu.cpp as the team's for the tick text of tick 0) under AddressSanitizer and
    UndefinedBehaviorSanitizer on the (N, S, ticks, max_iter, goal_tol) cases of emu_rollout.run_sanitized, exact-size heap buffers: per case the plain
    and the fully-featured kernel under wave orders 0 and 1, which must agree.  Returns the program's output lines; raises when the build fails, a run
    returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_team_rollout_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={NW}", "-DBMPC_EMU_TEAM_ROLLOUT_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_team_rollout.cpp"),
                               os.path.join(here, "bmpc_emu.cpp")])
        for i, (N, S, ticks, max_iter, goal_tol) in enumerate(cases):
            _, rec, T, ss = er.small_stream(N, S)
            case = os.path.join(tmp, f"case{i}.bin")
            er.write_case(case, N, S, 0.1, T, ss, rec, ticks, max_iter=max_iter, goal_tol=goal_tol)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} ticks {ticks} max_iter {max_iter}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized team rollout, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
