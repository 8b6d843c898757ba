"""TEST-ONLY: the CPU build of the rollout with the log (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with EV, AU and LG, through
tests/emu/bmpc_emu_rollout_log.cpp) and its exact checker: the per-tick loop {fused tick text, log text cut to the stages, disturb text, update text of
the record due}.

  python -m tests.emu.emu_rollout_log --sanitize    builds bmpc_emu_rollout_log.cpp as a stand-alone program with -fsanitize=address,undefined
                                                    and runs it
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_events as ee, emu_stream_log as el

ROLL, SS, TUBE, AUDIT, TRACK = bstream.ROLL, bstream.SS, bstream.TUBE, bstream.AUDIT, bstream.TRACK


def lib():
    L = emu._build("libbmpc_emu_rollout_log.so", "bmpc_emu_rollout_log.cpp", (),
                   ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl", "bmpc_stream_tube.inl", "bmpc_stream_log.inl"))
    assert L.bmpc_emu_stream_track_len() == bstream.track_len()
    return L


def rollout_log_len(N, stages):
    return lib().bmpc_emu_stream_rollout_log_len(ctypes.c_int(N), ctypes.c_int(int(stages)))


def rollout_log(N, S, h, T, A, ticks, replan=None, replan_tick=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True,
                goal_tol=0.0, opts=None, rt_tol=1e-4, lane_order=0, want_rc=False, audit=True, want_tube=True, audit_tol=1e-6, want_log=True, log_stages=1, track=True):
    """The CPU build of the rollout with events, audit and log on the tick arrays `A` of B streams (advanced in place), the path tables T [B][cap][48] and
    the records `replan` [B][len] (both written in place where a record is consumed), one workgroup striding over the streams ->
    dict(hist, traj_hist, ticks_run, replan_info, tube_hist, audit, log_hist [ticks][B][88 log_stages + 4], track [B][12], ran), or the return code with
    want_rc.  An array switched off is NULL; `ran`: the instantiation that ran (3 with the log code, 2 events and audit, 1 events)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run, info = np.full(B, -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
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
    ran = c.c_int(-1)
    rc = lib().bmpc_emu_stream_rollout_log(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), emu._p(T), c.c_int(T.shape[1]),
                                           emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["p"]), emu._p(A["x0"]), emu._p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                           emu._p(A["x"]), emu._p(A["g"]), emu._p(A["iters"]), emu._p(A["status"]), emu._p(A["kkt"]), emu._p(A["traj"]),
                                           c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(goal_tol), emu._p(hist), emu._p(th), emu._p(run),
                                           emu._p(replan), emu._p(rt), emu._p(info), c.c_int(int(update_flags)), emu._p(dz), emu._p(tube), emu._p(aud), c.c_double(audit_tol),
                                           emu._p(log), c.c_int(int(log_stages)), emu._p(trk), c.c_double(rt_tol), c.c_double(0.0), c.c_double(0.0), c.c_double(0.0),
                                           c.c_double(0.0), c.c_int(lane_order), c.byref(ran))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk, ran=ran.value)


def cut(row, N, stages):
    """a whole log row (bmpc_stream_log) cut to its first `stages` stages: the body's prefix and the trailer"""
    row = np.asarray(row)
    assert row.shape[-1] == bstream.log_len(N)
    return np.concatenate([row[..., :stages * bstream.LOG_STAGE], row[..., -4:]], axis=-1)


def per_tick_log_rows(N, S, h, T, A, ticks, stages, replan=None, replan_tick=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], record `replan` [len]; all advanced in place): per tick the fused tick's text,
    the log text (tests/emu/emu_stream_log.py) on what the tick left, cut to `stages`, then the disturb text on row `disturb[t]`, then the splice + update
    text when replan_tick == t; the rollout's stop rules.  -> (log rows [ticks][88 stages + 4], history rows [ticks][52]), NaN for the ticks not run"""
    rows, hist = np.full((ticks, bstream.rollout_log_len(stages)), np.nan), np.full((ticks, ROLL["LEN"]), np.nan)
    for t in range(ticks):
        row = er.tick(N, S, h, T, A, **kw)
        if row is None:                                           # lost its plan: the stream stops
            break
        hist[t] = row
        rows[t] = cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        if disturb is not None:
            A["rb"][:] = ee.stream_disturb(A["rb"], disturb[t])
        if replan is not None and replan_tick == t:
            _, rec, Tn, ss, rb = ee.stream_update_flags(N, S, h, replan, T, A["ss"], A["rb"], update_flags)
            replan[:], T[:], A["ss"][:], A["rb"][:] = rec, Tn, ss, rb
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return rows, hist


def run_sanitized(cases=((2, 2, 6, 0, 2, 7), (1, 2, 6, 0, 5, 3), (2, 2, 6, 1, 1, 3), (10, 4, 3, 0, 1, 3)), keep=None):
    """bmpc_emu_rollout_log.cpp with its own main under AddressSanitizer and UndefinedBehaviorSanitizer on the cases of the rollout with the audit
    ((N, S, ticks, max_iter, replan_tick, update_flags), disturbances on ticks 1 and 4), exact-size log and track buffers: rows of all N stages with the
    record, then the record alone.  Returns the program's output lines; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_rollout_log_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", "-DBMPC_EMU_ROLLOUT_LOG_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_log.cpp")])
        for i, (N, S, ticks, max_iter, rtick, uflags) in enumerate(cases):
            mpc, rec, T, ss = er.small_stream(N, S)
            record = bstream.replan_record(S, T.shape[0], *ee.leg_back(mpc, rec, T, S))
            case = os.path.join(tmp, f"case{i}.bin")
            ee.write_case(case, N, S, ee.H, T, ss, rec, ticks, record, ee.disturbances(ticks, 1)[:, 0], rtick, uflags, max_iter=max_iter)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} ticks {ticks} max_iter {max_iter} replan_tick {rtick} update_flags {uflags}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout with log, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
