"""TEST-ONLY: the CPU build of the rollout with the audit (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with EV and AU, through
tests/emu/bmpc_emu_rollout_audit.cpp) and its exact checker: the per-tick loop {fused tick text, disturb text} with the tube text run on the p every
tick packed.

  python -m tests.emu.emu_rollout_audit --sanitize    builds bmpc_emu_rollout_audit.cpp as a stand-alone program with -fsanitize=address,undefined
                                                      and runs it
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_events as ee, emu_stream_tube as et

ROLL, SS, TUBE, AUDIT = bstream.ROLL, bstream.SS, bstream.TUBE, bstream.AUDIT


def lib():
    return emu._build("libbmpc_emu_rollout_audit.so", "bmpc_emu_rollout_audit.cpp", (),
                      ("bmpc_stream.inl", "bmpc_rollout_kernel.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl", "bmpc_stream_tube.inl"))


def rollout_audit(N, S, h, T, A, ticks, replan=None, replan_tick=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True,
                  goal_tol=0.0, opts=None, rt_tol=1e-4, lane_order=0, want_rc=False, audit=True, want_tube=True, audit_tol=1e-6):
    """The CPU build of the rollout with events and audit on the tick arrays `A` of B streams (advanced in place) and the path tables T [B][cap][48],
    one workgroup striding over the streams -> dict(hist, traj_hist, ticks_run, replan_info, tube_hist [ticks][B][16], audit [B][12]), or the return
    code with want_rc.  audit / want_tube False: that array is NULL (both: the instantiation without the audit code runs)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run, info = np.full(B, -7, dtype=np.int32), np.full(B, -7, dtype=np.int32)
    tube = np.full((n, B, TUBE["LEN"]), 7.0) if want_tube else None
    aud = np.full((B, AUDIT["LEN"]), 7.0) if audit else None
    rt = None if replan_tick is None else np.ascontiguousarray(replan_tick, dtype=np.int32)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    c = ctypes
    rc = lib().bmpc_emu_stream_rollout_audit(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), emu._p(T), c.c_int(T.shape[1]),
                                             emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["p"]), emu._p(A["x0"]), emu._p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                             emu._p(A["x"]), emu._p(A["g"]), emu._p(A["iters"]), emu._p(A["status"]), emu._p(A["kkt"]), emu._p(A["traj"]),
                                             c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(goal_tol), emu._p(hist), emu._p(th), emu._p(run),
                                             emu._p(replan), emu._p(rt), emu._p(info), c.c_int(int(update_flags)), emu._p(dz), emu._p(tube), emu._p(aud), c.c_double(audit_tol),
                                             c.c_double(rt_tol), c.c_double(0.0), c.c_double(0.0), c.c_double(0.0), c.c_double(0.0), c.c_int(lane_order))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud)


def per_tick_tube_rows(N, S, h, T, A, ticks, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48]; advanced in place): per tick the fused tick's text, the tube text on the p
    that tick packed, then the disturb text on row `disturb[t]`; the rollout's stop rules.  -> (tube rows [ticks][16], the p of every tick [ticks][n_p]), NaN for the ticks not run"""
    rows, ps = np.full((ticks, TUBE["LEN"]), np.nan), np.full((ticks, A["p"].shape[0]), np.nan)
    for t in range(ticks):
        if er.tick(N, S, h, T, A, **kw) is None:
            break
        rows[t], ps[t] = et.stream_tube(N, S, A["p"])[0], A["p"]
        if disturb is not None:
            A["rb"][:] = ee.stream_disturb(A["rb"], disturb[t])
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return rows, ps


def run_sanitized(cases=((2, 2, 6, 0, 2, 7), (1, 2, 6, 0, 5, 3), (2, 2, 6, 1, 1, 3), (10, 4, 3, 0, 1, 3)), keep=None):
    """bmpc_emu_rollout_audit.cpp with its own main under AddressSanitizer and UndefinedBehaviorSanitizer on the cases of the rollout with events
    ((N, S, ticks, max_iter, replan_tick, update_flags), disturbances on ticks 1 and 4), exact-size tube and audit buffers.  Returns the program's
    output lines; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_rollout_audit_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", "-DBMPC_EMU_ROLLOUT_AUDIT_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_audit.cpp")])
        for i, (N, S, ticks, max_iter, rtick, uflags) in enumerate(cases):
            mpc, rec, T, ss = er.small_stream(N, S)
            record = bstream.replan_record(S, T.shape[0], *ee.leg_back(mpc, rec, T, S))
            case = os.path.join(tmp, f"case{i}.bin")
            ee.write_case(case, N, S, ee.H, T, ss, rec, ticks, record, ee.disturbances(ticks, 1)[:, 0], rtick, uflags, max_iter=max_iter)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} ticks {ticks} max_iter {max_iter} replan_tick {rtick} update_flags {uflags}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout with audit, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
