"""TEST-ONLY: the CPU build of the rollout (boundmpc_amd/csrc/bmpc_rollout_kernel.inl through tests/emu/bmpc_emu_rollout.cpp) and what the CPU and
the GPU tests of the rollout and of the fused tick share: the per-tick loop of the fused tick's own kernel text (emu.stream_tick) that is the
rollout's exact checker, and the small streams.

  python -m tests.emu.emu_rollout --sanitize    builds bmpc_emu_rollout.cpp (with bmpc_emu.cpp beside it: tick 0 of every case runs the fused tick's
                                                text) as a stand-alone program with -fsanitize=address,undefined and runs it
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream, workload
from tests.closed_loop import stream_arrays
from tests.emu import emu

TICK_ARRAYS = ("ss", "rb", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")
ROLL = bstream.ROLL


def lib():
    L = emu._build("libbmpc_emu_rollout.so", "bmpc_emu_rollout.cpp", (), ("bmpc_stream.inl", "bmpc_rollout_kernel.inl"))
    assert L.bmpc_emu_stream_rollout_len() == bstream.rollout_len()
    return L


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


def rollout(N, S, h, T, A, ticks, max_iter=0, warm_dual=True, accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0,
            level_rule=(0.0, 0.0, 0.0), lane_order=0, want_rc=False):
    """The CPU build of the rollout text on the tick arrays `A` of one stream (advanced in place) -> dict(hist [ticks][52], traj_hist, ticks_run),
    or the return code with want_rc."""
    T = np.ascontiguousarray(T, dtype=np.float64)
    n = max(int(ticks), 0)
    hist, th, run = np.zeros((n, ROLL["LEN"])), np.zeros((n, A["traj"].shape[0])), np.full(1, -1, dtype=np.int32)
    c = ctypes
    rc = lib().bmpc_emu_stream_rollout(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(int(ticks)), emu._p(T), c.c_int(T.shape[0]),
                                       emu._p(A["ss"]), emu._p(A["rb"]), emu._p(A["p"]), emu._p(A["x0"]), emu._p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                       emu._p(A["x"]), emu._p(A["g"]), emu._p(A["iters"]), emu._p(A["status"]), emu._p(A["kkt"]), emu._p(A["traj"]),
                                       c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)), c.c_double(goal_tol), emu._p(hist), emu._p(th), emu._p(run),
                                       c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]),
                                       c.c_int(lane_order))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=int(run[0]))


def tick(N, S, h, T, A, **kw):
    """ONE fused tick -- the kernel entry text, emu.stream_tick -- on the tick arrays `A` (advanced in place).  Returns the history row the rollout would
    write behind this tick (None for a stream that has lost its plan, which the tick skips)."""
    lost = A["ss"][bstream.SS["ERRCNT"]] >= N
    emu.stream_tick(N, S, h, T, A, **kw)
    return None if lost else history_row(A)


def history_row(A):
    """what `hist` holds behind a tick, from the tick arrays of one stream"""
    return np.concatenate([A["rb"], [A["ss"][bstream.SS["PHI"]], A["ss"][bstream.SS["ERRCNT"]], float(A["iters"][0]), float(A["status"][0]), float(A["kkt"][0])], A["traj"][-4:]])


def per_tick_loop(N, S, h, T, A, ticks, **kw):
    """`ticks` fused ticks, one after the other -> (rows [ticks][52] with NaN rows for skipped ticks, traj rows, snapshots of the arrays behind every tick)"""
    rows, trajs, snaps = [], [], []
    for _ in range(ticks):
        row = tick(N, S, h, T, A, **kw)
        rows.append(row if row is not None else np.full(ROLL["LEN"], np.nan))
        trajs.append(A["traj"].copy() if row is not None else np.full(A["traj"].shape[0], np.nan))
        snaps.append(copy_arrays(A))
    return np.array(rows), np.array(trajs), snaps


def assert_arrays_equal(A, B, what=""):
    for k in TICK_ARRAYS:
        assert np.array_equal(A[k], B[k], equal_nan=True), f"{what}: {k} differs (largest deviation {np.nanmax(np.abs(A[k].astype(float) - B[k].astype(float)))})"


def write_case(path, N, S, h, T, ss, rb, ticks, flags=1, goal_tol=0.0, max_iter=0, tick0_cap=100):
    """the case file of the stand-alone program (bmpc_emu_rollout.cpp with BMPC_EMU_ROLLOUT_MAIN)"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    with open(path, "wb") as f:
        np.array([N, S, h, ticks, T.shape[0], flags, goal_tol, max_iter, tick0_cap], dtype=np.float64).tofile(f)
        T.tofile(f); np.asarray(ss, dtype=np.float64).tofile(f); np.asarray(rb, dtype=np.float64).tofile(f)


def run_sanitized(cases=((2, 2, 6, 0, 0.0), (10, 4, 13, 2, 0.0), (10, 4, 3, 0, 0.0), (2, 2, 6, 0, 6.9242), (1, 2, 4, 0, 0.0)), keep=None):
    """bmpc_emu_rollout.cpp with its own main (and bmpc_emu.cpp for the tick text of tick 0) under AddressSanitizer and UndefinedBehaviorSanitizer, on (N, S, ticks, max_iter, goal_tol) cases:
    a converged loop, the reference's shape capped at two iterations (runs into the lost-plan stop, NaN rows behind it), converged, a goal that is
    reached inside the ticks, the smallest horizon.  Returns the program's output lines; raises when the build fails, a run returns non-zero or a
    sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_rollout_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", "-DBMPC_EMU_ROLLOUT_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout.cpp"), os.path.join(here, "bmpc_emu.cpp")])
        for i, (N, S, ticks, max_iter, goal_tol) in enumerate(cases):
            _, rec, T, ss = small_stream(N, S)
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, N, S, 0.1, T, ss, rec, ticks, max_iter=max_iter, goal_tol=goal_tol)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} ticks {ticks} max_iter {max_iter}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized rollout, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
