"""TEST-ONLY: the CPU build of the rollout with a queue of re-plan records per stream (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with QU through
tests/emu/bmpc_emu_rollout_legs.cpp, built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the missions
share: the contract's loop for one stream, mission_loop -- {fused tick's own kernel text, tube text, log text, disturb text, splice + update text of the
head record when it is due, stop rules} --, the exact checker of the entry.  The streams, batches, paths and the texts are emu_rollout's.

  python -m tests.emu.emu_rollout_legs --sanitize [4]   builds bmpc_emu_rollout_legs.cpp as a stand-alone program with -fsanitize=address,undefined
                                                        and runs it on the cases of tests/test_stream_rollout_legs.py
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu
from tests.emu.emu_rollout import (H, ROLL, SS, TUBE, AUDIT, TRACK, TICK_ARRAYS, _DEPS, small_stream, small_batch, fresh_arrays, copy_arrays, stack, unstack, leg_back,      # noqa: F401
                                   disturbances, opts, start, tick, history_row, cut, assert_arrays_equal, assert_track, et, el, eup)

AT_GOAL, ON_LOST, WHY_GOAL, WHY_LOST, WHY_TICK = 1, 2, 1, 2, 4


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout_legs.so" if nw == 1 else f"libbmpc_emu_rollout_legs_team{nw}.so", "bmpc_emu_rollout_legs.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_rollout_legs_waves() == nw and L.bmpc_emu_leg_bits() == AT_GOAL | ON_LOST << 4 | WHY_GOAL << 8 | WHY_LOST << 12 | WHY_TICK << 16
    return L


def _i32(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.int32)
    assert a.shape == shape, f"{name} must be {shape}, got {a.shape}"
    return a


def rollout_legs(N, S, h, T, A, ticks, nw=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None, legs=None, want_done=True, want_fired=True, update_flags=3, disturb=None,
                 max_iter=0, warm_dual=True, accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0), lane_order=0,
                 wave_order=0, want_rc=False, audit=True, want_tube=True, audit_tol=1e-6, want_log=True, log_stages=1, track=True):
    """The CPU build of bmpc_stream_rollout_legs (nw = 1: one wave per stream; 4: teams, the waves of a wide phase in `wave_order`) on the tick arrays `A` of B
    streams (advanced in place), the path tables T [B][cap][48] and the queues `replan` [B][K][len] (both written in place where a record is consumed);
    leg_tick, leg_on [B][K] int, leg_tol [B][K] or None; legs: K unless given (the refusals).  want_done / want_fired False: legs_done / leg_fired, leg_why
    and replan_info NULL.  -> dict(hist, traj_hist, ticks_run [B], replan_info [B][K], legs_done [B], leg_fired, leg_why [B][K], tube_hist, audit,
    log_hist, track, ran: the level that ran), or the return code with want_rc (1: what the C ABI refuses)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    Kb = replan.shape[1] if replan is not None else 1      # what the arrays hold; `legs` is what the entry is told
    K = Kb if legs is None else int(legs)
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    info, fired, why = (np.full((B, Kb), -7, dtype=np.int32) if want_fired else None for _ in range(3))
    done = np.full(B, -7, dtype=np.int32) if want_done else None
    tube = np.full((n, B, TUBE["LEN"]), 7.0) if want_tube else None
    aud = np.full((B, AUDIT["LEN"]), 7.0) if audit else None
    log = np.full((n, B, bstream.LOG_STAGE * max(int(log_stages), 0) + 4), 7.0) if want_log else None
    trk = np.full((B, TRACK["LEN"]), 7.0) if track else None
    if replan is not None:
        assert replan.flags.c_contiguous and replan.dtype == np.float64 and replan.shape[0] == B and replan.shape[2] == bstream.replan_len(S, T.shape[1])
    lt = None if leg_tick is None else _i32(leg_tick, (B, Kb), "leg_tick")
    lo = None if leg_on is None else _i32(leg_on, (B, Kb), "leg_on")
    ltol = None if leg_tol is None else np.ascontiguousarray(leg_tol, dtype=np.float64)
    assert ltol is None or ltol.shape == (B, Kb)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    c, p = ctypes, emu._p
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout_legs(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts)), c.c_int(B), c.c_int(int(ticks)), p(T), c.c_int(T.shape[1]),
                                              p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), p(A["x"]), p(A["g"]),
                                              p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                              c.c_double(goal_tol), p(hist), p(th), p(run), p(replan), p(info), c.c_int(int(update_flags)), p(dz), p(tube), p(aud),
                                              c.c_double(audit_tol), p(log), c.c_int(int(log_stages)), p(trk), c.c_int(K), p(lt), p(lo), p(ltol), p(done), p(fired), p(why),
                                              c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]),
                                              c.c_int(lane_order), c.c_int(wave_order), c.byref(ran))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, legs_done=done, leg_fired=fired, leg_why=why, tube_hist=tube, audit=aud, log_hist=log, track=trk,
                ran=ran.value)


# ---- the contract's loop ----
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


def mission_loop(N, S, h, T, A, ticks, stages=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], queue `replan` [K][len]; all advanced in place): per tick the fused tick's text
    (kw: the arguments of emu.stream_tick; nw=4: the team tick's), the tube text on the p that tick packed, the log text on what the tick left, cut to
    `stages`, then -- for a stream that still runs -- the disturb text on row `disturb[t]`, then the splice + update text on the HEAD record when one of
    its conditions holds (leg_tick, leg_on [K]; leg_tol [K] or None: goal_tol), the head advancing whatever the record's flag and validity.  The stop rules
    are the rollout's: a tick the stream lost its plan ahead of is not run, nor anything behind it; with goal_tol > 0 nothing runs behind the tick that
    leaves phi_max - phi <= goal_tol AFTER its events.
    -> dict(hist, traj_hist, tube_hist, p_hist, log_hist, ticks_run, legs_done, leg_fired [K], leg_why [K], replan_info [K], phi, phi_max: the two words
    behind every tick ahead of its events (NaN: not run)), NaN rows for the ticks not run"""
    K = 0 if replan is None else replan.shape[0]
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan), ticks_run=0, legs_done=0,
             leg_fired=np.full(K, -1, dtype=np.int32), leg_why=np.zeros(K, dtype=np.int32), replan_info=np.full(K, -1, dtype=np.int32), phi=np.full(ticks, np.nan),
             phi_max=np.full(ticks, np.nan))
    for t in range(ticks):
        row = tick(N, S, h, T, A, **kw)
        if row is None:                                           # lost its plan: the tick wrote status 3 and the stream stops
            break
        r["hist"][t], r["traj_hist"][t], r["p_hist"][t], r["ticks_run"] = row, A["traj"], A["p"], t + 1
        r["tube_hist"][t] = et.stream_tube(N, S, A["p"])[0]
        r["log_hist"][t] = cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        r["phi"][t], r["phi_max"][t] = A["ss"][SS["PHI"]], A["ss"][SS["PHIMAX"]]
        if disturb is not None:
            A["rb"][:] = eup.stream_disturb(A["rb"], disturb[t])
        k = r["legs_done"]
        if k < K:
            why = due(N, A["ss"], t, leg_tick[k], leg_on[k], goal_tol if leg_tol is None else leg_tol[k])
            if why:
                r["replan_info"][k], rec, Tn, ss, rb = eup.stream_update_flags(N, S, h, replan[k], T, A["ss"], A["rb"], update_flags)
                replan[k], T[:], A["ss"][:], A["rb"][:] = rec, Tn, ss, rb
                r["leg_fired"][k], r["leg_why"][k], r["legs_done"] = t, why, k + 1
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return r


def assert_equals_the_loop(N, S, A0, Tab, recs, ticks, leg_tick, leg_on, leg_tol, what, nw=1, wave_order=0, stages=1, **kw):
    """bmpc_emu_stream_rollout_legs on copies of (A0, Tab, recs [B][K][len]) against mission_loop, stream by stream, on other copies: every tick array, the
    path table, the queue, every history array, the audit and tracking records and the queue's outputs, bit for bit.  -> (result, arrays, tables, queues)"""
    A, Tb, R = copy_arrays(A0), Tab.copy(), recs.copy()
    r = rollout_legs(N, S, H, Tb, A, ticks, nw=nw, wave_order=wave_order, replan=R, leg_tick=leg_tick, leg_on=leg_on, leg_tol=leg_tol, log_stages=stages, **kw)
    assert r["ran"] == 4
    loop_kw = {k: v for k, v in kw.items() if k in ("update_flags", "goal_tol", "max_iter", "warm_dual", "accept_capped", "opts")}
    for b in range(Tab.shape[0]):
        Ab, Tl, Rl = unstack(A0, b), Tab[b].copy(), recs[b].copy()
        loop = mission_loop(N, S, H, Tl, Ab, ticks, stages=stages, replan=Rl, leg_tick=np.asarray(leg_tick)[b], leg_on=np.asarray(leg_on)[b],
                            leg_tol=None if leg_tol is None else np.asarray(leg_tol)[b], disturb=None if kw.get("disturb") is None else kw["disturb"][:, b], nw=nw, **loop_kw)
        assert_arrays_equal(Ab, unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl, Tb[b], equal_nan=True) and np.array_equal(Rl, R[b], equal_nan=True), f"{what}, stream {b}: table / queue"
        for k in ("hist", "traj_hist", "tube_hist", "log_hist"):
            assert np.array_equal(loop[k], r[k][:, b], equal_nan=True), f"{what}, stream {b}: {k}"
        got = (int(r["ticks_run"][b]), int(r["legs_done"][b]), r["leg_fired"][b].tolist(), r["leg_why"][b].tolist(), r["replan_info"][b].tolist())
        want = (loop["ticks_run"], loop["legs_done"], loop["leg_fired"].tolist(), loop["leg_why"].tolist(), loop["replan_info"].tolist())
        assert got == want, f"{what}, stream {b}: ticks_run, legs_done, leg_fired, leg_why, replan_info {got}, the loop's {want}"
    return r, A, Tb, R


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A, ticks, recs, leg_tick, leg_on, leg_tol=None, disturb=None, update_flags=3, flags=1, goal_tol=0.0, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_legs.cpp with BMPC_EMU_ROLLOUT_LEGS_MAIN): a batch behind its tick 0 and its queues"""
    B, K = recs.shape[:2]
    dist = np.zeros((ticks, B, bstream.DIST_LEN)) if disturb is None else disturb
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[1], flags, goal_tol, max_iter, update_flags, K, leg_tol is not None], dtype=np.float64).tofile(f)
        for a in [T] + [A[k] for k in ("ss", "rb", "p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] + [recs, leg_tick, leg_on] + ([leg_tol] if leg_tol is not None else []) + [dist]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout_legs.cpp with its own main (BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers, a child
    process per case.  cases: [(what, dict of write_case's arguments after the path)].  Returns the program's output, a line per case; raises when the
    build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_legs_san{nw}")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_ROLLOUT_LEGS_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_legs.cpp")])
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized mission rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_legs as cases_of
        nw = 4 if "4" in sys.argv else 1
        print("\n".join(run_sanitized(cases_of.sanitizer_cases(nw), nw)))
