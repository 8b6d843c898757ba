"""TEST-ONLY: the CPU build of the rollout with a table of controller settings per stream (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with TU through
tests/emu/bmpc_emu_rollout_tune.cpp, built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the sweeps
share: the table of the tests, a resolved row as the arguments of the entries that take their settings per call, and the exact checker of the entry --
stream b of a tuned rollout against the ONE-STREAM run of the queue entry's CPU build (emu_rollout_legs.rollout_legs) with the resolved row as its
options, real-time words, level rule and cap.  The streams, batches and paths are emu_rollout's.

  python -m tests.emu.emu_rollout_tune --sanitize [4]   builds bmpc_emu_rollout_tune.cpp as a stand-alone program with -fsanitize=address,undefined
                                                        and runs it on the cases of tests/test_stream_rollout_tune.py
"""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_legs as eq
from tests.emu.emu_rollout import H, ROLL, SS, TUBE, AUDIT, TRACK, TICK_ARRAYS, _DEPS, copy_arrays, unstack      # noqa: F401

TUNE, CROSS = bstream.TUNE, bstream.TUNE_CROSS
NAN = float("nan")
OUTPUTS = ("hist", "traj_hist", "tube_hist", "log_hist", "audit", "track")      # per stream: [ticks][B][..] or [B][..]


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout_tune.so" if nw == 1 else f"libbmpc_emu_rollout_tune_team{nw}.so", "bmpc_emu_rollout_tune.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_rollout_tune_waves() == nw and L.bmpc_emu_tune_slot(-1) == TUNE["LEN"] and L.bmpc_emu_tune_slot(-2) == CROSS
    return L


def slots():
    """the slots of the kernel text, by position of the header's enum"""
    return [lib().bmpc_emu_tune_slot(k) for k in range(14)]


# ---- the table of the tests ----
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
    """A RESOLVED row as the arguments the entries of the CPU build take per call: dict(opts, max_iter, rt_tol, rt_row_cap, level_rule).  base: the option
    record the words outside the table come from (None: emu_rollout.opts(N))."""
    u = bstream.unpack_tune(row)
    assert all(v is not None for v in u.values()), "a resolved row holds no NaN"
    o = emu.Opts.from_buffer_copy(base if base is not None else er.opts(N))
    o.max_iter, o.tol, o.mu_init, o.mu_warm, o.mu_min_fac, o.slack_push = u["max_iter"], u["tol"], u["mu_init"], u["mu_warm"], u["mu_min_fac"], u["slack_push"]
    o.bound_margin, o.hold_mu, o.stall_window = u["bound_margin"], u["hold"], u["stall_window"]
    return dict(opts=o, max_iter=0, rt_tol=u["rt_tol"], rt_row_cap=u["rt_row_cap"], level_rule=(u["lvl_c"], u["lvl_lo"], u["lvl_hi"]))


def tune_check(row, N, opts=None, max_iter=0, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0)):
    """the COMPILED validity rule (csrc/bmpc_args.h bmpc_tune_check) on one row against a launch's settings -> (mask, the row as resolved)"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    used = np.full(TUNE["LEN"], -7.0)
    c = ctypes
    bad = lib().bmpc_emu_tune_check(c.c_int(N), c.byref(emu.opts_for(N, opts if opts is not None else er.opts(N))), c.c_int(int(max_iter)), c.c_double(rt_tol), c.c_double(rt_row_cap),
                                    c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]), emu._p(row), emu._p(used))
    return bad, used


@functools.lru_cache(maxsize=None)
def start(N, S, nw=1, B=4):
    """emu_rollout.small_batch(N, S, B) with tick 0 of every stream solved out (nw = 4: by the team tick) -> (tick arrays, path tables, re-plan records);
    copy before use"""
    _, A0, Tab, recs = er.small_batch(N, S, B)
    for b in range(B):
        Ab = unstack(A0, b)
        er.tick(N, S, H, Tab[b], Ab, max_iter=100, warm_dual=True, opts=er.opts(N), nw=nw)
        for k in A0:
            A0[k][b] = Ab[k]
    assert (A0["status"] == 0).all()
    return A0, Tab, recs


def rollout_tuned(N, S, h, T, A, ticks, tune, nw=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True,
                  accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0), lane_order=0, wave_order=0, want_rc=False,
                  audit_tol=1e-6, log_stages=1, want_info=True, want_used=True):
    """The CPU build of bmpc_stream_rollout_tuned on the tick arrays `A` of B streams (advanced in place), the path tables T [B][cap][48], the queues `replan`
    [B][K][len] or None (no queue: replan NULL) and the table `tune` [B][16] or None, every other output array on.
    -> dict(hist, traj_hist, ticks_run, tube_hist, audit, log_hist, track, tune_info [B], tune_used [B][16], with a queue replan_info, legs_done, leg_fired,
    leg_why, ran: the level that ran), or the return code with want_rc."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    K = replan.shape[1] if replan is not None else 1
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    info, fired, why = (np.full((B, K), -7, dtype=np.int32) if replan is not None else None for _ in range(3))
    done = np.full(B, -7, dtype=np.int32) if replan is not None else None
    tube, aud = np.full((n, B, TUBE["LEN"]), 7.0), np.full((B, AUDIT["LEN"]), 7.0)
    log, trk = np.full((n, B, bstream.LOG_STAGE * int(log_stages) + 4), 7.0), np.full((B, TRACK["LEN"]), 7.0)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    lt, lo = i32(leg_tick), i32(leg_on)
    ltol = None if leg_tol is None else np.ascontiguousarray(leg_tol, dtype=np.float64)
    dz = None if disturb is None else np.ascontiguousarray(disturb, dtype=np.float64)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    tn = None if tune is None else np.ascontiguousarray(tune, dtype=np.float64)
    assert tn is None or tn.shape == (B, TUNE["LEN"])
    tinfo = np.full(B, -7, dtype=np.int32) if want_info else None
    used = np.full((B, TUNE["LEN"]), -7.0) if want_used else None
    c, p = ctypes, emu._p
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout_tuned(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts if opts is not None else er.opts(N))), c.c_int(B), c.c_int(int(ticks)),
                                               p(T), c.c_int(T.shape[1]), p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                               p(A["x"]), p(A["g"]), p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                               c.c_double(goal_tol), p(hist), p(th), p(run), p(replan), p(info), c.c_int(int(update_flags)), p(dz), p(tube), p(aud),
                                               c.c_double(audit_tol), p(log), c.c_int(int(log_stages)), p(trk), c.c_int(K), p(lt), p(lo), p(ltol), p(done), p(fired), p(why),
                                               p(tn), p(tinfo), p(used), c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]),
                                               c.c_double(level_rule[2]), c.c_int(lane_order), c.c_int(wave_order), c.byref(ran))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, legs_done=done, leg_fired=fired, leg_why=why, tube_hist=tube, audit=aud, log_hist=log, track=trk,
                tune_info=tinfo, tune_used=used, ran=ran.value)


def stream_of(r, b):
    """the outputs of stream b of a batch result"""
    return {k: (None if r[k] is None else r[k][:, b] if k in ("hist", "traj_hist", "tube_hist", "log_hist") else r[k][b])
            for k in OUTPUTS + ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why")}


def assert_streams_equal(got, want, what):
    for k, v in want.items():
        assert (v is None and got[k] is None) or np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True), f"{what}: {k} differs"


def assert_equals_one_stream_runs(N, S, A0, Tab, recs, ticks, tune, what, nw=1, wave_order=0, lane_order=0, rows=None, base=None, **kw):
    """bmpc_emu_stream_rollout_tuned on copies of (A0, Tab, recs [B][K][len] or None) with the table `tune` against, stream by stream, the ONE-STREAM run of
    the queue entry's CPU build with the settings of tune_used[b] (rows: the streams to check; None: those whose row is valid): every tick array, the path
    table, the queue, every history array, record and queue output, bit for bit.  kw: the arguments both take (leg_tick, leg_on, leg_tol, disturb,
    accept_capped, goal_tol, update_flags, log_stages); base: the launch's settings dict(opts, max_iter, rt_tol, rt_row_cap, level_rule).
    -> (result, arrays, tables, queues)"""
    base = dict(base or {})
    A, Tb, R = copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy()
    r = rollout_tuned(N, S, H, Tb, A, ticks, tune, nw=nw, wave_order=wave_order, lane_order=lane_order, replan=R, **base, **kw)
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
        if recs is None:
            one = eq.rollout_legs(N, S, H, Tl, Ab, ticks, nw=nw, wave_order=wave_order, lane_order=lane_order, want_done=False, want_fired=False, **s, **one_kw)
        else:
            one = eq.rollout_legs(N, S, H, Tl, Ab, ticks, nw=nw, wave_order=wave_order, lane_order=lane_order, replan=Rl, **s, **one_kw)
        er.assert_arrays_equal({k: Ab[k][0] for k in Ab}, unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl[0], Tb[b], equal_nan=True), f"{what}, stream {b}: path table"
        assert recs is None or np.array_equal(Rl[0], R[b], equal_nan=True), f"{what}, stream {b}: queue"
        assert_streams_equal(stream_of(r, b), stream_of(one, 0), f"{what}, stream {b}")
    return r, A, Tb, R


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A, ticks, tune, disturb=None, flags=1, goal_tol=0.0, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_tune.cpp with BMPC_EMU_ROLLOUT_TUNE_MAIN): a batch behind its tick 0 and its table"""
    B = T.shape[0]
    dist = np.zeros((ticks, B, bstream.DIST_LEN)) if disturb is None else disturb
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[1], flags, goal_tol, max_iter], dtype=np.float64).tofile(f)
        for a in [T] + [A[k] for k in ("ss", "rb", "p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] + [tune, dist]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout_tune.cpp with its own main (BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers, a child
    process per case.  cases: [(what, dict of write_case's arguments after the path)].  Returns the program's output, a line per case; raises when the
    build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_tune_san{nw}")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_ROLLOUT_TUNE_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_tune.cpp")])
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized tuned rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_tune as cases_of
        nw = 4 if "4" in sys.argv else 1
        print("\n".join(run_sanitized(cases_of.sanitizer_cases(nw), nw)))
