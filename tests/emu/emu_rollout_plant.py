"""TEST-ONLY: the CPU build of the rollout with a table of actuator models per stream (boundmpc_amd/csrc/bmpc_rollout_kernel.inl with PL through
tests/emu/bmpc_emu_rollout_plant.cpp, built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the plants
share: the table of the tests and the contract's loop for one stream, plant_loop -- {fused tick's own kernel text, the plant step's own text, tube text,
log text, disturb text, splice + update text of the head record when it is due, stop rules} --, the exact checker of the entry.  The streams, batches,
paths and the other texts are emu_rollout's, the queue's rule is emu_rollout_legs', a settings row as arguments is emu_rollout_tune's.

  python -m tests.emu.emu_rollout_plant --sanitize [4]   builds bmpc_emu_rollout_plant.cpp as a stand-alone program with -fsanitize=address,undefined
                                                         and runs it on the cases of tests/test_stream_rollout_plant.py
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_legs as eq, emu_rollout_tune as etu
from tests.emu.emu_rollout import H, ROLL, SS, TUBE, AUDIT, TRACK, TICK_ARRAYS, _DEPS, copy_arrays, unstack, cut, history_row, et, el, eup      # noqa: F401

PLANT, PLANT_STATE, PLANT_REC, TUNE = bstream.PLANT, bstream.PLANT_STATE, bstream.PLANT_REC, bstream.TUNE
NAN = float("nan")
HISTORIES = ("hist", "traj_hist", "tube_hist", "log_hist")


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout_plant.so" if nw == 1 else f"libbmpc_emu_rollout_plant_team{nw}.so", "bmpc_emu_rollout_plant.cpp", (f"-DBMPC_NW={nw}",),
                   _DEPS + ("bmpc_stream_plant.inl",))
    assert L.bmpc_emu_rollout_plant_waves() == nw and [L.bmpc_emu_plant_slot(w, -1) for w in range(3)] == [PLANT["LEN"], PLANT_STATE["LEN"], PLANT_REC["LEN"]]
    return L


def slots():
    """the enums of the kernel text, by position of the header's: (row, state, record)"""
    return tuple([lib().bmpc_emu_plant_slot(w, k) for k in range(n)] for w, n in ((0, 5), (1, 2), (2, 6)))


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


# ---- the entry ----
def rollout_plant(N, S, h, T, A, ticks, plant, plant_state, nw=1, tune=None, replan=None, leg_tick=None, leg_on=None, leg_tol=None, update_flags=3, disturb=None, max_iter=0,
                  warm_dual=True, accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0), lane_order=0,
                  wave_order=0, want_rc=False, audit_tol=1e-6, log_stages=1, want_rec=True, want_info=True):
    """The CPU build of bmpc_stream_rollout_plant on the tick arrays `A` of B streams (advanced in place), the path tables T [B][cap][48], the queues `replan`
    [B][K][len] or None, the settings table `tune` [B][16] or None, the plant table `plant` [B][20] or None and the plant state [B][16] (advanced in place; None
    passes NULL), every other output array on.  -> dict(hist, traj_hist, ticks_run, tube_hist, audit, log_hist, track, tune_info, tune_used, plant_info [B],
    plant_rec [B][8], with a queue replan_info, legs_done, leg_fired, leg_why, ran: the level that ran), or the return code with want_rc."""
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
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    lt, lo, ltol, dz, tn, pl = i32(leg_tick), i32(leg_on), f64(leg_tol), f64(disturb), f64(tune), f64(plant)
    assert dz is None or dz.shape == (n, B, bstream.DIST_LEN)
    assert tn is None or tn.shape == (B, TUNE["LEN"])
    assert pl is None or pl.shape == (B, PLANT["LEN"])
    assert plant_state is None or (plant_state.flags.c_contiguous and plant_state.dtype == np.float64 and plant_state.shape == (B, PLANT_STATE["LEN"]))
    tinfo, used = (np.full(B, -7, dtype=np.int32), np.full((B, TUNE["LEN"]), -7.0)) if tn is not None else (None, None)
    pinfo = np.full(B, -7, dtype=np.int32) if want_info else None
    prec = np.full((B, PLANT_REC["LEN"]), -7.0) if want_rec else None
    c, p = ctypes, emu._p
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout_plant(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(emu.opts_for(N, opts if opts is not None else er.opts(N))), c.c_int(B), c.c_int(int(ticks)),
                                               p(T), c.c_int(T.shape[1]), p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)),
                                               p(A["x"]), p(A["g"]), p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                               c.c_double(goal_tol), p(hist), p(th), p(run), p(replan), p(info), c.c_int(int(update_flags)), p(dz), p(tube), p(aud),
                                               c.c_double(audit_tol), p(log), c.c_int(int(log_stages)), p(trk), c.c_int(K), p(lt), p(lo), p(ltol), p(done), p(fired), p(why),
                                               p(tn), p(tinfo), p(used), p(pl), p(plant_state), p(pinfo), p(prec), c.c_double(rt_tol), c.c_double(rt_row_cap),
                                               c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]), c.c_int(lane_order), c.c_int(wave_order), c.byref(ran))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, legs_done=done, leg_fired=fired, leg_why=why, tube_hist=tube, audit=aud, log_hist=log, track=trk,
                tune_info=tinfo, tune_used=used, plant_info=pinfo, plant_rec=prec, ran=ran.value)


# ---- the contract's loop ----
def plant_loop(N, S, h, T, A, ticks, plant_row, plant_state, stages=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None, update_flags=3, disturb=None, goal_tol=0.0,
               with_rec=True, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], queue `replan` [K][len] or None, plant state [16]; all advanced in place): per tick
    the fused tick's text (kw: the arguments of emu.stream_tick -- the stream's settings; nw=4: the team tick's), then bmpc_stream_plant's text with tick t
    (plant_row None: no plant step at all), then the history row, the tube text on the p that tick packed, the log text on what the tick left, cut to `stages`,
    then the disturb text on row `disturb[t]`, then the splice + update text on the HEAD record when one of its conditions holds (emu_rollout_legs.due).  The
    stop rules are the rollout's.  -> dict(hist, traj_hist, tube_hist, p_hist: the p of every tick, log_hist, ticks_run, legs_done, leg_fired, leg_why, replan_info, plant_rec, cmd: the
    first planned jerk of every tick [ticks][7], NaN: not run), NaN rows for the ticks not run"""
    K = 0 if replan is None else replan.shape[0]
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan), ticks_run=0, legs_done=0, leg_fired=np.full(K, -1, dtype=np.int32),
             leg_why=np.zeros(K, dtype=np.int32), replan_info=np.full(K, -1, dtype=np.int32), plant_rec=fresh_rec() if with_rec else None, cmd=np.full((ticks, 7), np.nan))
    RB = bstream.RB
    for t in range(ticks):
        if A["ss"][SS["ERRCNT"]] >= N:                               # lost its plan: the tick writes the words of a skipped stream and the stream stops
            emu.stream_tick(N, S, h, T, A, **kw)
            break
        emu.stream_tick(N, S, h, T, A, **kw)
        r["cmd"][t] = A["rb"][RB["JERK"]:RB["JERK"] + 7]
        if plant_row is not None:
            code, rb, st, rec = stream_plant(N, h, A["rb"], A["ss"], plant_row, plant_state, r["plant_rec"], t)
            assert code in (0, -1)
            A["rb"][:], plant_state[:] = rb, st
            if with_rec:
                r["plant_rec"] = rec
        r["hist"][t], r["traj_hist"][t], r["p_hist"][t], r["ticks_run"] = history_row(A), A["traj"], A["p"], t + 1
        r["tube_hist"][t] = et.stream_tube(N, S, A["p"])[0]
        r["log_hist"][t] = cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        if disturb is not None:
            A["rb"][:] = eup.stream_disturb(A["rb"], disturb[t])
        k = r["legs_done"]
        if k < K:
            why = eq.due(N, A["ss"], t, leg_tick[k], leg_on[k], goal_tol if leg_tol is None else leg_tol[k])
            if why:
                r["replan_info"][k], rec_, Tn, ss, rb = eup.stream_update_flags(N, S, h, replan[k], T, A["ss"], A["rb"], update_flags)
                replan[k], T[:], A["ss"][:], A["rb"][:] = rec_, Tn, ss, rb
                r["leg_fired"][k], r["leg_why"][k], r["legs_done"] = t, why, k + 1
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return r


def assert_equals_the_loop(N, S, A0, Tab, recs, ticks, plant, state0, what, nw=1, wave_order=0, lane_order=0, stages=1, tune=None, leg_tick=None, leg_on=None, leg_tol=None,
                           disturb=None, **kw):
    """bmpc_emu_stream_rollout_plant on copies of (A0, Tab, recs [B][K][len] or None, state0 [B][16]) with the tables `plant` and `tune` against plant_loop,
    stream by stream, on other copies and with the settings of tune_used[b]: every tick array, the path table, the queue, every history array, the audit
    and tracking records, the queue's outputs, the plant state and the plant record, bit for bit.  kw: update_flags, goal_tol, accept_capped.
    -> (result, arrays, tables, queues, plant state)"""
    A, Tb, R, st = copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy(), state0.copy()
    r = rollout_plant(N, S, H, Tb, A, ticks, plant, st, nw=nw, wave_order=wave_order, lane_order=lane_order, tune=tune, replan=R, leg_tick=leg_tick, leg_on=leg_on,
                      leg_tol=leg_tol, disturb=disturb, log_stages=stages, **kw)
    assert r["ran"] == 6 and not r["plant_info"].any() and (tune is None or not r["tune_info"].any())
    for b in range(Tab.shape[0]):
        s = etu.settings(r["tune_used"][b], N) if tune is not None else dict(opts=er.opts(N))
        Ab, Tl, Rl, sl = unstack(A0, b), Tab[b].copy(), None if recs is None else recs[b].copy(), state0[b].copy()
        loop = plant_loop(N, S, H, Tl, Ab, ticks, plant[b], sl, stages=stages, replan=Rl, leg_tick=None if recs is None else np.asarray(leg_tick)[b],
                          leg_on=None if recs is None else np.asarray(leg_on)[b], leg_tol=None if leg_tol is None else np.asarray(leg_tol)[b],
                          disturb=None if disturb is None else disturb[:, b], nw=nw, wave_order=wave_order, lane_order=lane_order, **s, **kw)
        er.assert_arrays_equal(Ab, unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl, Tb[b], equal_nan=True) and (recs is None or np.array_equal(Rl, R[b], equal_nan=True)), f"{what}, stream {b}: table / queue"
        for k in HISTORIES:
            assert np.array_equal(loop[k], r[k][:, b], equal_nan=True), f"{what}, stream {b}: {k}"
        one = et_audit_track(N, loop, kw.get("audit_tol", 1e-6))
        assert np.array_equal(one[0], r["audit"][b], equal_nan=True) and np.array_equal(one[1], r["track"][b], equal_nan=True), f"{what}, stream {b}: audit / track"
        assert np.array_equal(sl, st[b], equal_nan=True), f"{what}, stream {b}: plant_state"
        assert np.array_equal(loop["plant_rec"], r["plant_rec"][b], equal_nan=True), f"{what}, stream {b}: plant_rec {r['plant_rec'][b]}, the loop's {loop['plant_rec']}"
        assert int(r["ticks_run"][b]) == loop["ticks_run"], f"{what}, stream {b}: ticks_run"
        if recs is not None:
            got = (int(r["legs_done"][b]), r["leg_fired"][b].tolist(), r["leg_why"][b].tolist(), r["replan_info"][b].tolist())
            want = (loop["legs_done"], loop["leg_fired"].tolist(), loop["leg_why"].tolist(), loop["replan_info"].tolist())
            assert got == want, f"{what}, stream {b}: legs_done, leg_fired, leg_why, replan_info {got}, the loop's {want}"
    return r, A, Tb, R, st


def et_audit_track(N, loop, audit_tol=1e-6):
    """the audit and tracking records over the loop's own tube and log rows: the audit's exact numpy reduction (emu_stream_tube.audit_of) and the record
    text of the CPU build over the log rows (stream_track_init, stream_track)"""
    rows, up = np.ascontiguousarray(loop["log_hist"]), np.ascontiguousarray(loop["traj_hist"][:, -3])
    trk = np.full(TRACK["LEN"], -7.0)
    lib().bmpc_emu_stream_track_rows(ctypes.c_int(rows.shape[0]), ctypes.c_int(rows.shape[1]), emu._p(rows), emu._p(up), emu._p(trk))
    return et.audit_of(loop["tube_hist"], audit_tol), trk


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A, ticks, plant, plant_state, disturb=None, flags=1, goal_tol=0.0, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_plant.cpp with BMPC_EMU_ROLLOUT_PLANT_MAIN): a batch behind its tick 0, its plant table and state"""
    B = T.shape[0]
    dist = np.zeros((ticks, B, bstream.DIST_LEN)) if disturb is None else disturb
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[1], flags, goal_tol, max_iter], dtype=np.float64).tofile(f)
        for a in [T] + [A[k] for k in ("ss", "rb", "p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] + [plant, plant_state, dist]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout_plant.cpp with its own main (BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers, a child
    process per case.  cases: [(what, dict of write_case's arguments after the path)].  Returns the program's output, a line per case; raises when the
    build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_plant_san{nw}")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_ROLLOUT_PLANT_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_plant.cpp")])
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized plant rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_plant as cases_of
        nw = 4 if "4" in sys.argv else 1
        print("\n".join(run_sanitized(cases_of.sanitizer_cases(nw), nw)))
