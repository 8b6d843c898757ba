"""TEST-ONLY: the CPU build of the rollout WITH A SENSOR MODEL (boundmpc_amd/csrc/bmpc_rollout_kernel.inl, the SE kernels, through
tests/emu/bmpc_emu_rollout_sensor.cpp, built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the sensors share:
the wrapper of the entry (rollout; the library's RArgs and NArgs records go in as their ctypes mirrors), the two steps on their own, and the contract's loop
{sense text, fused tick's own kernel text, unsense text, plant step text, tube text, log text, disturb text, splice + update text of the head record due, stop
rules} that is the exact checker of the entry.  Everything without a sensor -- the streams, the batches, the other steps -- is tests/emu/emu_rollout.py's.

  python -m tests.emu.emu_rollout_sensor --sanitize [4]   builds bmpc_emu_rollout_sensor.cpp as a stand-alone program with -fsanitize=address,undefined and
                                                          runs it on the cases of tests/test_stream_rollout_sensor.py
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_stream_log as el, emu_stream_tube as et, emu_stream_update as eup

SENSOR, SENSOR_STATE, SENSOR_REC = bstream.SENSOR, bstream.SENSOR_STATE, bstream.SENSOR_REC
ROLL, SS, TUBE, AUDIT, TRACK, TUNE, PLANT, PLANT_STATE, PLANT_REC = er.ROLL, er.SS, er.TUBE, er.AUDIT, er.TRACK, er.TUNE, er.PLANT, er.PLANT_STATE, er.PLANT_REC
RB, H, NAN = bstream.RB, er.H, er.NAN
HISTORIES = er.HISTORIES + ("meas_hist",)
_DEPS = er._DEPS + ("bmpc_rollout_body.inl", "bmpc_stream_sensor.inl")
RAN_SENSOR = 7      # *ran of the entry where the sensor kernels ran


class NArgs(ctypes.Structure):
    """the library's NArgs record (csrc/bmpc_args.h), member by member; tests/test_stream_rollout_sensor.py holds it to the offsets of both builds"""
    _fields_ = [("sensor", ctypes.c_void_p), ("sensor_state", ctypes.c_void_p), ("sensor_info", ctypes.c_void_p), ("sensor_rec", ctypes.c_void_p),
                ("sensor_noise", ctypes.c_void_p), ("meas_hist", ctypes.c_void_p)]


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout_sensor.so" if nw == 1 else f"libbmpc_emu_rollout_sensor_team{nw}.so", "bmpc_emu_rollout_sensor.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_sensor_waves() == nw
    assert L.bmpc_emu_sensor_rargs_size() == ctypes.sizeof(er.RArgs) and L.bmpc_emu_nargs_size() == ctypes.sizeof(NArgs), "the ctypes mirrors are not the library's records"
    assert [L.bmpc_emu_sensor_slot(w, -1) for w in range(3)] == [SENSOR["LEN"], SENSOR_STATE["LEN"], SENSOR_REC["LEN"]]
    return L


def sensor_slots():
    """the enums of the kernel text's sensor, by position of the header's: (row, state, record)"""
    return tuple([lib().bmpc_emu_sensor_slot(w, k) for k in range(n)] for w, n in ((0, 6), (1, 4), (2, 7)))


def sensor_check(row):
    """the COMPILED validity rule (csrc/bmpc_args.h bmpc_sensor_check) on one row -> (mask, the row as resolved)"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    assert row.shape == (SENSOR["LEN"],)
    used = np.full(SENSOR["LEN"], -7.0)
    return lib().bmpc_emu_sensor_check(emu._p(row), emu._p(used)), used


def fresh_rec():
    rec = np.full(SENSOR_REC["LEN"], -7.0)
    lib().bmpc_emu_stream_sensor_init(emu._p(rec))
    return rec


def stream_sense(N, rb, ss, row, state, noise=None, rec=None, tick=0):
    """what bmpc_stream_sense does with one stream, on copies -> (code, rb, state, rec, meas): code 0 behind a sample, -1 no plan (no sample, SAME = 1), else
    the mask of an invalid row (nothing touched); rec None or accumulated; meas: the record the pack will read (NaN where none was taken)"""
    rb, state, row, ss = (np.array(a, dtype=np.float64, order="C") for a in (rb, state, row, ss))
    rec = None if rec is None else np.array(rec, dtype=np.float64, order="C")
    noise = None if noise is None else np.array(noise, dtype=np.float64, order="C")
    meas = np.full(RB["LEN"], np.nan)
    code = lib().bmpc_emu_stream_sense(ctypes.c_int(N), emu._p(rb), emu._p(ss), emu._p(row), emu._p(noise), emu._p(state), emu._p(rec), emu._p(meas), ctypes.c_int(int(tick)))
    return code, rb, state, rec, meas


def stream_unsense(N, h, rb, ss, row, state):
    """what bmpc_stream_unsense does with one stream, on a copy -> (code, rb): code 0, or the mask of an invalid row (nothing touched)"""
    rb, state, row, ss = (np.array(a, dtype=np.float64, order="C") for a in (rb, state, row, ss))
    code = lib().bmpc_emu_stream_unsense(ctypes.c_int(N), ctypes.c_double(h), emu._p(rb), emu._p(ss), emu._p(row), emu._p(state))
    return code, rb


def noise(ticks, B, seed=11):
    """[ticks][B][21] unit draws"""
    return np.random.default_rng(seed).normal(size=(ticks, B, bstream.DIST_LEN))


# ---- the rollout text ----
def rollout(N, S, h, T, A, ticks, nw=1, sensor=None, sensor_state=None, sensor_noise=None, want_meas=True, want_sensor_rec=True, want_sensor_info=True, replan=None, leg_tick=None,
            leg_on=None, leg_tol=None, tune=None, plant=None, plant_state=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True,
            goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0, level_rule=(0.0, 0.0, 0.0), lane_order=0, wave_order=0, want_rc=False, audit_tol=1e-6, log_stages=1):
    """The CPU build of the sensor entry (nw = 1: one wave per stream; 4: teams) on the tick arrays `A` of B streams (er.fresh_arrays stacked; advanced in place) and
    the path tables T [B][cap][48]: the arguments of er.rollout with entry 6 -- the queue replan [B][K][len] with leg_tick, leg_on, leg_tol; tune [B][16]; plant
    [B][20] with plant_state [B][16], advanced in place -- and sensor [B][16] with sensor_state [B][64], advanced in place, sensor_noise [ticks][B][21] or None.
    Every output array of the plants' entry is on (the queue's with a queue, the table's with a table, the plant's with a plant table); want_meas,
    want_sensor_rec, want_sensor_info: the sensor's.
    -> the dict of er.rollout and sensor_info [B], sensor_rec [B][8], meas_hist [ticks][B][43]; ran: 7 where the sensor kernels ran, else the level of the text
    without a sensor; or the return code with want_rc (1: what the C ABI refuses)."""
    assert T.flags.c_contiguous and T.dtype == np.float64 and T.ndim == 3 and all(v.flags.c_contiguous for v in A.values())
    B, n = T.shape[0], max(int(ticks), 0)
    K = replan.shape[1] if replan is not None else 1
    i32 = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.int32).reshape(shape)
    f64 = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
    full = lambda want, shape, fill, dtype=np.float64: np.full(shape, fill, dtype=dtype) if want else None
    hist, th = np.zeros((n, B, ROLL["LEN"])), np.zeros((n, B, A["traj"].shape[-1]))
    run = np.full(B, -7, dtype=np.int32)
    tube, aud = np.full((n, B, TUBE["LEN"]), 7.0), np.full((B, AUDIT["LEN"]), 7.0)
    log, trk = np.full((n, B, bstream.LOG_STAGE * max(int(log_stages), 0) + 4), 7.0), np.full((B, TRACK["LEN"]), 7.0)
    info, fired, why = (full(replan is not None, (B, K), -7, np.int32) for _ in range(3))
    done = full(replan is not None, B, -7, np.int32)
    tinfo, used = full(tune is not None, B, -7, np.int32), full(tune is not None, (B, TUNE["LEN"]), -7.0)
    pinfo, prec = full(plant is not None, B, -7, np.int32), full(plant is not None, (B, PLANT_REC["LEN"]), -7.0)
    sinfo, srec = full(want_sensor_info, B, -7, np.int32), full(want_sensor_rec, (B, SENSOR_REC["LEN"]), -7.0)
    meas = full(want_meas, (n, B, RB["LEN"]), -7.0)
    for a, shape in ((replan, (B, K, bstream.replan_len(S, T.shape[1]))), (plant_state, (B, PLANT_STATE["LEN"])), (sensor_state, (B, SENSOR_STATE["LEN"]))):
        assert a is None or (a.flags.c_contiguous and a.dtype == np.float64 and a.shape == shape)
    lt, lo, ltol = i32(leg_tick, (B, K)), i32(leg_on, (B, K)), f64(leg_tol, (B, K))
    dz, tn, pl = f64(disturb, (n, B, bstream.DIST_LEN)), f64(tune, (B, TUNE["LEN"])), f64(plant, (B, PLANT["LEN"]))
    se, nz = f64(sensor, (B, SENSOR["LEN"])), f64(sensor_noise, (n, B, bstream.DIST_LEN))
    c, p = ctypes, emu._p
    r = er.RArgs(ticks=int(ticks), goal_tol=goal_tol, hist=p(hist), traj_hist=p(th), ticks_run=p(run), replan=p(replan), replan_tick=None, replan_info=p(info),
                 update_flags=int(update_flags), disturb=p(dz), tube_hist=p(tube), audit=p(aud), audit_tol=audit_tol, log_hist=p(log), log_stages=int(log_stages), track=p(trk),
                 legs=K if replan is not None else 0, leg_tick=p(lt), leg_on=p(lo), leg_tol=p(ltol), legs_done=p(done), leg_fired=p(fired), leg_why=p(why),
                 tune=p(tn), tune_info=p(tinfo), tune_used=p(used), plant=p(pl), plant_state=p(plant_state), plant_info=p(pinfo), plant_rec=p(prec))
    na = NArgs(sensor=p(se), sensor_state=p(sensor_state), sensor_info=p(sinfo), sensor_rec=p(srec), sensor_noise=p(nz), meas_hist=p(meas))
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout_sensor(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(opts if opts is not None else er.opts(N)), c.c_int(B), p(T), c.c_int(T.shape[1]),
                                                p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), p(A["x"]), p(A["g"]),
                                                p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                                c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]),
                                                c.c_int(lane_order), c.c_int(wave_order), c.byref(ran), c.byref(r), c.byref(na))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk, legs_done=done, leg_fired=fired, leg_why=why,
                tune_info=tinfo, tune_used=used, plant_info=pinfo, plant_rec=prec, sensor_info=sinfo, sensor_rec=srec, meas_hist=meas, ran=ran.value)


# ---- the contract's loop ----
def contract_loop(N, S, h, T, A, ticks, sensor_row, sensor_state, sensor_noise=None, stages=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None, plant_row=None,
                  plant_state=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream (tick arrays A, table T [cap][48], the queue `replan` [K][len], the plant state [16] and the sensor state [64]; all
    advanced in place), in the order of the kernel: per tick the sense text with tick t and the noise row sensor_noise[t], the fused tick's text (kw: the
    arguments of emu.stream_tick; nw=4: the team tick's), the unsense text, bmpc_stream_plant's text when a row is given, then the history row, the tube text
    on the p that tick packed, the log text on what the tick left, the disturb text, the splice + update text of the head record due -- er.contract_loop with
    the two steps around the tick, and the same stop rules: a tick the stream lost its plan ahead of runs nothing, the sample included.
    -> the dict of er.contract_loop and meas_hist [ticks][43], truth_hist [ticks][43] (the record ahead of every sample), sensor_rec"""
    K = replan.shape[0] if replan is not None else 0
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), truth_hist=np.full((ticks, RB["LEN"]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan), meas_hist=np.full((ticks, RB["LEN"]), np.nan),
             ticks_run=0, replan_info=np.full(K, -1, dtype=np.int32), legs_done=0, leg_fired=np.full(K, -1, dtype=np.int32), leg_why=np.zeros(K, dtype=np.int32),
             plant_rec=er.fresh_rec() if plant_row is not None else None, sensor_rec=fresh_rec())
    for t in range(ticks):
        if A["ss"][SS["ERRCNT"]] >= N:                            # lost its plan: the tick writes the words of a skipped stream and the stream stops
            emu.stream_tick(N, S, h, T, A, **kw)
            break
        r["truth_hist"][t] = A["rb"]
        code, rb, st, rec, meas = stream_sense(N, A["rb"], A["ss"], sensor_row, sensor_state, None if sensor_noise is None else sensor_noise[t], r["sensor_rec"], t)
        assert code == 0
        A["rb"][:], sensor_state[:], r["sensor_rec"], r["meas_hist"][t] = rb, st, rec, meas
        emu.stream_tick(N, S, h, T, A, **kw)
        code, rb = stream_unsense(N, h, A["rb"], A["ss"], sensor_row, sensor_state)
        assert code == 0
        A["rb"][:] = rb
        if plant_row is not None:
            code, rb, st, rec = er.stream_plant(N, h, A["rb"], A["ss"], plant_row, plant_state, r["plant_rec"], t)
            assert code in (0, -1)
            A["rb"][:], plant_state[:], r["plant_rec"] = rb, st, rec
        r["hist"][t], r["traj_hist"][t], r["p_hist"][t], r["ticks_run"] = er.history_row(A), A["traj"], A["p"], t + 1
        r["tube_hist"][t] = et.stream_tube(N, S, A["p"])[0]
        r["log_hist"][t] = er.cut(el.stream_log(N, S, h, T, A["ss"], A["p"], A["traj"]), N, stages)
        if disturb is not None:
            A["rb"][:] = eup.stream_disturb(A["rb"], disturb[t])
        k = r["legs_done"]
        why = er.due(N, A["ss"], t, leg_tick[k], leg_on[k], goal_tol if leg_tol is None else leg_tol[k]) if k < K else 0
        if why:
            info, replan[k][:], T[:], A["ss"][:], A["rb"][:] = eup.stream_update_flags(N, S, h, replan[k], T, A["ss"], A["rb"], update_flags)
            r["replan_info"][k], r["leg_fired"][k], r["leg_why"][k], r["legs_done"] = info, t, why, k + 1
        if goal_tol > 0.0 and A["ss"][SS["PHIMAX"]] - A["ss"][SS["PHI"]] <= goal_tol:
            break
    return r


def assert_equals_the_loop(N, S, A0, Tab, recs, ticks, sensor, what, sensor_noise=None, leg_tick=None, leg_on=None, leg_tol=None, plant=None, pstate0=None, tune=None, nw=1,
                           wave_order=0, lane_order=0, stages=1, disturb=None, **kw):
    """The sensor entry on copies of (A0, Tab, recs [B][K][len] or None, pstate0 [B][16], a fresh sensor state) with the tables `sensor`, `plant` and `tune` against
    contract_loop, stream by stream, on other copies and with the settings of tune_used[b]: every tick array, the path table, the queue, every history array
    (meas_hist among them), the audit and tracking records, the queue's outputs, the plant and sensor states and records, bit for bit.  kw: update_flags,
    goal_tol, accept_capped, max_iter, warm_dual, opts, audit_tol.  -> (result, arrays, tables, queues, plant state, sensor state, the loops' results)"""
    B = Tab.shape[0]
    A, Tb, R, pst = er.copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy(), None if pstate0 is None else pstate0.copy()
    sst = np.zeros((B, SENSOR_STATE["LEN"]))
    r = rollout(N, S, H, Tb, A, ticks, nw=nw, wave_order=wave_order, lane_order=lane_order, sensor=sensor, sensor_state=sst, sensor_noise=sensor_noise, replan=R, leg_tick=leg_tick,
                leg_on=leg_on, leg_tol=leg_tol, tune=tune, plant=plant, plant_state=pst, disturb=disturb, log_stages=stages, **kw)
    assert r["ran"] == RAN_SENSOR and not r["sensor_info"].any() and (plant is None or not r["plant_info"].any()) and (tune is None or not r["tune_info"].any())
    loop_kw = {k: v for k, v in kw.items() if k not in ("audit_tol", "opts")}
    per = lambda v, b: None if v is None else np.asarray(v)[b]
    loops = []
    for b in range(B):
        s = er.settings(r["tune_used"][b], N) if tune is not None else dict(opts=kw["opts"] if kw.get("opts") is not None else er.opts(N))
        Ab, Tl, Rl, pl, sl = er.unstack(A0, b), Tab[b].copy(), per(recs, b), per(pstate0, b), np.zeros(SENSOR_STATE["LEN"])
        Rl, pl = (None if v is None else v.copy() for v in (Rl, pl))
        loop = contract_loop(N, S, H, Tl, Ab, ticks, sensor[b], sl, None if sensor_noise is None else sensor_noise[:, b], stages, replan=Rl, leg_tick=per(leg_tick, b),
                             leg_on=per(leg_on, b), leg_tol=per(leg_tol, b), plant_row=per(plant, b), plant_state=pl, disturb=None if disturb is None else disturb[:, b], nw=nw,
                             wave_order=wave_order, lane_order=lane_order, **{**loop_kw, **s})
        loops.append(loop)
        er.assert_arrays_equal(Ab, er.unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl, Tb[b], equal_nan=True) and (recs is None or np.array_equal(Rl, R[b], equal_nan=True)), f"{what}, stream {b}: table / queue"
        for k in HISTORIES:
            assert np.array_equal(loop[k], r[k][:, b], equal_nan=True), f"{what}, stream {b}: {k}"
        one = er.et_audit_track(N, loop, kw.get("audit_tol", 1e-6))
        assert np.array_equal(one[0], r["audit"][b], equal_nan=True) and np.array_equal(one[1], r["track"][b], equal_nan=True), f"{what}, stream {b}: audit / track"
        assert int(r["ticks_run"][b]) == loop["ticks_run"], f"{what}, stream {b}: ticks_run {r['ticks_run'][b]}, the loop's {loop['ticks_run']}"
        assert np.array_equal(sl, sst[b], equal_nan=True), f"{what}, stream {b}: sensor_state"
        assert np.array_equal(loop["sensor_rec"], r["sensor_rec"][b], equal_nan=True), f"{what}, stream {b}: sensor_rec {r['sensor_rec'][b]}, the loop's {loop['sensor_rec']}"
        if plant is not None:
            assert np.array_equal(pl, pst[b], equal_nan=True), f"{what}, stream {b}: plant_state"
            assert np.array_equal(loop["plant_rec"], r["plant_rec"][b], equal_nan=True), f"{what}, stream {b}: plant_rec"
        if recs is not None:
            got = (int(r["legs_done"][b]), r["leg_fired"][b].tolist(), r["leg_why"][b].tolist(), r["replan_info"][b].tolist())
            want = (loop["legs_done"], loop["leg_fired"].tolist(), loop["leg_why"].tolist(), loop["replan_info"].tolist())
            assert got == want, f"{what}, stream {b}: legs_done, leg_fired, leg_why, replan_info {got}, the loop's {want}"
    return r, A, Tb, R, pst, sst, loops


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A, ticks, sensor, sensor_state=None, sensor_noise=None, plant=None, plant_state=None, disturb=None, flags=1, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_sensor.cpp with BMPC_EMU_SENSOR_MAIN): a header with the mask of the sections, a batch behind its
    tick 0 (T [B][cap][48], A: its tick arrays), the sensor table and state (None: fresh), then the sections given"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    B = T.shape[0]
    assert (plant is None) == (plant_state is None)
    sections = [(1, sensor_noise), (2, plant), (2, plant_state), (4, disturb)]
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[-2], flags, max_iter, sum({bit for bit, a in sections if a is not None})], dtype=np.float64).tofile(f)
        for a in [T] + [A[k] for k in ("ss", "rb", "p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] + \
                 [sensor, np.zeros((B, SENSOR_STATE["LEN"])) if sensor_state is None else sensor_state] + [a for _, a in sections if a is not None]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout_sensor.cpp with its own main (BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers, a child process
    per case, nothing preloaded.  cases: [(what, dict of write_case's arguments after the path)].  The runs of a case must agree.  Returns the program's output, a
    line per case; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_sensor_san{nw}")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_SENSOR_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_sensor.cpp")])
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized sensor rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_sensor
        nw = 4 if "4" in sys.argv else 1
        print("\n".join(run_sanitized(test_stream_rollout_sensor.sanitizer_cases(nw), nw)))
