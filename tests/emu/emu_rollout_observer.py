"""TEST-ONLY: the CPU build of the rollout WITH A STATE OBSERVER (boundmpc_amd/csrc/bmpc_rollout_kernel.inl, the OB kernels, through
tests/emu/bmpc_emu_rollout_observer.cpp, built once for one wave per stream and once for teams of four) and what the CPU and the GPU tests of the observers
share: the wrapper of the entry (rollout; the library's RArgs, NArgs and OArgs records go in as their ctypes mirrors), the step on its own, and the contract's
loop {observe text, fused tick's own kernel text, unsense text, plant step text, tube text, log text, disturb text, splice + update text of the head record
due, stop rules} that is the exact checker of the entry.  Everything of the sensor is tests/emu/emu_rollout_sensor.py's, everything below it
tests/emu/emu_rollout.py's.

  python -m tests.emu.emu_rollout_observer --sanitize [4]   builds bmpc_emu_rollout_observer.cpp as a stand-alone program with -fsanitize=address,undefined and
                                                            runs it on the cases of tests/test_stream_rollout_observer.py
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_rollout_sensor as es, emu_stream_log as el, emu_stream_tube as et, emu_stream_update as eup

OBSERVER, OBSERVER_STATE, OBSERVER_REC = bstream.OBSERVER, bstream.OBSERVER_STATE, bstream.OBSERVER_REC
SENSOR, SENSOR_STATE, SENSOR_REC = es.SENSOR, es.SENSOR_STATE, es.SENSOR_REC
ROLL, SS, TUBE, AUDIT, TRACK, TUNE, PLANT, PLANT_STATE, PLANT_REC = er.ROLL, er.SS, er.TUBE, er.AUDIT, er.TRACK, er.TUNE, er.PLANT, er.PLANT_STATE, er.PLANT_REC
RB, H, NAN = bstream.RB, er.H, er.NAN
HISTORIES = es.HISTORIES + ("sample_hist",)
_DEPS = es._DEPS + ("bmpc_stream_observer.inl",)
RAN_OBSERVER, RAN_SENSOR = 8, es.RAN_SENSOR      # *ran of the entry where the observer kernels ran, where the sensor kernels did


class OArgs(ctypes.Structure):
    """the library's OArgs record (csrc/bmpc_args.h), member by member; tests/test_stream_rollout_observer.py holds it to the offsets of both builds"""
    _fields_ = [("observer", ctypes.c_void_p), ("observer_state", ctypes.c_void_p), ("observer_info", ctypes.c_void_p), ("observer_rec", ctypes.c_void_p),
                ("sample_hist", ctypes.c_void_p)]


def lib(nw=1):
    L = emu._build("libbmpc_emu_rollout_observer.so" if nw == 1 else f"libbmpc_emu_rollout_observer_team{nw}.so", "bmpc_emu_rollout_observer.cpp", (f"-DBMPC_NW={nw}",), _DEPS)
    assert L.bmpc_emu_observer_waves() == nw
    assert L.bmpc_emu_observer_rargs_size() == ctypes.sizeof(er.RArgs) and L.bmpc_emu_observer_nargs_size() == ctypes.sizeof(es.NArgs) and L.bmpc_emu_oargs_size() == ctypes.sizeof(OArgs), \
        "the ctypes mirrors are not the library's records"
    assert [L.bmpc_emu_observer_slot(w, -1) for w in range(3)] == [OBSERVER["LEN"], OBSERVER_STATE["LEN"], OBSERVER_REC["LEN"]]
    return L


def observer_slots():
    """the enums of the kernel text's observer, by position of the header's: (row, state, record)"""
    return tuple([lib().bmpc_emu_observer_slot(w, k) for k in range(n)] for w, n in ((0, 5), (1, 5), (2, 8)))


def observer_check(row):
    """the COMPILED validity rule (csrc/bmpc_args.h bmpc_observer_check) on one row -> (mask, the row as resolved)"""
    row = np.ascontiguousarray(row, dtype=np.float64)
    assert row.shape == (OBSERVER["LEN"],)
    used = np.full(OBSERVER["LEN"], -7.0)
    return lib().bmpc_emu_observer_check(emu._p(row), emu._p(used)), used


def fresh_rec():
    rec = np.full(OBSERVER_REC["LEN"], -7.0)
    lib().bmpc_emu_stream_observer_init(emu._p(rec))
    return rec


def stream_observe(N, h, rb, ss, row, state, orow, ostate, noise=None, rec=None, orec=None, tick=0):
    """what bmpc_stream_observe does with one stream, on copies -> (code, rb, state, ostate, rec, orec, meas, sample, masks): code 0 behind an estimate, -1 no plan
    (no sample, no estimate, SAME = 1), -2 an invalid sensor or observer row (nothing touched; masks = (sensor's, observer's)); rec, orec None or accumulated;
    meas: the record the pack will read, sample: the raw sample (NaN where none was taken)"""
    rb, state, row, ss, orow, ostate = (np.array(a, dtype=np.float64, order="C") for a in (rb, state, row, ss, orow, ostate))
    rec, orec, noise = (None if a is None else np.array(a, dtype=np.float64, order="C") for a in (rec, orec, noise))
    meas, sample = np.full(RB["LEN"], np.nan), np.full(bstream.DIST_LEN, np.nan)
    info, oinfo = ctypes.c_int(-7), ctypes.c_int(-7)
    code = lib().bmpc_emu_stream_observe(ctypes.c_int(N), ctypes.c_double(h), emu._p(rb), emu._p(ss), emu._p(row), emu._p(noise), emu._p(state), emu._p(rec), emu._p(meas),
                                         ctypes.c_int(int(tick)), emu._p(orow), emu._p(ostate), emu._p(orec), emu._p(sample), ctypes.byref(info), ctypes.byref(oinfo))
    return code, rb, state, ostate, rec, orec, meas, sample, (info.value, oinfo.value)


# ---- the rollout text ----
def rollout(N, S, h, T, A, ticks, nw=1, sensor=None, sensor_state=None, sensor_noise=None, observer=None, observer_state=None, want_meas=True, want_sensor_rec=True,
            want_sensor_info=True, want_sample=True, want_observer_rec=True, want_observer_info=True, replan=None, leg_tick=None, leg_on=None, leg_tol=None, tune=None, plant=None,
            plant_state=None, update_flags=3, disturb=None, max_iter=0, warm_dual=True, accept_capped=False, simulate=True, goal_tol=0.0, opts=None, rt_tol=1e-4, rt_row_cap=0.0,
            level_rule=(0.0, 0.0, 0.0), lane_order=0, wave_order=0, want_rc=False, audit_tol=1e-6, log_stages=1):
    """The CPU build of the observer entry (nw = 1: one wave per stream; 4: teams): the arguments and the result of es.rollout, and observer [B][8] with
    observer_state [B][40], advanced in place; want_sample, want_observer_rec, want_observer_info: the observer's outputs (given only with a table).
    -> the dict of es.rollout and observer_info [B], observer_rec [B][8], sample_hist [ticks][B][21]; ran: 8 where the observer kernels ran, 7 the sensor
    kernels, else the level of the text without a sensor; or the return code with want_rc (1: what the C ABI refuses)."""
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
    ob = observer is not None
    oinfo, orec = full(ob and want_observer_info, B, -7, np.int32), full(ob and want_observer_rec, (B, OBSERVER_REC["LEN"]), -7.0)
    smp = full(ob and want_sample, (n, B, bstream.DIST_LEN), -7.0)
    for a, shape in ((replan, (B, K, bstream.replan_len(S, T.shape[1]))), (plant_state, (B, PLANT_STATE["LEN"])), (sensor_state, (B, SENSOR_STATE["LEN"])),
                     (observer_state, (B, OBSERVER_STATE["LEN"]))):
        assert a is None or (a.flags.c_contiguous and a.dtype == np.float64 and a.shape == shape)
    lt, lo, ltol = i32(leg_tick, (B, K)), i32(leg_on, (B, K)), f64(leg_tol, (B, K))
    dz, tn, pl = f64(disturb, (n, B, bstream.DIST_LEN)), f64(tune, (B, TUNE["LEN"])), f64(plant, (B, PLANT["LEN"]))
    se, nz, obt = f64(sensor, (B, SENSOR["LEN"])), f64(sensor_noise, (n, B, bstream.DIST_LEN)), f64(observer, (B, OBSERVER["LEN"]))
    c, p = ctypes, emu._p
    r = er.RArgs(ticks=int(ticks), goal_tol=goal_tol, hist=p(hist), traj_hist=p(th), ticks_run=p(run), replan=p(replan), replan_tick=None, replan_info=p(info),
                 update_flags=int(update_flags), disturb=p(dz), tube_hist=p(tube), audit=p(aud), audit_tol=audit_tol, log_hist=p(log), log_stages=int(log_stages), track=p(trk),
                 legs=K if replan is not None else 0, leg_tick=p(lt), leg_on=p(lo), leg_tol=p(ltol), legs_done=p(done), leg_fired=p(fired), leg_why=p(why),
                 tune=p(tn), tune_info=p(tinfo), tune_used=p(used), plant=p(pl), plant_state=p(plant_state), plant_info=p(pinfo), plant_rec=p(prec))
    na = es.NArgs(sensor=p(se), sensor_state=p(sensor_state), sensor_info=p(sinfo), sensor_rec=p(srec), sensor_noise=p(nz), meas_hist=p(meas))
    oa = OArgs(observer=p(obt), observer_state=p(observer_state), observer_info=p(oinfo), observer_rec=p(orec), sample_hist=p(smp))
    ran = c.c_int(-1)
    rc = lib(nw).bmpc_emu_stream_rollout_observer(c.c_int(N), c.c_int(S), c.c_double(h), c.byref(opts if opts is not None else er.opts(N)), c.c_int(B), p(T), c.c_int(T.shape[1]),
                                                  p(A["ss"]), p(A["rb"]), p(A["p"]), p(A["x0"]), p(A["dual"]) if warm_dual else None, c.c_int(int(max_iter)), p(A["x"]), p(A["g"]),
                                                  p(A["iters"]), p(A["status"]), p(A["kkt"]), p(A["traj"]), c.c_int(int(bool(simulate)) | (2 if accept_capped else 0)),
                                                  c.c_double(rt_tol), c.c_double(rt_row_cap), c.c_double(level_rule[0]), c.c_double(level_rule[1]), c.c_double(level_rule[2]),
                                                  c.c_int(lane_order), c.c_int(wave_order), c.byref(ran), c.byref(r), c.byref(na), c.byref(oa))
    if want_rc:
        return rc
    assert rc == 0
    return dict(hist=hist, traj_hist=th, ticks_run=run, replan_info=info, tube_hist=tube, audit=aud, log_hist=log, track=trk, legs_done=done, leg_fired=fired, leg_why=why,
                tune_info=tinfo, tune_used=used, plant_info=pinfo, plant_rec=prec, sensor_info=sinfo, sensor_rec=srec, meas_hist=meas, observer_info=oinfo, observer_rec=orec,
                sample_hist=smp, ran=ran.value)


# ---- the contract's loop ----
def contract_loop(N, S, h, T, A, ticks, sensor_row, sensor_state, observer_row, observer_state, sensor_noise=None, stages=1, replan=None, leg_tick=None, leg_on=None, leg_tol=None,
                  plant_row=None, plant_state=None, update_flags=3, disturb=None, goal_tol=0.0, **kw):
    """The contract's loop on ONE stream: es.contract_loop with the observe text in the place of the sense text (the observer state [40] advanced in place too).
    -> the dict of es.contract_loop and sample_hist [ticks][21], observer_rec"""
    K = replan.shape[0] if replan is not None else 0
    r = dict(hist=np.full((ticks, ROLL["LEN"]), np.nan), traj_hist=np.full((ticks, A["traj"].shape[0]), np.nan), tube_hist=np.full((ticks, TUBE["LEN"]), np.nan),
             p_hist=np.full((ticks, A["p"].shape[0]), np.nan), truth_hist=np.full((ticks, RB["LEN"]), np.nan), log_hist=np.full((ticks, bstream.rollout_log_len(stages)), np.nan),
             meas_hist=np.full((ticks, RB["LEN"]), np.nan), sample_hist=np.full((ticks, bstream.DIST_LEN), np.nan),
             ticks_run=0, replan_info=np.full(K, -1, dtype=np.int32), legs_done=0, leg_fired=np.full(K, -1, dtype=np.int32), leg_why=np.zeros(K, dtype=np.int32),
             plant_rec=er.fresh_rec() if plant_row is not None else None, sensor_rec=es.fresh_rec(), observer_rec=fresh_rec())
    for t in range(ticks):
        if A["ss"][SS["ERRCNT"]] >= N:                            # lost its plan: the tick writes the words of a skipped stream and the stream stops
            emu.stream_tick(N, S, h, T, A, **kw)
            break
        r["truth_hist"][t] = A["rb"]
        code, rb, st, ost, rec, orec, meas, smp, _ = stream_observe(N, h, A["rb"], A["ss"], sensor_row, sensor_state, observer_row, observer_state,
                                                                     None if sensor_noise is None else sensor_noise[t], r["sensor_rec"], r["observer_rec"], t)
        assert code == 0
        A["rb"][:], sensor_state[:], observer_state[:], r["sensor_rec"], r["observer_rec"], r["meas_hist"][t], r["sample_hist"][t] = rb, st, ost, rec, orec, meas, smp
        emu.stream_tick(N, S, h, T, A, **kw)
        code, rb = es.stream_unsense(N, h, A["rb"], A["ss"], sensor_row, sensor_state)
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


def assert_equals_the_loop(N, S, A0, Tab, recs, ticks, sensor, observer, what, sensor_noise=None, leg_tick=None, leg_on=None, leg_tol=None, plant=None, pstate0=None, tune=None, nw=1,
                           wave_order=0, lane_order=0, stages=1, disturb=None, **kw):
    """The observer entry on copies of (A0, Tab, recs [B][K][len] or None, pstate0 [B][16], fresh sensor and observer states) with the tables `sensor`, `observer`,
    `plant` and `tune` against contract_loop, stream by stream, on other copies and with the settings of tune_used[b]: what es.assert_equals_the_loop compares,
    and sample_hist, the observer state and the observer record, bit for bit.
    -> (result, arrays, tables, queues, plant state, sensor state, observer state, the loops' results)"""
    B = Tab.shape[0]
    A, Tb, R, pst = er.copy_arrays(A0), Tab.copy(), None if recs is None else recs.copy(), None if pstate0 is None else pstate0.copy()
    sst, ost = np.zeros((B, SENSOR_STATE["LEN"])), np.zeros((B, OBSERVER_STATE["LEN"]))
    r = rollout(N, S, H, Tb, A, ticks, nw=nw, wave_order=wave_order, lane_order=lane_order, sensor=sensor, sensor_state=sst, sensor_noise=sensor_noise, observer=observer,
                observer_state=ost, replan=R, leg_tick=leg_tick, leg_on=leg_on, leg_tol=leg_tol, tune=tune, plant=plant, plant_state=pst, disturb=disturb, log_stages=stages, **kw)
    assert r["ran"] == RAN_OBSERVER and not r["sensor_info"].any() and not r["observer_info"].any() and (plant is None or not r["plant_info"].any()) and (tune is None or not r["tune_info"].any())
    loop_kw = {k: v for k, v in kw.items() if k not in ("audit_tol", "opts")}
    per = lambda v, b: None if v is None else np.asarray(v)[b]
    loops = []
    for b in range(B):
        s = er.settings(r["tune_used"][b], N) if tune is not None else dict(opts=kw["opts"] if kw.get("opts") is not None else er.opts(N))
        Ab, Tl, Rl, pl, sl, ol = er.unstack(A0, b), Tab[b].copy(), per(recs, b), per(pstate0, b), np.zeros(SENSOR_STATE["LEN"]), np.zeros(OBSERVER_STATE["LEN"])
        Rl, pl = (None if v is None else v.copy() for v in (Rl, pl))
        loop = contract_loop(N, S, H, Tl, Ab, ticks, sensor[b], sl, observer[b], ol, None if sensor_noise is None else sensor_noise[:, b], stages, replan=Rl, leg_tick=per(leg_tick, b),
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
        assert np.array_equal(ol, ost[b], equal_nan=True), f"{what}, stream {b}: observer_state"
        assert np.array_equal(loop["sensor_rec"], r["sensor_rec"][b], equal_nan=True), f"{what}, stream {b}: sensor_rec {r['sensor_rec'][b]}, the loop's {loop['sensor_rec']}"
        assert np.array_equal(loop["observer_rec"], r["observer_rec"][b], equal_nan=True), f"{what}, stream {b}: observer_rec {r['observer_rec'][b]}, the loop's {loop['observer_rec']}"
        if plant is not None:
            assert np.array_equal(pl, pst[b], equal_nan=True), f"{what}, stream {b}: plant_state"
            assert np.array_equal(loop["plant_rec"], r["plant_rec"][b], equal_nan=True), f"{what}, stream {b}: plant_rec"
        if recs is not None:
            got = (int(r["legs_done"][b]), r["leg_fired"][b].tolist(), r["leg_why"][b].tolist(), r["replan_info"][b].tolist())
            want = (loop["legs_done"], loop["leg_fired"].tolist(), loop["leg_why"].tolist(), loop["replan_info"].tolist())
            assert got == want, f"{what}, stream {b}: legs_done, leg_fired, leg_why, replan_info {got}, the loop's {want}"
    return r, A, Tb, R, pst, sst, ost, loops


# ---- the stand-alone program under the sanitizers ----
def write_case(path, N, S, h, T, A, ticks, sensor, observer, sensor_state=None, observer_state=None, sensor_noise=None, plant=None, plant_state=None, disturb=None, flags=1, max_iter=0):
    """the case file of the stand-alone program (bmpc_emu_rollout_observer.cpp with BMPC_EMU_OBSERVER_MAIN): a header with the mask of the sections, a batch behind
    its tick 0 (T [B][cap][48], A: its tick arrays), the sensor table and state, the observer table and state (None: fresh), then the sections given"""
    T = np.ascontiguousarray(T, dtype=np.float64)
    B = T.shape[0]
    assert (plant is None) == (plant_state is None)
    sections = [(1, sensor_noise), (2, plant), (2, plant_state), (4, disturb)]
    with open(path, "wb") as f:
        np.array([N, S, h, B, ticks, T.shape[-2], flags, max_iter, sum({bit for bit, a in sections if a is not None})], dtype=np.float64).tofile(f)
        for a in [T] + [A[k] for k in ("ss", "rb", "p", "x0", "dual", "x", "g", "traj", "iters", "status", "kkt")] + \
                 [sensor, np.zeros((B, SENSOR_STATE["LEN"])) if sensor_state is None else sensor_state, observer,
                  np.zeros((B, OBSERVER_STATE["LEN"])) if observer_state is None else observer_state] + [a for _, a in sections if a is not None]:
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def run_sanitized(cases, nw=1, keep=None):
    """bmpc_emu_rollout_observer.cpp with its own main (BMPC_NW = nw) under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers, a child process
    per case, nothing preloaded.  cases: [(what, dict of write_case's arguments after the path)].  The runs of a case must agree.  Returns the program's output, a
    line per case; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, f"bmpc_emu_rollout_observer_san{nw}")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", f"-DBMPC_NW={nw}", "-DBMPC_EMU_OBSERVER_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_rollout_observer.cpp")])
        for i, (what, kw) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, **kw)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"{what}: {r.stdout.strip()}")
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized observer rollout, nw {nw}, case {what}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        from tests import test_stream_rollout_observer
        nw = 4 if "4" in sys.argv else 1
        print("\n".join(run_sanitized(test_stream_rollout_observer.sanitizer_cases(nw), nw)))
