"""The rollout -- many closed-loop ticks of a stream in one launch -- as device code (csrc/bmpc_rollout_kernel.inl compiled for the CPU, tests/emu)
against its exact checker: a loop of the fused tick's own kernel text (csrc/bmpc_tick_kernel.inl compiled for the CPU, emu.stream_tick), one tick at
a time (tests/emu/emu_rollout.py contract_loop; tests/test_stream_tick.py holds that text to the separate pack, solve and post).  Bit for bit on every tick array, `hist` and `traj_hist` against the per-tick values,
and the stop rules: a lost plan, the goal.  Every case asserts that each stream ran at least one tick."""
import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er

SS, ROLL = bstream.SS, bstream.ROLL
H = 0.1


def _loop(N, S, T, A, ticks, **kw):
    """`ticks` fused ticks, one after the other -> (rows [ticks][52] with NaN rows for skipped ticks, traj rows, snapshots of the arrays behind every tick)"""
    loop = er.contract_loop(N, S, H, T, A, ticks, **kw)
    return loop["hist"], loop["traj_hist"], loop["snaps"]


def _compare(N, S, T, A0, ticks, what, goal_tol=0.0, **kw):
    """rollout(ticks) on a copy of the arrays A0 against `ticks` single ticks on another; returns (rollout result, its arrays, per-tick rows, snapshots)"""
    A, B = er.copy_arrays(A0), er.copy_arrays(A0)
    rows, trajs, snaps = _loop(N, S, T, A, ticks, **kw)
    r = er.rollout(N, S, H, T, B, ticks, goal_tol=goal_tol, **kw)
    assert r["ticks_run"] >= 1, what
    if goal_tol == 0.0:
        er.assert_arrays_equal(A, B, what)
        assert r["ticks_run"] == int(np.isfinite(rows[:, ROLL["STATUS"]]).sum()), what
        assert np.array_equal(r["hist"], rows, equal_nan=True) and np.array_equal(r["traj_hist"], trajs, equal_nan=True), what
    return r, B, rows, snaps


@pytest.mark.parametrize("N,S", [(2, 2), (1, 2)])
def test_rollout_equals_the_per_tick_loop_bit_for_bit(N, S):
    """T = 4 converged ticks with the dual state carried, from the cold start; every tick runs."""
    _, rec, T, ss = er.small_stream(N, S)
    r, B, rows, _ = _compare(N, S, T, er.fresh_arrays(N, S, ss, rec), 4, f"N {N} S {S}", warm_dual=True)
    assert r["ticks_run"] == 4 and np.isfinite(r["hist"]).all() and (r["hist"][:, ROLL["STATUS"]] == 0).all()
    assert (np.diff(r["hist"][:, ROLL["PHI"]]) > 0).all()                   # the plant moves: a second tick does not repeat the first
    # the history row: the robot record and the named scalars of the arrays behind the last tick, the trailer of its trajectory record
    last = bstream.unpack_rollout(r["hist"][3])
    assert np.array_equal(last["q"], B["rb"][:7]) and np.array_equal(last["jerk"], B["rb"][36:43]) and last["phi"] == B["ss"][SS["PHI"]]
    assert last["iters"] == B["iters"][0] > 0 and last["status"] == 0 and last["kkt"] == B["kkt"][0] and last["error_count"] == 0
    _, fl = bstream.unpack_traj(B["traj"], N)
    assert (last["n_valid"], last["using_previous"], last["success"], last["g_viol"]) == (fl["n_valid"], fl["using_previous"], fl["success"], fl["g_viol"])
    assert np.array_equal(r["traj_hist"][3], B["traj"])


def test_rollout_without_the_dual_state_and_in_any_lane_order():
    """cold duals on every tick (dual_state NULL), and the solver's phases with their lanes reversed and scrambled: the same bits"""
    N, S = 2, 2
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    r, B, _, _ = _compare(N, S, T, A0, 4, "cold duals", warm_dual=False)
    assert r["ticks_run"] == 4 and (B["dual"] == 0.0).all()
    ref = er.copy_arrays(A0); want = er.rollout(N, S, H, T, ref, 4, warm_dual=True)
    for order in (1, 2):
        C = er.copy_arrays(A0); got = er.rollout(N, S, H, T, C, 4, warm_dual=True, lane_order=order)
        er.assert_arrays_equal(ref, C, f"lane order {order}")
        assert np.array_equal(got["hist"], want["hist"])


def test_one_tick_rollout_equals_one_tick():
    N, S = 2, 2
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    r, _, _, _ = _compare(N, S, T, A0, 1, "T = 1", warm_dual=True)
    assert r["ticks_run"] == 1 and r["hist"].shape == (1, ROLL["LEN"])
    warm = er.copy_arrays(A0); er.tick(N, S, H, T, warm, warm_dual=True)      # ... and one tick of a stream that already holds a plan
    r, _, _, _ = _compare(N, S, T, warm, 1, "T = 1, warm", warm_dual=True)
    assert r["ticks_run"] == 1


def test_a_stream_that_loses_its_plan_stops():
    """Tick 0 solved out, then two iterations per tick without the real-time rule: every capped iterate fails the reference's acceptance rule, the error
    count climbs to N and the stream stops.  At (10, 4): the two-iteration ticks of the smallest shape stay feasible (summed violation 0) and never fail."""
    N, S, ticks = 10, 4, 13                                               # T > N + 1
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    er.tick(N, S, H, T, A0, max_iter=100, warm_dual=True)
    assert A0["status"][0] == 0 and A0["ss"][SS["ERRCNT"]] == 0
    r, B, rows, snaps = _compare(N, S, T, A0, ticks, "lost plan", max_iter=2, warm_dual=True)
    ec = rows[:, ROLL["ERRCNT"]]
    implied = int(np.argmax(ec >= N)) + 1                                  # the tick that raises the error count to N is the last one run
    assert (ec >= N).any() and 1 <= implied < ticks and r["ticks_run"] == implied
    assert np.array_equal(ec[:implied], np.arange(1, implied + 1)) and (rows[:implied, ROLL["STATUS"]] == 1).all()
    assert np.isnan(r["hist"][implied:]).all() and np.isnan(r["traj_hist"][implied:]).all() and np.isfinite(r["hist"][:implied]).all()
    assert B["status"][0] == 3 and B["iters"][0] == 0 and B["kkt"][0] == 0.0 and B["ss"][SS["ERRCNT"]] == N
    # everything else keeps its last value: the arrays behind the last tick that ran, but for the three words above
    keep = er.copy_arrays(snaps[implied - 1]); keep["status"][0], keep["iters"][0], keep["kkt"][0] = 3, 0, 0.0
    er.assert_arrays_equal(keep, B, "behind the stop")
    # lost on entry: no tick, all rows NaN, the same three words
    C = er.copy_arrays(B); C["status"][0], C["iters"][0], C["kkt"][0] = 7, 7, 7.0
    r2 = er.rollout(N, S, H, T, C, 3, max_iter=2, warm_dual=True)
    assert r2["ticks_run"] == 0 and np.isnan(r2["hist"]).all() and np.isnan(r2["traj_hist"]).all()
    er.assert_arrays_equal(B, C, "lost on entry")


def test_a_stream_stops_at_its_goal():
    """goal_tol from the per-tick loop's own phi trace, so that the stop falls strictly inside the T ticks on the reference path alone: ticks_run is
    the first crossing and the state is that of the per-tick loop stopped there."""
    N, S, ticks = 2, 2, 4
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    A = er.copy_arrays(A0)
    rows, trajs, snaps = _loop(N, S, T, A, ticks, warm_dual=True)
    gap = A0["ss"][SS["PHIMAX"]] - rows[:, ROLL["PHI"]]
    assert (np.diff(gap) < 0).all()
    goal_tol = float(gap[1])                                               # reached behind tick 1, not behind tick 0
    first = int(np.argmax(gap <= goal_tol)) + 1
    assert first == 2 < ticks
    B = er.copy_arrays(A0)
    r = er.rollout(N, S, H, T, B, ticks, goal_tol=goal_tol, warm_dual=True)
    assert r["ticks_run"] == first
    er.assert_arrays_equal(snaps[first - 1], B, "stopped at the goal")
    assert np.array_equal(r["hist"][:first], rows[:first]) and np.array_equal(r["traj_hist"][:first], trajs[:first])
    assert np.isnan(r["hist"][first:]).all() and np.isnan(r["traj_hist"][first:]).all()
    C = er.copy_arrays(A0)                                                 # a tolerance nobody reaches stops nobody
    assert er.rollout(N, S, H, T, C, ticks, goal_tol=float(gap[-1]) * 0.5, warm_dual=True)["ticks_run"] == ticks
    er.assert_arrays_equal(A, C, "goal never reached")


def test_argument_errors_of_the_entry():
    """what the C ABI refuses, on the entry of the CPU build (the time budget lives on a handle: tests/test_gpu_stream_rollout.py)"""
    N, S = 2, 2
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    for kw in (dict(ticks=0), dict(ticks=-1), dict(ticks=2, simulate=False), dict(ticks=2, goal_tol=-1e-3), dict(ticks=2, goal_tol=np.nan), dict(ticks=2, goal_tol=np.inf)):
        A = er.copy_arrays(A0)
        assert er.rollout(N, S, H, T, A, warm_dual=True, want_rc=True, **kw) == 1, kw
        er.assert_arrays_equal(A0, A, f"{kw}: nothing runs")
    assert er.rollout(N, S, H, T, er.copy_arrays(A0), ticks=2, warm_dual=True, want_rc=True) == 0


def test_history_slots_and_unpack():
    assert bstream.rollout_len() == ROLL["LEN"] == 52 and ROLL["PHI"] == bstream.RB["LEN"] == 43
    assert [ROLL[k] for k in ("ROBOT", "PHI", "ERRCNT", "ITERS", "STATUS", "KKT", "NVALID", "USINGPREV", "SUCCESS", "GVIOL")] == [0] + list(range(43, 52))
    row = np.arange(52, dtype=float)
    d = bstream.unpack_rollout(row)
    assert d["q"].tolist() == list(range(7)) and d["p"].tolist() == list(range(21, 27)) and d["x_phi_d"].tolist() == [33, 34, 35] and d["jerk"].tolist() == list(range(36, 43))
    assert (d["phi"], d["error_count"], d["iters"], d["status"], d["kkt"], d["n_valid"], d["g_viol"]) == (43.0, 44, 45, 46, 47.0, 48, 51.0)
    assert bstream.unpack_rollout(np.full(52, np.nan)) is None


def test_the_entry_rule_of_the_library():
    """The rule of csrc/bmpc_args.h bmpc_rollout_level -- which the C ABI's four entries and the CPU build both ask -- walked through the CPU build's entry
    at (2, 2), B = 1, one tick: entry x arrays given x fault -> the level that runs, or a refusal ("R").  An entry is handed only what it has an argument
    for.  The table is written out from the rule: entry 0 runs level 0 whatever else; entry 1 runs level 1; entry 2 runs 2 with an audit array, else 1, and
    refuses a bad audit_tol either way; entry 3 runs 3 with a log array (and only then looks at log_stages), else it is entry 2; every entry above 0
    refuses a record buffer without its ticks."""
    R = "R"
    table = {  # arrays: (good, audit_tol = -1, log_stages = 0, replan without replan_tick)
        0: {"none": (0, 0, 0, 0), "audit": (0, 0, 0, 0), "log": (0, 0, 0, 0)},
        1: {"none": (1, 1, 1, R), "audit": (1, 1, 1, R), "log": (1, 1, 1, R)},
        2: {"none": (1, R, 1, R), "audit": (2, R, 2, R), "log": (1, R, 1, R)},
        3: {"none": (1, R, 1, R), "audit": (2, R, 2, R), "log": (3, R, R, R)},
    }
    N, S = 2, 2
    _, A0, Tab, recs = er.small_batch(N, S, B=1)
    for entry, rows in table.items():
        for arrays, want in rows.items():
            for fault, level in zip(("good", "audit_tol", "log_stages", "replan"), want):
                kw = dict(audit=arrays == "audit" and entry >= 2, want_tube=arrays == "audit" and entry >= 2, want_log=arrays == "log" and entry >= 3,
                          track=arrays == "log" and entry >= 3, audit_tol=-1.0 if fault == "audit_tol" else 1e-6, log_stages=0 if fault == "log_stages" else 1,
                          replan=recs.copy() if fault == "replan" and entry >= 1 else None)
                A = er.copy_arrays(A0)
                if level == R:
                    assert er.rollout(N, S, H, Tab.copy(), A, 1, entry=entry, want_rc=True, **kw) == 1, (entry, arrays, fault)
                    for k in A:
                        assert np.array_equal(A[k], A0[k], equal_nan=True), (entry, arrays, fault, k)
                else:
                    r = er.rollout(N, S, H, Tab.copy(), A, 1, entry=entry, **kw)
                    assert r["ran"] == level and r["ticks_run"].tolist() == [1], (entry, arrays, fault)


def test_the_entry_choice_of_the_python_layer_is_the_table():
    """stream.rollout_entry -- the one place StreamBatch.rollout picks its C ABI entry, which decides the kernel that runs -- against the table, first row
    that holds, over every combination of the ten presence flags that the argument checks of rollout pass (replan and replan_tick together, and neither
    with legs, tune or plant); and how many combinations each entry serves, counted by hand: of 256 without and 32 with a scheduled record."""
    import itertools
    from boundmpc_amd import _lib
    table = [(lambda f: f["plant"], "bmpc_stream_rollout_plant"),
             (lambda f: f["tune"], "bmpc_stream_rollout_tuned"),                                                    # with or without legs
             (lambda f: f["legs"], "bmpc_stream_rollout_legs"),
             (lambda f: not any(f[k] for k in ("replan", "replan_tick", "disturb", "audit", "want_tube", "want_log", "track")), "bmpc_stream_rollout"),
             (lambda f: f["want_log"] or f["track"], "bmpc_stream_rollout_log"),
             (lambda f: f["audit"] or f["want_tube"], "bmpc_stream_rollout_audit"),
             (lambda f: True, "bmpc_stream_rollout_events")]
    names = ("replan", "replan_tick", "disturb", "audit", "want_tube", "want_log", "track", "legs", "tune", "plant")
    served = {}
    for bits in itertools.product((False, True), repeat=len(names)):
        f = dict(zip(names, bits))
        if f["replan"] != f["replan_tick"] or (f["replan"] and (f["legs"] or f["tune"] or f["plant"])):
            continue
        want = next(entry for holds, entry in table if holds(f))
        assert bstream.rollout_entry(**f) == want, f
        served[want] = served.get(want, 0) + 1
    assert served == {"bmpc_stream_rollout_plant": 128, "bmpc_stream_rollout_tuned": 64, "bmpc_stream_rollout_legs": 32, "bmpc_stream_rollout": 1,
                      "bmpc_stream_rollout_log": 48, "bmpc_stream_rollout_audit": 12, "bmpc_stream_rollout_events": 3}
    assert bstream.ROLLOUT_ENTRIES == tuple(sorted(served, key=lambda e: len(_lib.SIGNATURES[e][1]))) and bstream.rollout_entry() == bstream.ROLLOUT_ENTRIES[0]


@pytest.mark.parametrize("nw", [1, 4])
def test_the_rargs_mirror_is_the_librarys_record(nw):
    """emu_rollout.RArgs, the ctypes record the one entry of the CPU build takes, against csrc/bmpc_args.h RArgs: the members the header declares, in its
    order, and the size and every offset as the build lays the record out -- a new member is one field there and one here, and no argument position"""
    import ctypes
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "boundmpc_amd", "csrc", "bmpc_args.h")).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"struct RArgs \{(.*?)\n\};", text, re.S).group(1))
    declared = [name.strip(" *\n") for decl in body.split(";") if decl.strip() for name in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",")]
    names = [n for n, _ in er.RArgs._fields_]
    assert names == declared and len(names) == 30
    L = er.lib(nw)
    assert L.bmpc_emu_rargs_size() == ctypes.sizeof(er.RArgs)
    assert [L.bmpc_emu_rargs_offset(n.encode()) for n in names] == [getattr(er.RArgs, n).offset for n in names]
    assert L.bmpc_emu_rargs_offset(b"no_such_member") == -1
