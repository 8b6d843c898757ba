"""TEST-ONLY: the CPU build of the tube measurement (boundmpc_amd/csrc/bmpc_stream_tube.inl through tests/emu/bmpc_emu_stream_tube.cpp) and what the
CPU and the GPU tests of it share: the numpy reference row (boundmpc_amd.stream.tube_excess_of_state and the joint limits), the numpy reduction of
tube rows to an audit record, the parameter vectors of the fixtures and the hand-made rows.

  python -m tests.emu.emu_stream_tube --sanitize    builds bmpc_emu_stream_tube.cpp as a stand-alone program with -fsanitize=address,undefined and
                                                    runs it on the hand-made rows
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden")
TUBE, AUDIT = bstream.TUBE, bstream.AUDIT
# the reference's joint limits (BoundMPC's RobotModel: q_lim_upper, dq_lim_upper), the ones csrc/bmpc_wave.inl qlim() / dqlim() restate
QLIM = np.deg2rad([165.0, 115.0, 165.0, 115.0, 165.0, 115.0, 170.0])
DQLIM = np.deg2rad([85.0, 85.0, 100.0, 75.0, 130.0, 135.0, 135.0])
JOINT_TOL = 1e-9


def lib():
    L = emu._build("libbmpc_emu_stream_tube.so", "bmpc_emu_stream_tube.cpp", (), ("bmpc_stream.inl", "bmpc_stream_tube.inl"))
    assert L.bmpc_emu_stream_tube_len() == bstream.tube_len() and L.bmpc_emu_stream_audit_len() == AUDIT["LEN"]
    return L


def stream_tube(N, S, p, ss=None, want_rc=False, B=None):
    """p [B][141 + 91 S] (or one vector), ss [B][ss_len(N)] or None -> tube rows [B][16] of the CPU build; the return code with want_rc (p = None
    passes NULL, B: the batch size passed instead of the arrays')"""
    p = None if p is None else np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
    ss = None if ss is None else np.ascontiguousarray(np.atleast_2d(ss), dtype=np.float64)
    rows = 1 if p is None else p.shape[0]
    assert p is None or p.shape[1] == 141 + 91 * S
    assert ss is None or ss.shape == (rows, bstream.ss_len(N))
    out = np.zeros((rows, TUBE["LEN"]))
    rc = lib().bmpc_emu_stream_tube(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_int(rows if B is None else B), emu._p(p), emu._p(ss), emu._p(out))
    if want_rc:
        return rc
    assert rc == 0
    return out


def numpy_rows(p, S):
    """the reference row [B][16]: stream.tube_excess_of_state in both of its forms, the joint figures, the segment and phi0"""
    p = np.atleast_2d(np.asarray(p, dtype=float))
    o = bstream._poff(S)
    l, w = bstream.tube_excess_of_state(p, S, rows=True)
    ex_p, ex_r = bstream.tube_excess_of_state(p, S)
    phi, sw = p[:, o["phi0"]], p[:, o["sw"]:o["sw"] + S + 1]
    seg = np.full(len(p), S - 1)
    for i in range(S - 2, -1, -1):
        seg = np.where(phi < sw[:, i + 1], i, seg)
    out = np.zeros((len(p), TUBE["LEN"]))
    out[:, TUBE["L"]:TUBE["L"] + 5], out[:, TUBE["W"]:TUBE["W"] + 5] = l, w
    with np.errstate(invalid="ignore"):
        out[:, TUBE["EX_POS"]], out[:, TUBE["EX_ROT"]] = ex_p.max(axis=1), ex_r.max(axis=1)
        out[:, TUBE["EX_Q"]] = (np.abs(p[:, o["q0"]:o["q0"] + 7]) - QLIM).max(axis=1)
        out[:, TUBE["EX_DQ"]] = (np.abs(p[:, o["dq0"]:o["dq0"] + 7]) - DQLIM).max(axis=1)
    out[:, TUBE["SEG"]], out[:, TUBE["PHI"]] = seg, phi
    return out


GROUPS = {"l": slice(0, 5), "w": slice(5, 10), "excess": slice(10, 12), "joints": slice(12, 14), "phi": slice(15, 16)}


def deviations(got, want):
    """largest abs difference per slot group (NaN slots must be NaN on both sides); SEG is compared exactly"""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN slots differ"
    assert np.array_equal(got[:, TUBE["SEG"]], want[:, TUBE["SEG"]], equal_nan=True), "segments differ"
    with np.errstate(invalid="ignore"):
        return {k: float(np.nanmax(np.abs(got[:, s] - want[:, s]), initial=0.0)) for k, s in GROUPS.items()}


def audit_of(rows, tol):
    """The numpy reduction of the tube rows of ONE stream [T][16] (NaN rows: ticks it did not run) to its audit record [12] (slots AUDIT)."""
    rows = np.asarray(rows, dtype=float)
    run = [t for t in range(len(rows)) if not np.isnan(rows[t, TUBE["SEG"]])]
    a = np.zeros(AUDIT["LEN"])
    a[AUDIT["SAMPLES"]] = len(run)
    a[[AUDIT["TICK_POS"], AUDIT["TICK_ROT"], AUDIT["FIRST_OUT"]]] = -1.0
    a[[AUDIT["MAX_POS"], AUDIT["MAX_ROT"], AUDIT["MAX_Q"], AUDIT["MAX_DQ"]]] = -np.inf
    if not run:
        return a
    r = rows[run]
    for key, tick in (("POS", "TICK_POS"), ("ROT", "TICK_ROT"), ("Q", None), ("DQ", None)):
        ex = r[:, TUBE["EX_" + key]]
        bad = ~np.isfinite(ex)
        first = int(np.argmax(bad)) if bad.any() else int(np.argmax(ex))      # argmax: the first of equal maxima, as the device's `>` keeps it
        a[AUDIT["MAX_" + key]] = np.nan if bad.any() else ex[first]
        if tick:
            a[AUDIT[tick]] = run[first]
    out = lambda key, t: ~np.isfinite(r[:, TUBE[key]]) | (r[:, TUBE[key]] > t)
    op, orot, oj = out("EX_POS", tol), out("EX_ROT", tol), out("EX_Q", JOINT_TOL) | out("EX_DQ", JOINT_TOL)
    a[AUDIT["N_POS"]], a[AUDIT["N_ROT"]], a[AUDIT["N_JOINT"]] = op.sum(), orot.sum(), oj.sum()
    if (op | orot).any():
        a[AUDIT["FIRST_OUT"]] = run[int(np.argmax(op | orot))]
    return a


def audit_of_batch(tube_hist, tol):
    """[T][B][16] -> [B][12]"""
    return np.stack([audit_of(tube_hist[:, b], tol) for b in range(tube_hist.shape[1])])


def g7_p():
    return np.concatenate([np.load(os.path.join(G, f"g7_closedloop_exp{w}.npz"))["p"] for w in (1, 2)])


def g14_p():
    d = np.load(os.path.join(G, "g14_slsqp_closed_loops.npz"))
    return np.concatenate([d[k] for k in sorted(d.files) if k.startswith(("oracle_p_", "slsqp_p_"))])


def g9_p():
    """{(N, S): parameter vectors} of fixture G9 for the other shapes"""
    d = np.load(os.path.join(G, "g9_nlp.npz"))
    return {(N, S): d[f"n{N}s{S}_p"] for N, S in ((3, 2), (5, 3), (4, 5))}


def hand_made(S=4):
    """A g7 parameter vector changed four ways -> dict name -> p: `pos` p0 moved 5 cm along bp1 of its segment, `q` q0[1] = 2.1 (limit 115 degrees),
    `dq` dq0[3] = -1.4 (limit 75 degrees / s), `nan` one NaN in p0; `base` the vector itself."""
    base = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))["p"][40].copy()
    o = bstream._poff(S)
    seg = int(numpy_rows(base, S)[0, TUBE["SEG"]])
    segb = min(seg, S - 2)
    out = {"base": base}
    p = base.copy(); p[o["p0"]:o["p0"] + 3] += 0.05 * np.array([base[o["bp1"] + c * S + segb] for c in range(3)]); out["pos"] = p
    p = base.copy(); p[o["q0"] + 1] = 2.1; out["q"] = p
    p = base.copy(); p[o["dq0"] + 3] = -1.4; out["dq"] = p
    p = base.copy(); p[o["p0"] + 1] = np.nan; out["nan"] = p
    return out


def write_case(path, N, S, p, ss=None):
    """the case file of the stand-alone program (bmpc_emu_stream_tube.cpp with BMPC_EMU_STREAM_TUBE_MAIN)"""
    p = np.ascontiguousarray(np.atleast_2d(p), dtype=np.float64)
    with open(path, "wb") as f:
        np.array([N, S, p.shape[0], 0 if ss is None else 1], dtype=np.float64).tofile(f)
        p.tofile(f)
        if ss is not None:
            np.ascontiguousarray(ss, dtype=np.float64).tofile(f)


def run_sanitized(keep=None):
    """bmpc_emu_stream_tube.cpp with its own main under AddressSanitizer and UndefinedBehaviorSanitizer on exact-size buffers: the hand-made rows at
    (10, 4) without and with state rows (one of them without a plan), the G9 vectors of the other shapes, and vectors of NaN and of huge numbers.
    Returns the program's output lines; raises when the build fails, a run returns non-zero or a sanitizer reports."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep or tmp
        exe = os.path.join(tmp, "bmpc_emu_stream_tube_san")
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-unknown-pragmas",
                               "-Wno-enum-compare", "-DBMPC_EMU_STREAM_TUBE_MAIN", "-o", exe, os.path.join(here, "bmpc_emu_stream_tube.cpp")])
        hm = np.stack(list(hand_made().values()))
        ss = np.zeros((len(hm), bstream.ss_len(10))); ss[1, bstream.SS["ERRCNT"]] = 10
        wild = np.stack([np.full(505, np.nan), np.full(505, 1e300), np.full(505, -1e300), np.full(505, np.inf)])
        cases = [(10, 4, hm, None), (10, 4, hm, ss), (10, 4, wild, None)] + [(N, S, p, None) for (N, S), p in g9_p().items()]
        for i, (N, S, p, s) in enumerate(cases):
            case = os.path.join(tmp, f"case{i}.bin")
            write_case(case, N, S, p, s)
            r = subprocess.run([exe, case], capture_output=True, text=True)
            out.append(f"N {N} S {S} rows {len(p)} state {s is not None}: " + r.stdout.strip().splitlines()[-1])
            if r.returncode != 0 or r.stderr.strip():
                raise RuntimeError(f"sanitized tube measurement, case {i}: exit {r.returncode}\n{r.stdout}\n{r.stderr}")
    return out


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print("\n".join(run_sanitized()))
