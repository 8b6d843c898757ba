"""Test support (not a test module): the acceptance rule of stream_post (boundmpc_amd/csrc/bmpc_stream.inl, phase 0) as a SPECIFICATION in numpy, and the battery
of crafted cases that tests/test_rt_acceptance.py (CPU build, one lane) and tests/test_gpu_rt_acceptance.py (the device, 64 lanes) hold the built rule to.

The specification is written from RobotModel's limits and oracle/nlp.integrate_chain, never from the kernel text.  Given x [N][44], g [N][43], status, the
robot record, flags, rt_tol and row_cap:

    viol  = sum of -v over g[:, :36] with v < -1e-6  +  sum of v over all g with v > 1e-6
    veto  = #non-finite g
    if flags & 2:
      veto += #(g[:, 39:41] > row_cap)                       when row_cap > 0
      veto += #not(-lim-1e-9 <= x[:, :22] <= lim+1e-9)       lim = 35 x 8, qlim, dqlim (the reference's limits, NO bound_margin)
      veto += #not(x[:, 41] >= -1e-9)  +  #non-finite entries of the other unbounded columns
      veto += #(joint j, stage i) whose chain, integrated from rb's q, dq, ddq, jerk with the plan's jerks, is not within |q| <= qlim_j and |dq| <= dqlim_j
    g_viol  = viol + 1e6 * veto
    success = (status == 0 and g_viol < 1e6) or g_viol < rt_tol     if flags & 2
              status == 0 or g_viol < 1e-4                           otherwise

and the consequences (`consequences`): the traj trailer (n_valid, using_previous, success, g_viol), ERRCNT (0 on success, else + 1, and 0 again without a
previous plan), HASPREV, the stored previous plan (x exactly on success, otherwise untouched), the continuation word (1 iff flags bit 1 and status != 3).

ORDER OF THE SUM.  The device adds the terms as 64 strided partial sums and folds them in lane order; numpy adds them in row order.  n non-negative terms
summed in two orders differ by at most about n eps relative: below 2e-13 for the 1 720 terms of N = 40, so g_viol is compared to 1e-12 relative, bit-equal
where at most one term contributes.  No case with more than one term may sit within 1e-10 relative of a threshold (`assert_battery`)."""
import functools

import numpy as np

from boundmpc_amd import stream as bstream, workload
from boundmpc_amd.robot_model import RobotModel
from oracle import nlp

H_, S_ = 0.1, 4
NZ, NG = 44, 43
_RM = RobotModel()
QLIM, DQLIM = np.array(_RM.q_lim_upper), np.array(_RM.dq_lim_upper)
XLIM = np.concatenate([np.full(8, 35.0), QLIM, DQLIM])      # of the stage variables 0:22
UNBOUNDED = np.array([c for c in range(22, NZ) if c != 41])
CLAUSES = ("sum", "cap", "bounds", "chain", "nonfinite")
GROUPS = [(fl, tol, cap) for fl in (1, 3) for tol in (1e-4, 1e-2) for cap in (0.0, 1e-5)]      # what a launch reads from the handle


# ---- the specification ---------------------------------------------------------------------------------------------------------------------
def chain_of(rb, x, N, h=H_):
    """q, dq [N][7] of the joint chains re-integrated from the measured state of the robot record with the plan's jerks"""
    R = bstream.RB
    q, dq, ddq, up = (np.array(rb[R[k]:R[k] + 7], dtype=float) for k in ("Q", "DQ", "DDQ", "JERK"))
    Q, DQ = np.zeros((N, 7)), np.zeros((N, 7))
    for i in range(N):
        u = x.reshape(N, NZ)[i, :7]
        q, dq, ddq = nlp.integrate_chain(q, dq, ddq, up, u, h)
        up = u
        Q[i], DQ[i] = q, dq
    return Q, DQ


def verdict(x, g, status, rb, flags, rt_tol, row_cap, N, h=H_):
    """-> dict: success, g_viol, viol, terms (summed terms), and per clause of CLAUSES its veto count (`sum`: 1 where viol alone reaches the threshold)"""
    x, g = np.asarray(x, dtype=float).reshape(N, NZ), np.asarray(g, dtype=float).reshape(N, NG)
    with np.errstate(invalid="ignore"):
        lo, hi = (g < -1e-6) & (np.arange(NG) < 36), g > 1e-6
        viol = float((-g[lo]).sum() + g[hi].sum())
        n = dict.fromkeys(CLAUSES, 0)
        n["nonfinite"] = int((~np.isfinite(g)).sum())
        if flags & 2:
            if row_cap > 0:
                n["cap"] = int((g[:, 39:41] > row_cap).sum())
            xb = x[:, :22]
            n["bounds"] = int((~((xb <= XLIM + 1e-9) & (xb >= -XLIM - 1e-9))).sum()) + int((~(x[:, 41] >= -1e-9)).sum())
            n["nonfinite"] += int((~np.isfinite(x[:, UNBOUNDED])).sum())
            Q, DQ = chain_of(rb, x, N, h)
            n["chain"] = int((~((Q <= QLIM) & (Q >= -QLIM) & (DQ <= DQLIM) & (DQ >= -DQLIM))).sum())
    veto = sum(n.values())
    g_viol = viol + 1e6 * veto
    thr = rt_tol if flags & 2 else 1e-4
    success = bool((status == 0 and g_viol < 1e6) or g_viol < rt_tol) if flags & 2 else bool(status == 0 or g_viol < 1e-4)
    n["sum"] = int(viol >= thr)
    return dict(success=success, g_viol=g_viol, viol=viol, veto=veto, terms=int(lo.sum() + hi.sum()), clauses=n, threshold=thr)


def consequences(v, ss, x, status, flags, N):
    """what the post leaves behind for the verdict v on the stream state ss (before the post)"""
    S = bstream.SS
    ec, has = int(ss[S["ERRCNT"]]), ss[S["HASPREV"]] > 0.5
    if v["success"]:
        ec, using = 0, 0
    else:
        ec, using = (ec + 1 if has else 0), 1
    return dict(errcnt=ec, hasprev=bool(has or v["success"]), using_previous=using, n_valid=N - ec if ec < N else 0, success=int(v["success"]),
                prev=np.asarray(x, dtype=float).ravel() if v["success"] else ss[S["PREV"]:S["PREV"] + NZ * N].copy(), cont=int(bool(flags & 2) and status != 3))


def assert_consequences(what, c, v, ss_after, traj, N):
    """state row and traj trailer after the post against the specification's; g_viol to 1e-12 relative, bit-equal where at most one term contributes"""
    S = bstream.SS
    got = (traj[-4], traj[-3], traj[-2], ss_after[S["ERRCNT"]], ss_after[S["HASPREV"]] > 0.5, ss_after[bstream.ss_updated(N) + 1])
    want = (c["n_valid"], c["using_previous"], c["success"], c["errcnt"], c["hasprev"], c["cont"])
    assert got == want, (what, got, want, traj[-1], v)
    gv = traj[-1]
    if v["terms"] + v["veto"] <= 1 or not np.isfinite(v["g_viol"]):
        assert gv == v["g_viol"], (what, gv, v["g_viol"])
    else:
        assert abs(gv - v["g_viol"]) <= 1e-12 * v["g_viol"], (what, gv, v["g_viol"])
    assert gv >= v["veto"] * 1e6, (what, gv, v["veto"])
    assert np.array_equal(ss_after[S["PREV"]:S["PREV"] + NZ * N].view(np.uint64), np.ascontiguousarray(c["prev"]).view(np.uint64)), (what, "stored plan")
    return abs(gv - v["g_viol"]) / v["g_viol"] if np.isfinite(v["g_viol"]) and v["g_viol"] > 0 else 0.0


# ---- the base stream -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(N):
    """A stream two accepted ticks into a closed loop with the oracle as solver (stream functions: the CPU build), and the oracle's converged answer to the
    third tick's problem, not yet posted -> dict(mpc, T, ss, rb, x, g, status): nothing counted, nothing vetoed (asserted by `battery`)."""
    from tests.closed_loop import Oracle, stream_arrays
    from tests.emu import emu
    mpcs, recs = workload.make_streams(3, seed=7, N=N, take=2)
    mpc, rb = mpcs[1], recs[1].copy()
    T, ss = stream_arrays(mpc, N)
    sol = Oracle(N=N, nthreads=4)
    for _ in range(2):
        p, x0 = emu.stream_pack(N, S_, T, ss, rb)
        x, g, st, _ = sol.solve(p, x0)
        assert st == 0
        tr = emu.stream_post(N, S_, H_, T, ss, rb, x, g, st, simulate=True, flags=2)
        assert tr[-2] == 1.0
    p, x0 = emu.stream_pack(N, S_, T, ss, rb)
    x, g, st, _ = sol.solve(p, x0)
    assert st == 0
    out = dict(mpc=mpc, T=T, ss=ss, rb=rb, x=x.copy(), g=g.copy(), status=st)
    for a in (T, ss, rb, out["x"], out["g"]):
        a.setflags(write=False)
    return out


# ---- the battery -------------------------------------------------------------------------------------------------------------------------
def _stages(N):
    """the first stage, the last stage, and (N >= 3) stage 2, whose flat indices are >= 64: the second trip of a lane"""
    return sorted({0, N - 1, min(2, N - 1)})


@functools.lru_cache(maxsize=None)
def battery(N):
    """The cases of horizon N: list of dicts (name, x, g, status, rb, ss, flags, rt_tol, row_cap, v = the specification's verdict), each changing one thing
    on one entry of the base stream."""
    b = base(N)
    cases = []
    up, dn = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))

    def add(name, flags=3, rt_tol=1e-4, row_cap=0.0, status=1, gset=(), xset=(), rbset=(), ssset=()):
        x, g, rb, ss = b["x"].reshape(N, NZ).copy(), b["g"].reshape(N, NG).copy(), b["rb"].copy(), b["ss"].copy()
        for (k, i, val) in gset:
            g[k, i] = val
        for (k, i, val) in xset:
            x[k, i] = val
        for (i, val) in rbset:
            rb[i] = val
        for (i, val) in ssset:
            ss[i] = val
        cases.append(dict(name=name, x=x.ravel(), g=g.ravel(), status=status, rb=rb, ss=ss, flags=flags, rt_tol=rt_tol, row_cap=row_cap,
                          v=verdict(x, g, status, rb, flags, rt_tol, row_cap, N)))

    add("base")
    st = _stages(N)
    # -- dead band and sum --
    for k in st:
        for fl in (1, 3):
            add(f"equality row at -1e-6, stage {k}, flags {fl}", flags=fl, gset=[(k, 5, -1e-6)])
            add(f"equality row just beyond -1e-6, stage {k}, flags {fl}", flags=fl, gset=[(k, 5, dn(-1e-6))])
            add(f"equality row at +1e-6, stage {k}, flags {fl}", flags=fl, gset=[(k, 35, 1e-6)])
            add(f"inequality row at -1, stage {k}, flags {fl}", flags=fl, gset=[(k, 37, -1.0)])
            add(f"inequality row at +1e-6, stage {k}, flags {fl}", flags=fl, gset=[(k, 41, 1e-6)])
            add(f"inequality row just above +1e-6, stage {k}, flags {fl}", flags=fl, gset=[(k, 41, up(1e-6))])
        for tol in (1e-4, 1e-2):
            for cap in (0.0, 1e-5):
                add(f"one row at rt_tol {tol:g}, stage {k}, cap {cap:g}", rt_tol=tol, row_cap=cap, gset=[(k, 42, tol)])
                add(f"one row just below rt_tol {tol:g}, stage {k}, cap {cap:g}", rt_tol=tol, row_cap=cap, gset=[(k, 0, -dn(tol))])
        add(f"one row at 1e-4, reference mode, stage {k}", flags=1, rt_tol=1e-2, gset=[(k, 36, 1e-4)])
        add(f"one row just below 1e-4, reference mode, stage {k}", flags=1, rt_tol=1e-2, gset=[(k, 36, dn(1e-4))])
    rng = np.random.default_rng(N)
    for fl, tol, cap in GROUPS:
        thr = tol if fl & 2 else 1e-4
        for fac in (0.5, 2.0):
            rows = [(k, i) for k in range(N) for i in range(NG) if not (cap > 0 and i in (39, 40))]
            n = min(len(rows), int(fac * thr / 2e-6))      # every term clear of the dead band
            pick = [rows[j] for j in np.sort(rng.choice(len(rows), n, replace=False))]
            w = rng.uniform(0.5, 1.5, n)
            w *= fac * thr / w.sum()
            add(f"{n} rows summing to {fac:g} x {thr:g}, flags {fl}, rt_tol {tol:g}, cap {cap:g}", flags=fl, rt_tol=tol, row_cap=cap,
                gset=[(k, i, (-v if i < 36 and (k + i) % 2 else v)) for (k, i), v in zip(pick, w)])
    # -- the last lane of the 64: the entries with flat index 63 + 64 t, which a fold one lane short would lose --
    for idx in range(63, min(NG * N, 64 * 3), 64):
        add(f"last lane: one row of g at 5e-5, flat index {idx}", gset=[(idx // NG, idx % NG, 5e-5 if idx % NG >= 36 else -5e-5)])
        add(f"last lane: one row of g at 2e-4, flat index {idx}", gset=[(idx // NG, idx % NG, 2e-4 if idx % NG >= 36 else -2e-4)])
    for idx in range(63, min(NZ * N, 64 * 12), 64):
        if idx % NZ in range(8, 22):
            add(f"last lane: x at lim + 1e-3, flat index {idx}", xset=[(idx // NZ, idx % NZ, XLIM[idx % NZ] + 1e-3)])
    # -- status --
    for status in (0, 1, 2, 3):
        for fl in (1, 3):
            add(f"status {status}, clean g, flags {fl}", flags=fl, status=status)
            add(f"status {status}, large violation, flags {fl}", flags=fl, status=status, gset=[(st[-1], 3, 0.5)])
            add(f"status {status}, one bound veto, flags {fl}", flags=fl, status=status, xset=[(st[0], 9, QLIM[1] + 1e-3)])
    # -- row cap --
    for k in st:
        for row in (39, 40):
            for fac in (0.5, 2.0):
                add(f"row {row} at {fac:g} x cap, stage {k}", row_cap=1e-5, gset=[(k, row, fac * 1e-5)])
            add(f"row {row} at 2e-5, cap 0, stage {k}", row_cap=0.0, gset=[(k, row, 2e-5)])
            add(f"row {row} at 2 x cap, reference mode, stage {k}", flags=1, row_cap=1e-5, gset=[(k, row, 2e-5)])
            add(f"row {row} at 2 x cap, rt_tol 1e-2, stage {k}", rt_tol=1e-2, row_cap=1e-5, gset=[(k, row, 2e-5)])
        for row in (38, 41, 42):
            add(f"row {row} at 2 x cap, stage {k}", row_cap=1e-5, gset=[(k, row, 2e-5)])
    # -- variable bounds --
    n = 0
    for col in range(22):
        for sign in (1, -1):
            for off in (-1e-9, 5e-10, 2e-9, 1e-3):
                k = N - 1 if col < 7 else st[n % len(st)]; n += 1      # (a joint jerk at its bound moves the re-integrated chain behind it: the last stage moves least)
                fl, tol, cap = GROUPS[4 + n % 4]
                add(f"x column {col} at {'+' if sign > 0 else '-'}(lim {off:+g}), stage {k}", flags=fl, rt_tol=tol, row_cap=cap, xset=[(k, col, sign * (XLIM[col] + off))])
    for k in st:
        for val in (0.0, -5e-10, -2e-9):
            add(f"phi at {val:g}, stage {k}", xset=[(k, 41, val)])
        for bad in (np.nan, np.inf):
            for fl in (1, 3):
                add(f"{bad} in a bounded column, stage {k}, flags {fl}", flags=fl, xset=[(k, 12, bad)])
                add(f"{bad} in an unbounded column, stage {k}, flags {fl}", flags=fl, xset=[(k, 30, bad)])
                add(f"{bad} in g, stage {k}, flags {fl}", flags=fl, gset=[(k, 20, bad)])
        add(f"-inf in an inequality row, stage {k}", gset=[(k, 38, -np.inf)])
        for bad in (np.nan, np.inf, -np.inf):      # reference mode trusts a solver that calls it converged
            for row in (20, 38):
                add(f"{bad} in row {row}, status 0, reference mode, stage {k}", flags=1, status=0, gset=[(k, row, bad)])
    # -- re-integrated chain: the plan inside its own bounds, the measured state moved towards a limit --
    Q, DQ = chain_of(b["rb"], b["x"], N)
    R = bstream.RB
    for var, (traj_, lim, slot, per_u) in enumerate(((Q, QLIM, R["Q"], H_ ** 3 / 24), (DQ, DQLIM, R["DQ"], H_ ** 2 / 6))):
        for j in range(7):
            for sign in (1, -1):
                e = sign * (traj_[:, j] - b["rb"][slot + j])      # excursion of every stage beyond the measured value, towards the limit
                name = f"{'dq' if var else 'q'}{j} {'upper' if sign > 0 else 'lower'}"
                fl, tol, cap = GROUPS[4 + (j + var) % 4]
                kw = dict(flags=fl, rt_tol=tol, row_cap=cap)
                add(f"chain {name}: never leaves", rbset=[(slot + j, sign * (lim[j] - (e.max() + 1e-7)))], **kw)
                add(f"chain {name}: leaves at stage {int(e.argmax())}", rbset=[(slot + j, sign * (lim[j] - (e.max() - 1e-7)))], **kw)
                # the last jerk of the joint moves the last stage only: pushed 2e-7 beyond the largest excursion, where the plan's own jerk bound allows it
                u_last = b["x"].reshape(N, NZ)[N - 1, j] + sign * (e.max() - e[-1] + 2e-7) / per_u
                if abs(u_last) < 34.0:
                    add(f"chain {name}: leaves at the last stage only", rbset=[(slot + j, sign * (lim[j] - (e.max() + 1e-7)))], xset=[(N - 1, j, u_last)], **kw)
                add(f"chain {name}: reference mode does not look", flags=1, rbset=[(slot + j, sign * (lim[j] - (e.max() - 1e-7)))])
    # -- the state before the post: no previous plan, earlier failures --
    S = bstream.SS
    for status, gset in ((1, ()), (1, [(0, 2, 0.5)]), (0, [(0, 2, 0.5)])):
        for fl in (1, 3):
            add(f"no previous plan, status {status}, {'bad' if gset else 'clean'} g, flags {fl}", flags=fl, status=status, gset=gset, ssset=[(S["HASPREV"], 0.0)])
            add(f"two failures before, status {status}, {'bad' if gset else 'clean'} g, flags {fl}", flags=fl, status=status, gset=gset, ssset=[(S["ERRCNT"], 2.0)])
    for c in cases:
        for a in (c["x"], c["g"], c["rb"], c["ss"]):
            a.setflags(write=False)
    return cases


def clause_counts(cases):
    """per clause: (cases in which it ALONE flips the verdict -- rejected with it, accepted by the same rule without it --, cases in which it is present and
    the iterate is accepted all the same)"""
    out = {}
    for cl in CLAUSES:
        flips = present = 0
        for c in cases:
            n = c["v"]["clauses"]
            if n[cl] and not any(n[k] for k in CLAUSES if k != cl):
                if not c["v"]["success"]:
                    flips += 1
            if cl == "sum":
                present += int(c["v"]["terms"] > 0 and c["v"]["success"])
            elif cl == "nonfinite":
                present += int(n[cl] > 0 and c["v"]["success"])
            else:      # the clause's subject is in the case (a capped row above the dead band, a bound within 2e-9, a chain within 1e-6 of a limit) and passes
                present += int(c["v"]["success"] and c["name"].startswith({"cap": ("row 39", "row 40"), "bounds": "x column", "chain": "chain"}[cl]))
        out[cl] = (flips, present)
    return out


def assert_battery(N):
    """the conditions on the battery, on the specification alone"""
    cases = battery(N)
    v0 = cases[0]["v"]
    assert v0["success"] and v0["g_viol"] == 0.0 and v0["terms"] == 0, v0      # the base: nothing counted, nothing vetoed
    counts = clause_counts(cases)
    for cl, (flips, present) in counts.items():
        assert flips >= 4 and present >= 4, (N, cl, flips, present)
    for c in cases:
        v = c["v"]
        if v["terms"] > 1 and np.isfinite(v["g_viol"]):
            for thr in (v["threshold"], 1e6):
                assert abs(v["g_viol"] - thr) > 1e-10 * thr, (c["name"], v)
    by = {c["name"]: c["v"]["success"] for c in cases}
    assert len(by) == len(cases)      # names are ids
    for k in _stages(N):
        for fl in (1, 3):      # the accepted / rejected pairs
            assert by[f"equality row at -1e-6, stage {k}, flags {fl}"] and by[f"equality row just beyond -1e-6, stage {k}, flags {fl}"]
        for tol in (1e-4, 1e-2):
            for cap in (0.0, 1e-5):
                assert not by[f"one row at rt_tol {tol:g}, stage {k}, cap {cap:g}"] and by[f"one row just below rt_tol {tol:g}, stage {k}, cap {cap:g}"]
        assert not by[f"one row at 1e-4, reference mode, stage {k}"] and by[f"one row just below 1e-4, reference mode, stage {k}"]
        for row in (39, 40):
            assert by[f"row {row} at 0.5 x cap, stage {k}"] and not by[f"row {row} at 2 x cap, stage {k}"] and by[f"row {row} at 2e-5, cap 0, stage {k}"]
            assert by[f"row {row} at 2 x cap, reference mode, stage {k}"] and not by[f"row {row} at 2 x cap, rt_tol 1e-2, stage {k}"]
        for row in (38, 41, 42):
            assert by[f"row {row} at 2 x cap, stage {k}"]
        assert by[f"phi at 0, stage {k}"] and by[f"phi at -5e-10, stage {k}"] and not by[f"phi at -2e-09, stage {k}"]
    for fl in (1, 3):
        assert by[f"status 0, large violation, flags {fl}"] and not by[f"status 1, large violation, flags {fl}"]
    assert by["status 0, one bound veto, flags 1"] and not by["status 0, one bound veto, flags 3"]
    for name, ok in by.items():
        if name.startswith("x column") and not next(c for c in cases if c["name"] == name)["v"]["clauses"]["chain"]:
            assert ok == (not name.split("(lim ")[1].startswith(("+2e-09", "+0.001"))), name
        if name.startswith("chain q"):      # (a moved dq_j also carries q_j away, by (i + 1) h per stage: the specification decides those)
            assert ok == name.endswith(("never leaves", "does not look")), name
    return counts
