"""ONE and THREE iterations of the shipped kernels from points far from a solution, on every launch shape, against the CPU lane emulator of the
same wave count (and the C oracle where its option record covers the case).  A converged solve hides a slightly wrong Newton direction (it
converges to the same point in about the same number of iterations); one step of size 0.3 .. 18 from a far-off point does not: the CPU builds
agree on it to 1e-12 of the step.  What only the GPU executes -- the MFMA Schur update, the butterfly reductions, the per-wave folds of teams,
the register allocation around the prefetch registers -- is compared here four to five decades tighter than at a KKT point.

INPUTS.  B = 8 problems of workload.make_batch(seed=3) per (N, S); x0 = the cold start + N(0, 0.05) noise on every variable; the dual state seeded
with nu = 10^U(-6, 2), mu = 0.05; solve_batch(p, x0, state=..., max_iter=K), K = 1 and 3: status 1 on every row.

TOLERANCE (measured on the CPU, never from the GPU's output).  Differences in x are taken relative to the row's max |x - x0| (the step), in nu
relative to the row's max |nu|.  The FLOOR of a shape and K is the oracle-versus-emulator discrepancy on the same rows: two CPU implementations
of the same iteration with different summation orders.  The GPU must agree with the emulator within FACTOR = 100 x floor: FMA contraction, the
accumulation order of the matrix cores, the butterfly order.  The bound_margin shapes take their own floor like every other: the oracle's option
record carries the margin (oracle/bmpc_oracle.c eval).  On these inputs the CPU builds take the same accept / reject decisions on every row (equal iteration counts;
the team and pair emulators equal the one-wave emulator bit for bit): asserted below, on the CPU, before any GPU result is looked at.

THE RESTORATION PHASE'S STEP (last test): set A of tests/entry_path_sets.py, restoration mode 1, one short step counts as a jam, iteration
caps K* and K* + 1 where K* <= 8 is the smallest cap at which at least 4 rows of the emulator differ between mode 1 and mode 0 -- those rows have
taken an elastic-row step; on the GPU the batch kernel has handed them to the restoration kernel with status 4.

tests/newton_step_profile.py --gpu appends the observed GPU discrepancies per shape to profiles/newton_step.txt."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from tests import entry_path_sets as eps
from tests.emu import emu

pytestmark = pytest.mark.gpu

B, H_, FACTOR = 8, 0.1, 100.0
KS = (1, 3)
# name -> N, S, set_team_waves (None: the handle's own choice), waves team_info must report, emulator (1, 4, "pair"), options (handle keyword = field
# of both option records unless noted), oracle covers the options
SHAPES = {
    "one_wave_N10":        dict(N=10, S=4, waves=1, nw=1),
    "pair_N1":             dict(N=1, S=4, waves=2, nw="pair"),
    "pair_N2":             dict(N=2, S=4, waves=2, nw="pair"),
    "pair_N10":            dict(N=10, S=4, waves=2, nw="pair"),
    "pair_N11":            dict(N=11, S=4, waves=2, nw="pair"),
    "team_N3":             dict(N=3, S=4, waves=4, nw=4),
    "team_N10":            dict(N=10, S=4, waves=4, nw=4),
    "slab_N12":            dict(N=12, S=4, waves=None, nw=1),
    "slab_N6_S5_resto1":   dict(N=6, S=5, waves=None, nw=1, opts=dict(restoration=1)),      # the restoration instantiation as the batch kernel
    "slab_N6_S5_resto2":   dict(N=6, S=5, waves=None, nw=1, opts=dict(restoration=2)),
    "gauss_newton_one":    dict(N=10, S=4, waves=1, nw=1, opts=dict(exact_hessian=0)),
    "gauss_newton_team":   dict(N=10, S=4, waves=4, nw=4, opts=dict(exact_hessian=0)),
    "bound_margin_one":    dict(N=10, S=4, waves=1, nw=1, opts=dict(bound_margin=0.05)),
    "bound_margin_pair":   dict(N=10, S=4, waves=2, nw="pair", opts=dict(bound_margin=0.05)),
    "bound_margin_team":   dict(N=10, S=4, waves=4, nw=4, opts=dict(bound_margin=0.05)),
}


@functools.lru_cache(maxsize=None)
def inputs(N, S):
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(B, seed=3, N=N, S=S, workers=1)
    rng = np.random.default_rng(3)
    x0 = X + rng.normal(size=X.shape) * 0.05
    st = np.zeros((B, c_oracle.state_len(N)))
    st[:, :N * 57] = 10.0 ** rng.uniform(-6, 2, (B, N * 57)); st[:, N * 57] = 0.05
    for a in (P, x0, st):
        a.setflags(write=False)
    return P, x0, st


def rel_x(x, ref, x0):
    """largest difference of a row relative to the row's step max |ref - x0| -> [B]"""
    return np.abs(x - ref).max(axis=1) / np.abs(ref - x0).max(axis=1)


def rel_nu(st, ref, N):
    return np.abs(st[:, :N * 57] - ref[:, :N * 57]).max(axis=1) / np.abs(ref[:, :N * 57]).max(axis=1)


def _emu_solve(nw, P, x0, N, S, opts, state=None):
    if nw == 1:
        return emu.solve(P, x0, N, S, H_, opts=opts, nthreads=4, state=state)
    return emu.solve_team(P, x0, N, S, H_, nw=nw, opts=opts, nthreads=4, state=state)


@functools.lru_cache(maxsize=None)
def cpu_side(name, K):
    """The emulator of the shape's wave count on the shape's inputs (x, state, iters, status), the floors of x and nu (oracle versus emulator), and
    the CPU-side facts the comparison rests on: status 1 after exactly K iterations on every row of both builds, team / pair == one wave bit for bit."""
    sh = SHAPES[name]
    N, S, kw = sh["N"], sh["S"], sh.get("opts", {})
    P, x0, st0 = inputs(N, S)
    se = st0.copy()
    e = _emu_solve(sh["nw"], P, x0, N, S, emu.opts_for(N, max_iter=K, **kw), se)
    assert (e["status"] == 1).all() and (e["iters"] == K).all(), (name, K, e["status"], e["iters"])
    if sh["nw"] != 1:
        s1 = st0.copy()
        one = emu.solve(P, x0, N, S, H_, opts=emu.opts_for(N, max_iter=K, **kw), nthreads=4, state=s1)
        assert np.array_equal(one["x"], e["x"]) and np.array_equal(s1, se) and np.array_equal(one["iters"], e["iters"]), (name, K)
    out = dict(x=e["x"], state=se, iters=e["iters"], status=e["status"], step=np.abs(e["x"] - x0).max(axis=1))
    so = st0.copy()
    o = c_oracle.solve(P, x0, N, S, H_, opts=c_oracle.opts_for(N, max_iter=K, **kw), nthreads=4, state=so)
    assert (o["status"] == 1).all() and (o["iters"] == K).all(), (name, K, o["status"], o["iters"])
    assert np.array_equal(so[:, N * 57 + 1], se[:, N * 57 + 1])
    out.update(floor_x=float(rel_x(o["x"], e["x"], x0).max()), floor_nu=float(rel_nu(so, se, N).max()),
               floor_mu=float(np.abs(so[:, N * 57] / se[:, N * 57] - 1).max()), oracle=dict(x=o["x"], state=so))
    return out


def _handle(name, **more):
    from boundmpc_amd import BatchedOCPSolver
    sh = SHAPES[name]
    kw = dict(sh.get("opts", {}))
    if "exact_hessian" in kw:
        kw["exact_hessian"] = bool(kw["exact_hessian"])
    s = BatchedOCPSolver(sh["N"], sh["S"], H_, **kw, **more)
    if sh["waves"] is not None:
        s.set_team_waves(sh["waves"])
    assert s.team_info(B)["waves"] == (sh["waves"] or 1), (name, s.team_info(B))
    return s


def gpu_side(name, K, s):
    """solve_batch(state, max_iter=K) on the shape's inputs, twice -> (x, state, iters, status) as numpy, and whether the second launch gave the same bits"""
    import torch
    sh = SHAPES[name]
    P, x0, st0 = inputs(sh["N"], sh["S"])
    p, x = torch.tensor(P, device="cuda"), torch.tensor(x0, device="cuda")
    runs = []
    for _ in range(2):
        st = torch.tensor(st0, device="cuda")
        o = s.solve_batch(p, x, state=st, max_iter=K, out={})
        torch.cuda.synchronize()
        runs.append((o["x"].cpu().numpy(), st.cpu().numpy(), o["iters"].cpu().numpy(), o["status"].cpu().numpy()))
    return runs[0], all(np.array_equal(a, b) for a, b in zip(*runs))


def measure(name, K, s):
    """the GPU's discrepancies against the emulator (and the oracle) with the CPU floors -> dict; asserts nothing"""
    sh = SHAPES[name]
    N = sh["N"]
    _, x0, _ = inputs(N, sh["S"])
    c = cpu_side(name, K)
    (x, st, it, status), same = gpu_side(name, K, s)
    m = dict(name=name, K=K, floor_x=c["floor_x"], floor_nu=c["floor_nu"], step_min=float(c["step"].min()), step_max=float(c["step"].max()),
             x=float(rel_x(x, c["x"], x0).max()), nu=float(rel_nu(st, c["state"], N).max()), mu=float(np.abs(st[:, N * 57] / c["state"][:, N * 57] - 1).max()),
             count_equal=bool(np.array_equal(st[:, N * 57 + 1], c["state"][:, N * 57 + 1])), iters_equal=bool(np.array_equal(it, c["iters"])),
             status_equal=bool(np.array_equal(status, c["status"])), repeat_equal=bool(same), gpu_x=x)
    if c["oracle"] is not None:
        m.update(x_oracle=float(rel_x(x, c["oracle"]["x"], x0).max()), nu_oracle=float(rel_nu(st, c["oracle"]["state"], N).max()))
    return m


def line_of(m):
    return (f"{m['name']} K={m['K']}: step {m['step_min']:.2f}..{m['step_max']:.2f} floor_x = {m['floor_x']:.3e} gpu_x = {m['x']:.3e} floor_nu = {m['floor_nu']:.3e} "
            f"gpu_nu = {m['nu']:.3e} gpu_mu = {m['mu']:.3e}" + (f" gpu_x_vs_oracle = {m['x_oracle']:.3e} gpu_nu_vs_oracle = {m['nu_oracle']:.3e}" if "x_oracle" in m else ""))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_capped_solve_from_a_far_point_equals_the_emulator_within_the_cpu_floor(name, K):
    c = cpu_side(name, K)      # (asserts the CPU-side facts first)
    assert 0 < c["floor_x"] < 1e-9 and 0 < c["floor_nu"] < 1e-9, (c["floor_x"], c["floor_nu"])      # the floors resolve what they are for
    assert c["step"].min() > 0.1, c["step"]      # every row takes a step worth the name
    s = _handle(name)
    try:
        m = measure(name, K, s)
    finally:
        s.close()
    print("\n" + line_of(m))
    assert m["status_equal"] and m["iters_equal"] and m["count_equal"], m
    assert m["x"] <= FACTOR * m["floor_x"], line_of(m)
    assert m["nu"] <= FACTOR * m["floor_nu"], line_of(m)
    assert m["mu"] <= FACTOR * max(m["floor_nu"], m["floor_x"]), line_of(m)      # (one number per row, a function of the same reductions)
    if "x_oracle" in m:      # two sides, each within 100 floors of the emulator, one floor apart
        assert m["x_oracle"] <= (FACTOR + 1) * m["floor_x"] and m["nu_oracle"] <= (FACTOR + 1) * m["floor_nu"], line_of(m)
    if SHAPES[name]["nw"] != 1:
        assert m["repeat_equal"], name      # pairs and teams: a second launch gives the same bits


@pytest.mark.parametrize("name,one", [("team_N10", "one_wave_N10"), ("pair_N10", "one_wave_N10"), ("gauss_newton_team", "gauss_newton_one")])
def test_team_and_pair_step_equals_the_one_wave_kernels(name, one):
    """x after ONE iteration of the multi-wave kernels against the one-wave kernel's on the same rows, within the same tolerance (on the CPU the
    two are bit-equal: cpu_side asserts it)."""
    c = cpu_side(name, 1)
    _, x0, _ = inputs(SHAPES[name]["N"], SHAPES[name]["S"])
    xs = []
    for n in (name, one):
        s = _handle(n)
        try:
            xs.append(gpu_side(n, 1, s)[0][0])
        finally:
            s.close()
    d = float(rel_x(xs[0], xs[1], x0).max())
    print(f"\n{name} vs {one}, K=1: {d:.3e} (floor {c['floor_x']:.3e})")
    assert d <= FACTOR * c["floor_x"], (d, c["floor_x"])


# ---- the restoration phase's step --------------------------------------------------------------------------------------------------------
RESTO_KW = dict(restoration=1, resto_short=1, start_rollout=0)


@functools.lru_cache(maxsize=None)
def resto_rows():
    """(K*, rows): the smallest cap K* <= 8 at which at least 4 rows of set A differ between restoration mode 1 and mode 0 on the one-wave emulator
    (short_steps = 1, x0 as given), and those rows.  Set A suffices (no widening to set D or to noise 0.3 was needed): asserted."""
    P, X, N, S, dt = eps.problem_set("A")
    for K in range(1, 9):
        a = emu.solve(P, X, N, S, dt, opts=emu.default_opts(max_iter=K, **RESTO_KW), nthreads=8)
        b = emu.solve(P, X, N, S, dt, opts=emu.default_opts(max_iter=K, **{**RESTO_KW, "restoration": 0}), nthreads=8)
        rows = np.flatnonzero((a["x"] != b["x"]).any(axis=1))
        if len(rows) >= 4:
            return K, rows
    raise AssertionError("no cap <= 8 at which 4 rows of set A have taken a restoration step")


@functools.lru_cache(maxsize=None)
def resto_cpu(nw, K):
    """emulator of the wave count and oracle on the rows of resto_rows() with the cap K -> emulator outputs and the floor of x"""
    P, X, N, S, dt = eps.problem_set("A")
    _, rows = resto_rows()
    P, X = np.ascontiguousarray(P[rows]), np.ascontiguousarray(X[rows])
    e = _emu_solve(nw, P, X, N, S, emu.default_opts(max_iter=K, **RESTO_KW))
    o = c_oracle.solve(P, X, N, S, dt, opts=c_oracle.default_opts(max_iter=K, **RESTO_KW), nthreads=8)
    assert np.array_equal(e["iters"], o["iters"]) and np.array_equal(e["status"], o["status"]), (nw, K, e["iters"], o["iters"], e["status"], o["status"])
    return dict(P=P, X=X, x=e["x"], iters=e["iters"], status=e["status"], floor_x=float(rel_x(o["x"], e["x"], X).max()))


def measure_resto(waves, nw, K):
    import torch
    from boundmpc_amd import BatchedOCPSolver
    c = resto_cpu(nw, K)
    s = BatchedOCPSolver(10, 4, H_, max_iter=K, start_rollout=False, restoration=1, resto_short=1)
    try:
        s.set_team_waves(waves)
        assert s.team_info(len(c["P"]))["waves"] == waves
        o = s.solve_batch(torch.tensor(c["P"], device="cuda"), torch.tensor(c["X"], device="cuda"), out={})
        torch.cuda.synchronize()
        x, it, st = o["x"].cpu().numpy(), o["iters"].cpu().numpy(), o["status"].cpu().numpy()
    finally:
        s.close()
    return dict(waves=waves, K=K, rows=len(c["P"]), floor_x=c["floor_x"], x=float(rel_x(x, c["x"], c["X"]).max()), iters_equal=bool(np.array_equal(it, c["iters"])),
                status_equal=bool(np.array_equal(st, c["status"])), statuses=eps.counts(c["status"]))


def resto_line_of(m):
    return f"restoration waves={m['waves']} K={m['K']}: rows {m['rows']} emulator statuses {m['statuses']} floor_x = {m['floor_x']:.3e} gpu_x = {m['x']:.3e}"


@pytest.mark.parametrize("dK", [0, 1])
@pytest.mark.parametrize("waves,nw", [(1, 1), (2, "pair"), (4, 4)])
def test_restoration_step_behind_the_hand_over_equals_the_emulator(waves, nw, dK):
    Ks, rows = resto_rows()
    m = measure_resto(waves, nw, Ks + dK)
    print(f"\nK* = {Ks}, rows {rows.tolist()}\n" + resto_line_of(m))
    assert 0 < m["floor_x"] < 1e-9, m["floor_x"]
    assert m["iters_equal"] and m["status_equal"], m
    assert m["x"] <= FACTOR * m["floor_x"], resto_line_of(m)
