"""Test support for closed loops (not a test module): the two reference experiments of fixture G6 as streams, the nlpsol-shaped CPU oracle,
and the CPU mirror of `StreamBatch.closed_loop` -- the g++ build of the stream functions (tests/emu) around the CPU oracle.  The benchmark
streams themselves are `boundmpc_amd.workload.make_streams`."""
import os

import numpy as np

from boundmpc_amd import stream as bstream, workload
from boundmpc_amd.bound_mpc import BoundMPC
from boundmpc_amd.robot_model import RobotModel
from oracle import c_oracle
from tests.emu import emu

G = os.path.join(os.path.dirname(__file__), "golden")


class Oracle:
    """nlpsol-shaped solver backed by the CPU oracle; `fail_at` ticks report failure with a wildly infeasible g."""

    def __init__(self, fail_at=(), N=10, S=4, H=0.1, nthreads=1):
        self.calls, self.fail_at, self.dims, self.nthreads = 0, set(fail_at), (N, S, H), nthreads

    def generate_dependencies(self, *a, **k):
        pass

    def solve(self, p, x0):
        r = c_oracle.solve(p, x0, *self.dims, nthreads=self.nthreads)
        x, g, st = r["x"][0], r["g"][0].copy(), int(r["status"][0])
        if self.calls in self.fail_at:
            g[:] = 1.0; st = 3
        self.calls += 1
        return x, g, st, int(r["iters"][0])

    def __call__(self, x0=None, lbx=None, ubx=None, lbg=None, ubg=None, p=None):
        x, g, st, it = self.solve(np.asarray(p, dtype=float), np.asarray(x0, dtype=float))
        self._st = dict(iter_count=it, success=st == 0, return_status="x")
        return dict(x=x, g=g, lam_g=np.zeros_like(g), lam_x=np.zeros_like(x), f=0.0)

    def stats(self):
        return self._st


def fixture_mpc(which, solver=None, **params):
    """Host `BoundMPC` of reference experiment `which` (1, 2) as fixture G6 recorded its inputs; `params`: other fields of workload.Params."""
    d6 = np.load(os.path.join(G, f"g6_pack_exp{which}_tick0.npz"))
    mk = lambda k: [np.array(v) for v in d6[k]]
    params.setdefault("weights", d6["weights_f64"])
    mpc = BoundMPC(mk("p_via"), mk("r_via"), [mk("p_lower"), mk("p_upper")], [mk("r_lower"), mk("r_upper")], mk("bp1_in"), mk("br1_in"),
                   list(d6["s_in"]), list(d6["e_p_min_in"]), list(d6["e_r_min_in"]), list(d6["e_p_max_in"]), list(d6["e_r_max_in"]),
                   p0=d6["p0fk"].copy(), params=workload.Params(**params), solver=solver if solver is not None else Oracle())
    return mpc, d6


def fixture_robot_record(mpc, d6):
    """Robot record of a reference experiment at rest in its start configuration."""
    q = d6["q0"].copy()
    return bstream.robot_record(q, np.zeros(7), np.zeros(7), RobotModel().forward_kinematics(q, np.zeros(7))[0], np.zeros(6),
                                np.array([mpc.phi_max[0], 0, 0]), np.zeros(7))


def reference_experiment_streams():
    """The sibling of workload.make_streams for the reference's two experiments -> (mpcs [2], robot records [2][RB_LEN], fixtures G6 [2])."""
    ms = [fixture_mpc(which) for which in (1, 2)]
    return [m for m, _ in ms], np.stack([fixture_robot_record(m, d) for m, d in ms]), [d for _, d in ms]


def stream_arrays(mpc, N):
    """(path table, stream state) of a fresh host object, as StreamBatch builds them for one stream."""
    T, M = bstream.path_table(mpc.ref_path)
    ss = bstream.initial_state(mpc, N); ss[bstream.SS["NENT"]] = M
    return T, ss


def cpu_mirror_loop(mpc, rec, ticks, N=10, S=4, H=0.1, solve=None, cap=0, first_cap=100, accept_capped=False, rt_tol=1e-4, level_rule=(0.0, 0.0, 0.0),
                    opts_kw=None):
    """One stream of StreamBatch.closed_loop on the CPU: emu.stream_pack -> solve -> emu.stream_post with the plant simulation, per tick.
    `solve(p, x0) -> (x, g, status, iters)` (an `Oracle().solve`), or the oracle with `opts_kw` and the iteration caps `first_cap` (tick 0) /
    `cap` (later ticks).  accept_capped: the real-time ticks -- dual state and last iterate carried into the pack (with `level_rule`), the capped
    iterates of the ticks after the first judged with `rt_tol`.  Yields after every tick a dict of the tick's arrays; `ss` and `rb` are the
    live stream state and robot record (advanced in place), `q` and `phi` what they held before the pack."""
    T, ss = stream_arrays(mpc, N)
    rb = np.array(rec, dtype=float)
    state = np.zeros((1, c_oracle.state_len(N))) if accept_capped else None
    xlast = None
    for t in range(ticks):
        q, phi = rb[:7].copy(), float(bstream.phi(ss))
        p, x0 = emu.stream_pack(N, S, T, ss, rb, dual=state[0] if accept_capped else None, xlast=xlast, level_rule=level_rule)
        level = float(bstream.level(state[0], N)) if accept_capped else None
        if solve is not None:
            x, g, st, it = solve(p, x0); kkt = np.nan
        else:
            r = c_oracle.solve(p, x0, N, S, H, opts=c_oracle.default_opts(max_iter=cap if t else first_cap, **(opts_kw or {})), nthreads=1, state=state)
            x, g, st, it, kkt = r["x"][0], r["g"][0], int(r["status"][0]), int(r["iters"][0]), float(r["kkt"][0])
        tr = emu.stream_post(N, S, H, T, ss, rb, x, g, st, simulate=True, flags=2 if accept_capped and t else 0, rt_tol=rt_tol)
        if accept_capped:
            xlast = x
        yield dict(t=t, q=q, phi=phi, p=p, x0=x0, x=x, g=g, status=st, iters=it, kkt=kkt, traj=tr, ss=ss, rb=rb, level=level)
