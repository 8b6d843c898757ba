"""GPU: the fused tick (bmpc_stream_tick of the C ABI, StreamBatch.tick) -- one wave per stream with the iterate in LDS and in the workspace, and the team
of 4 -- against the g++ build of the same kernel entry text (csrc/bmpc_tick_kernel.inl through tests/emu, emu.stream_tick) on the same inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,S,waves", [(2, 2, 1), (2, 2, 4), (3, 5, 1)])
def test_fused_tick_on_the_gpu_equals_the_cpu_build_of_the_same_text(N, S, waves):
    """B = 3 distinct streams, 3 fused ticks from the cold start, converged with the dual state carried: the device arrays (state, robot, p, x0, x, g, traj)
    behind every tick against emu.stream_tick on the same inputs (waves = 4: the team text against the team entry), 1e-11 -- the tolerance of the rollout,
    log and update tests: device libm and contraction against the host's.  iters and kkt are left out: the residual at the solution is round-off itself,
    and iterations may differ by one where the test sits on the tolerance.
    Measured largest deviation on an MI355X: (2, 2) one wave 1.5e-13, (2, 2) team 1.5e-13, (3, 5) 3.5e-13."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    from tests.emu import emu, emu_rollout as er
    B, ticks = 3, 3
    made = [er.small_stream(N, S, which=i) for i in range(B)]
    solver = BatchedOCPSolver(N, S, 0.1)
    solver.set_team_waves(waves)
    assert solver.team_info(B)["waves"] == waves
    sb = bstream.StreamBatch(solver, [m[0] for m in made])
    sb.set_robot(np.stack([m[1] for m in made]))
    cpu = [er.fresh_arrays(N, S, m[3], m[1]) for m in made]
    worst = 0.0
    for t in range(ticks):
        sb.tick(warm_dual=True, simulate=True)
        torch.cuda.synchronize()
        got = {k: getattr(sb, k).cpu().numpy() for k in ("state", "robot", "p", "x0", "x", "g", "traj", "status")}
        for b in range(B):
            A = cpu[b]
            emu.stream_tick(N, S, 0.1, made[b][2], A, warm_dual=True, opts=emu.opts_for(N, start_rollout=0), nw=waves)
            assert got["status"][b] == A["status"][0] == 0, (t, b)
            for k, h in (("state", "ss"), ("robot", "rb"), ("p", "p"), ("x0", "x0"), ("x", "x"), ("g", "g"), ("traj", "traj")):
                assert np.isfinite(got[k][b]).all() and np.isfinite(A[h]).all(), (t, b, k)
                worst = max(worst, float(np.abs(got[k][b] - A[h]).max()))
    print(f"N {N} S {S} waves {waves}: largest deviation GPU - CPU build over state, robot, p, x0, x, g, traj in {ticks} ticks: {worst:.3e}")
    assert worst <= 1e-11
    sb.close(); solver.close()
