"""The acceptance rule of stream_post on the MI355X (bmpc_stream_post: 64 lanes stride over the entries of g and x, seven of them integrate a joint chain each,
lane 0 folds the 64 partial sums) against the numpy specification of tests/rt_acceptance.py, on the battery that tests/test_rt_acceptance.py runs through the
one-lane CPU build.  The stride and the fold run nowhere but here: N = 1 leaves 21 lanes without an entry of g (they must contribute 0), N = 33 and 40 take
the post's role map beyond 32 stages, every horizon above 1 has entries on the second trip of a lane.

The cases of a horizon are the streams of ONE batch: the base stream's arrays replicated, x / g / status / robot / state rows overwritten per stream.  The
threshold, the row cap and the mode are read from the handle at launch, so a horizon takes one launch per (flags, rt_tol, row_cap) group, each on freshly
uploaded arrays; only the rows of the launch's group are looked at.

The fused tick and the team tick call the same function behind a solve whose x cannot be crafted, so the battery cannot be put to them.  The rule reaches
them through tests that exist: tests/test_gpu_stream_tick.py holds every device array behind fused one-wave and team ticks (state, traj with its trailer) to
the CPU build of the same entry text, tests/test_gpu_stream.py the fused tick to the three-kernel tick (pack, solve, this post).  `pytest -m gpu`."""
import numpy as np
import pytest

from tests import rt_acceptance as ra

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [1, 10, 33, 40])
def test_device_post_follows_the_specification(N):
    import torch
    from boundmpc_amd import BatchedOCPSolver
    from boundmpc_amd.stream import StreamBatch
    ra.assert_battery(N)      # (the conditions on the inputs, on the specification alone, first)
    b, cases = ra.base(N), ra.battery(N)
    B = len(cases)
    s = BatchedOCPSolver(N, ra.S_, ra.H_)
    sb = StreamBatch(s, [b["mpc"]] * B)
    try:
        assert np.array_equal(sb.path[0].cpu().numpy(), b["T"]) and sb.entries == b["T"].shape[0]      # the batch's table is the base stream's
        host = {k: np.stack([c[k] for c in cases]) for k in ("ss", "rb", "x", "g")}
        status = np.array([c["status"] for c in cases], dtype=np.int32)
        worst, seen = 0.0, 0
        for fl, tol, cap in ra.GROUPS:
            rows = [i for i, c in enumerate(cases) if (c["flags"], c["rt_tol"], c["row_cap"]) == (fl, tol, cap)]
            if not rows:
                continue
            sb.state.copy_(torch.as_tensor(host["ss"])); sb.robot.copy_(torch.as_tensor(host["rb"])); sb.x.copy_(torch.as_tensor(host["x"]))
            sb.g.copy_(torch.as_tensor(host["g"])); sb.status.copy_(torch.as_tensor(status)); sb.traj.zero_()
            s.set_rt_feasibility_tol(tol); s.set_rt_position_row_cap(cap)
            sb.post(simulate=True, accept_capped=bool(fl & 2))
            torch.cuda.synchronize()
            state, traj = sb.state.cpu().numpy(), sb.traj.cpu().numpy()
            for i in rows:
                c = cases[i]
                want = ra.consequences(c["v"], c["ss"], c["x"], c["status"], c["flags"], N)
                worst = max(worst, ra.assert_consequences((N, c["name"]), want, c["v"], state[i], traj[i], N))
            seen += len(rows)
        assert seen == B
        print(f"\nN = {N}: {B} cases in {len(ra.GROUPS)} launches; worst relative g_viol deviation on the device {worst:.2e}")
    finally:
        sb.close(); s.close()
