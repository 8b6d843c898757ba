"""The acceptance rule of stream_post (boundmpc_amd/csrc/bmpc_stream.inl phase 0; real-time mode = flags bit 1) against its numpy specification
(tests/rt_acceptance.py: written from RobotModel's limits and oracle/nlp.integrate_chain, not from the kernel text) on the battery of crafted cases of that
module -- here through the CPU build of the function (emu.stream_post: one lane, nl = 1).  tests/test_gpu_rt_acceptance.py runs the same battery on the
device, where 64 lanes stride over the entries and lane 0 folds their partial sums.

Per case: the verdict and every consequence (traj trailer, ERRCNT, HASPREV, the stored plan, the continuation word) equal the specification's; g_viol within
1e-12 relative, bit-equal where at most one term contributes; k vetoes report g_viol >= k 1e6.  The conditions on the battery itself -- every clause flips
the verdict alone and is present without flipping it in at least 4 cases per horizon, every accepted / rejected pair of the dead band, the threshold, the cap
and the slack is in, no multi-term sum sits within 1e-10 of a threshold -- are asserted on the specification alone, first."""
import numpy as np
import pytest

from tests import rt_acceptance as ra
from tests.emu import emu

HORIZONS = (1, 10, 33, 40)


@pytest.mark.parametrize("N", HORIZONS)
def test_battery_meets_its_conditions_on_the_specification(N):
    counts = ra.assert_battery(N)
    print(f"\nN = {N}: {len(ra.battery(N))} cases; per clause (flips the verdict alone, present and accepted): {counts}")


def test_specification_against_hand_worked_values():
    """the specification itself, on values worked by hand (N = 1): independent of battery and kernel"""
    b = ra.base(1)
    g = np.zeros(43); x = b["x"].copy()
    g[0], g[1], g[36], g[40] = -3e-6, 2e-6, -5.0, 4e-6
    v = ra.verdict(x, g, 1, b["rb"], 3, 1e-4, 0.0, 1)
    assert v["terms"] == 3 and abs(v["viol"] - 9e-6) < 1e-20 and v["veto"] == 0 and v["success"]
    v = ra.verdict(x, g, 1, b["rb"], 3, 1e-4, 3e-6, 1)
    assert v["veto"] == 1 and v["clauses"]["cap"] == 1 and not v["success"] and abs(v["g_viol"] - (1e6 + 9e-6)) < 1e-9
    assert ra.verdict(x, g, 1, b["rb"], 1, 1e-4, 3e-6, 1)["success"]      # reference mode: no cap
    x2 = x.copy(); x2[8] = ra.QLIM[0] + 2e-9
    assert not ra.verdict(x2, g, 0, b["rb"], 3, 1e-2, 0.0, 1)["success"] and ra.verdict(x2, g, 0, b["rb"], 1, 1e-2, 0.0, 1)["success"]
    rb = b["rb"].copy(); rb[0] = ra.QLIM[0] + 1.0      # the measured q_0 far outside: the chain clause, whatever the plan says
    v = ra.verdict(x, g, 0, rb, 3, 1e-2, 0.0, 1)
    assert v["clauses"]["chain"] == 1 and v["clauses"]["bounds"] == 0 and not v["success"]


@pytest.mark.parametrize("N", HORIZONS)
def test_cpu_build_follows_the_specification(N):
    b = ra.base(N)
    worst = 0.0
    for c in ra.battery(N):
        ss, rb = c["ss"].copy(), c["rb"].copy()
        tr = emu.stream_post(N, ra.S_, ra.H_, b["T"], ss, rb, c["x"], c["g"], c["status"], simulate=True, rt_tol=c["rt_tol"], flags=c["flags"] & 2, rt_row_cap=c["row_cap"])
        want = ra.consequences(c["v"], c["ss"], c["x"], c["status"], c["flags"], N)
        worst = max(worst, ra.assert_consequences((N, c["name"]), want, c["v"], ss, tr, N))
    print(f"\nN = {N}: worst relative g_viol deviation of the CPU build {worst:.2e}")
