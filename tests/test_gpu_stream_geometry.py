"""GPU: the device build of the stream kernels (bmpc_stream_pack / _post / _log / _tube / _update, the fused tick) against the host mirror on random paths --
the cases of tests/stream_geometry.py as DIFFERENT streams of one batch per (N, S), at the bounds of tests/test_stream_geometry.py (the CPU build of the
same text meets them with three orders to spare: profiles/stream_geometry.txt).  What is new against the CPU tests is the device: 64-lane phases, device
libm, contraction, streams that differ from each other inside one launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import stream_geometry as sg      # noqa: E402

_SHAPES = sg.shapes("replay") + [s for s in sg.shapes("replan") if s not in sg.shapes("replay")]


@pytest.mark.parametrize("N,S", _SHAPES)
def test_device_equals_the_mirror(N, S):
    """every replay and re-plan case of the shape in one batch, per tick pack -> (x, g, status of the mirror's tick) -> post, log, tube; the re-plan cases through
    update_device at their tick, beside streams whose record carries no flag"""
    cases = sg.names("replay", (N, S)) + sg.names("replan", (N, S))
    assert len(cases) >= (16 if (N, S) == (10, 4) else 2)
    devs = sg.gpu_run(cases, update=True)
    for name in cases:
        assert set(devs[name]) == set(sg.GROUPS) | ({"update"} if sg.BY_NAME[name]["kind"] == "replan" else set()), name
        sg.assert_within(devs[name], name, "device")


def test_device_pack_equals_the_mirror_on_the_angle_sweep():
    """one pack launch, each angle and axis one stream"""
    cases = sg.names("sweep")
    devs = sg.gpu_run(cases)
    for name in cases:
        assert set(devs[name]) == {"p", "x0", "tube"}
        sg.assert_within(devs[name], name, "device")


def test_fused_tick_packs_what_the_mirror_packs():
    """two (10, 4) replay cases through the fused tick of a handle capped at one iteration, from the mirror's state rows: the p and x0 the launch leaves"""
    cases = ["r10_4_5", "r10_4_8"]
    devs = sg.gpu_run(cases, fused=True)
    for name in cases:
        assert set(devs[name]) == {"p", "x0"}
        sg.assert_within(devs[name], name, "fused tick")


def test_dphi_max_survives_a_replan_on_the_device():
    """tests/test_stream_geometry.py test_dphi_max_survives_a_replan_with_new_weights on the device: stream 0 re-plans through update_device, stream 1 through
    the host's StreamBatch.update (apply_update), stream 2 not at all; the packed dphi_max stays the constructor's weights[4], the packed weight is the new one"""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    name = "u10_4"
    c, run = sg.BY_NAME[name], sg.mirror_run(name)
    N, S, args = c["N"], c["S"], run["update"]["args"]
    o = bstream._poff(S)
    mpcs = [sg.fresh(name)["mpc"] for _ in range(3)]
    old, new = float(mpcs[0].weights[4]), float(args[-1][4])
    assert abs(old - new) > 0.1
    solver = BatchedOCPSolver(N, S, sg.H)
    sb = bstream.StreamBatch(solver, mpcs)
    try:
        sb.set_robot(np.stack([run["ticks"][0]["rb"]] * 3))
        sb.pack(); torch.cuda.synchronize()
        p = sb.p.cpu().numpy()
        assert (p[:, o["dphimax"]] == old).all() and (p[:, o["w"] + 4] == old).all()
        recs = np.zeros((3, bstream.replan_len(S, sb.entries)))
        recs[0] = bstream.replan_record(S, sb.entries, *args)
        info = sb.update_device(recs)
        sb.update(1, *args)
        sb.pack(); torch.cuda.synchronize()
        p = sb.p.cpu().numpy()
        assert info.cpu().numpy().tolist() == [0, 0, 0]
        assert p[:, o["w"] + 4].tolist() == [new, new, old]
        assert p[:, o["dphimax"]].tolist() == [old, old, old], f"dphi_max behind update_device, update, no re-plan: {p[:, o['dphimax']]}; {old} before, new weights[4] {new}"
    finally:
        sb.close(); solver.close()
