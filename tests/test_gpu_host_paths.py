"""The four host-buffer entry points (bmpc_solve_batch_host, bmpc_solve_batch_host_dual, bmpc_kkt_batch_host, bmpc_sens_batch_host) share ONE staging
arena of the handle and one routine that lays a call's record out in it (host_call in bmpc_hip.hip).  What that sharing can get wrong: a call that
runs on an arena another KIND of call sized, growth between kinds, reuse at a smaller batch, a left-out multiplier or output whose slot still holds
an earlier call's bytes, growth while a captured graph is alive, and a handle whose device is not the current one.  Every host result is compared
bit for bit with the same call on device tensors on a FRESH handle: the same kernels on the same inputs, so no tolerance (row and batch-size
invariance of the kernels are tests of their own).

Handles of fixture G12: n5s2 (N = 5, S = 2, 12 problems: iterate in LDS) and n6s5 (N = 6, S = 5, 10 problems: iterate in the workspace), started
as the sets B / C of tests/entry_path_sets.py."""
import ctypes
import functools

import numpy as np
import pytest
from numpy.testing import assert_array_equal

from tests import entry_path_sets as eps

pytestmark = pytest.mark.gpu

SOLVE_KEYS = ("x", "g", "lam_g", "lam_x", "f", "iters", "status", "kkt")


def _handle(name):
    from boundmpc_amd import BatchedOCPSolver
    _, _, N, S, dt = eps.problem_set(name)
    return BatchedOCPSolver(N, S, dt, start_rollout=False)


@functools.lru_cache(maxsize=None)
def _device(name):
    """Per batch size (1, 2, the full set): the results of the device calls on one fresh handle, as numpy; plus the inputs the host calls get.
    The point (x, lam_g, lam_x) of the certificate and the sensitivity is the full-set solve's output, dp a fixed random direction."""
    import torch
    P, X0, N, S, dt = eps.problem_set(name)
    full = P.shape[0]
    dP = np.random.default_rng(5).normal(size=P.shape) * 1e-2
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device="cuda")
    npy = lambda o, keys: {k: o[k].cpu().numpy() for k in keys}
    s = _handle(name)
    try:
        sol = npy(s.solve_batch(t(P), t(X0), out={}), SOLVE_KEYS)
        inp = dict(p=P, x0=X0, dp=dP, x=sol["x"], lam_g=sol["lam_g"], lam_x=sol["lam_x"])
        out = {}
        for B in (1, 2, full):
            r = slice(0, B)
            p, x0, dp, x, lg, lx = (t(inp[k][r]) for k in ("p", "x0", "dp", "x", "lam_g", "lam_x"))
            o = out[B] = {}
            o["solve"] = npy(s.solve_batch(p, x0, out={}), SOLVE_KEYS)
            o["dual"] = npy(s.solve_batch(p, x0, out={}, lam_g0=lg, lam_x0=lx), SOLVE_KEYS)
            o["dual_g"] = npy(s.solve_batch(p, x0, out={}, lam_g0=lg), SOLVE_KEYS)
            o["cert"] = npy(s.certify(p, x, lg, lx, want=("g", "lam_g", "rj")), ("cert", "g", "lam_g", "rj"))
            o["cert0"] = npy(s.certify(p, x), ("cert",))
            o["sens"] = npy(s.sensitivity(p, x, dp, lg, lx, want_duals=True), ("dx", "rec", "dlam_eq", "dnu"))
            o["sens0"] = npy(s.sensitivity(p, x, dp), ("dx", "rec"))
        torch.cuda.synchronize()
    finally:
        s.close()
    return inp, out, full


def _same(got, ref, tag):
    for k, v in ref.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, (tag, k)
        assert_array_equal(got[k], v, err_msg=f"{tag}: {k}")


def _host_round(s, inp, ref, B, tag):
    """the four entry points in turn at batch size B, every optional array present"""
    r = slice(0, B)
    p, x0, dp, x, lg, lx = (inp[k][r] for k in ("p", "x0", "dp", "x", "lam_g", "lam_x"))
    _same(s.solve_host(p, x0), ref["solve"], f"{tag} solve_host B={B}")
    _same(s.solve_host(p, x0, lam_g0=lg, lam_x0=lx), ref["dual"], f"{tag} solve_host(lam) B={B}")
    _same(s.certify_host(p, x, lg, lx, want=("g", "lam_g", "rj")), ref["cert"], f"{tag} certify_host B={B}")
    _same(s.sensitivity_host(p, x, dp, lg, lx, want_duals=True), ref["sens"], f"{tag} sensitivity_host B={B}")


def _host_round_absent(s, inp, ref, B, tag):
    """the same with everything optional left out: no multipliers (one of the two for the warm solve, which needs one to be that call), no optional
    outputs; the bare solve through the C ABI, which alone can leave the outputs of a solve out"""
    r = slice(0, B)
    p, x0, dp, x, lg = (inp[k][r] for k in ("p", "x0", "dp", "x", "lam_g"))
    _same(s.certify_host(p, x), ref["cert0"], f"{tag} certify_host() B={B}")
    _same(s.sensitivity_host(p, x, dp), ref["sens0"], f"{tag} sensitivity_host() B={B}")
    _same(s.solve_host(p, x0, lam_g0=lg), ref["dual_g"], f"{tag} solve_host(lam_g0) B={B}")
    xo = np.full_like(ref["solve"]["x"], np.nan)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pc, x0c = np.ascontiguousarray(p), np.ascontiguousarray(x0)
    rc = s._lib.bmpc_solve_batch_host(s._h, B, vp(pc), vp(x0c), vp(xo), None, None, None, None, None, None, None)
    assert rc == 0
    assert_array_equal(xo, ref["solve"]["x"], err_msg=f"{tag}: bmpc_solve_batch_host with x alone B={B}")


@pytest.mark.parametrize("name", ["B", "C"])
def test_interleaved_host_calls_on_one_handle_equal_the_device_calls(name):
    """ONE handle, the four entry points interleaved at batch sizes 1, the full set, 2: every call but the first runs on an arena that a call of
    another kind sized, the full set grows it, 2 reuses it at a smaller size (other offsets inside the same bytes); then the pass with the optional
    arrays left out at the same three sizes, on slots that hold the previous calls' multipliers."""
    inp, dev, full = _device(name)
    s = _handle(name)
    try:
        for B in (1, full, 2):
            _host_round(s, inp, dev[B], B, name)
        for B in (1, full, 2):
            _host_round_absent(s, inp, dev[B], B, name)
        _host_round(s, inp, dev[full], full, name + " again")
    finally:
        s.close()


def test_host_calls_grow_the_arena_beside_a_live_step_graph():
    """A captured step holds the handle's WORKSPACE, which therefore may not grow; the staging arena is not part of any graph and must stay free to:
    host calls of every kind, first small then at the full set, between two replays.  The replays' outputs are bit-equal, the host calls correct."""
    import torch
    inp, dev, full = _device("B")
    s = _handle("B")
    try:
        p, x0 = torch.tensor(inp["p"], device="cuda"), torch.tensor(inp["x0"], device="cuda")
        graph = s.capture_step(p, x0, want=("g", "lam_g", "lam_x", "f", "iters", "status", "kkt"))
        before = {k: v.clone() for k, v in graph.launch().items()}
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in before.items()}, dev[full]["solve"], "replay before")
        for B in (1, full):
            _host_round(s, inp, dev[B], B, "beside a graph")
        for v in graph.out.values():
            v.zero_()
        after = graph.launch()
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in after.items()}, {k: v.cpu().numpy() for k, v in before.items()}, "replay after")
        graph.close()
    finally:
        s.close()


def test_solve_host_on_a_handle_of_another_device():
    """The handle lives on cuda:1, the call comes while cuda:0 is current: staging, stream and launch belong to the handle's device."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    from boundmpc_amd import BatchedOCPSolver
    P, X0, N, S, dt = eps.problem_set("B")
    with torch.cuda.device(1):
        s = BatchedOCPSolver(N, S, dt, start_rollout=False)
        ref = s.solve_batch(torch.tensor(P, device="cuda:1"), torch.tensor(X0, device="cuda:1"), out={})
        ref = {k: ref[k].cpu().numpy() for k in SOLVE_KEYS}
    try:
        with torch.cuda.device(0):
            got = s.solve_host(P, X0)
            assert torch.cuda.current_device() == 0
        _same(got, ref, "solve_host from cuda:0")
    finally:
        s.close()
