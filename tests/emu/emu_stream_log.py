"""TEST-ONLY: the CPU build of the stream log (boundmpc_amd/csrc/bmpc_stream_log.inl through tests/emu/bmpc_emu_stream_log.cpp) and what the
CPU and the GPU tests of the log share: the open-loop replay of the recorded experiments and the comparison with fixture G10."""
import ctypes
import os

import numpy as np

from boundmpc_amd import stream as bstream
from tests.emu import emu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden")
REF_KEYS = tuple(k for k, _ in bstream.LOG_REF)
ERR_KEYS = tuple(k for k, _ in bstream.LOG_ERR)


def lib():
    return emu._build("libbmpc_emu_stream_log.so", "bmpc_emu_stream_log.cpp", (), ("bmpc_stream.inl", "bmpc_stream_log.inl"))


def stream_log(N, S, h, path, ss, p, traj):
    """path [M][48], ss, p, traj of one stream as a tick left them -> log row [88 N + 4]"""
    L = lib()
    assert L.bmpc_emu_stream_log_len(ctypes.c_int(N)) == bstream.log_len(N)
    path, ss, p, traj = (np.ascontiguousarray(a, dtype=np.float64) for a in (path, ss, p, traj))
    assert path.shape[1] == bstream.PT["LEN"] and ss.shape == (bstream.ss_len(N),) and p.shape == (141 + 91 * S,) and traj.shape == (emu.stream_lengths(N)["traj"],)
    log = np.zeros(bstream.log_len(N))
    L.bmpc_emu_stream_log(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), emu._p(path), ctypes.c_int(path.shape[0]), emu._p(ss), emu._p(p), emu._p(traj),
                          emu._p(log))
    return log


def g10_passes(which):
    """The ticks of recorded experiment `which` as fixture G10 was made (tests/golden/make_g10.py): a pass with the solver failure forced at
    fail_tick, stopped behind it, then a pass without it.  Yields (with_failure, t, robot record, x, g, status, checked): `checked` says
    whether G10 holds this tick of this pass."""
    from oracle import c_oracle
    d7 = np.load(os.path.join(G, f"g7_closedloop_exp{which}.npz"))
    d10 = np.load(os.path.join(G, "g10_logging.npz"))
    ticks, fail = [int(t) for t in d10[f"exp{which}_ticks"]], int(d10[f"exp{which}_fail_tick"])
    for with_failure in (True, False):
        for t in range(len(d7["x"])):
            if with_failure and t > fail:
                break
            failing = with_failure and t == fail
            g = np.ones(430) if failing else c_oracle.eval_fg(d7["p"][t], d7["x"][t], 10, 4, 0.1)[1]
            rec = lambda xphid, t=t: bstream.robot_record(d7["q"][t], d7["dq"][t], d7["ddq"][t], d7["p_lie"][t], d7["v"][t], xphid, d7["jerk"][t])
            yield with_failure, t, rec, d7["x"][t], g, 1 if failing else int(d7["status"][t]), t in ticks and (t <= fail) == with_failure


def g10_ticks(which):
    return len(np.load(os.path.join(G, "g10_logging.npz"))[f"exp{which}_ticks"])


def assert_equals_g10(row, which, t, ref_atol=1e-10, err_atol=1e-9):
    """one log row against the reference's own dictionaries of tick t (all 16 + 11 keys, widths as in the fixture)"""
    d10 = np.load(os.path.join(G, "g10_logging.npz"))
    pre = f"exp{which}_t{t}_"
    ec = int(d10[pre + "error_count"])
    assert int(row[-3]) == ec and int(row[-4]) == 10 - ec == d10[pre + "ref_p"].shape[0]
    ref, err = bstream.unpack_log(row, 10)
    n = 10 - ec
    assert np.isnan(row[n * bstream.LOG_STAGE:10 * bstream.LOG_STAGE]).all()
    for k in REF_KEYS:
        got, want = np.array(ref[k]), d10[pre + "ref_" + k].copy()
        assert got.shape == want.shape, k
        if k == "p":      # a rotation vector of angle pi and its negative are the same rotation (tests/test_host.py test_logging_dictionaries_g10)
            flip = (np.abs(np.linalg.norm(want[:, 3:], axis=1) - np.pi) < 1e-9) & (np.sum(got[:, 3:] * want[:, 3:], axis=1) < 0)
            want[flip, 3:] *= -1.0
        np.testing.assert_allclose(got, want, atol=ref_atol, rtol=0, err_msg=f"exp{which} tick {t} ref {k}")
    for k in ERR_KEYS:
        got, want = np.array(err[k]), d10[pre + "err_" + k]
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, atol=err_atol, rtol=0, err_msg=f"exp{which} tick {t} err {k}")
