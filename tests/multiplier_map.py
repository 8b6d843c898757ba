"""The ABI's multiplier convention in numpy, once, shared by tests/test_dual_warm_start.py, tests/test_kkt_certificate.py and
tests/test_sensitivity.py (and through them by their GPU modules): the multiplier map of include/boundmpc_hip.h bmpc_state_from_multipliers
(boundmpc_amd/csrc/bmpc_dual.inl dual_row) and its inverse, the output map of a solve (bmpc_wave.inl out_g_entry / out_lam_x_entry)."""
import numpy as np

from oracle.nlp import internal_ineq

NZ, NG, NI = 44, 43, 57
NU_CAP = 1e12      # DUAL_NU_CAP of bmpc_dual.inl


def _fin(a):
    a = np.array(a, dtype=float)
    a[~np.isfinite(a)] = 0.0
    return a


def _cap(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.minimum(v, NU_CAP), 0.0)      # (NaN -> 0)


def nu_of(p, x, lam_g, lam_x, N, S, bound_margin=0.0):
    """One problem: nu [N][57] of the internal rows from multipliers in CasADi's convention (None = zeros), the rounding scale lam (|c| + wd)
    of its tube rows, c and wd [N][5] of the squared tube rows at x (from the oracle's internal rows h[47 + 2m] = c - wd, h[48 + 2m] = -c - wd)
    and those rows H [N][57] (of a handle with options.bound_margin = bound_margin)."""
    g = np.zeros((N, NG)) if lam_g is None else _fin(lam_g).reshape(N, NG)
    z = np.zeros((N, NZ)) if lam_x is None else _fin(lam_x).reshape(N, NZ)
    H = internal_ineq(np.asarray(x, dtype=float), np.asarray(p, dtype=float), N, S, bound_margin).reshape(N, NI)
    up, lo = H[:, 47::2], H[:, 48::2]
    c, wd = (up - lo) / 2, -(up + lo) / 2
    nu, sc = np.zeros((N, NI)), np.zeros((N, NI))
    for r0, zs in ((0, slice(0, 8)), (16, slice(8, 15)), (30, slice(15, 22))):
        n = zs.stop - zs.start
        nu[:, r0:r0 + n], nu[:, r0 + n:r0 + 2 * n] = z[:, zs], -z[:, zs]
    nu[:, 44] = -z[:, 41]
    nu[:, 45], nu[:, 46] = g[:, 36], g[:, 37]
    lam = np.maximum(g[:, 38:43], 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        nu[:, 47::2], nu[:, 48::2] = lam * (wd + c), lam * (wd - c)
        sc[:, 47::2] = sc[:, 48::2] = lam * (np.abs(c) + wd)
    return _cap(nu), np.nan_to_num(sc), c, wd, H


def export_of(nu, wd):
    """lam_g[36:43] [N][7] and lam_x [N][44] of internal multipliers nu: the output map of a solve."""
    N = nu.shape[0]
    lg, lx = np.zeros((N, 7)), np.zeros((N, NZ))
    lg[:, 0], lg[:, 1] = nu[:, 45], nu[:, 46]
    with np.errstate(invalid="ignore", divide="ignore"):
        lg[:, 2:] = np.where(wd > 0, (nu[:, 47::2] + nu[:, 48::2]) / (2 * wd), 0.0)
    lx[:, 0:8] = nu[:, 0:8] - nu[:, 8:16]
    lx[:, 8:15] = nu[:, 16:23] - nu[:, 23:30]
    lx[:, 15:22] = nu[:, 30:37] - nu[:, 37:44]
    lx[:, 41] = -nu[:, 44]
    return lg, lx
