"""The Lagrangian L = f + LAM . g_eq + nu . h of the per-step NLP and its derivatives through oracle/nlp.py alone (numpy; nothing of the code
under test), shared by the dense checkers: tests/test_kkt_certificate.py (gradient), tests/test_sensitivity.py (tangent of the solution),
tests/newton_reference.py (one Newton step).  g_eq: the 36 equality rows per stage; h: the 57 internal inequality rows per stage
(nlp.internal_ineq).  First derivatives by complex step (exact to rounding).  Second derivatives only as MIXED DIRECTIONAL derivatives of the
scalar L: one direction by complex step, the other by the five-point central difference (truncation step^4 L^(5) / 30, rounding
1e-16 |grad| / step), so a full Hessian (n^2 evaluations) is never formed."""
import numpy as np

from oracle import nlp

NZ, NG, NE, NI, NU = 44, 43, 36, 57, 8
EPS = 1e-30


def g_eq(xc, pc, N, S, h):
    return nlp.nlp_eval(xc, pc, N, S, h)[1].reshape(N, NG)[:, :NE].reshape(-1)


def lagrangian(xc, pc, lam_eq, nu, N, S, h):
    f, g = nlp.nlp_eval(xc, pc, N, S, h)
    return f + lam_eq @ g.reshape(N, NG)[:, :NE].reshape(-1) + nu @ nlp.internal_ineq(xc, pc, N, S)


def lagrangian_gradient(p, x, lam_eq, nu, N, S, h=0.1):
    """d/dx (f + lam_eq . g_eq + nu . h) by complex step, [N][44] -- independent of the C oracle's adjoint."""
    lam_eq, nu = np.asarray(lam_eq).ravel(), np.asarray(nu).ravel()
    gl, xc = np.zeros(x.size), x.astype(complex)
    for i in range(x.size):
        xc[i] += 1j * EPS; gl[i] = lagrangian(xc, p, lam_eq, nu, N, S, h).imag / EPS; xc[i] = x[i]
    return gl.reshape(N, NZ)


def grad_along(x, p, lam_eq, nu, U, N, S, h):
    """U^T grad_x L at (x, p) by complex step, one evaluation per column"""
    pc = np.asarray(p).astype(complex)
    return np.array([lagrangian(x + 1j * EPS * U[:, a], pc, lam_eq, nu, N, S, h).imag / EPS for a in range(U.shape[1])])


def fd5(fun, step=1e-3):
    """five-point central difference of fun(t) at 0"""
    return (8.0 * (fun(step) - fun(-step)) - (fun(2 * step) - fun(-2 * step))) / (12.0 * step)


def mixed_second(x, p, lam_eq, nu, U, v, N, S, h, step=1e-3):
    """U^T (grad^2_xx L) v: complex step along the columns of U, five-point difference along v"""
    return fd5(lambda t: grad_along(x + t * v, p, lam_eq, nu, U, N, S, h), step)


def jacobians(p, x, N, S, h):
    """grad f [n], Jg_eq [36 N][n], Jh [57 N][n] at x by complex step"""
    n = x.size
    gf, Jg = nlp.jac_g_complex_step(x, p, N, S, h)
    Jg = Jg.reshape(N, NG, n)[:, :NE].reshape(N * NE, n)
    Jh, xc = np.zeros((N * NI, n)), x.astype(complex)
    for i in range(n):
        xc[i] += 1j * EPS; Jh[:, i] = nlp.internal_ineq(xc, p, N, S).imag / EPS; xc[i] = x[i]
    return gf, Jg, Jh


def column_split(n):
    """indices of the jerk columns J and of the state columns S of x: Jg_eq restricted to S is square and regular"""
    z = np.arange(n) % NZ
    return np.flatnonzero(z < NU), np.flatnonzero(z >= NU)


def lam_from_state_columns(gf, Jg, Jh, nu):
    """LAM from the state columns of the stationarity equation grad f + Jg^T LAM + Jh^T nu = 0"""
    _, Sc = column_split(gf.size)
    return np.linalg.solve(Jg[:, Sc].T, -(gf + Jh.T @ nu)[Sc])


def null_space(Jg):
    """Z = [I; -Jg_S^-1 Jg_J] (Jg Z = 0) and the factor Jg_S"""
    n = Jg.shape[1]
    Jc, Sc = column_split(n)
    JgS = Jg[:, Sc]
    Z = np.zeros((n, len(Jc)))
    Z[Jc] = np.eye(len(Jc)); Z[Sc] = -np.linalg.solve(JgS, Jg[:, Jc])
    return Z, JgS


def reduced_hessian(x, p, lam_eq, nu, Z, N, S, h, step=1e-3):
    """Z^T (grad^2_xx L) Z: complex step along Z_a, five-point difference along Z_b (upper triangle, mirrored)"""
    m = Z.shape[1]
    Hzz = np.zeros((m, m))
    for b in range(m):
        col = mixed_second(x, p, lam_eq, nu, Z[:, :b + 1], Z[:, b], N, S, h, step)
        Hzz[:b + 1, b] = col; Hzz[b, :b + 1] = col
    return Hzz
