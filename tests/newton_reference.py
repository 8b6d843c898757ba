"""An independent dense reference of ONE Newton step of the interior-point method (numpy.linalg on derivatives taken through oracle/nlp.py;
nothing of the code under test: not the C oracle, not the kernel text).

THE SYSTEM at (p, x, t, nu, mu, delta).  g_eq: the 36 equality rows per stage; h: the 57 internal inequality rows per stage
(nlp.internal_ineq); sg = nu / t; nuh = (mu + nu (h + t)) / t; LAM from the state columns of the stationarity equation
grad f + Jg_eq^T LAM + Jh^T nu = 0 (Jg_eq restricted to the state columns is square and regular); H = grad^2 (f + LAM . g_eq + nu . h):
    (H + Jh^T diag(sg) Jh + delta R) dZ + Jg_eq^T dLAM = -(grad f + Jg_eq^T LAM + Jh^T nuh),      Jg_eq dZ = -g_eq.

R, THE BLOCK OF THE REGULARISATION.  riccati() of oracle/bmpc_oracle.c adds delta to the diagonal of the value-function matrix P of every
stage (the last node's before the sweep, P of stage k - 1 when stage k has been eliminated) -- a matrix on the 35 REDUCED STATE coordinates
s of a stage, which the oracle's map dZ = rloc + T s ties to the 44 stage variables: 32 of them are stage variables themselves (the 8 jerks,
q, dq, ddq, phi, dphi, ddphi; rloc is zero on these rows), the last 3 are iota = iw - (h / 2) omega, linearised:
    iota_c = dZ[iw_c] - (h / 2) (d omega_c / dq . dZ[q] + d omega_c / d(dq) . dZ[dq]),
omega = J_w(q) dq evaluated where the equality rows evaluate it: at the node integrated from the previous stage (nlp.nlp_eval: vn[3:]).  The
lifted task-space variables (pos, v, w) carry no regularisation.  So R = blockdiag(S_k^T S_k) with S_k [35][44] the rows above, and
delta dZ^T R dZ = delta sum_k |s_k|^2.

HOW IT IS SOLVED: in the null space of Jg_eq, as the sensitivity checker does (tests/test_sensitivity.py): dZ = xp + Z y with
Jg_eq xp = -g_eq on the state columns, Z = [I; -Jg_S^-1 Jg_J], and
    Z^T (H + Jh^T sg Jh + delta R) Z y = -Z^T (grad f + Jh^T nuh) - Z^T (H + Jh^T sg Jh + delta R) xp
(Z^T Jg_eq^T = 0: LAM enters through H only).  Second derivatives: tests/lagrangian.py -- a complex step in one direction, the five-point
central difference with step `step` in the other; Z^T H Z takes (8 N)^2 / 2 pairs, Z^T H xp another 8 N."""
import numpy as np

from oracle import nlp
from tests import lagrangian as lg

NZ, NE, NI = lg.NZ, lg.NE, lg.NI


def regularisation_block(p, x, N, S, h):
    """R [44 N][44 N] of the module docstring"""
    P = nlp.unpack_p(np.asarray(p, float), S)
    z = np.asarray(x, float).reshape(N, NZ)
    qk, dqk, ddqk, u_prev = P["q0"], P["dq0"], P["ddq0"], P["jerk_cur"]
    R = np.zeros((N * NZ, N * NZ))
    for k in range(N):
        qn, dqn, _ = nlp.integrate_chain(qk, dqk, ddqk, u_prev, z[k, :7], h)
        dw = np.zeros((3, 14))      # d omega / d(q, dq) at the integrated node, by complex step
        for i in range(14):
            e = np.zeros(14, complex); e[i] = 1j * lg.EPS
            dw[:, i] = nlp.omega_ee(qn + e[:7], dqn + e[7:]).imag / lg.EPS
        Sk = np.zeros((35, NZ))
        direct = list(range(0, 8)) + list(range(nlp.IQ, nlp.IQ + 21)) + [nlp.IPHI, nlp.IDPHI, nlp.IDDPHI]
        for r, c in enumerate(direct):
            Sk[r, c] = 1.0
        for c in range(3):
            Sk[32 + c, nlp.IIW + c] = 1.0
            Sk[32 + c, nlp.IQ:nlp.IQ + 7] = -0.5 * h * dw[c, :7]
            Sk[32 + c, nlp.IDQ:nlp.IDQ + 7] = -0.5 * h * dw[c, 7:]
        R[k * NZ:(k + 1) * NZ, k * NZ:(k + 1) * NZ] = Sk.T @ Sk
        qk, dqk, ddqk, u_prev = z[k, nlp.IQ:nlp.IQ + 7], z[k, nlp.IDQ:nlp.IDQ + 7], z[k, nlp.IDDQ:nlp.IDDQ + 7], z[k, :7]
    return R


class NewtonReference:
    """The system of one point (p, x, t, nu, mu); dz(delta) solves it.  The derivatives are taken once per point and difference step."""

    def __init__(self, p, x, t, nu, mu, N, S, h, step=1e-3):
        p, x, t, nu = (np.asarray(a, float).ravel() for a in (p, x, t, nu))
        self.N = N
        gf, Jg, Jh = lg.jacobians(p, x, N, S, h)
        hin = nlp.internal_ineq(x, p, N, S)
        sg, nuh = nu / t, (mu + nu * (hin + t)) / t
        self.lam = lg.lam_from_state_columns(gf, Jg, Jh, nu)
        Z, JgS = lg.null_space(Jg)
        _, Sc = lg.column_split(x.size)
        xp = np.zeros(x.size); xp[Sc] = np.linalg.solve(JgS, -lg.g_eq(x, p, N, S, h))
        Hzz = lg.reduced_hessian(x, p, self.lam, nu, Z, N, S, h, step)
        ZHxp = lg.mixed_second(x, p, self.lam, nu, Z, xp, N, S, h, step) if np.any(xp) else np.zeros(Z.shape[1])
        JhZ = Jh @ Z
        self.K0 = Hzz + JhZ.T @ (sg[:, None] * JhZ)
        self.rhs0 = -Z.T @ (gf + Jh.T @ nuh) - ZHxp - JhZ.T @ (sg * (Jh @ xp))
        self.R, self.Z, self.xp = regularisation_block(p, x, N, S, h), Z, xp

    def dz(self, delta=0.0):
        Z, xp, R = self.Z, self.xp, self.R
        y = np.linalg.solve(self.K0 + delta * (Z.T @ R @ Z), self.rhs0 - delta * (Z.T @ (R @ xp)))
        return xp + Z @ y


def newton_dz(p, x, t, nu, mu, delta, N, S, h, step=1e-3):
    """dZ [44 N] of the module docstring's system"""
    return NewtonReference(p, x, t, nu, mu, N, S, h, step).dz(delta)
