// bmpc_stream_tube.inl -- the error bound of BoundMPC measured on the device: how far is the MEASURED state of a tick outside its tubes and its
// joint limits?  Host mirror and specification: boundmpc_amd.stream.tube_excess_of_state (the five tube rows of casadi_ocp_formulation.py:316-349
// at NODE 0 of a packed parameter vector, the state the plant is in), with the joint figures of q0, dq0 against qlim() / dqlim() of the wave
// program -- the reference's limits, without bound_margin.
//
// stream_tube: one stream per 64-lane wave, phases over `nl` cooperating lanes like stream_log / stream_update (the CPU test build runs it with
// one lane).  It reads only p as stream_pack wrote it (offsets: make_poff) and, where a state row is given, its error count; it writes the row
//   tube [TUBE_LEN = 16] = l 5 | w 5 | ex_pos | ex_rot | ex_q | ex_dq | segment | phi0          (BMPC_TUBE_* of include/boundmpc_hip.h)
// l, w in the row order 38..42 of a stage: orientation tangential, position bp1, position bp2, orientation br1, orientation br2 (the reference's rows
// are l^2 - w^2); ex_pos = max over rows 39, 40 of |l| - |w| (metres), ex_rot the same over rows 38, 41, 42 (radians), <= 0: inside;
// ex_q = max_j |q0_j| - qlim_j, ex_dq = max_j |dq0_j| - dqlim_j.
// The segment is not a word of p: it is selected by comparisons of phi0 with phi_switch (bound_mpc_functions.py:13-20), which leave it in 0..S-1
// whatever p holds (a NaN fails every comparison: S - 1), and it is clamped once more before it addresses anything; bp1 / bp2 never select the last
// window segment (:34-40).  Loads are unconditional on such indices and selects follow, so non-finite inputs give non-finite slots, never a fault;
// a maximum with a NaN among its terms is NaN.  A stream without a plan (a state row whose error count is not in 0..N-1: step() returns Nones, the
// fused tick skips the stream and its p is stale) gets an all-NaN row.
// `out` may be global memory or LDS; the excess slots are reduced by lane 0 from what the row lanes stored, behind a phase boundary.
//
// stream_audit_init / stream_audit: the per-stream verdict of a rollout (bmpc_rollout_kernel.inl, AU) over the tube rows of its ticks,
//   audit [AUDIT_LEN = 12] = samples | max_pos, tick_pos | max_rot, tick_rot | max_q | max_dq | n_pos | n_rot | n_joint | first_out | pad
// (BMPC_AUDIT_*).  Both are the work of ONE lane (lane 0: the lane that wrote the excess slots of the row, or saw them behind stream_tube's phase
// boundary); the record lives in global memory between the ticks.
// The same text is compiled by g++ for the CPU tests (tests/emu/bmpc_emu_stream_tube.cpp, bmpc_emu_rollout.cpp).
#pragma once

namespace bmpcs {
enum { TUBE_L = 0, TUBE_W = 5, TUBE_EX_POS = 10, TUBE_EX_ROT = 11, TUBE_EX_Q = 12, TUBE_EX_DQ = 13, TUBE_SEG = 14, TUBE_PHI = 15, TUBE_LEN = 16 };
enum { AUDIT_SAMPLES = 0, AUDIT_MAX_POS, AUDIT_TICK_POS, AUDIT_MAX_ROT, AUDIT_TICK_ROT, AUDIT_MAX_Q, AUDIT_MAX_DQ, AUDIT_N_POS, AUDIT_N_ROT, AUDIT_N_JOINT,
       AUDIT_FIRST_OUT, AUDIT_PAD, AUDIT_LEN };
constexpr double AUDIT_JOINT_TOL = 1e-9;      // a joint figure above it counts as a limit violation (the bound of bench_stream.py's count)

// max(m, a) that keeps a NaN once it has seen one
BMPC_HD inline double tube_max(double m, double a) { return (a > m || a != a) ? a : m; }

BMPC_HD inline void stream_tube(int N, int S, const double *p, const double *ss, double *out, int lane, int nl) {
    const double qnan = __builtin_nan("");
    if (ss) {                                                      // (uniform over the lanes)
        const double ecd = ss[SS_ERRCNT];
        if (!(ecd >= 0.0 && ecd < (double)N)) {
            for (int i = lane; i < TUBE_LEN; i += nl) out[i] = qnan;
            return;
        }
    }
    const BMPC_NAMESPACE::POff o = BMPC_NAMESPACE::make_poff(S);
    const double phi = p[o.phi0];
    int seg = S - 1;
    for (int j = S - 2; j >= 0; j--) if (phi < p[o.sw + j + 1]) seg = j;
    seg = seg < 0 ? 0 : (seg > S - 1 ? S - 1 : seg);
    const int segb = seg < S - 2 ? seg : (S - 2 > 0 ? S - 2 : 0);
    const double x = phi - p[o.sw + seg];
    // ---- phase 1: lanes 0..4 one tube row each, lane 5 the joint positions, lane 6 the joint velocities, lane 7 the two scalars ----
    for (int r = lane; r < 8; r += nl) {
        if (r < 5) {
            // the row's upper and lower quartic (row 38: the one bound of the tangential orientation error, no offset)
            const int cu = r == 0 ? 8 : (r < 3 ? r - 1 : r + 1), cl = r == 0 ? 8 : cu + 2;
            double bu, bl;
            { const int id = cu * (S + 1) + seg; bu = (((p[o.a[0] + id] * x + p[o.a[1] + id]) * x + p[o.a[2] + id]) * x + p[o.a[3] + id]) * x + p[o.a[4] + id]; }
            { const int id = cl * (S + 1) + seg; bl = (((p[o.a[0] + id] * x + p[o.a[1] + id]) * x + p[o.a[2] + id]) * x + p[o.a[3] + id]) * x + p[o.a[4] + id]; }
            // the row's two vectors: a basis vector of the segment ([coord][seg] blocks) against the position error p0 - (pref + dpref x), or
            // against the packed initial orientation error of the segment ([seg][xyz] blocks)
            const bool pos = r == 1 || r == 2;
            const int oa = r == 0 ? o.dpn : (r == 1 ? o.bp1 : (r == 2 ? o.bp2 : (r == 3 ? o.br1 : o.br2))), sa = pos ? segb : seg;
            const int ob = r == 3 ? o.io1 : (r == 4 ? o.io2 : o.ipar);
            double d = 0.0;
            for (int c = 0; c < 3; c++) {
                const double ini = p[ob + 3 * seg + c], ep = p[o.p0 + c] - (p[o.pref + c * S + seg] + p[o.dpref + c * S + seg] * x);
                d += p[oa + c * S + sa] * (pos ? ep : ini);
            }
            out[TUBE_L + r] = r == 0 ? d : d - 0.5 * (bu + bl);
            out[TUBE_W + r] = r == 0 ? bu : 0.5 * (bu - bl);
        } else if (r < 7) {
            const int oq = r == 5 ? o.q0 : o.dq0;
            double m = 0.0;
            for (int j = 0; j < 7; j++) {
                const double e = BMPC_FABS(p[oq + j]) - (r == 5 ? BMPC_NAMESPACE::qlim(j) : BMPC_NAMESPACE::dqlim(j));
                m = j == 0 ? e : tube_max(m, e);
            }
            out[r == 5 ? TUBE_EX_Q : TUBE_EX_DQ] = m;
        } else {
            out[TUBE_SEG] = (double)seg; out[TUBE_PHI] = phi;
        }
    }
    BMPCS_SYNC();
    // ---- phase 2 (one lane): the two excesses from the rows ----
    if (lane == 0) {
        double e[5];
        for (int r = 0; r < 5; r++) e[r] = BMPC_FABS(out[TUBE_L + r]) - BMPC_FABS(out[TUBE_W + r]);
        out[TUBE_EX_POS] = tube_max(e[1], e[2]);
        out[TUBE_EX_ROT] = tube_max(tube_max(e[0], e[3]), e[4]);
    }
}

BMPC_HD inline void stream_audit_init(double *audit) {
    const double ninf = -__builtin_inf();
    audit[AUDIT_SAMPLES] = 0.0; audit[AUDIT_MAX_POS] = ninf; audit[AUDIT_TICK_POS] = -1.0; audit[AUDIT_MAX_ROT] = ninf; audit[AUDIT_TICK_ROT] = -1.0;
    audit[AUDIT_MAX_Q] = ninf; audit[AUDIT_MAX_DQ] = ninf; audit[AUDIT_N_POS] = 0.0; audit[AUDIT_N_ROT] = 0.0; audit[AUDIT_N_JOINT] = 0.0;
    audit[AUDIT_FIRST_OUT] = -1.0; audit[AUDIT_PAD] = 0.0;
}
// one figure of one sample into its maximum (and, where tick_slot >= 0, the tick of the maximum): a larger figure replaces it, a non-finite one
// makes it NaN for good.  Returns whether the figure is outside (`tol`; a non-finite figure is).
BMPC_HD inline bool audit_figure(double *audit, int max_slot, int tick_slot, double ex, double tol, int t) {
    const bool bad = !(ex - ex == 0.0);
    const double m = audit[max_slot];
    if (bad ? m == m : ex > m) {
        audit[max_slot] = bad ? __builtin_nan("") : ex;
        if (tick_slot >= 0) audit[tick_slot] = (double)t;
    }
    return bad || ex > tol;
}
// the tube row of tick t into the record; tol: the excess above which a sample counts as outside a tube (joints: AUDIT_JOINT_TOL)
BMPC_HD inline void stream_audit(const double *tube, double *audit, int t, double tol) {
    audit[AUDIT_SAMPLES] += 1.0;
    const bool op = audit_figure(audit, AUDIT_MAX_POS, AUDIT_TICK_POS, tube[TUBE_EX_POS], tol, t);
    const bool orot = audit_figure(audit, AUDIT_MAX_ROT, AUDIT_TICK_ROT, tube[TUBE_EX_ROT], tol, t);
    const bool oq = audit_figure(audit, AUDIT_MAX_Q, -1, tube[TUBE_EX_Q], AUDIT_JOINT_TOL, t);
    const bool odq = audit_figure(audit, AUDIT_MAX_DQ, -1, tube[TUBE_EX_DQ], AUDIT_JOINT_TOL, t);
    if (op) audit[AUDIT_N_POS] += 1.0;
    if (orot) audit[AUDIT_N_ROT] += 1.0;
    if (oq || odq) audit[AUDIT_N_JOINT] += 1.0;
    if ((op || orot) && audit[AUDIT_FIRST_OUT] < 0.0) audit[AUDIT_FIRST_OUT] = (double)t;
}

}  // namespace bmpcs
