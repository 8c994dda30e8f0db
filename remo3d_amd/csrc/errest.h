// errest.h — goal-oriented error estimates of linear measurement functionals (remo_job_error_t.err): the facet term of the
// indicator, shared by host and gfx950 code, and the launchers of errest.hip.
//
// For a solution column v (a forward solution u_c or an adjoint solution lambda_j), an element e with sorted vertices and a facet
// F of e (a face in 3D, an edge in 2D) with unit normal n pointing out of e, q_e = n . Sigma_e grad v_h|_e:
//     interior facet, shared with e':     [q] = q_e - n . Sigma_e' grad v_h|_e',  s_F = (n.Sigma_e n + n.Sigma_e' n) / 2,  c_F = 1/2
//     boundary facet, not Dirichlet:      [q] = q_e,                              s_F = n.Sigma_e n,                       c_F = 1
//     Dirichlet facet:                    0
//     eta_e(v)^2 = sum_F c_F h_F / (2 p s_F) int_F [q]^2 dS,   p = 3, h_F the longest edge of F, dS with 2 pi r in 2D.
// [q]^2 is a polynomial of degree 4 on F (degree 5 with the weight r): three Gauss-Legendre points on an edge and the symmetric
// six-point rule of degree 4 on a triangle integrate it exactly.  Per functional j that reads right-hand side c(j):
//     E_je = eta_e(u_c(j)) eta_e(lambda_j),   E_j = sum_e E_je   (J(u) - J(u_h) = a(u - u_h, lambda - lambda_h), bounded element by element).
// The constant is the conventional one, not a sharp one; the delta sources are not part of the residual.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.h"

namespace remo {

// facet rule: per point the DIM barycentrics of the facet's (sorted) vertices and the weight, weights summing to 1
template <int DIM> struct ErrRule {
    static constexpr int NQ = (DIM == 2) ? 3 : 6;
    static constexpr int STRIDE = DIM + 1;
    static constexpr int NTAB = NQ * STRIDE;
};
const double *err_rule(int dim);   // host table (errest.hip)

// n^T Sigma n for the scalar or the upper-triangle tensor S
template <int DIM, bool TENSOR> REMO_HD double err_nSn(const double *n, const double *S) {
    if constexpr (!TENSOR) return S[0];
    else if constexpr (DIM == 2) return S[0] * n[0] * n[0] + 2.0 * S[1] * n[0] * n[1] + S[2] * n[1] * n[1];
    else
        return S[0] * n[0] * n[0] + S[3] * n[1] * n[1] + S[5] * n[2] * n[2] + 2.0 * (S[1] * n[0] * n[1] + S[2] * n[0] * n[2] + S[4] * n[1] * n[2]);
}

// c_F h_F / (2 p s_F) int_F [q]^2 dS of facet f of element e (f: 3D the faces 012 013 023 123, 2D the edges 01 02 12 - the facet
// opposite vertex DIM - f).  Xe, ge, vol_e: sorted vertex coordinates, bary_gradients and measure of e; xe: its element vector
// (constrained dofs 0); Se: its conductivity (one scalar or the upper triangle).  interior: the same of the neighbour e' in
// Xn, xn, Sn, else the facet is a natural boundary.  rule: ErrRule<DIM>.  A degenerate neighbour gives 0.
template <int DIM, bool TENSOR>
REMO_HD double error_facet(const double *rule, int f, const double *Xe, const double (*ge)[DIM], double vol_e, const double *xe, const double *Se,
                           bool interior, const double *Xn, const double *xn, const double *Sn) {
    constexpr int NB = DIM + 1, NO = FieldOut<DIM>::N;
    const int o = DIM - f;   // the vertex opposite the facet
    double n[DIM], gl = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) s += (o == 0) ? -ge[a][k] : ((a == o - 1) ? ge[a][k] : 0.0);
        n[k] = -s;   // -grad(l_o): out of e
        gl += s * s;
    }
    gl = sqrt(gl);
#pragma unroll
    for (int k = 0; k < DIM; ++k) n[k] /= gl;
    const double area = double(DIM) * vol_e * gl;   // |F| = DIM |T| |grad(l_o)|
    double h2 = 0.0;   // the longest edge of F
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int j = i + 1; j < DIM; ++j) {
            const int vi = (i < o) ? i : i + 1, vj = (j < o) ? j : j + 1;
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) { const double d = Xe[vi * DIM + k] - Xe[vj * DIM + k]; d2 += d * d; }
            h2 = d2 > h2 ? d2 : h2;
        }
    double gn[DIM][DIM];
    double sF = err_nSn<DIM, TENSOR>(n, Se);
    if (interior) {
        if (!(bary_gradients<DIM>(Xn, gn) > 0.0)) return 0.0;
        sF = 0.5 * (sF + err_nSn<DIM, TENSOR>(n, Sn));
    }
    double acc = 0.0;
    for (int q = 0; q < ErrRule<DIM>::NQ; ++q) {
        const double *rq = rule + q * ErrRule<DIM>::STRIDE;
        double l[NB], P[DIM], out[NO];
#pragma unroll
        for (int k = 0; k < DIM; ++k) P[k] = 0.0;
#pragma unroll
        for (int a = 0; a < NB; ++a) {
            const int j = (a < o) ? a : a - 1;   // position of vertex a among the facet's vertices
            l[a] = (a == o) ? 0.0 : rq[j];
#pragma unroll
            for (int k = 0; k < DIM; ++k) P[k] += l[a] * Xe[a * DIM + k];
        }
        field_element<DIM, TENSOR>(ge, l, xe, Se, out);
        double jump = 0.0;   // n . Sigma grad v = -n . J
#pragma unroll
        for (int k = 0; k < DIM; ++k) jump -= n[k] * out[1 + DIM + k];
        if (interior) {
            double ln[NB];
            bary_from_gradients<DIM>(Xn, gn, P, ln);
            field_element<DIM, TENSOR>(gn, ln, xn, Sn, out);
#pragma unroll
            for (int k = 0; k < DIM; ++k) jump += n[k] * out[1 + DIM + k];
        }
        const double w = (DIM == 2) ? rq[DIM] * 6.283185307179586476925286766559 * P[0] : rq[DIM];
        acc += w * jump * jump;
    }
    return (interior ? 0.5 : 1.0) * sqrt(h2) / (6.0 * sF) * area * acc;
}

// ---- launchers (errest.hip) ---------------------------------------------------------------------------------------------------------
// eta2[c * nt + t] = eta_t(column c)^2 for the k columns of the solution block x[n][k] and every device element t, one launch.  The
// neighbour across a facet comes from the adjacency list of the facet's dof row (eldof: local dofs 16 .. 19 in 3D, the first dof of
// each edge in 2D; row -1: a Dirichlet facet).  src: the chunk's axis points (2D, condensed: the bubble loads, as k_field_eval reads
// them).  rule: device copy of err_rule(dim).
void launch_error_facets(const ElemMesh &em, const double *rule, int k, const double *x, const PointLoads &src, double *eta2, hipStream_t s);
// ev[t] = -sqrt(eu[t] * el[t]) (ev may be nullptr) and part[workgroup] = the workgroup's sum of them, sens_grid(nt) workgroups in a
// fixed order: launch_sens_reduce / launch_sens_group_sum, which negate, then give E_j and the group sums.
void launch_error_combine(int64_t nt, const double *eu, const double *el, double *ev, double *part, hipStream_t s);

}  // namespace remo
