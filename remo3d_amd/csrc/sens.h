// sens.h — adjoint sensitivities of linear measurement functionals to the material conductivities (remo_solve_batch_sens):
// the element contraction shared by host and gfx950 code, and the launchers of sens.hip (per material, and per caller-defined
// group of elements: remo_solve_batch_sens_groups).
//
// With A(sigma) u = f, J = g^T u and A lambda = g:  dJ/dsigma_m = -lambda^T (dA/dsigma_m) u, and dA/dsigma_m is the sum of the
// element matrices of material m with their sigma taken out.  Per element (fem_p3.h: K_e = sum_t C_e[t] M[t], C = sigma-free
// geometry times sigma), with x_l / x_u the element vectors of lambda / u:
//   3D: through the factorised reference tensors, g^l = B x_l, g^u = B x_u (B[a][m][i], ref_tables.cpp), mapped to physical
//       gradients G[p][m] = sum_a grad(l_a)[p] g[a][m]:   T_pq = |T| sum_m G^l[p][m] G^u[q][m]  ( = int d_p lambda d_q u )
//   2D: h_t = sum_k r_k x_l^T M[3k + t] x_u  (t = (a,b), a <= b; M symmetrised in (a,b) and weighted by l_k as in k_metric_terms),
//       value = 2 pi |T| sum_t h_t d(grad(l_a)^T S grad(l_b)) / dS_pq
// Scalar sigma: the trace (S = sigma I).  Tensor sigma: the upper triangle in the layout of sigma_tensor, the derivative with
// respect to the parameter that sets both S_pq and S_qp, so off-diagonal components carry both halves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elem_access.h"
#include "fem_p3.h"

namespace remo {

template <int DIM, bool TENSOR> struct SensOut { static constexpr int N = TENSOR ? SigmaTensor<DIM>::N : 1; };

// lambda_e^T (dK_e / d component) u_e of one element.  X: sorted vertex coordinates; tab: 2D the reference tensors M[9][10][10],
// 3D the factors B[3][10][20]; xl / xu: element vectors (constrained dofs 0).  Returns false for a degenerate element.
template <int DIM, bool TENSOR>
REMO_HD bool sens_element(const double *X, const double *tab, const double *xl, const double *xu, double *out) {
    constexpr int N = P3<DIM>::NLD;
    double g[DIM][DIM];
    const double vol = bary_gradients<DIM>(X, g);
    if (!(vol > 0.0)) return false;
    if constexpr (DIM == 3) {
        double T[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
        for (int m = 0; m < 10; ++m) {
            double gl[3], gu[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double *Bam = tab + (a * 10 + m) * N;
                double sl = 0.0, su = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i) { sl += Bam[i] * xl[i]; su += Bam[i] * xu[i]; }
                gl[a] = sl; gu[a] = su;
            }
            double Gl[3], Gu[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                Gl[p] = g[0][p] * gl[0] + g[1][p] * gl[1] + g[2][p] * gl[2];
                Gu[p] = g[0][p] * gu[0] + g[1][p] * gu[1] + g[2][p] * gu[2];
            }
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) T[p][q] += Gl[p] * Gu[q];
        }
        if constexpr (TENSOR) {
            out[0] = vol * T[0][0]; out[1] = vol * (T[0][1] + T[1][0]); out[2] = vol * (T[0][2] + T[2][0]);
            out[3] = vol * T[1][1]; out[4] = vol * (T[1][2] + T[2][1]); out[5] = vol * T[2][2];
        } else {
            out[0] = vol * (T[0][0] + T[1][1] + T[2][2]);
        }
    } else {
        double h[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double r = X[2 * k];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const double *Mt = tab + (3 * k + t) * N * N;
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    double w = 0.0;
#pragma unroll
                    for (int j = 0; j < N; ++j) w += Mt[i * N + j] * xu[j];
                    s += xl[i] * w;
                }
                h[t] += r * s;
            }
        }
        const double s2 = 6.283185307179586476925286766559 * vol;
        // t = (0,0), (0,1), (1,1): d(g_a^T S g_b)/dS_pq = g_a[p] g_b[q] (+ g_a[q] g_b[p] off the diagonal)
        if constexpr (TENSOR) {
            out[0] = s2 * (h[0] * g[0][0] * g[0][0] + h[1] * g[0][0] * g[1][0] + h[2] * g[1][0] * g[1][0]);
            out[1] = s2 * (h[0] * 2.0 * g[0][0] * g[0][1] + h[1] * (g[0][0] * g[1][1] + g[0][1] * g[1][0]) + h[2] * 2.0 * g[1][0] * g[1][1]);
            out[2] = s2 * (h[0] * g[0][1] * g[0][1] + h[1] * g[0][1] * g[1][1] + h[2] * g[1][1] * g[1][1]);
        } else {
            out[0] = s2 * (h[0] * (g[0][0] * g[0][0] + g[0][1] * g[0][1]) + h[1] * (g[0][0] * g[1][0] + g[0][1] * g[1][1]) +
                           h[2] * (g[1][0] * g[1][0] + g[1][1] * g[1][1]));
        }
    }
    return true;
}

const double *ref_factors3();   // ref_tables.cpp

// Which solution columns one functional contracts, and (2D, condensed) the points whose bubble loads belong to them.
struct SensColumns {
    const double *xu; int ku, cu;     // forward block [n][ku], column cu
    const double *xl; int kl, cl;     // adjoint block [n][kl], column cl
    int qu0, nqu, ql0, nql;           // points of the forward / adjoint chunk (indices into the point arrays)
};

constexpr int kSensBlock = 256;       // elements per tile of k_sens_contract
// materials x components a workgroup accumulates in LDS (dynamic, beside 14 KB of static tables)
constexpr int kSensMaxAcc = 4096;
int sens_grid(int64_t nt);
// part[grid][nmat * nc]: per-workgroup sums of lambda_e^T (dK_e/d component) u_e by material, every entry written
// pl: the point arrays of the whole batch (SensColumns indexes them); its nq is not read
void launch_sens_contract(const ElemMesh &em, const double *tab, const SensColumns &col, const PointLoads &pl, double *part, hipStream_t s,
                          bool per_elem = false);   // per_elem: part = ev[nt][nc], the values of every device element instead (no material sums)
// dJ[j][nmat * nc] = -(sum over the workgroups, in index order) for n_fun functionals whose partials lie one after the other
void launch_sens_reduce(int n_fun, int grid, int nmc, const double *part, double *dJ, hipStream_t s);

// ---- sums per group of elements (remo_solve_batch_sens_groups) ------------------------------------------------------------------
constexpr int kSensChunk = 1024;      // sorted positions per workgroup of the chunk pass; longer segments are summed in two levels
size_t sens_group_sort_bytes(int64_t nt, int32_t n_group);   // temporary storage of the radix sort (no device work)
int64_t sens_group_chunks(int64_t nt);                        // cpart holds 2 * nc doubles per chunk
// Once per batch: keys_in[t] = group[eperm ? eperm[t] : t] (-1 -> n_group), ids[t] = t, sorted (stable) into keys / perm, and
// off[0 .. n_group]: the segment of group g is perm[off[g] .. off[g + 1]); the elements in no group lie behind off[n_group].
void sens_group_order(int64_t nt, const int32_t *group, const int32_t *eperm, int32_t n_group, uint32_t *keys_in, int32_t *ids, uint32_t *keys, int32_t *perm,
                      int32_t *off, void *tmp, size_t tmp_bytes, hipStream_t s);
// dJg[n_group][nc] = -(sum of ev over the group's segment), fixed order, every entry written (an empty group: 0)
void launch_sens_group_sum(int nc, int64_t nt, int32_t n_group, const uint32_t *keys, const int32_t *perm, const int32_t *off, const double *ev,
                           double *cpart, double *dJg, hipStream_t s);
// The same for nq functionals in one launch of either kernel (the pairs of a slice, pairs.h): the values of functional q at
// ev + q * ev_stride, its sums to dJg + q * out_stride, cpart[nq][chunks][2][nc].  Per (q, group) the additions are those above.
void launch_sens_group_sum_batch(int nc, int64_t nt, int32_t n_group, const uint32_t *keys, const int32_t *perm, const int32_t *off, const double *ev,
                                 double *cpart, double *dJg, int nq, int64_t ev_stride, int64_t out_stride, hipStream_t s);

}  // namespace remo
