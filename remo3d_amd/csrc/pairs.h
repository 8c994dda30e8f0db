// pairs.h — derivatives of all transfer impedances of an electrode array by reciprocity (remo_job_pairs_t): the element arithmetic
// shared by host and gfx950 code, and the launcher of pairs.hip.
//
// A is symmetric, so the adjoint of "read u at electrode i" is the forward solution of a source at electrode i:
//     Z_ij = e_i^T A^{-1} f_j,    dZ_ij/dsigma_m = -u_i^T (dA/dsigma_m) u_j,
// with u_i, u_j both forward columns of the batch.  sens_element (sens.h) forms x_l^T (dK_e / d component) x_u of one pair of
// columns in 1200 multiply-adds.  Its value factorises through MOMENTS that belong to one column alone:
//   3D: G[p][m] = sum_a grad(l_a)[p] (B x)[a][m], 30 numbers, the physical gradient moments of sens.h;
//       value(a, b) = |T| sum_m G^a[p][m] G^b[q][m]   (scalar sigma: p = q summed; tensor: T_pq + T_qp off the diagonal)
//   2D: W[t][i] = sum_k r_k sum_j M[3k + t][i][j] x_j, 30 numbers, beside x itself (40 in all);
//       h_t(a, b) = x^a . W^b[t], then the combination with grad(l) of sens_element.
// So an element forms the moments of every column once (600 multiply-adds in 3D, 900 in 2D) and every pair costs an inner
// product of 30 (tensor 3D: 90) more.  M[3k + t] is symmetric in (i, j): value(a, b) = value(b, a) up to rounding.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sens.h"

namespace remo {

template <int DIM> struct PairMom { static constexpr int N = (DIM == 3) ? 30 : 40; };   // doubles per column and element

// moments of one column.  X: sorted vertex coordinates; g: their bary_gradients; tab: 2D M[9][10][10], 3D B[3][10][20] (as sens_element);
// x: the element vector (constrained dofs 0); mom[PairMom<DIM>::N]
template <int DIM>
REMO_HD void pair_moments(const double *X, const double (*g)[DIM], const double *tab, const double *x, double *mom) {
    constexpr int N = P3<DIM>::NLD;
    // (the outer loops stay loops: unrolled whole, the 600 / 900 multiply-adds hoist their table reads and run out of registers;
    // mom is written element by element, so that the kernel hands its LDS slot and keeps no copy)
    if constexpr (DIM == 3) {
#pragma unroll 1
        for (int m = 0; m < 10; ++m) {
            double gm[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double *Bam = tab + (a * 10 + m) * N;
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < N; ++i) s += Bam[i] * x[i];
                gm[a] = s;
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) mom[p * 10 + m] = g[0][p] * gm[0] + g[1][p] * gm[1] + g[2][p] * gm[2];
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) mom[i] = x[i];
#pragma unroll 1
        for (int ti = 0; ti < 3 * N; ++ti) {   // ti = t * N + i
            const int t = ti / N, i = ti - t * N;
            double w = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double *Mt = tab + ((3 * k + t) * N + i) * N;
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < N; ++j) s += Mt[j] * x[j];
                w += X[2 * k] * s;
            }
            mom[N + ti] = w;
        }
    }
}

// x_a^T (dK_e / d component) x_b from the moments of columns a and b; out[SensOut<DIM, TENSOR>::N], the components of sens_element
template <int DIM, bool TENSOR>
REMO_HD void pair_value(double vol, const double (*g)[DIM], const double *ma, const double *mb, double *out) {
    if constexpr (DIM == 3) {
        if constexpr (TENSOR) {
            double T[3][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 10; ++m) s += ma[p * 10 + m] * mb[q * 10 + m];
                    T[p][q] = s;
                }
            out[0] = vol * T[0][0]; out[1] = vol * (T[0][1] + T[1][0]); out[2] = vol * (T[0][2] + T[2][0]);
            out[3] = vol * T[1][1]; out[4] = vol * (T[1][2] + T[2][1]); out[5] = vol * T[2][2];
        } else {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 30; ++i) s += ma[i] * mb[i];
            out[0] = vol * s;
        }
    } else {
        double h[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 10; ++i) s += ma[i] * mb[10 + t * 10 + i];
            h[t] = s;
        }
        const double s2 = 6.283185307179586476925286766559 * vol;
        if constexpr (TENSOR) {
            out[0] = s2 * (h[0] * g[0][0] * g[0][0] + h[1] * g[0][0] * g[1][0] + h[2] * g[1][0] * g[1][0]);
            out[1] = s2 * (h[0] * 2.0 * g[0][0] * g[0][1] + h[1] * (g[0][0] * g[1][1] + g[0][1] * g[1][0]) + h[2] * 2.0 * g[1][0] * g[1][1]);
            out[2] = s2 * (h[0] * g[0][1] * g[0][1] + h[1] * g[0][1] * g[1][1] + h[2] * g[1][1] * g[1][1]);
        } else {
            out[0] = s2 * (h[0] * (g[0][0] * g[0][0] + g[0][1] * g[0][1]) + h[1] * (g[0][0] * g[1][0] + g[0][1] * g[1][1]) +
                           h[2] * (g[1][0] * g[1][0] + g[1][1] * g[1][1]));
        }
    }
}

// ---- the element pass (pairs.hip) ---------------------------------------------------------------------------------------------
constexpr int kPairBlock = 256;       // lanes per workgroup
constexpr int kPairMaxCols = 16;      // columns one launch stages: two chunks of REMO_MAX_RHS
constexpr int kPairTileMax = 32;      // elements per tile at most (pair_tile: fewer with more columns)
constexpr int kPairMomBytes = 40960;  // LDS of a tile's moments; with the tables (7.2 KB), the values of a round (12 KB) and the
                                      // accumulators (16 KB) two workgroups share the 160 KB of a CU
constexpr int kPairSliceAcc = 2048;   // accumulators (pairs x materials x components) a launch keeps in LDS: more pairs, more launches

// One launch: the columns of one or two chunks of right-hand sides and the pairs among them.  Slot s of the staged columns is column
// col[s] & 7 of block (col[s] >> 3); a pair names two slots.
struct PairColumns {
    const double *x[2];               // solution blocks [n][k[i]]
    int k[2];
    int q0[2], nq[2];                 // the points of either chunk (2D, condensed: their bubble loads)
    int ncol;
    int8_t col[kPairMaxCols];
};

// elements per tile: the largest power of two whose moments fit kPairMomBytes (less where the accumulators take more than a slice's 16 KB)
int pair_tile(int dim, int ncol, size_t acc_bytes);
int pair_grid(int64_t nt);            // workgroups of every launch of a job (one count, so that one k_sens_reduce sums them all)
// part[p][grid][nmat * nc] for the np pairs slots[2 * p], slots[2 * p + 1] (device array): per-workgroup sums by material of
// x_a^T (dK_e / d component) x_b in element order, every entry written.  np * nmat * nc <= kSensMaxAcc.
// pl: the point arrays of the whole batch (PairColumns::q0 / nq index them); its nq is not read
void launch_pair_contract(const ElemMesh &em, const double *tab, const PairColumns &pc, int np, const int32_t *slots, const PointLoads &pl, int grid,
                          double *part, hipStream_t s, bool per_elem = false);
// per_elem: part = ev[np][nt][nc], the value of every (pair, device element) instead - every entry written, a dead element 0; no
// material sums, no bound on np (the caller slices by the bytes of ev: kPairEvBytes)
constexpr size_t kPairEvBytes = size_t(128) << 20;   // ev of one per-element launch (remo_debug_tune key 43); always one pair at least
constexpr int kPairEvMaxPairs = 65535;                // pairs of one launch: the second grid dimension of the group sums

}  // namespace remo
