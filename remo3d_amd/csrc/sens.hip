// sens.hip — gfx950 kernels of the adjoint sensitivities (remo_solve_batch_sens; the functional is the reading of
// worker.py:113-131): one pass over the elements per functional, contracting the element vectors of the adjoint and the forward
// solution with the sigma-free element terms (sens.h), summed per material in a fixed order.
//
// k_sens_contract: one lane per element, tiles of 256 elements walked grid-stride by at most kMaxPartialBlocks workgroups.  The
// element values of a tile go to LDS; lane (material, component) then adds the tile's values of its material in element order
// to its accumulator - no floating-point atomics, so the result depends only on the mesh.  k_sens_reduce adds the workgroups'
// partial sums in index order.  The gathers of the 2 x 20 (10) rows of x are what the kernel waits for; the tables (B: 4.8 KB,
// 2D M: 7.2 KB) sit in LDS and are read as broadcasts.
#include <limits.h>

#include "kernels.h"
#include "sens.h"

namespace remo {

namespace {

// element vector of column c of x[n][k]: constrained rows read 0; NK rows are gathered (2D condensed: the bubble follows below)
template <int N, int NK>
__device__ __forceinline__ void gather_rows(const int32_t *__restrict__ ed, const double *__restrict__ x, int k, int c, double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int32_t row = (i < NK) ? ed[i] : -1;
        v[i] = (row >= 0) ? x[int64_t(row) * k + c] : 0.0;
    }
}

// condensed cell bubble of one column, as k_eval recovers it: x_9 = (f_9 - sum_j K_9j x_j) / K_99, f_9 the bubble loads of the
// column's points that lie in this element
__device__ __forceinline__ void recover_bubble(int32_t t, const double *ce, const double *M, int c, int q0, int nq, const int32_t *__restrict__ pt_rhs,
                                               const double *__restrict__ pt_I, const int32_t *__restrict__ found, const double *__restrict__ fint,
                                               double (&v)[10]) {
    double acc = 0.0;
    for (int w = q0; w < q0 + nq; ++w)
        if (pt_I[w] != 0.0 && found[w] == t && pt_rhs[w] == c) acc += fint[w];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc -= kentry<2>(ce, M, 9, j) * v[j];
    v[9] = acc / kentry<2>(ce, M, 9, 9);
}

}  // namespace

template <int DIM, bool CONDENSE, bool TENSOR>
__global__ void __launch_bounds__(kSensBlock) k_sens_contract(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                              const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm,
                                                              const int32_t *__restrict__ eldof, const double *__restrict__ C,
                                                              const double *__restrict__ M, const double *__restrict__ tab, SensColumns col,
                                                              const int32_t *__restrict__ pt_rhs, const double *__restrict__ pt_I,
                                                              const int32_t *__restrict__ found, const double *__restrict__ fint, int nmat,
                                                              double *__restrict__ part) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = (DIM == 2 && CONDENSE) ? 9 : N, NC = SensOut<DIM, TENSOR>::N;
    constexpr int NTAB = (DIM == 2) ? 9 * N * N : 3 * 10 * N;
    __shared__ double s_tab[NTAB];
    __shared__ double s_val[kSensBlock * NC];
    __shared__ int32_t s_mat[kSensBlock];
    __shared__ int32_t s_range[2];
    extern __shared__ double s_acc[];   // [nmat * NC]
    const int tid = threadIdx.x, nmc = nmat * NC;
    for (int i = tid; i < NTAB; i += kSensBlock) s_tab[i] = tab[i];
    for (int i = tid; i < nmc; i += kSensBlock) s_acc[i] = 0.0;
    const int64_t ntiles = (nt + kSensBlock - 1) / kSensBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) { s_range[0] = INT_MAX; s_range[1] = -1; }
        __syncthreads();   // (first tile: the tables; later tiles: the scan of the tile before)
        const int64_t t = tile * kSensBlock + tid;
        double out[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) out[c] = 0.0;
        int32_t m = -1;
        if (t < nt) {
            m = mat[eperm ? int64_t(eperm[t]) : t];
            if (m < 0 || m >= nmat) m = -1;   // (k_metric_terms has flagged it: the batch fails before these sums are read)
            double X[NB * DIM];
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                const int64_t v = conn[t * NB + a];
#pragma unroll
                for (int k = 0; k < DIM; ++k) X[a * DIM + k] = coords[v * DIM + k];
            }
            const int32_t *ed = eldof + t * N;
            double xl[N], xu[N];
            gather_rows<N, NK>(ed, col.xu, col.ku, col.cu, xu);
            gather_rows<N, NK>(ed, col.xl, col.kl, col.cl, xl);
            if constexpr (DIM == 2 && CONDENSE) {
                const double *ce = C + t * NT;
                recover_bubble(int32_t(t), ce, M, col.cu, col.qu0, col.nqu, pt_rhs, pt_I, found, fint, xu);
                recover_bubble(int32_t(t), ce, M, col.cl, col.ql0, col.nql, pt_rhs, pt_I, found, fint, xl);
            }
            if (m >= 0 && !sens_element<DIM, TENSOR>(X, s_tab, xl, xu, out)) {
#pragma unroll
                for (int c = 0; c < NC; ++c) out[c] = 0.0;
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) s_val[tid * NC + c] = out[c];
        s_mat[tid] = m;
        if (m >= 0) { atomicMin(&s_range[0], m); atomicMax(&s_range[1], m); }   // integer LDS atomics: the span of materials of the tile
        __syncthreads();
        const int m0 = s_range[0], span = s_range[1] - m0 + 1;
        for (int idx = tid; idx < span * NC; idx += kSensBlock) {
            const int mm = m0 + idx / NC, c = idx - (idx / NC) * NC;
            double s = 0.0;
            for (int e = 0; e < kSensBlock; ++e) s += (s_mat[e] == mm) ? s_val[e * NC + c] : 0.0;   // element order
            s_acc[mm * NC + c] += s;
        }
        __syncthreads();
    }
    __syncthreads();
    for (int i = tid; i < nmc; i += kSensBlock) part[int64_t(blockIdx.x) * nmc + i] = s_acc[i];
}

// one lane per (functional, material, component): the workgroups' partial sums in index order; dJ = -lambda^T A_k u
__global__ void __launch_bounds__(256) k_sens_reduce(int n_fun, int grid, int nmc, const double *__restrict__ part, double *__restrict__ dJ) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fun * nmc) return;
    const int j = i / nmc, mc = i - j * nmc;
    const double *p = part + int64_t(j) * grid * nmc + mc;
    double s = 0.0;
    for (int w = 0; w < grid; ++w) s += p[int64_t(w) * nmc];
    dJ[i] = -s;
}

int sens_grid(int64_t nt) {
    const int64_t ntiles = (nt + kSensBlock - 1) / kSensBlock;
    return int(ntiles < kMaxPartialBlocks ? (ntiles > 0 ? ntiles : 1) : kMaxPartialBlocks);
}

void launch_sens_contract(int dim, bool condense, bool tensor, int64_t nt, const double *coords, const int32_t *conn, const int32_t *mat,
                          const int32_t *eperm, const int32_t *eldof, const double *C, const double *M, const double *tab, const SensColumns &col,
                          const int32_t *pt_rhs, const double *pt_I, const int32_t *found, const double *fint, int nmat, double *part, hipStream_t s) {
    const int grid = sens_grid(nt);
    const size_t lds = sizeof(double) * size_t(nmat) * (tensor ? (dim == 2 ? 3 : 6) : 1);
#define REMO_SENS_LAUNCH(D, CO, TE) \
    hipLaunchKernelGGL((k_sens_contract<D, CO, TE>), dim3(grid), dim3(kSensBlock), lds, s, nt, coords, conn, mat, eperm, eldof, C, M, tab, col, pt_rhs, \
                       pt_I, found, fint, nmat, part)
    if (dim == 3) {
        if (tensor) REMO_SENS_LAUNCH(3, false, true); else REMO_SENS_LAUNCH(3, false, false);
    } else if (condense) {
        if (tensor) REMO_SENS_LAUNCH(2, true, true); else REMO_SENS_LAUNCH(2, true, false);
    } else {
        if (tensor) REMO_SENS_LAUNCH(2, false, true); else REMO_SENS_LAUNCH(2, false, false);
    }
#undef REMO_SENS_LAUNCH
}

void launch_sens_reduce(int n_fun, int grid, int nmc, const double *part, double *dJ, hipStream_t s) {
    const int total = n_fun * nmc;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_sens_reduce, dim3((total + 255) / 256), dim3(256), 0, s, n_fun, grid, nmc, part, dJ);
}

}  // namespace remo
