// pairs.hip — gfx950 kernel of the pair derivatives (remo_job_pairs_t, pairs.h): one pass over the elements for all pairs of the
// columns of one or two chunks of right-hand sides.
//
// k_pair_contract: tiles of `te` elements (pair_tile: 8 to 32, by the number of staged columns) walked grid-stride.  Per tile
//   0. lane e < te: material, |T|, grad(l) and (2D) the radii of element e -> LDS;
//   1. one lane per (element, column), the column running fastest - a row of x[n][k] brings the chunk's columns in one segment:
//      the element vector is gathered once (2D, condensed: the bubble recovered with the point loads of the column's own chunk),
//      the moments formed (pair_moments: the tables are LDS broadcasts) and staged in LDS.  Strides of an odd number of doubles
//      per column and per element keep the lanes of phases 1 and 2 on different banks;
//   2. rounds of 256 / te pairs: one lane per (pair, element) forms the value from the two staged moment vectors (pair_value);
//      the values go to LDS and lane (pair, material, component) adds those of its material in element order to its
//      accumulator - the scheme of k_sens_contract, no floating-point atomics.
// The workgroups' accumulators go to part[pair][workgroup][material * component]; k_sens_reduce (sens.hip) adds them in index
// order.  Every sum depends only on the mesh, the job and the grid.
//
// k_pair_contract<.., PER_ELEM = true> (remo_job_pair_groups_t): phases 0 and 1 as above; phase 2 writes the value of every (pair,
// element) to ev[q][t][NC] - q the pair's position in the launch, t the device element - instead of scanning by material: lane =
// (pair, element) with the element fastest, so a tile's values of one pair are one contiguous segment.  Every t < nt is written, a
// dead element writes 0.  No accumulators, no span of materials, no value buffer in LDS; sens.hip's group sums read ev.
// The reads of an element (vertices, material, a column's element vector, the condensed bubble) are elem_access.h's, as in k_sens_contract.
#include <limits.h>

#include "elem_access.h"
#include "kernels.h"
#include "pairs.h"

namespace remo {

namespace {

template <int DIM> constexpr int pair_col_stride() { return PairMom<DIM>::N + 1; }                         // 31 / 41 doubles
__host__ __device__ inline int pair_elem_stride(int dim, int ncol) { return (ncol * (dim == 3 ? 31 : 41)) | 1; }

}  // namespace

// colbits: 4 bits per slot - bit 3 the block, bits 0 .. 2 the column in it (PairColumns::col, packed: a run-time index into a
// kernel argument would send the array through scratch)
template <int DIM, bool CONDENSE, bool TENSOR, bool PER_ELEM>
__global__ void __launch_bounds__(kPairBlock) k_pair_contract(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                              const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm,
                                                              const int32_t *__restrict__ eldof, const double *__restrict__ C,
                                                              const double *__restrict__ M, const double *__restrict__ tab,
                                                              const double *__restrict__ x0, const double *__restrict__ x1, int k0, int k1, int q00,
                                                              int nq0, int q01, int nq1, int ncol, unsigned long long colbits, int te, int np,
                                                              const int32_t *__restrict__ slots, const int32_t *__restrict__ pt_rhs,
                                                              const double *__restrict__ pt_I, const int32_t *__restrict__ found,
                                                              const double *__restrict__ fint, int nmat, double *__restrict__ part) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = (DIM == 2 && CONDENSE) ? 9 : N, NC = SensOut<DIM, TENSOR>::N;
    constexpr int NTAB = (DIM == 2) ? 9 * N * N : 3 * 10 * N, CS = pair_col_stride<DIM>();
    constexpr int NGEO = 1 + DIM * DIM + (DIM == 2 ? 3 : 0);   // |T|, grad(l_a)[p], 2D: r_k
    __shared__ double s_tab[NTAB];
    __shared__ double s_val[PER_ELEM ? 1 : kPairBlock * NC];
    __shared__ double s_geo[kPairTileMax * NGEO];
    __shared__ int32_t s_mat[kPairTileMax];
    __shared__ int32_t s_range[2];
    extern __shared__ double s_dyn[];   // moments [te][es], then (!PER_ELEM) the accumulators [np][nmat * NC]
    const int tid = threadIdx.x, nmc = PER_ELEM ? 0 : nmat * NC, es = pair_elem_stride(DIM, ncol);
    double *s_mom = s_dyn, *s_acc = s_dyn + te * es;
    for (int i = tid; i < NTAB; i += kPairBlock) s_tab[i] = tab[i];
    for (int i = tid; i < np * nmc; i += kPairBlock) s_acc[i] = 0.0;
    const int64_t ntiles = (nt + te - 1) / te;
    const int ppr = kPairBlock / te;   // pairs per round
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (!PER_ELEM && tid == 0) { s_range[0] = INT_MAX; s_range[1] = -1; }
        __syncthreads();   // (first tile: the tables; later tiles: the scan / the pair values of the tile before)
        // ---- 0: the elements of the tile ------------------------------------------------------------------------------------
        if (tid < te) {
            const int64_t t = tile * te + tid;
            int32_t m = -1;
            if (t < nt) {
                m = elem_material(mat, eperm, t, nmat);
                double X[NB * DIM], g[DIM][DIM];
                load_vertices<DIM>(coords, conn, t, X);
                const double vol = bary_gradients<DIM>(X, g);
                if (!(vol > 0.0)) m = -1;
                double *geo = s_geo + tid * NGEO;
                geo[0] = vol;
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int p = 0; p < DIM; ++p) geo[1 + a * DIM + p] = g[a][p];
                if constexpr (DIM == 2) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) geo[1 + DIM * DIM + k] = X[2 * k];
                }
            }
            s_mat[tid] = m;
            if (!PER_ELEM && m >= 0) { atomicMin(&s_range[0], m); atomicMax(&s_range[1], m); }   // integer LDS atomics: the span of materials of the tile
        }
        __syncthreads();
        // ---- 1: moments of every (element, column) ------------------------------------------------------------------------------
        for (int it = tid; it < te * ncol; it += kPairBlock) {
            const int e = it / ncol, sl = it - e * ncol;
            const int64_t t = tile * te + e;
            if (t >= nt || s_mat[e] < 0) continue;
            const int cb = int(colbits >> (4 * sl)) & 15, blk = cb >> 3, c = cb & 7;
            const double *__restrict__ x = blk ? x1 : x0;
            const int k = blk ? k1 : k0;
            const int32_t *ed = eldof + t * N;
            double v[N];
            gather_column<N, NK>(ed, x, k, c, v);
            if constexpr (DIM == 2 && CONDENSE) recover_bubble(int32_t(t), C + t * NT, M, c, blk ? q01 : q00, blk ? nq1 : nq0, pt_rhs, pt_I, found, fint, v);
            const double *geo = s_geo + e * NGEO;
            double g[DIM][DIM], X[NB * DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a)
#pragma unroll
                for (int p = 0; p < DIM; ++p) g[a][p] = geo[1 + a * DIM + p];
#pragma unroll
            for (int i = 0; i < NB * DIM; ++i) X[i] = 0.0;
            if constexpr (DIM == 2) {
#pragma unroll
                for (int k2 = 0; k2 < 3; ++k2) X[2 * k2] = geo[1 + DIM * DIM + k2];   // (pair_moments reads the radii alone)
            }
            pair_moments<DIM>(X, g, s_tab, v, s_mom + e * es + sl * CS);
        }
        __syncthreads();
        // ---- 2: the pairs, a round at a time; sums per material in element order ----------------------------------------------------
        if constexpr (PER_ELEM) {   // ... or every value to ev[q][t][NC] (part = ev): nothing in LDS is written, so no barrier between rounds
            const int e = tid % te, pl = tid / te;
            const int64_t t = tile * te + e;
            if (pl < ppr && t < nt) {
                const double *geo = s_geo + e * NGEO;
                double g[DIM][DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int q = 0; q < DIM; ++q) g[a][q] = geo[1 + a * DIM + q];
                const bool live = s_mat[e] >= 0;
                for (int p = pl; p < np; p += ppr) {
                    double out[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) out[c] = 0.0;
                    if (live) pair_value<DIM, TENSOR>(geo[0], g, s_mom + e * es + slots[2 * p] * CS, s_mom + e * es + slots[2 * p + 1] * CS, out);
                    double *dst = part + (int64_t(p) * nt + t) * NC;
#pragma unroll
                    for (int c = 0; c < NC; ++c) dst[c] = out[c];
                }
            }
            continue;
        }
        const int m0 = s_range[0], span = s_range[1] - m0 + 1;   // (span <= 0: no live element in the tile)
        for (int p0 = 0; p0 < np; p0 += ppr) {
            const int e = tid % te, pl = tid / te, p = p0 + pl;
            double out[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) out[c] = 0.0;
            if (pl < ppr && p < np && s_mat[e] >= 0) {
                const int sa = slots[2 * p], sb = slots[2 * p + 1];
                const double *geo = s_geo + e * NGEO;
                double g[DIM][DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a)
#pragma unroll
                    for (int q = 0; q < DIM; ++q) g[a][q] = geo[1 + a * DIM + q];
                pair_value<DIM, TENSOR>(geo[0], g, s_mom + e * es + sa * CS, s_mom + e * es + sb * CS, out);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) s_val[tid * NC + c] = out[c];
            __syncthreads();
            const int npr = (np - p0 < ppr) ? np - p0 : ppr;
            for (int idx = tid; idx < npr * span * NC; idx += kPairBlock) {
                const int q = idx / (span * NC), rem = idx - q * (span * NC), mm = m0 + rem / NC, c = rem - (rem / NC) * NC;
                double s = 0.0;
                for (int i = 0; i < te; ++i) s += (s_mat[i] == mm) ? s_val[(q * te + i) * NC + c] : 0.0;   // element order
                s_acc[(p0 + q) * nmc + mm * NC + c] += s;
            }
            __syncthreads();
        }
    }
    if constexpr (!PER_ELEM) {
        __syncthreads();
        for (int i = tid; i < np * nmc; i += kPairBlock) {
            const int p = i / nmc, mc = i - p * nmc;
            part[(int64_t(p) * gridDim.x + blockIdx.x) * nmc + mc] = s_acc[i];
        }
    }
}

int pair_tile(int dim, int ncol, size_t acc_bytes) {
    // with the largest accumulator block (kSensMaxAcc doubles) the moments give way, so that a workgroup stays below 80 KB
    const size_t room = 57344 - (acc_bytes < 57344 - 8192 ? acc_bytes : 57344 - 8192);
    const size_t budget = room < size_t(kPairMomBytes) ? room : size_t(kPairMomBytes);
    int te = kPairTileMax;
    while (te > 2 && size_t(te) * size_t(pair_elem_stride(dim, ncol)) * 8 > budget) te >>= 1;
    return te;
}

int pair_grid(int64_t nt) {
    const int64_t ntiles = (nt + kPairTileMax - 1) / kPairTileMax;
    return int(ntiles < kMaxPartialBlocks ? (ntiles > 0 ? ntiles : 1) : kMaxPartialBlocks);
}

void launch_pair_contract(const ElemMesh &em, const double *tab, const PairColumns &pc, int np, const int32_t *slots, const PointLoads &pl, int grid,
                          double *part, hipStream_t s, bool per_elem) {
    const int dim = em.dim, nc = em.tensor() ? (dim == 2 ? 3 : 6) : 1;
    const size_t acc = per_elem ? 0 : sizeof(double) * size_t(np) * size_t(em.n_mat) * nc;
    const int te = pair_tile(dim, pc.ncol, acc);
    const size_t lds = sizeof(double) * size_t(te) * size_t(pair_elem_stride(dim, pc.ncol)) + acc;
    unsigned long long colbits = 0;
    for (int i = 0; i < pc.ncol; ++i) colbits |= (unsigned long long)(pc.col[i] & 15) << (4 * i);
    for_elem_kind(dim, em.condense, em.tensor(), [&](auto d, auto co, auto tens) {
        constexpr int D = decltype(d)::value;
        constexpr bool CO = decltype(co)::value, TE = decltype(tens)::value;
        auto launch = [&](auto pe) {
            constexpr bool PE = decltype(pe)::value;
            static bool sized = false;   // static + dynamic LDS pass 64 KB: the kernel is allowed them once (one `sized` per instantiation of this body)
            if (!sized) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pair_contract<D, CO, TE, PE>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
                sized = true;
            }
            hipLaunchKernelGGL((k_pair_contract<D, CO, TE, PE>), dim3(grid), dim3(kPairBlock), lds, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.eldof, em.C, em.M, tab, pc.x[0],
                               pc.x[1], pc.k[0], pc.k[1], pc.q0[0], pc.nq[0], pc.q0[1], pc.nq[1], pc.ncol, colbits, te, np, slots, pl.pt_rhs, pl.pt_I, pl.found,
                               pl.fint, em.n_mat, part);
        };
        if (per_elem) launch(std::true_type{}); else launch(std::false_type{});
    });
}

}  // namespace remo
