// sens.hip — gfx950 kernels of the adjoint sensitivities (remo_solve_batch_sens; the functional is the reading of
// worker.py:113-131): one pass over the elements per functional, contracting the element vectors of the adjoint and the forward
// solution with the sigma-free element terms (sens.h), summed per material in a fixed order.
//
// k_sens_contract: one lane per element, tiles of 256 elements walked grid-stride by at most kMaxPartialBlocks workgroups.  The
// element values of a tile go to LDS; lane (material, component) then adds the tile's values of its material in element order
// to its accumulator - no floating-point atomics, so the result depends only on the mesh.  k_sens_reduce adds the workgroups'
// partial sums in index order.  The gathers of the 2 x 20 (10) rows of x are what the kernel waits for; the tables (B: 4.8 KB,
// 2D M: 7.2 KB) sit in LDS and are read as broadcasts.
//
// Per group of elements (remo_solve_batch_sens_groups): k_sens_contract<.., PER_ELEM = true> writes the element values to
// ev[t][nc] instead of scanning them by material; the elements are sorted by group once per batch (rocPRIM's stable radix sort:
// within a group the device element numbers ascend) and k_sens_group_long / k_sens_group_sum add every group's segment of the
// sorted list in an order that depends only on that list - lane l of the group's lanes adds the entries congruent to l in
// ascending order, a fixed butterfly combines the lanes; segments longer than kSensChunk are first summed per chunk of the
// sorted list by whole workgroups.  No floating-point atomics anywhere.
// The reads of an element (vertices, material, the two element vectors, the condensed bubble) are elem_access.h's.
#include <limits.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <stdexcept>

#include "elem_access.h"
#include "kernels.h"
#include "sens.h"
#include "wave_util.h"

namespace remo {

// PER_ELEM: the nc values of device element t go to part[t * nc + c] (part = ev) and the material scan is skipped
template <int DIM, bool CONDENSE, bool TENSOR, bool PER_ELEM>
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
    __shared__ double s_val[PER_ELEM ? 1 : kSensBlock * NC];
    __shared__ int32_t s_mat[PER_ELEM ? 1 : kSensBlock];
    __shared__ int32_t s_range[2];
    extern __shared__ double s_acc[];   // [nmat * NC]
    const int tid = threadIdx.x, nmc = PER_ELEM ? 0 : nmat * NC;
    for (int i = tid; i < NTAB; i += kSensBlock) s_tab[i] = tab[i];
    for (int i = tid; i < nmc; i += kSensBlock) s_acc[i] = 0.0;
    const int64_t ntiles = (nt + kSensBlock - 1) / kSensBlock;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (!PER_ELEM && tid == 0) { s_range[0] = INT_MAX; s_range[1] = -1; }
        __syncthreads();   // (first tile: the tables; later tiles: the scan of the tile before)
        const int64_t t = tile * kSensBlock + tid;
        double out[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) out[c] = 0.0;
        int32_t m = -1;
        if (t < nt) {
            m = elem_material(mat, eperm, t, nmat);
            double X[NB * DIM];
            load_vertices<DIM>(coords, conn, t, X);
            const int32_t *ed = eldof + t * N;
            double xl[N], xu[N];
            gather_column<N, NK>(ed, col.xu, col.ku, col.cu, xu);
            gather_column<N, NK>(ed, col.xl, col.kl, col.cl, xl);
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
        if constexpr (PER_ELEM) {
            if (t < nt) {
#pragma unroll
                for (int c = 0; c < NC; ++c) part[t * NC + c] = out[c];
            }
            continue;   // (no LDS is written after the tables: nothing to wait for between tiles)
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

// ---- sums per group of elements ------------------------------------------------------------------------------------------------
// sort key of device element t: its group in the caller's element order (indexed through eperm like mat); "in no group" (-1)
// becomes n_group, which sorts last and lies behind off[n_group]
__global__ void __launch_bounds__(256) k_sens_group_keys(int64_t nt, const int32_t *__restrict__ group, const int32_t *__restrict__ eperm, int32_t n_group,
                                                         uint32_t *__restrict__ keys, int32_t *__restrict__ ids) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= nt) return;
    const int32_t g = group[caller_element(eperm, t)];
    keys[t] = (g < 0 || g >= n_group) ? uint32_t(n_group) : uint32_t(g);   // (the host has checked the range)
    ids[t] = int32_t(t);
}

// off[g] = first sorted position whose key is >= g, g = 0 .. n_group (lower_bound per group)
__global__ void __launch_bounds__(256) k_sens_group_offsets(int64_t nt, int32_t n_group, const uint32_t *__restrict__ keys, int32_t *__restrict__ off) {
    const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (g > n_group) return;
    int64_t lo = 0, hi = nt;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < uint32_t(g)) lo = mid + 1; else hi = mid;
    }
    off[g] = int32_t(lo);
}

// One workgroup per chunk of kSensChunk sorted positions.  A segment longer than a chunk that meets this chunk holds the chunk's
// first position (slot 0) or its last one (slot 1) - a third one would have to lie inside the chunk.  cpart[chunk][slot][NC]: the
// sum of that segment's entries inside the chunk (0 where the slot has no long segment), every entry written.
// blockIdx.y = q: one of several functionals (the pairs of a slice, pairs.h) on the same sorted list - ev and cpart of q lie
// q * ev_stride and q * cpart_stride doubles on; the additions of every q are those of a launch of its own.
template <int NC>
__global__ void __launch_bounds__(256) k_sens_group_long(int64_t nt, int32_t n_group, const uint32_t *__restrict__ keys, const int32_t *__restrict__ perm,
                                                         const int32_t *__restrict__ off, const double *__restrict__ ev, double *__restrict__ cpart,
                                                         int64_t ev_stride, int64_t cpart_stride) {
    __shared__ double s_w[4 * NC];
    const int tid = threadIdx.x;
    ev += int64_t(blockIdx.y) * ev_stride;
    cpart += int64_t(blockIdx.y) * cpart_stride;
    const int64_t p0 = int64_t(blockIdx.x) * kSensChunk, p1 = (p0 + kSensChunk < nt) ? p0 + kSensChunk : nt;
    const uint32_t gA = keys[p0], gB = keys[p1 - 1];
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const uint32_t g = slot ? gB : gA;
        bool active = g < uint32_t(n_group) && (slot == 0 || gB != gA);   // the same for every lane of the workgroup
        int64_t a = 0, b = 0;
        if (active) { a = off[g]; b = off[g + 1]; active = (b - a) > kSensChunk; }
        double *dst = cpart + (int64_t(blockIdx.x) * 2 + slot) * NC;
        if (!active) {
            if (tid < NC) dst[tid] = 0.0;
            continue;
        }
        double acc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        const int64_t lo = a > p0 ? a : p0, hi = b < p1 ? b : p1;
        for (int64_t i = lo + tid; i < hi; i += 256) {
            const int64_t e = perm[i];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += ev[e * NC + c];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = wave_sum(acc[c]);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) s_w[(tid >> 6) * NC + c] = acc[c];
        }
        __syncthreads();
        if (tid < NC) dst[tid] = ((s_w[tid] + s_w[NC + tid]) + s_w[2 * NC + tid]) + s_w[3 * NC + tid];
        __syncthreads();
    }
}

// W lanes per group: dJg[g][c] = -(sum of the group's segment).  Short segments: lane l adds the entries l, l + W, ... of the
// segment; long ones: the chunk sums of k_sens_group_long in the same way.  Then the butterfly over the W lanes.
// blockIdx.y = q as in k_sens_group_long; the sums of q go to dJg + q * out_stride.
template <int NC, int W>
__global__ void __launch_bounds__(256) k_sens_group_sum(int32_t n_group, const uint32_t *__restrict__ keys, const int32_t *__restrict__ perm,
                                                        const int32_t *__restrict__ off, const double *__restrict__ ev, const double *__restrict__ cpart,
                                                        double *__restrict__ dJg, int64_t ev_stride, int64_t cpart_stride, int64_t out_stride) {
    ev += int64_t(blockIdx.y) * ev_stride;
    cpart += int64_t(blockIdx.y) * cpart_stride;
    dJg += int64_t(blockIdx.y) * out_stride;
    const int64_t gid = (int64_t(blockIdx.x) * 256 + threadIdx.x) / W;
    const int sub = threadIdx.x % W;
    const bool live = gid < n_group;   // (lanes behind the last group stay for the exchanges)
    const int64_t a = live ? off[gid] : 0, b = live ? off[gid + 1] : 0;
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    if (b - a > kSensChunk) {
        const int64_t k1 = (b - 1) / kSensChunk;
        for (int64_t k = a / kSensChunk + sub; k <= k1; k += W) {
            const int slot = (keys[k * kSensChunk] == uint32_t(gid)) ? 0 : 1;
            const double *src = cpart + (k * 2 + slot) * NC;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += src[c];
        }
    } else {
        for (int64_t i = a + sub; i < b; i += W) {
            const int64_t e = perm[i];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += ev[e * NC + c];
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = group_sum<W>(acc[c]);
    if (live && sub == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) dJg[gid * NC + c] = 0.0 - acc[c];   // (an empty group reads +0)
    }
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

void launch_sens_contract(const ElemMesh &em, const double *tab, const SensColumns &col, const PointLoads &pl, double *part, hipStream_t s, bool per_elem) {
    const int grid = sens_grid(em.nt);
    for_elem_kind(em.dim, em.condense, em.tensor(), [&](auto d, auto co, auto te) {
        constexpr int D = decltype(d)::value;
        constexpr bool CO = decltype(co)::value, TE = decltype(te)::value;
        auto launch = [&](auto pe) {
            constexpr bool PE = decltype(pe)::value;
            const size_t lds = PE ? 0 : sizeof(double) * size_t(em.n_mat) * SensOut<D, TE>::N;
            hipLaunchKernelGGL((k_sens_contract<D, CO, TE, PE>), dim3(grid), dim3(kSensBlock), lds, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.eldof, em.C,
                               em.M, tab, col, pl.pt_rhs, pl.pt_I, pl.found, pl.fint, em.n_mat, part);
        };
        if (per_elem) launch(std::true_type{}); else launch(std::false_type{});
    });
}

void launch_sens_reduce(int n_fun, int grid, int nmc, const double *part, double *dJ, hipStream_t s) {
    const int total = n_fun * nmc;
    if (total <= 0) return;
    hipLaunchKernelGGL(k_sens_reduce, dim3((total + 255) / 256), dim3(256), 0, s, n_fun, grid, nmc, part, dJ);
}

// ---- group order (once per batch) and the sums per group -------------------------------------------------------------------
static unsigned group_key_bits(int32_t n_group) {   // the keys run from 0 to n_group
    unsigned bits = 1;
    while (bits < 32 && (uint32_t(n_group) >> bits) != 0) ++bits;
    return bits;
}

size_t sens_group_sort_bytes(int64_t nt, int32_t n_group) {
    size_t tb = 0;
    uint32_t *k = nullptr;
    int32_t *v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, tb, k, k, v, v, size_t(nt), 0u, group_key_bits(n_group), hipStream_t(nullptr)) != hipSuccess)
        throw std::runtime_error("rocprim::radix_sort_pairs: size query failed");
    return tb;
}

int64_t sens_group_chunks(int64_t nt) { return (nt + kSensChunk - 1) / kSensChunk; }

void sens_group_order(int64_t nt, const int32_t *group, const int32_t *eperm, int32_t n_group, uint32_t *keys_in, int32_t *ids, uint32_t *keys, int32_t *perm,
                      int32_t *off, void *tmp, size_t tmp_bytes, hipStream_t s) {
    hipLaunchKernelGGL(k_sens_group_keys, dim3(unsigned((nt + 255) / 256)), dim3(256), 0, s, nt, group, eperm, n_group, keys_in, ids);
    if (rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys, ids, perm, size_t(nt), 0u, group_key_bits(n_group), s) != hipSuccess)
        throw std::runtime_error("rocprim::radix_sort_pairs failed");
    hipLaunchKernelGGL(k_sens_group_offsets, dim3(unsigned((int64_t(n_group) + 1 + 255) / 256)), dim3(256), 0, s, nt, n_group, keys, off);
}

void launch_sens_group_sum_batch(int nc, int64_t nt, int32_t n_group, const uint32_t *keys, const int32_t *perm, const int32_t *off, const double *ev,
                                 double *cpart, double *dJg, int nq, int64_t ev_stride, int64_t out_stride, hipStream_t s) {
    // lanes per group by the mean segment length (a property of the grouping: the order of the additions stays fixed)
    const int64_t mean = nt / (n_group > 0 ? n_group : 1);
    const int w = mean <= 8 ? 4 : (mean <= 128 ? 16 : 64);
    const unsigned nchunk = unsigned(sens_group_chunks(nt)), grid = unsigned((int64_t(n_group) * w + 255) / 256);
    const int64_t cs = int64_t(nchunk) * 2 * nc;
    if (nq <= 0 || nt <= 0) return;
#define REMO_GROUP_LAUNCH(NC) \
    do { \
        hipLaunchKernelGGL((k_sens_group_long<NC>), dim3(nchunk, nq), dim3(256), 0, s, nt, n_group, keys, perm, off, ev, cpart, ev_stride, cs); \
        if (grid == 0) break; \
        if (w == 4) hipLaunchKernelGGL((k_sens_group_sum<NC, 4>), dim3(grid, nq), dim3(256), 0, s, n_group, keys, perm, off, ev, cpart, dJg, ev_stride, cs, out_stride); \
        else if (w == 16) hipLaunchKernelGGL((k_sens_group_sum<NC, 16>), dim3(grid, nq), dim3(256), 0, s, n_group, keys, perm, off, ev, cpart, dJg, ev_stride, cs, out_stride); \
        else hipLaunchKernelGGL((k_sens_group_sum<NC, 64>), dim3(grid, nq), dim3(256), 0, s, n_group, keys, perm, off, ev, cpart, dJg, ev_stride, cs, out_stride); \
    } while (0)
    if (nc == 1) REMO_GROUP_LAUNCH(1);
    else if (nc == 3) REMO_GROUP_LAUNCH(3);
    else REMO_GROUP_LAUNCH(6);
#undef REMO_GROUP_LAUNCH
}

void launch_sens_group_sum(int nc, int64_t nt, int32_t n_group, const uint32_t *keys, const int32_t *perm, const int32_t *off, const double *ev,
                           double *cpart, double *dJg, hipStream_t s) {
    launch_sens_group_sum_batch(nc, nt, n_group, keys, perm, off, ev, cpart, dJg, 1, 0, 0, s);
}

}  // namespace remo
