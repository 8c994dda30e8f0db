// pcg_kernels.hip — the kernels of a PCG step other than the operator, gfx950 (CDNA4, wave64): init, update, direction and final
// launches (k_pcg_update_folded takes the first Chebyshev step along), the residual replacement of the mixed mode, and their launchers (kernels.h).
// The operator q = A p is kernels.hip (CSR) or patch.hip (patch operator); C r on the P1 vertex block is vertex_solver.hip or amg.hip (cycle).
// All of it is HBM/L2-bound streaming: the levers are whole-line accesses, loads in flight, few launches per step and, since every
// form of a launch is a kernel of its own, the occupancy each form's own code allows.
#include "kernels.h"
#include "amg.h"

#include <math.h>

#include <stdexcept>
#include <type_traits>

#include "wave_util.h"
#include "kutil.h"

namespace remo {

#ifdef REMO_PROBES
constexpr bool kProbes = true;     // the build of tools/: rejected variants and their remo_debug_tune keys are compiled in
#else
constexpr bool kProbes = false;
#endif

// Probe builds: where a workgroup of k_pcg_direction_flat / k_pcg_update_tile spends its time - three clocks of its wave 0 (on entry |
// scalars in LDS | at the end), four words per workgroup, written together at the end (a launch that finds the solve over leaves none)
// where remo_debug_vector_heads points the launches (set_vector_stamps): direction launch in rows [0, kMaxPartialBlocks), update launch behind
#ifdef REMO_PROBES
__device__ long long *g_vec_stamps = nullptr;
#define REMO_VEC_CLOCK(var) const long long var = (long long)__builtin_readcyclecounter();
#define REMO_VEC_STAMPS(which, t0, t1)                                                                \
    if (g_vec_stamps && threadIdx.x == 0) {                                                           \
        long long *w_ = g_vec_stamps + (int64_t(which) * kMaxPartialBlocks + int64_t(blockIdx.x)) * 4; \
        w_[0] = t0; w_[1] = t1; w_[2] = (long long)__builtin_readcyclecounter();                      \
    }
#else
#define REMO_VEC_CLOCK(var)
#define REMO_VEC_STAMPS(which, t0, t1)
#endif

// Progress records live in mapped, coherent host memory: the stores bypass the caches (sc0 sc1).  A system-scope RELEASE
// store would also write back the whole L2 of the XCD (buffer_wbl2) on every PCG step; the record only needs its data to
// land before its step number, so the data stores are relaxed, the wave waits for their acknowledgement, then stores the
// step number.
__device__ __forceinline__ void publish_progress(PcgProgress *pr, const double *rz, int k, int step) {
    for (int c = 0; c < k; ++c) __hip_atomic_store(&pr->rz[c], rz[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(&pr->step, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------------
// Jacobi-PCG vector kernels (CGSolver(a.mat, c.mat), ngsolve_functions.py:50-51), K columns at
// once with per-column step lengths.  Three launches per step:
//   spmm      q = A p, partials of <p,q>
//   update    alpha = <Cr,r>/<p,q>;  x += alpha p;  r -= alpha q;  partials of <C r, r>
//   direction beta = <Cr,r>_new/<Cr,r>_old;  p = C r + beta p
// Scalars never visit the host: every block re-reduces the (<= 1024 x K) per-block partials of
// the previous launch in a fixed order, so results are bit-reproducible and there is no atomic.
// A column whose <Cr,r> has dropped below tol^2 <Cr0,r0> (or that broke down) is frozen
// (alpha = beta = 0), which makes post-convergence steps harmless.

// q = A p of the patch operator with the rows shared by several patches still in the boundary slab (PcgBuffersT::defer_q)
template <class T> struct QViewT {
    const int32_t *bptr = nullptr, *bslot = nullptr;
    const T *Yb = nullptr;
    int skip_x = 0;     // 1: x += alpha p is left to the direction launch of the step (PcgBuffersT::x_in_direction)
    const int32_t *row4 = nullptr;   // PatchTables::row4 (tile form)
    uint64_t slab_bytes = 0;   // size of the slab behind its buffer descriptor (masked row form, tile form: slab below 4 GB)
};
// x_ev[j] += alpha p[at[j]] (PcgBuffersT::x_ev): the values of x the evaluation points read, formed by the update launch
template <class T> struct EvSlotsT {
    const int64_t *at = nullptr;
    T *x = nullptr;
    int n = 0;
};
// FIRST Chebyshev step folded into the update launch (k_pcg_update_folded)
template <class T> struct FoldArgsT {
    int nb_flat = 0;             // workgroups [0, nb_flat) do the flat update of the rows >= nv, the rest the vertex rows
    const int32_t *rowptr = nullptr, *col = nullptr;
    const T *val = nullptr;
    T *d_new = nullptr, *stage = nullptr;
    double c1 = 0.0, c2 = 0.0;
};
// what every form of the update launch needs for its scalars (pcg_update_head)
template <class T> struct UpdHeadT {
    int step = 0;
    double tol2 = 0.0;
    int nb_spmv = 0, nb_rz = 0;            // workgroups that left partials of <p, A p> / of <Cr, r>
    const double *part_pq = nullptr, *part_rz_cur = nullptr;
    double *rz0 = nullptr;                 // PcgBuffersT::rz0
    PcgProgress *progress = nullptr;
    int progress_len = 0;
    double *clear_bins = nullptr;          // the <p, A p> bins of the next step (PcgBuffersT::pq_bins), or nullptr
    EvSlotsT<T> ev;
};
// All PCG kernels are templates on the storage type T of matrix values and vectors: double = the
// product path, float = the inner solver of the mixed-precision mode (BASELINE config 5).  Scalars,
// partial sums and the convergence test are double in both.
// scal[kFloorSlot + c]: absolute floor of <Cr,r> below which column c is frozen as well (0 in the plain
// fp64 solve; the outer target of the refinement in the mixed mode)
constexpr int kFloorSlot = 5 * 8;

// TP, here and in the launches below: the storage type of the search direction p - T, or float inside an fp64 solve
// (PcgBuffersT::p32).  Every reader widens the stored value; nothing keeps an unrounded copy.
template <class T, int K, class TP = T>
__global__ void __launch_bounds__(256) k_pcg_init(int64_t n, ChebArgsT<T> ch, const T *__restrict__ f, const T *__restrict__ dinv,
                                                  T *__restrict__ x, T *__restrict__ r, TP *__restrict__ p,
                                                  double *__restrict__ part_rz) {
    __shared__ double smem[16 * K];
    double rz[K];
#pragma unroll
    for (int c = 0; c < K; ++c) rz[c] = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        const T d = dinv[i];
        const bool coarse = i < ch.nv;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const T ri = f[i * K + c];
            const T zi = d * ri;
            if (x) x[i * K + c] = T(0);   // (evaluated values only: x_ev is cleared by the host)
            r[i * K + c] = ri;
            p[i * K + c] = TP(coarse ? T(0) : zi);
            rz[c] += coarse ? 0.0 : double(ri) * double(zi);   // the vertex block's share comes from the Chebyshev kernels
        }
    }
    block_sum<K>(rz, smem);
    if (threadIdx.x < K) part_rz[blockIdx.x * K + threadIdx.x] = rz[threadIdx.x];
}

// ------------------------------------------------------------------------------------------
// The update launch: alpha = <Cr,r>/<p,q>;  x += alpha p;  r -= alpha q;  partials of <C r, r>.  One kernel per FORM, chosen by
// launch_pcg_update (x_only: launch_pcg_replace); what the forms share is in the device functions below, inlined into each.
//   k_pcg_update         the ROW form, the general one: a k-wide row per lane; MASKED: the slab slots a row does not have are not fetched
//   k_pcg_update_tile    64 rows per wave, a value per lane and pass (patch operator, fp64 storage)
//   k_pcg_update_folded  the row form on the rows >= nv, and workgroups of its own that run the FIRST Chebyshev step on the vertex rows
//   k_pcg_update_x       x += alpha p alone (residual replacement of the mixed mode)

// What every form does first.  Returns false when an earlier step froze every column (the launch is a no-op); else alpha[] of the step.
// scal = rz0[8] | pq[8] | rz of even steps[8] | rz of odd steps[8]: totals forwarded between launches
// by workgroup 0, so every launch re-reduces only the ONE partial array that is new to it
// block_sum (kutil.h) for a workgroup of exactly 256 threads: the same tree, the same bits - but the number of waves is not read from the
// dispatch packet: that load would be the YOUNGEST of the wave, and waiting for it waits for every vector load requested before it
template <int K> __device__ __forceinline__ void block_sum_256(double (&v)[K], double *smem /* [4*K] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < K; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) smem[wave * K + c] = v[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += smem[w * K + c];
        v[c] = s;
    }
}
#ifndef REMO_UPD_EARLY
#define REMO_UPD_EARLY 1      /* 0: k_pcg_update_tile beside an fp32 direction reduces its scalars before its first load (the form before) */
#endif
// PRE: the rows threadIdx.x + 256 i of part_pq are in pre[] already (requested before the caller's first vector loads, so that the wait
// for them does not wait for those); a row beyond nb_spmv read as zero.  Same order of additions as reduce_partials: the same bits.
template <class T, int K, class TP = T, bool PRE = false, int NPRE = 1>
__device__ __forceinline__ bool pcg_update_head(const UpdHeadT<T> &hd, const TP *__restrict__ p, double (&alpha)[K], double *smem /* [16*3*K] */,
                                                const double (*pre)[K] = nullptr) {
    double *scal = hd.rz0;
    const int step = hd.step;
    if (solve_done(scal, step)) return false;
    double pq[K], rz[K], unused[K];
    if (step == 0) {
        reduce_partials3<K>(hd.part_pq, hd.nb_spmv, hd.part_rz_cur, hd.nb_rz, nullptr, 0, pq, rz, unused, smem);
    } else {
        if constexpr (PRE) {
#pragma unroll
            for (int c = 0; c < K; ++c) pq[c] = 0.0;
#pragma unroll
            for (int i = 0; i < NPRE; ++i)
#pragma unroll
                for (int c = 0; c < K; ++c) pq[c] += pre[i][c];
            block_sum_256<K>(pq, smem);
        } else {
            reduce_partials<K>(hd.part_pq, hd.nb_spmv, pq, smem);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) rz[c] = scal[16 + 8 * (step & 1) + c];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const double r0 = (step == 0) ? rz[c] : hd.rz0[c];
        const bool live = (rz[c] > hd.tol2 * r0) && (rz[c] > scal[kFloorSlot + c]) && (pq[c] > 0.0);
        alpha[c] = live ? rz[c] / pq[c] : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        bool any_live = false;
#pragma unroll
        for (int c = 0; c < K; ++c) any_live |= (alpha[c] != 0.0);
        if (!any_live) {   // every column frozen: later launches of this solve are no-ops; tell the host where it ended
            reinterpret_cast<int *>(scal + kDoneSlot)[0] = step + 1;   // acts on the launches of steps > step only (solve_done)
            publish_progress(hd.progress + (hd.progress_len - 1), rz, K, step);
        }
#pragma unroll
        for (int c = 0; c < K; ++c) scal[8 + c] = pq[c];
        if (step == 0)
#pragma unroll
            for (int c = 0; c < K; ++c) { hd.rz0[c] = rz[c]; scal[16 + c] = rz[c]; }
        // progress record in mapped host memory: data first, then the step number (system scope)
        publish_progress(hd.progress + (step % (hd.progress_len - 1)), rz, K, step);   // the last slot is the "done" record
    }
    if (hd.clear_bins) {     // the patch operator's <p, A p> bins of the NEXT step (PcgBuffersT::pq_bins): this launch is the last reader of that set
        for (int i = int(blockIdx.x) * int(blockDim.x) + int(threadIdx.x); i < kPqBins * K; i += int(gridDim.x) * int(blockDim.x)) hd.clear_bins[i] = 0.0;
    }
    // the values of x the evaluation points read (a few thousand, PcgBuffersT::x_ev): p is not written before the direction launch,
    // so this is x += alpha p of the step with the operands and the expression of the direction launch
    for (int j = int(blockIdx.x) * int(blockDim.x) + int(threadIdx.x); j < hd.ev.n; j += int(gridDim.x) * int(blockDim.x)) {
        const int64_t at = hd.ev.at[j];
        if (at < 0) continue;
        const int col = int(at % K);
        double a = 0.0;
#pragma unroll
        for (int c = 0; c < K; ++c) a = (c == col) ? alpha[c] : a;
        const T xv = hd.ev.x[j], pv = T(p[at]);
        hd.ev.x[j] = xv + T(a) * pv;
    }
    return true;
}

// ROW form: a k-wide row per lane, rows i0 + (workgroup, thread) in strides of nb * 256; leaves the workgroup's <C r, r> partials.
// MASKED (launcher: slab below 4 GB): the slots a row does not have are not fetched at all (buffer loads, offset out of range);
// else every shared row fetches four slots and weights the ones it does not have by zero.
// AHEAD = false (probe builds, remo_debug_tune key 27): the slots of a shared row one by one.
#ifndef REMO_UPD_UNROLL
#define REMO_UPD_UNROLL 2
#endif
template <class T, int K, bool MASKED, bool AHEAD>
__device__ __forceinline__ void pcg_update_rows(int64_t i0, int64_t n, int nb, int64_t nv, const double (&alpha)[K], const T *__restrict__ p,
                                                const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r, const T *__restrict__ dinv,
                                                const QViewT<T> &qv, double *__restrict__ part_rz_next, double *smem /* [16*K] */) {
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
#pragma unroll REMO_UPD_UNROLL
    for (int64_t i = i0 + int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(nb) * blockDim.x) {
        const T d = dinv[i];
        const bool coarse = i < nv;
        T qi[K];
        int32_t b0 = 0, b1 = 0;
        if (qv.bptr) { b0 = qv.bptr[i]; b1 = qv.bptr[i + 1]; }
        // x, p and r of the row are requested HERE, with the row's slab pointers, not behind the branch that gathers q: three more
        // vectors in flight while the slab slots make their two round trips
        T xv[K], pv[K], rv[K];
        if (qv.skip_x) {      // x += alpha p rides on the direction launch, which reads p anyway: neither x nor p is touched here
#pragma unroll
            for (int c = 0; c < K; ++c) { xv[c] = T(0); pv[c] = T(0); rv[c] = r[i * K + c]; }
        } else {
#pragma unroll
            for (int c = 0; c < K; ++c) { xv[c] = x[i * K + c]; pv[c] = p[i * K + c]; rv[c] = r[i * K + c]; }
        }
        if (b1 > b0) {      // a row shared by several patches: its q is still spread over the slab, one slot per patch, ascending
            // the first kSlabAhead slots without a branch and with all their loads in flight together (slot numbers, then slab
            // rows: two round trips; the plain loop made two per slot, and a wave waits for its row with the most slots) - a
            // missing slot reads slot 0 and counts for nothing; further slots (rare) one by one
            constexpr int kSlabAhead = 4;
            if constexpr (AHEAD) {
                int32_t at[kSlabAhead];
#pragma unroll
                for (int j = 0; j < kSlabAhead; ++j) at[j] = qv.bslot[b0 + j < b1 ? b0 + j : b0];
                T part[kSlabAhead][K];
                if constexpr (MASKED) {
                    // a row has 1.84 slots on average (44 % of the rows exactly one, now that every row goes through the slab): a lane asks
                    // only for the slots its row has - the others get an offset beyond the buffer, which sends no request and returns 0
                    const rsrc_t rs = make_rsrc(qv.Yb, qv.slab_bytes);
#pragma unroll
                    for (int j = 0; j < kSlabAhead; ++j)
                        buf_load<T, K>(rs, b0 + j < b1 ? uint32_t(at[j]) * uint32_t(K * sizeof(T)) : kOutOfRange, part[j]);
#pragma unroll
                    for (int c = 0; c < K; ++c) qi[c] = part[0][c];
#pragma unroll
                    for (int j = 1; j < kSlabAhead; ++j)
#pragma unroll
                        for (int c = 0; c < K; ++c) qi[c] += part[j][c];
                } else {
#pragma unroll
                    for (int j = 0; j < kSlabAhead; ++j)
#pragma unroll
                        for (int c = 0; c < K; ++c) part[j][c] = qv.Yb[int64_t(at[j]) * K + c];
#pragma unroll
                    for (int c = 0; c < K; ++c) qi[c] = part[0][c];
#pragma unroll
                    for (int j = 1; j < kSlabAhead; ++j) {
                        const T w = b0 + j < b1 ? T(1) : T(0);
#pragma unroll
                        for (int c = 0; c < K; ++c) qi[c] += w * part[j][c];
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < K; ++c) qi[c] = T(0);
            }
            for (int32_t sl = b0 + (AHEAD ? kSlabAhead : 0); sl < b1; ++sl) {
                const int64_t a2 = qv.bslot[sl];
#pragma unroll
                for (int c = 0; c < K; ++c) qi[c] += qv.Yb[a2 * K + c];
            }
        } else {
#pragma unroll
            for (int c = 0; c < K; ++c) qi[c] = q[i * K + c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const T a = T(alpha[c]);
            const T xi = xv[c] + a * pv[c];
            const T ri = rv[c] - a * qi[c];
            if (!qv.skip_x) x[i * K + c] = xi;
            r[i * K + c] = ri;
            acc[c] += coarse ? 0.0 : double(ri) * double(ri) * double(d);   // the vertex block's share comes from the Chebyshev kernels
        }
    }
    __syncthreads();
    block_sum<K>(acc, smem);
    if (threadIdx.x < K) part_rz_next[blockIdx.x * K + threadIdx.x] = acc[threadIdx.x];
}

template <class T, int K, bool MASKED, bool AHEAD = true>
__global__ void __launch_bounds__(256) k_pcg_update(int64_t n, UpdHeadT<T> hd, int64_t nv, double *__restrict__ part_rz_next,
                                                        const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                        const T *__restrict__ dinv, QViewT<T> qv) {
    __shared__ double smem[16 * 3 * K];
    double alpha[K];
    if (!pcg_update_head<T, K>(hd, p, alpha, smem)) return;
    pcg_update_rows<T, K, MASKED, AHEAD>(0, n, int(gridDim.x), nv, alpha, p, q, x, r, dinv, qv, part_rz_next, smem);
}

// the row form beside an fp32 search direction (evaluated values only: x and p belong to the direction launch, qv.skip_x; p is read by the x_ev slots alone)
template <int K, bool MASKED>
__global__ void __launch_bounds__(256) k_pcg_update_p32(int64_t n, UpdHeadT<double> hd, int64_t nv, double *__restrict__ part_rz_next,
                                                        const float *__restrict__ p, const double *__restrict__ q, double *__restrict__ r,
                                                        const double *__restrict__ dinv, QViewT<double> qv) {
    __shared__ double smem[16 * 3 * K];
    double alpha[K];
    if (!pcg_update_head<double, K, float>(hd, p, alpha, smem)) return;
    pcg_update_rows<double, K, MASKED, true>(0, n, int(gridDim.x), nv, alpha, (const double *)nullptr, q, (double *)nullptr, r, dinv, qv, part_rz_next, smem);
}

// x += alpha p alone: the residual replacement step of the mixed mode (r and the <Cr,r> partials come from k_mixed_replace)
template <class T, int K>
__global__ void __launch_bounds__(256) k_pcg_update_x(int64_t n, UpdHeadT<T> hd, const T *__restrict__ p, T *__restrict__ x) {
    __shared__ double smem[16 * 3 * K];
    double alpha[K];
    if (!pcg_update_head<T, K>(hd, p, alpha, smem)) return;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
#pragma unroll
        for (int c = 0; c < K; ++c) x[i * K + c] += T(alpha[c]) * p[i * K + c];
    }
}

// FOLDED form: the workgroups behind the first fold.nb_flat take the vertex rows, 8 lanes per row, and run the FIRST
// Chebyshev step on them in the same pass (its operand D^-1 (r - alpha q) / theta is formed per gathered entry from
// the OLD r and q, both complete at this point).  The new vertex residual goes to a staging vector (fold.stage =
// the free one of the two direction buffers): r itself is still being gathered by the neighbours' rows; the next
// Chebyshev launch commits it.  One launch less per PCG step.  The first fold.nb_flat workgroups: the row form on the rows >= nv
// (q is whole: the launcher never folds while the shared rows of the patch operator are still in the slab).
template <class T, int K>
__device__ __forceinline__ void pcg_update_vertex_rows(const ChebArgsT<T> &ch, const FoldArgsT<T> &fold, int skip_x, const double (&alpha)[K],
                                                       const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, const T *__restrict__ r,
                                                       const T *__restrict__ dinv) {
    constexpr int LPR = 8, RPB = 256 / LPR;
    static_assert(K <= LPR, "one column per lane after the transposing reduction");
    const int nb_flat = fold.nb_flat;
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    int idx[K], own[K];
    towner_init<K, LPR>(idx, own, sub);
    const int mycol = idx[0];
    const bool mine = own[0] != 0;
    const T inv_theta = T(ch.inv_theta), c1 = T(fold.c1), c2 = T(fold.c2);
    T al[K], a_mine = T(0);
#pragma unroll
    for (int c = 0; c < K; ++c) { al[c] = T(alpha[c]); a_mine = (c == mycol) ? al[c] : a_mine; }
    const int64_t nv = ch.nv;
    for (int64_t row = int64_t(int(blockIdx.x) - nb_flat) * RPB + grp; row < nv; row += int64_t(int(gridDim.x) - nb_flat) * RPB) {
        const int32_t rs = fold.rowptr[row], re = fold.rowptr[row + 1];
        const int64_t at = row * K + mycol;
        T di = T(0), rn = T(0);
        if (mine) {
            di = dinv[row];
            if (!skip_x) x[at] += a_mine * p[at];
            rn = r[at] - a_mine * q[at];
        }
        T t[K];
#pragma unroll
        for (int c = 0; c < K; ++c) t[c] = T(0);
        for (int32_t pp = rs + sub; pp < re; pp += LPR) {
            const int32_t j = fold.col[pp];
            if (j >= nv) break;  // columns ascend: the vertex block leads the row
            const T v = fold.val[pp] * dinv[j] * inv_theta;
            const T *rj = r + int64_t(j) * K, *qj = q + int64_t(j) * K;
#pragma unroll
            for (int c = 0; c < K; ++c) t[c] += v * (rj[c] - al[c] * qj[c]);
        }
        TReduce<K, LPR>::run(t, sub);
        if (mine) {
            const T dold = di * rn * inv_theta;
            const T ri = rn - t[0];
            ch.z[at] = dold;
            ch.res[at] = ri;
            fold.d_new[at] = c1 * dold + c2 * di * ri;
            fold.stage[at] = rn;
        }
    }
}

template <class T, int K>
__global__ void __launch_bounds__(256) k_pcg_update_folded(int64_t n, UpdHeadT<T> hd, ChebArgsT<T> ch, double *__restrict__ part_rz_next,
                                                           const T *__restrict__ p, const T *__restrict__ q, T *__restrict__ x, T *__restrict__ r,
                                                           const T *__restrict__ dinv, FoldArgsT<T> fold, int skip_x) {
    __shared__ double smem[16 * 3 * K];
    double alpha[K];
    if (!pcg_update_head<T, K>(hd, p, alpha, smem)) return;
    if (int(blockIdx.x) >= fold.nb_flat) {
        pcg_update_vertex_rows<T, K>(ch, fold, skip_x, alpha, p, q, x, r, dinv);
        return;
    }
    QViewT<T> qv;
    qv.skip_x = skip_x;
    pcg_update_rows<T, K, false, true>(ch.nv, n, fold.nb_flat, ch.nv, alpha, p, q, x, r, dinv, qv, part_rz_next, smem);
}

// TILE form (launcher: patch operator with every row in the slab and its row4 table, x left to the direction launch, no folded
// Chebyshev step, n K sizeof(T) and the slab below 4 GB).  A wave takes 64 rows = 64 K values at a time.  Lane l fetches the
// four slots of row l of the tile (ONE 16-byte load per lane: 1 KB per wave); then, pass by pass, lane l handles value
// 64 t + l of the tile: r as 512 consecutive bytes per wave and instruction, the slots of the value's row from the lane that
// holds them (ds_bpermute), and ITS column of each slab slot - the K lanes of a row read a slot's 40 bytes side by side.
// All 6 K loads of a lane are in flight together.  Same sums, same order as the row form (rows of five or more patches, the
// first vertex rows: their further slots are summed by the row's lane and handed over through LDS - another association).
// The tile form beside an fp32 direction (the one-shot solves; REMO_UPD_EARLY): the same tiles, sums and order as k_pcg_update_tile
// below, but the partial sums of <p, A p> and then the FIRST tile's slots, r, Jacobi factors and slab values are requested before
// the scalars are reduced, and the head runs while they are in flight - no load depends on alpha.
template <int K>
__device__ __forceinline__ void pcg_update_tile_early(int64_t n, const UpdHeadT<double> &hd, int64_t nv, double *__restrict__ part_rz_next,
                                                      const float *__restrict__ p, double *__restrict__ r, const double *__restrict__ dinv,
                                                      const QViewT<double> &qv, double *smem /* [16*3*K] */, double *ex_lds /* [4*64*K] */) {
    using T = double;
    double alpha[K], acc[K];
    REMO_VEC_CLOCK(t_in)
    constexpr uint32_t S = sizeof(T);
    constexpr int NPRE = kMaxPartialBlocks / 256;
    double pre[NPRE][K];
    if (solve_done(hd.rz0, hd.step)) return;       // (a finished solve leaves before any request)
    {
        const rsrc_t rq = make_rsrc(hd.part_pq, uint64_t(hd.nb_spmv) * (K * 8));
#pragma unroll
        for (int i = 0; i < NPRE; ++i) buf_load<double, K>(rq, (uint32_t(threadIdx.x) + 256u * i) * uint32_t(K * 8), pre[i]);
        __builtin_amdgcn_sched_barrier(0);      // the OLDEST loads of the wave: the head's wait for them leaves the tile's loads in flight
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t N = uint32_t(n) * K, NV = uint32_t(nv) * K;
    const rsrc_t rr = make_rsrc(r, uint64_t(N) * S), rd = make_rsrc(dinv, uint64_t(n) * S), rs = make_rsrc(qv.Yb, qv.slab_bytes),
                 r4 = make_rsrc(qv.row4, uint64_t(n) * 16);
    uint32_t rowof[K], colof[K];      // pass t: this lane's value is (row rowof[t] of the tile, column colof[t]) - the same for every tile
    T al[K];
    double accv[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const uint32_t v = 64u * t + lane;
        rowof[t] = v / uint32_t(K); colof[t] = v - rowof[t] * uint32_t(K);
        accv[t] = 0.0;
    }
    double *exw = ex_lds + wave * (64 * K);
    const uint32_t nwaves = uint32_t(gridDim.x) * 4u;
    // (the slots of the NEXT tile are requested before this tile's values: one memory round trip per tile on a wave's critical path, not two)
    int32_t w4n[4];
    {
        const uint32_t row0 = (uint32_t(blockIdx.x) * 4u + wave) * 64u + lane;
        buf_load<int32_t, 4>(r4, row0 < uint32_t(n) ? row0 * 16u : kOutOfRange, w4n);
    }
    int32_t w4[4];
    T rv[K], dv[K], part[K][4];
    // the slots of the tile at R0 (requested one tile ahead), the request for the next tile's, and this tile's r, Jacobi factors and slab values
    auto request = [&](uint32_t R0) {
        const uint32_t myrow = R0 + lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) w4[j] = myrow < uint32_t(n) ? w4n[j] : -1;
        {
            const uint32_t nrow = myrow + nwaves * 64u;
            buf_load<int32_t, 4>(r4, nrow < uint32_t(n) ? nrow * 16u : kOutOfRange, w4n);
        }
        const uint32_t e0 = R0 * uint32_t(K);
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const uint32_t e = e0 + 64u * t + lane;
            T one[1];
            buf_load<T, 1>(rr, e < N ? e * S : kOutOfRange, one);
            rv[t] = one[0];
            buf_load<T, 1>(rd, e < N ? (R0 + rowof[t]) * S : kOutOfRange, one);
            dv[t] = one[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t sj = __builtin_amdgcn_ds_bpermute(int(rowof[t] << 2), w4[j]);
                buf_load<T, 1>(rs, sj >= 0 ? (uint32_t(sj) * uint32_t(K) + colof[t]) * S : kOutOfRange, one);
                part[t][j] = one[0];
            }
        }
    };
    request((uint32_t(blockIdx.x) * 4u + wave) * 64u);      // (a wave with no tile asks for nothing: every offset is out of range)
    bool requested = true;
    if (!pcg_update_head<T, K, float, true, NPRE>(hd, p, alpha, smem, pre)) return;
    __syncthreads();          // (the reductions' last reads of smem)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) smem[c] = alpha[c];
    }
    __syncthreads();
    REMO_VEC_CLOCK(t_head)
#pragma unroll
    for (int t = 0; t < K; ++t) al[t] = T(smem[colof[t]]);
    for (uint32_t R0 = (uint32_t(blockIdx.x) * 4u + wave) * 64u; R0 < uint32_t(n); R0 += nwaves * 64u) {
        const uint32_t myrow = R0 + lane;
        const uint32_t e0 = R0 * uint32_t(K);
        if (!requested) request(R0);
        requested = false;
        const bool more = w4[3] == -2;
        const bool any_more = __builtin_amdgcn_ballot_w64(more) != 0;
        if (any_more) {       // (wave-uniform) rows of five or more patches in this tile: their lanes sum the slots from the fourth on
#pragma unroll
            for (int c = 0; c < K; ++c) exw[lane * K + c] = 0.0;
            if (more) {
                const int32_t c0 = qv.bptr[myrow], c1 = qv.bptr[myrow + 1];
                for (int32_t sl = c0 + 3; sl < c1; ++sl) {
                    const int64_t a2 = qv.bslot[sl];
#pragma unroll
                    for (int c = 0; c < K; ++c) exw[lane * K + c] += double(qv.Yb[a2 * K + c]);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's LDS writes are done before its lanes read each other's
        }
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const uint32_t e = e0 + 64u * t + lane;
            T qi = part[t][0];
#pragma unroll
            for (int j = 1; j < 4; ++j) qi += part[t][j];
            if (any_more) qi += T(exw[64 * t + lane]);
            const T ri = rv[t] - al[t] * qi;
            T one[1] = {ri};
            buf_store<T, 1>(rr, e < N ? e * S : kOutOfRange, one);
            accv[t] += (e < NV || e >= N) ? 0.0 : double(ri) * double(ri) * double(dv[t]);
        }
        if (any_more) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next tile's zeros
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double tsum = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) tsum += (colof[t] == uint32_t(c)) ? accv[t] : 0.0;
        acc[c] = tsum;
    }
    __syncthreads();
    const double mine = block_sum_column<K>(acc, smem);
    if (threadIdx.x < K) part_rz_next[blockIdx.x * K + threadIdx.x] = mine;
    REMO_VEC_STAMPS(1, t_in, t_head)
}

template <class T, int K, class TP = T>
__global__ void __launch_bounds__(256) k_pcg_update_tile(int64_t n, UpdHeadT<T> hd, int64_t nv, double *__restrict__ part_rz_next,
                                                         const TP *__restrict__ p, T *__restrict__ r, const T *__restrict__ dinv, QViewT<T> qv) {
    __shared__ double smem[16 * 3 * K];
    __shared__ double ex_lds[4 * 64 * K];
    if constexpr (!std::is_same<TP, T>::value && REMO_UPD_EARLY) {
        pcg_update_tile_early<K>(n, hd, nv, part_rz_next, p, r, dinv, qv, smem, ex_lds);
        return;
    }
    double alpha[K], acc[K];
    REMO_VEC_CLOCK(t_in)
    if (!pcg_update_head<T, K, TP>(hd, p, alpha, smem)) return;
    constexpr uint32_t S = sizeof(T);
    __syncthreads();          // (the reductions' last reads of smem)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) smem[c] = alpha[c];
    }
    __syncthreads();
    REMO_VEC_CLOCK(t_head)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t N = uint32_t(n) * K, NV = uint32_t(nv) * K;
    const rsrc_t rr = make_rsrc(r, uint64_t(N) * S), rd = make_rsrc(dinv, uint64_t(n) * S), rs = make_rsrc(qv.Yb, qv.slab_bytes),
                 r4 = make_rsrc(qv.row4, uint64_t(n) * 16);
    uint32_t rowof[K], colof[K];      // pass t: this lane's value is (row rowof[t] of the tile, column colof[t]) - the same for every tile
    T al[K];
    double accv[K];
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const uint32_t v = 64u * t + lane;
        rowof[t] = v / uint32_t(K); colof[t] = v - rowof[t] * uint32_t(K);
        al[t] = T(smem[colof[t]]); accv[t] = 0.0;
    }
    double *exw = ex_lds + wave * (64 * K);
    const uint32_t nwaves = uint32_t(gridDim.x) * 4u;
    // (the slots of the NEXT tile are requested before this tile's values: one memory round trip per tile on a wave's critical path, not two)
    int32_t w4n[4];
    {
        const uint32_t row0 = (uint32_t(blockIdx.x) * 4u + wave) * 64u + lane;
        buf_load<int32_t, 4>(r4, row0 < uint32_t(n) ? row0 * 16u : kOutOfRange, w4n);
    }
    for (uint32_t R0 = (uint32_t(blockIdx.x) * 4u + wave) * 64u; R0 < uint32_t(n); R0 += nwaves * 64u) {
        const uint32_t myrow = R0 + lane;
        int32_t w4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w4[j] = myrow < uint32_t(n) ? w4n[j] : -1;
        {
            const uint32_t nrow = myrow + nwaves * 64u;
            buf_load<int32_t, 4>(r4, nrow < uint32_t(n) ? nrow * 16u : kOutOfRange, w4n);
        }
        const uint32_t e0 = R0 * uint32_t(K);
        T rv[K], dv[K], part[K][4];
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const uint32_t e = e0 + 64u * t + lane;
            T one[1];
            buf_load<T, 1>(rr, e < N ? e * S : kOutOfRange, one);
            rv[t] = one[0];
            buf_load<T, 1>(rd, e < N ? (R0 + rowof[t]) * S : kOutOfRange, one);
            dv[t] = one[0];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t sj = __builtin_amdgcn_ds_bpermute(int(rowof[t] << 2), w4[j]);
                buf_load<T, 1>(rs, sj >= 0 ? (uint32_t(sj) * uint32_t(K) + colof[t]) * S : kOutOfRange, one);
                part[t][j] = one[0];
            }
        }
        const bool more = w4[3] == -2;
        const bool any_more = __builtin_amdgcn_ballot_w64(more) != 0;
        if (any_more) {       // (wave-uniform) rows of five or more patches in this tile: their lanes sum the slots from the fourth on
#pragma unroll
            for (int c = 0; c < K; ++c) exw[lane * K + c] = 0.0;
            if (more) {
                const int32_t c0 = qv.bptr[myrow], c1 = qv.bptr[myrow + 1];
                for (int32_t sl = c0 + 3; sl < c1; ++sl) {
                    const int64_t a2 = qv.bslot[sl];
#pragma unroll
                    for (int c = 0; c < K; ++c) exw[lane * K + c] += double(qv.Yb[a2 * K + c]);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this wave's LDS writes are done before its lanes read each other's
        }
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const uint32_t e = e0 + 64u * t + lane;
            T qi = part[t][0];
#pragma unroll
            for (int j = 1; j < 4; ++j) qi += part[t][j];
            if (any_more) qi += T(exw[64 * t + lane]);
            const T ri = rv[t] - al[t] * qi;
            T one[1] = {ri};
            buf_store<T, 1>(rr, e < N ? e * S : kOutOfRange, one);
            accv[t] += (e < NV || e >= N) ? 0.0 : double(ri) * double(ri) * double(dv[t]);
        }
        if (any_more) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next tile's zeros
    }
#pragma unroll
    for (int c = 0; c < K; ++c) {
        double tsum = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t) tsum += (colof[t] == uint32_t(c)) ? accv[t] : 0.0;
        acc[c] = tsum;
    }
    __syncthreads();
    const double mine = block_sum_column<K>(acc, smem);
    if (threadIdx.x < K) part_rz_next[blockIdx.x * K + threadIdx.x] = mine;
    REMO_VEC_STAMPS(1, t_in, t_head)
}

// ------------------------------------------------------------------------------------------
// The direction launch: beta = <Cr,r>_new/<Cr,r>_old;  p = C r + beta p (and x += alpha p of the step, PcgBuffersT::x_in_direction).
// Two kernels, chosen by launch_pcg_direction: k_pcg_direction_flat (the vectors as flat arrays, 16 bytes per lane) and
// k_pcg_direction_row (a k-wide row per lane; also p0 = C r0 of launch_pcg_init).

// What both do first: beta and the step's alpha; the new <Cr,r> forwarded to the next update launch.  False: the solve is over.
template <int K>
__device__ __forceinline__ bool pcg_direction_head(int step, double tol2, int nb_rz, const double *__restrict__ part_rz_new, double *__restrict__ scal,
                                                   double (&beta)[K], double (&alpha)[K], double *smem /* [16*K] */) {
    if (solve_done(scal, step)) return false;
    double rzn[K];
    reduce_partials<K>(part_rz_new, nb_rz, rzn, smem);
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const double pq = scal[8 + c], rzo = scal[16 + 8 * (step & 1) + c];   // forwarded by the update launch
        const bool live = (rzo > tol2 * scal[c]) && (rzo > scal[kFloorSlot + c]) && (pq > 0.0);
        beta[c] = live ? rzn[c] / rzo : 0.0;
        alpha[c] = live ? rzo / pq : 0.0;      // the step's alpha, from the same operands as in its update launch: the same bits
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) scal[16 + 8 * ((step + 1) & 1) + c] = rzn[c];   // read by the next update launch
    return true;
}

// FLAT form (launcher: n K sizeof(T) below 4 GB): the vectors as arrays of n K values, 16 bytes per lane and access, consecutive
// lanes on consecutive bytes - every load and store instruction of a wave covers 1 KB of whole lines (the row form's cover 1 KB
// out of a 2.5 KB span, three instructions per line).  The column of a value is its index mod K: beta and alpha come from LDS
// (an index into registers would put them into scratch memory); the Jacobi factor of its row is an 8-byte load (an L1 hit for
// four of five).  Buffer accesses: the range check drops what lies behind the last value, dword by dword.
// TP = float beside T = double: a lane still moves 16 bytes per access - FOUR consecutive values, one 16-byte access of p and two of r
// (values e0, e0 + 1 and e0 + 2, e0 + 3: the two accesses of a wave cover the same 2 KB of whole lines); as many load sets in flight.
// TP = float beside T = double, REMO_DIR_P32_MAP = 1 (0: the map above, four consecutive values per lane - a measuring aid only, for a
// library built beside this one; no product build and no test takes it):
// a lane takes TWO consecutive values per access - 16 bytes of r, 8 of p - so that every wave instruction on r covers 1 KB of
// consecutive bytes (on p: 512) and no line is asked for twice; a load set is kDirJ such instructions, values
// base + 128 j + 2 lane, + 1.  The Jacobi factors of the two values' rows (the same row, or two neighbours) come as ONE 16-byte load
// and are chosen in registers; the z load is skipped, wave by wave, once the wave is past the vertex rows.  The first load sets are
// requested BEFORE the scalars are reduced - the partial sums first, so that the wait for them does not wait for the vectors - and
// the head runs while they are in flight: no load depends on beta.  Same operands, same expression: the same bits of p.
#ifndef REMO_DIR_P32_MAP
#define REMO_DIR_P32_MAP 1
#endif
constexpr int kDirUF = 4, kDirJ = 2;     // load sets in flight per lane, wave instructions on r per set: 16 values per lane, as in the map above
template <int K>
__device__ __forceinline__ void pcg_direction_flat_p32(int64_t n, int first, int step, double tol2, int nb_rz, const ChebArgsT<double> &ch,
                                                       const double *__restrict__ part_rz_new, double *__restrict__ scal,
                                                       const double *__restrict__ r, float *__restrict__ p, const double *__restrict__ dinv,
                                                       double *smem /* [16*K] */) {
    REMO_VEC_CLOCK(t_in)
    if (solve_done(scal, step)) return;
    constexpr int UF = kDirUF, NJ = kDirJ;
    constexpr uint32_t WV = 128;          // values per wave instruction
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t N = uint32_t(n) * K, NV = uint32_t(ch.nv) * K;
    const rsrc_t rr = make_rsrc(r, uint64_t(N) * 8), rz = make_rsrc(ch.z, uint64_t(NV) * 8), rp = make_rsrc(p, uint64_t(N) * 4),
                 rd = make_rsrc(dinv, uint64_t(n) * 8), rq = make_rsrc(part_rz_new, uint64_t(nb_rz) * (K * 8));
    // the partial sums of the update launch: rows threadIdx.x + 256 i, the order of reduce_partials (a row beyond nb_rz reads as zero)
    constexpr int NP = kMaxPartialBlocks / 256;
    double part[NP][K];
#pragma unroll
    for (int i = 0; i < NP; ++i) buf_load<double, K>(rq, (uint32_t(threadIdx.x) + 256u * i) * uint32_t(K * 8), part[i]);
    const uint32_t span = uint32_t(gridDim.x) * 4u * (NJ * WV);     // values of one load set of the whole grid
    uint32_t g0 = (uint32_t(blockIdx.x) * 4u + wave) * (NJ * WV) + 2u * lane;
    double rv[UF][NJ][2], zz[UF][NJ][2], dd[UF][NJ][2];
    float pv[UF][NJ][2];
    auto request = [&](uint32_t g) {
#pragma unroll
        for (int u = 0; u < UF; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint32_t e = g + u * span + j * WV;
                buf_load<double, 2>(rr, e < N ? e * 8u : kOutOfRange, rv[u][j]);
                buf_load<float, 2>(rp, e < N ? e * 4u : kOutOfRange, pv[u][j]);
                buf_load<double, 2>(rd, e < N ? (e / uint32_t(K)) * 8u : kOutOfRange, dd[u][j]);
                // vertex rows: the vertex-block solver's result (stored pre-divided by the Jacobi factor) instead of r
                zz[u][j][0] = 0.0; zz[u][j][1] = 0.0;
                if (uint32_t(__builtin_amdgcn_readfirstlane(int(e))) < NV) buf_load<double, 2>(rz, e < NV ? e * 8u : kOutOfRange, zz[u][j]);
            }
    };
    request(g0);
    double rzn[K], beta[K];
#pragma unroll
    for (int c = 0; c < K; ++c) rzn[c] = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < K; ++c) rzn[c] += part[i][c];
    block_sum_256<K>(rzn, smem);
#pragma unroll
    for (int c = 0; c < K; ++c) {
        const double pq = scal[8 + c], rzo = scal[16 + 8 * (step & 1) + c];   // forwarded by the update launch
        const bool live = (rzo > tol2 * scal[c]) && (rzo > scal[kFloorSlot + c]) && (pq > 0.0);
        beta[c] = live ? rzn[c] / rzo : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) scal[16 + 8 * ((step + 1) & 1) + c] = rzn[c];   // read by the next update launch
    __syncthreads();          // (block_sum's last reads of smem)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) smem[c] = first ? 0.0 : beta[c];      // first (no launcher passes it): p = C r, the old direction counts for nothing
    }
    __syncthreads();
    REMO_VEC_CLOCK(t_head)
    while (g0 < N) {
#pragma unroll
        for (int u = 0; u < UF; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const uint32_t e = g0 + u * span + j * WV;
                const uint32_t c0 = e % uint32_t(K);
                float pn[2];
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const bool next_row = c0 + v >= uint32_t(K);
                    const uint32_t c = next_row ? 0u : c0 + v;
                    const double d = next_row ? dd[u][j][1] : dd[u][j][0];
                    const double zi = d * ((e + v < NV) ? zz[u][j][v] : rv[u][j][v]), po = first ? 0.0 : double(pv[u][j][v]);
                    // one rounded product and one fused multiply-add, spelled out: what the compiler makes of `first ? zi : zi + beta * po`
                    // in the other forms (it fuses beta * po), without the branch on `first` around every read of beta
                    pn[v] = float(__builtin_fma(smem[c], po, zi));
                }
                buf_store<float, 2>(rp, e < N ? e * 4u : kOutOfRange, pn);
            }
        g0 += UF * span;
        if (g0 < N) request(g0);
    }
    REMO_VEC_STAMPS(0, t_in, t_head)
}

template <class T, int K, class TP = T>
__global__ void __launch_bounds__(256) k_pcg_direction_flat(int64_t n, int first, int step, double tol2, int nb_rz, ChebArgsT<T> ch,
                                                            const double *__restrict__ part_rz_new, double *__restrict__ scal,
                                                            const T *__restrict__ r, TP *__restrict__ p,
                                                            const T *__restrict__ dinv, T *__restrict__ x) {
    __shared__ double smem[16 * K];
    REMO_VEC_CLOCK(t_in)
    if constexpr (!std::is_same<TP, T>::value && REMO_DIR_P32_MAP == 1) {
        pcg_direction_flat_p32<K>(n, first, step, tol2, nb_rz, ch, part_rz_new, scal, r, p, dinv, smem);
        return;
    }
    double beta[K], alpha[K];
    if (!pcg_direction_head<K>(step, tol2, nb_rz, part_rz_new, scal, beta, alpha, smem)) return;
    constexpr bool SAME = std::is_same<TP, T>::value;
    constexpr int VEC = 16 / int(sizeof(TP));     // values per lane and load set: 16 bytes of p
    constexpr int RV = 16 / int(sizeof(T));       // values per 16-byte access of r
    constexpr int NR = VEC / RV;                  // accesses of r per load set
    constexpr uint32_t S = sizeof(T), SP = sizeof(TP);
    constexpr int UF = 4;
    __syncthreads();          // (block_sum's last reads of smem)
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c) { smem[c] = beta[c]; smem[K + c] = alpha[c]; }
    }
    __syncthreads();
    REMO_VEC_CLOCK(t_head)
    const uint32_t N = uint32_t(n) * K, NV = uint32_t(ch.nv) * K;
    const rsrc_t rr = make_rsrc(r, uint64_t(N) * S), rz = make_rsrc(ch.z, uint64_t(NV) * S), rp = make_rsrc(p, uint64_t(N) * SP),
                 rd = make_rsrc(dinv, uint64_t(n) * S), rx = make_rsrc((SAME && x) ? (const void *)x : (const void *)p, uint64_t(N) * S);
    const bool with_x = SAME && x != nullptr && !first;      // (evaluated values only - the one case with TP != T - has no x)
    const uint32_t span = uint32_t(gridDim.x) * blockDim.x * VEC;
    for (uint32_t g0 = (uint32_t(blockIdx.x) * blockDim.x + threadIdx.x) * VEC; g0 < N; g0 += UF * span) {
        T zv[UF][VEC], xv[UF][VEC], dv[UF][VEC];
        TP pv[UF][VEC];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const uint32_t e0 = g0 + u * span;
            const uint32_t off = e0 < N ? e0 * SP : kOutOfRange;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const uint32_t ej = e0 + uint32_t(RV * j);
                T rj[RV];
                buf_load<T, RV>(rr, ej < N ? ej * S : kOutOfRange, rj);
                // vertex rows: the vertex-block solver's result (stored pre-divided by the Jacobi factor) instead of r
                T zz[RV];       // (no branch: the other lanes hand over an offset out of range and send no request)
                buf_load<T, RV>(rz, ej < NV ? ej * S : kOutOfRange, zz);
#pragma unroll
                for (int v = 0; v < RV; ++v) zv[u][RV * j + v] = (ej + v < NV) ? zz[v] : rj[v];
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T one[1];
                buf_load<T, 1>(rd, e0 < N ? ((e0 + v) / uint32_t(K)) * S : kOutOfRange, one);
                dv[u][v] = one[0];
            }
            if (!first) buf_load<TP, VEC>(rp, off, pv[u]);
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) pv[u][v] = TP(0);
            }
            if (with_x) buf_load<T, VEC>(rx, off, xv[u]);
            else {
#pragma unroll
                for (int v = 0; v < VEC; ++v) xv[u][v] = T(0);
            }
        }
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const uint32_t e0 = g0 + u * span;
            const uint32_t off = e0 < N ? e0 * SP : kOutOfRange;
            TP pn[VEC];
            T xn[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const uint32_t c = (e0 + v) % uint32_t(K);
                const T zi = dv[u][v] * zv[u][v], po = T(pv[u][v]);
                pn[v] = TP(first ? zi : zi + T(smem[c]) * po);      // (the launchers pass first = 0; kept: it fixes which product the compiler fuses)
                xn[v] = xv[u][v] + T(smem[K + c]) * po;
            }
            buf_store<TP, VEC>(rp, off, pn);
            if (with_x) buf_store<T, VEC>(rx, off, xn);
        }
    }
    REMO_VEC_STAMPS(0, t_in, t_head)
}
// ROW form.  first: p0 = C r0 (no scalars, no old direction).
// U rows per thread are loaded before any of them is stored: p is read and written through the same pointer, and a store
// of one row otherwise holds back the loads of the next (one row in flight per thread: 2.7 TB/s at 5.4 M rows in fp32)
#ifndef REMO_DIR_U
#define REMO_DIR_U 4
#endif
template <class T, int K, class TP = T>
__global__ void __launch_bounds__(256) k_pcg_direction_row(int64_t n, int first, int step, double tol2, int nb_rz, ChebArgsT<T> ch,
                                                           const double *__restrict__ part_rz_new, double *__restrict__ scal,
                                                           const T *__restrict__ r, TP *__restrict__ p,
                                                           const T *__restrict__ dinv, T *__restrict__ x) {
    __shared__ double smem[16 * K];
    double beta[K], alpha[K];
    if (first) {
        if (solve_done(scal, step)) return;
#pragma unroll
        for (int c = 0; c < K; ++c) { beta[c] = 0.0; alpha[c] = 0.0; }
    } else if (!pcg_direction_head<K>(step, tol2, nb_rz, part_rz_new, scal, beta, alpha, smem)) {
        return;
    }
    constexpr int U = REMO_DIR_U;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i0 = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i0 < n; i0 += U * stride) {
        T d[U], zv[U][K], pv[U][K], xv[U][K];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            d[u] = T(0);
#pragma unroll
            for (int c = 0; c < K; ++c) { zv[u][c] = T(0); pv[u][c] = T(0); xv[u][c] = T(0); }
            if (i < n) {
                d[u] = dinv[i];
                const T *src = (i < ch.nv) ? ch.z : r;   // C r: Chebyshev result on the vertex block (stored as z / dinv), Jacobi elsewhere
#pragma unroll
                for (int c = 0; c < K; ++c) zv[u][c] = src[i * K + c];
                if (!first)
#pragma unroll
                    for (int c = 0; c < K; ++c) pv[u][c] = T(p[i * K + c]);
                if (x && !first)
#pragma unroll
                    for (int c = 0; c < K; ++c) xv[u][c] = x[i * K + c];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = i0 + u * stride;
            if (i < n)
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    const T zi = d[u] * zv[u][c];
                    // (the compiler contracts beta * p into one fma on the rounded zi; pcg_direction_flat_p32 spells the same two operations
                    // out, and tests/test_gpu_vector_launches.py holds the two forms to the same bits)
                    p[i * K + c] = TP(first ? zi : zi + T(beta[c]) * pv[u][c]);
                    // x += alpha p of THIS step, with the old direction that is in registers anyway (PcgBuffersT::x_in_direction):
                    // the update launch then neither reads p nor touches x - one pass over p less per step
                    if (x && !first) x[i * K + c] = xv[u][c] + T(alpha[c]) * pv[u][c];
                }
        }
    }
}
template <int K>
__global__ void __launch_bounds__(256) k_pcg_final(int step, int nb_rz, const double *__restrict__ part_rz, const double *__restrict__ scal,
                                                   PcgProgress *progress, int progress_len) {
    __shared__ double smem[16 * K];
    if (solve_done(scal, step)) return;   // the "done" record already holds the final <Cr,r>
    double rz[K];
    reduce_partials<K>(part_rz, nb_rz, rz, smem);
    if (threadIdx.x == 0) publish_progress(progress + (step % (progress_len - 1)), rz, K, step);
}

int vec_grid(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > kMaxPartialBlocks / 2) g = kMaxPartialBlocks / 2;
    if (g < 1) g = 1;
    return int(g);
}

template <class T> static int nb_rz(const PcgBuffersT<T> &b) { return b.nb_vec + ((b.vs.degree > 0 && b.vs.nv > 0) ? cheb_grid(b.vs.nv) : 0); }

template <class T> void launch_pcg_init(const CsrViewT<T> &A, int k, const T *f, const PcgBuffersT<T> &b, hipStream_t s) {
    const int64_t n = A.n;
    const int g = b.nb_vec;
    const ChebArgsT<T> ch = cheb_args(b.vs);
    auto go = [&](auto *p) {      // p: the search direction in its storage type TP
        using TP = std::remove_pointer_t<decltype(p)>;
        for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; launch256(k_pcg_init<T, K, TP>, g, s, n, ch, f, b.dinv, b.x, b.r, p, b.part_rz); });
        launch_vertex_solve(b.vs, k, 0, b.r, b.dinv, b.rz0, b.nb_vec, b.part_rz, s);
        if (ch.nv > 0)
            for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; launch256(k_pcg_direction_row<T, K, TP>, g, s, n, 1, 0, 0.0, nb_rz(b), ch, b.part_rz, b.rz0, b.r, p, b.dinv, (T *)nullptr); });
    };
    if constexpr (sizeof(T) == 8) {
        if (b.p32) { go(b.p32); return; }      // the search direction in fp32 storage: the same launches, TP = float
    }
    go(b.p);
}

template <class T> static UpdHeadT<T> update_head(const CsrViewT<T> &A, int step, double tol2, const PcgBuffersT<T> &b) {
    UpdHeadT<T> hd;
    // the patch operator's <p, A p> bins: two sets taken in turn by step parity, this launch clears the set of the next step
    const bool bins = b.pq_bins && b.defer_q && A.patch && !vertex_first_folds(b.vs);
    hd.step = step; hd.tol2 = tol2;
    hd.nb_spmv = bins ? kPqBins : b.nb_spmv; hd.nb_rz = nb_rz(b);
    hd.part_pq = bins ? b.part_pq + (step & 1) * (kPqBins * 8) : b.part_pq;
    hd.part_rz_cur = b.part_rz + (step & 1) * (kMaxPartialBlocks * 8);
    hd.rz0 = b.rz0;
    hd.progress = b.progress; hd.progress_len = b.progress_len;
    hd.clear_bins = bins ? b.part_pq + ((step + 1) & 1) * (kPqBins * 8) : nullptr;
    return hd;
}

template <class T> void launch_pcg_update(const CsrViewT<T> &A, int k, int step, double tol2, const PcgBuffersT<T> &b, hipStream_t s) {
    const int64_t n = A.n;
    const int g = b.nb_vec;
    double *nxt = b.part_rz + ((step + 1) & 1) * (kMaxPartialBlocks * 8);
    constexpr uint64_t kBufferLimit = 0xFFFFF000ull;   // what a buffer descriptor's range check covers (kutil.h kOutOfRange)
    // 1. the form
    const bool folded = vertex_first_folds(b.vs);
    const bool slab = b.defer_q && A.patch && !folded;      // the shared rows of q = A p are still in the patch operator's boundary slab
    const bool skip_x = b.x_in_direction;
    uint64_t slab_bytes = 0;
    if (slab && g_tune.slab_masked) {
        const uint64_t bytes = uint64_t(A.patch->t.nslot_cap) * uint64_t(k) * sizeof(T);
        slab_bytes = bytes < kBufferLimit ? bytes : 0;
    }
    const bool masked = slab_bytes != 0;
    // (fp32 storage: 256 bytes per wave and access - the row form is ahead there, 74.7 against 76.3 ms)
    const bool tile = g_tune.tile_update && sizeof(T) == 8 && masked && A.patch->t.row4 && skip_x && uint64_t(n) * uint64_t(k) * sizeof(T) < kBufferLimit &&
                      uint64_t(n) * 16 < kBufferLimit;
    const bool one_by_one = kProbes && slab && !g_tune.slab_ahead;      // key 27 = 0: no product build reaches it
    // 2. its arguments
    UpdHeadT<T> hd = update_head(A, step, tol2, b);
    hd.ev = EvSlotsT<T>{b.x_ev_at, b.x_ev, b.x_ev_n};
    const ChebArgsT<T> ch = cheb_args(b.vs);
    QViewT<T> qv;
    qv.skip_x = skip_x ? 1 : 0;
    if (slab) { qv.bptr = A.patch->t.bptr; qv.bslot = A.patch->t.bslot; qv.Yb = A.patch->Yb; }
    if (masked) { qv.slab_bytes = slab_bytes; qv.row4 = A.patch->t.row4; }
    // 3. the launch
    // fp32 search direction (fp64 storage): read by the x_ev slots alone (the host grants it with defer_q, x in the direction launch and no x: set_launch_shape)
    if (sizeof(T) == 8 && b.p32 && (!slab || !skip_x || b.x || one_by_one)) throw std::logic_error("update launch: an fp32 search direction outside the evaluated-values path of the patch operator");
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if constexpr (sizeof(T) == 8) {
            if (b.p32) {
                if (tile) launch256(k_pcg_update_tile<double, K, float>, g, s, n, hd, ch.nv, nxt, b.p32, b.r, b.dinv, qv);
                else if (masked) launch256(k_pcg_update_p32<K, true>, g, s, n, hd, ch.nv, nxt, b.p32, b.q, b.r, b.dinv, qv);
                else launch256(k_pcg_update_p32<K, false>, g, s, n, hd, ch.nv, nxt, b.p32, b.q, b.r, b.dinv, qv);
                return;
            }
        }
        if (folded) {
            FoldArgsT<T> fold;
            const ChebStep cs = cheb_step(b.vs);      // the chain's first step
            fold.nb_flat = g;
            fold.rowptr = b.vs.rowptr; fold.col = b.vs.col; fold.val = b.vs.val;
            fold.d_new = b.vs.d[1]; fold.stage = b.vs.d[0];
            fold.c1 = cs.c1; fold.c2 = cs.c2;
            const int grid = g + int((b.vs.nv + 31) / 32);   // the vertex workgroups leave no partial sums: one row group each
            launch256(k_pcg_update_folded<T, K>, grid, s, n, hd, ch, nxt, b.p, b.q, b.x, b.r, b.dinv, fold, qv.skip_x);
        } else if (tile) {
            if constexpr (sizeof(T) == 8) launch256(k_pcg_update_tile<T, K>, g, s, n, hd, ch.nv, nxt, b.p, b.r, b.dinv, qv);
        } else if (one_by_one) {
            if constexpr (kProbes) launch256(k_pcg_update<T, K, false, false>, g, s, n, hd, ch.nv, nxt, b.p, b.q, b.x, b.r, b.dinv, qv);
        } else {
            for_bool(masked, [&](auto mc) { launch256(k_pcg_update<T, K, decltype(mc)::value>, g, s, n, hd, ch.nv, nxt, b.p, b.q, b.x, b.r, b.dinv, qv); });
        }
    });
    launch_vertex_solve(b.vs, k, step, b.r, b.dinv, b.rz0, b.nb_vec, nxt, s, folded);      // (an fp32 direction never goes with the folded step: it needs the slab)
}

// Residual replacement of the mixed mode, in place of launch_pcg_update at the chosen steps:
//   x32 += alpha p;  x64 += x32, x32 = 0;  r32 = float(f - A64 x64);  C r;  <Cr,r> partials
// The search direction and the scalars carry on, so the Krylov process is not restarted; what is
// removed is the drift of the fp32 recurrence residual from the true one.
template <int K>
__global__ void __launch_bounds__(256) k_mixed_replace(int64_t n, int64_t nv, const double *__restrict__ f, const double *__restrict__ q64,
                                                       float *__restrict__ r, const float *__restrict__ dinv, double *__restrict__ part_rz_next,
                                                       const double *__restrict__ scal, int step) {
    __shared__ double smem[16 * K];
    if (solve_done(scal, step)) return;
    double acc[K];
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        const float d = dinv[i];
        const bool coarse = i < nv;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const float ri = float(f[i * K + c] - q64[i * K + c]);
            r[i * K + c] = ri;
            acc[c] += coarse ? 0.0 : double(ri) * double(ri) * double(d);
        }
    }
    block_sum<K>(acc, smem);
    if (threadIdx.x < K) part_rz_next[blockIdx.x * K + threadIdx.x] = acc[threadIdx.x];
}

void launch_pcg_replace(const CsrViewT<float> &A, const CsrViewT<double> &A64, int k, int step, double tol2, const PcgBuffersT<float> &b,
                        const double *f64, double *x64, double *q64, hipStream_t s) {
    const int64_t n = A.n;
    const int g = b.nb_vec;
    double *nxt = b.part_rz + ((step + 1) & 1) * (kMaxPartialBlocks * 8);
    const ChebArgsT<float> ch = cheb_args(b.vs);
    const UpdHeadT<float> hd = update_head(A, step, tol2, b);
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; launch256(k_pcg_update_x<float, K>, g, s, n, hd, b.p, b.x); });
    launch_mixed_accumulate(n * k, x64, b.x, 1, s);
    launch_spmm(A64, k, (const double *)x64, q64, (double *)nullptr, (const double *)nullptr, b.nb_spmv, s, 0);
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; launch256(k_mixed_replace<K>, g, s, n, ch.nv, f64, q64, b.r, b.dinv, nxt, b.rz0, step); });
    launch_vertex_solve(b.vs, k, step, b.r, b.dinv, b.rz0, b.nb_vec, nxt, s);
}

// add_x: this launch also forms x += alpha p of the step (b.x_in_direction and the step's update launch left x alone; a residual
// replacement of the mixed mode updates x itself)
template <class T> void launch_pcg_direction(const CsrViewT<T> &A, int k, int step, double tol2, const PcgBuffersT<T> &b, hipStream_t s, bool add_x) {
    const int64_t n = A.n;
    const int g = b.nb_vec;
    const double *nw = b.part_rz + ((step + 1) & 1) * (kMaxPartialBlocks * 8);
    const ChebArgsT<T> ch = cheb_args(b.vs);
    T *xp = (add_x && b.x_in_direction) ? b.x : nullptr;
    const bool flat = g_tune.flat_direction && uint64_t(n) * uint64_t(k) * sizeof(T) < 0xFFFFF000ull;
    auto go = [&](auto *p, T *x) {      // p: the search direction in its storage type TP
        using TP = std::remove_pointer_t<decltype(p)>;
        for_k(k, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            if (flat) launch256(k_pcg_direction_flat<T, K, TP>, g, s, n, 0, step, tol2, nb_rz(b), ch, nw, b.rz0, b.r, p, b.dinv, x);
            else launch256(k_pcg_direction_row<T, K, TP>, g, s, n, 0, step, tol2, nb_rz(b), ch, nw, b.rz0, b.r, p, b.dinv, x);
        });
    };
    if constexpr (sizeof(T) == 8) {
        if (b.p32) { go(b.p32, nullptr); return; }      // fp32 search direction (no x: evaluated values only)
    }
    go(b.p, xp);
}

// One direction launch on the caller's own vectors and scalars, fp64 storage with the direction in fp32 (remo_debug_direction_forms):
// flat != 0: k_pcg_direction_flat<double, k, float>, else k_pcg_direction_row<double, k, float>; `grid` workgroups.
void launch_direction_form(bool flat, int grid, int64_t n, int64_t nv, int k, int step, double tol2, int nb_rz, const double *part_rz_new,
                           double *scal, const double *r, float *p, const double *dinv, double *z, hipStream_t s) {
    ChebArgsT<double> ch;
    ch.nv = nv; ch.inv_theta = 0.0; ch.z = z; ch.res = nullptr; ch.d0 = nullptr;
    if (uint64_t(n) * uint64_t(k) * 8 >= 0xFFFFF000ull || nb_rz > kMaxPartialBlocks || grid < 1) throw std::invalid_argument("launch_direction_form: sizes");
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (flat) launch256(k_pcg_direction_flat<double, K, float>, grid, s, n, 0, step, tol2, nb_rz, ch, part_rz_new, scal, r, p, dinv, (double *)nullptr);
        else launch256(k_pcg_direction_row<double, K, float>, grid, s, n, 0, step, tol2, nb_rz, ch, part_rz_new, scal, r, p, dinv, (double *)nullptr);
    });
}

// probe builds: where the vector launches leave their clocks (nullptr: nowhere) - four words per workgroup, REMO_VEC_STAMPS
void set_vector_stamps(long long *stamps) {
#ifdef REMO_PROBES
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_vec_stamps), &stamps, sizeof stamps) != hipSuccess) throw std::runtime_error("set_vector_stamps: hipMemcpyToSymbol failed");
#else
    (void)stamps;
#endif
}

template <class T> void launch_pcg_final(int k, int step, const PcgBuffersT<T> &b, hipStream_t s) {
    const double *cur = b.part_rz + (step & 1) * (kMaxPartialBlocks * 8);
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; launch256(k_pcg_final<K>, 1, s, step, nb_rz(b), cur, b.rz0, b.progress, b.progress_len); });
}

#define REMO_INSTANTIATE_PCG(T)                                                                                          \
    template void launch_pcg_init<T>(const CsrViewT<T> &, int, const T *, const PcgBuffersT<T> &, hipStream_t);          \
    template void launch_pcg_update<T>(const CsrViewT<T> &, int, int, double, const PcgBuffersT<T> &, hipStream_t);      \
    template void launch_pcg_direction<T>(const CsrViewT<T> &, int, int, double, const PcgBuffersT<T> &, hipStream_t, bool);   \
    template void launch_pcg_final<T>(int, int, const PcgBuffersT<T> &, hipStream_t);
REMO_INSTANTIATE_PCG(double)
REMO_INSTANTIATE_PCG(float)
#undef REMO_INSTANTIATE_PCG

}  // namespace remo
