// amg.hip — smoothed-aggregation multigrid on the P1 (vertex) block, gfx950.
//
// Why: in 2D (graded axisymmetric meshes, 80 k vertices at config 2) the Chebyshev polynomial on the vertex block needs degree
// 28 on [lmax / 2400, lmax] - 14 paired launches, two thirds of a PCG step - and still takes twice the steps of an exact
// vertex solve (offline, tools/amg_study_2d.py: exact 58, Chebyshev(28) 119, this cycle 71 steps at 3.7 sweeps of the block).
//
// Setup per batch (the matrix changes with every batch), all on the device, deterministic (no floating-point atomics):
//   aggregation   distance-2 maximal independent set of the matrix graph by hashed priorities (Bell / Dalton / Olson 2012):
//                 roots, then their neighbours, then the neighbours' neighbours by the strongest connection
//   prolongator   P = (I - 4 / (3 lmax) D^-1 A) P0, one generic row-wise sparse product (LDS hash set per wave for the
//                 pattern, sorted; values: every product of the row formed once, handed to its column through an LDS
//                 table and added there in the order of the row - a fixed order),
//                 R = P^T by count / scan / scatter and an LDS sort of every row
//   coarse matrix A' = R (A P), two more products
//   coarsest      dense inverse (Gauss-Jordan in LDS, <= 64 rows)
// Cycle: V(1,1) with damped Jacobi (omega = 1.6 / lmax, the one-term Chebyshev polynomial of [lmax / 4, lmax]), symmetric, so
// the PCG sees a fixed symmetric positive definite preconditioner.  The host waits ONCE per level during the setup (number of
// aggregates); product sizes stay on the device (capacity-bound arrays, clamped row pointers, flags read at the next wait).
#include <hip/hip_runtime.h>
#include <limits.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "amg.h"
#include "remo_internal.h"
#include "wave_util.h"
#include "kutil.h"

namespace remo {
namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool amg_done(const double *scal, int step) {
    if (!scal) return false;
    const int d = reinterpret_cast<const int *>(scal + kDoneSlot)[0];
    return d != 0 && d <= step;
}

// ---- leading block -> compact CSR ---------------------------------------------------------------------------------------
template <int PASS>
__global__ void __launch_bounds__(256) k_block_copy(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, int32_t *__restrict__ cnt, const int32_t *__restrict__ orp,
                                                    int32_t *__restrict__ oc, double *__restrict__ ov) {
    const int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= nv) return;
    const int32_t rs = rowptr[row], re = rowptr[row + 1];
    if (PASS == 0) {
        cnt[row] = lower_bound_i32(col, rs, re, int32_t(nv)) - rs;
    } else {
        const int32_t at = orp[row], len = orp[row + 1] - at;
        for (int32_t e = 0; e < len; ++e) { oc[at + e] = col[rs + e]; ov[at + e] = val[rs + e]; }
    }
}

// Jacobi factors and the Gershgorin bound of D^-1 A; flag |= 1 when a diagonal entry is missing or not positive
__global__ void __launch_bounds__(256) k_level_diag(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, double *__restrict__ dinv, unsigned long long *bound_bits,
                                                    int32_t *flag) {
    double m = 0.0;
    const int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row < n) {
        double s = 0.0, d = 0.0;
        for (int32_t p = rowptr[row]; p < rowptr[row + 1]; ++p) {
            s += fabs(val[p]);
            if (col[p] == row) d = val[p];
        }
        if (!(d > 0.0)) { atomicOr(flag, 1); d = 1.0; }
        dinv[row] = 1.0 / d;
        m = s / d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(bound_bits, (unsigned long long)__double_as_longlong(m));   // positive doubles order like their bits
}

// ---- aggregation: distance-2 maximal independent set ---------------------------------------------------------------------
// tuple = state (2 bits: 2 root, 1 undecided, 0 removed) | hashed priority (30 bits) | index (32 bits): unique, so maxima are too
constexpr uint64_t kTupMask = (uint64_t(1) << 62) - 1;

__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(256) k_mis_init(int64_t n, uint64_t *__restrict__ tup) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) tup[i] = (uint64_t(1) << 62) | (uint64_t(hash_u32(uint32_t(i)) >> 2) << 32) | uint64_t(uint32_t(i));
}

__global__ void __launch_bounds__(256) k_mis_max(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 const uint64_t *__restrict__ tup, uint64_t *__restrict__ m1) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t m = tup[i];
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) { const uint64_t t = tup[col[p]]; m = t > m ? t : m; }
    m1[i] = m;
}

// second hop + decision; tup is updated in place (the other threads read m1 only)
__global__ void __launch_bounds__(256) k_mis_update(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    uint64_t *__restrict__ tup, const uint64_t *__restrict__ m1) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t t = tup[i];
    if ((t >> 62) != 1) return;
    uint64_t m = m1[i];
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) { const uint64_t v = m1[col[p]]; m = v > m ? v : m; }
    if (m == t) tup[i] = (uint64_t(2) << 62) | (t & kTupMask);
    else if ((m >> 62) == 2) tup[i] = t & kTupMask;
}

// After the fixed number of iterations a few nodes (0.6 % at 80 k rows after six) are still undecided: they have no root
// within two hops.  One more sweep settles them without further iterations: root if no undecided neighbour has a higher tuple,
// removed otherwise (such a node sits next to a new root or next to a node that does, and joins through k_agg_near / k_agg_far;
// the odd node at the end of a longer chain stays without an aggregate: it is smoothed, not coarse-corrected).  out = final tuples.
__global__ void __launch_bounds__(256) k_mis_finish(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const uint64_t *__restrict__ tup, uint64_t *__restrict__ out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t t = tup[i];
    uint64_t r = t;
    if ((t >> 62) == 1) {
        bool top = true;
        for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            const uint64_t v = tup[col[p]];
            if ((v >> 62) == 1 && v > t) top = false;
        }
        r = top ? ((uint64_t(2) << 62) | (t & kTupMask)) : (t & kTupMask);
    }
    out[i] = r;
}

__global__ void __launch_bounds__(256) k_mis_flags(int64_t n, const uint64_t *__restrict__ tup, int32_t *__restrict__ isroot) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) isroot[i] = (tup[i] >> 62) == 2 ? 1 : 0;
}

// roots take their number, the others the root neighbour of the highest priority (-1: none)
__global__ void __launch_bounds__(256) k_agg_near(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                  const uint64_t *__restrict__ tup, const int32_t *__restrict__ id, int32_t *__restrict__ agg) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if ((tup[i] >> 62) == 2) { agg[i] = id[i]; return; }
    uint64_t best = 0;
    int32_t bj = -1;
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
        const int32_t j = col[p];
        const uint64_t t = tup[j];
        if ((t >> 62) == 2 && t > best) { best = t; bj = j; }
    }
    agg[i] = bj >= 0 ? id[bj] : -1;
}

// the rest: the aggregate of the neighbour with the strongest connection (ties: the lower index, columns ascend)
__global__ void __launch_bounds__(256) k_agg_far(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 const double *__restrict__ val, const int32_t *__restrict__ agg_in, int32_t *__restrict__ agg_out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t a = agg_in[i];
    if (a < 0) {
        double w = -1.0;
        for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
            const int32_t j = col[p];
            if (j == i) continue;
            const int32_t aj = agg_in[j];
            const double v = fabs(val[p]);
            if (aj >= 0 && v > w) { w = v; a = aj; }
        }
    }
    agg_out[i] = a;
}

// S = I - wp D^-1 A on the pattern of A, and the tentative prolongator (one unit entry per row) as CSR
__global__ void __launch_bounds__(256) k_smoothing_factor(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                          const double *__restrict__ val, const double *__restrict__ dinv, const unsigned long long *bound_bits,
                                                          double *__restrict__ sval, const int32_t *__restrict__ agg, int32_t *__restrict__ p0rp,
                                                          int32_t *__restrict__ p0c, double *__restrict__ p0v) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    p0rp[i] = int32_t(i);
    if (i == n) return;
    const double f = 4.0 / (3.0 * __longlong_as_double((long long)bound_bits[0])) * dinv[i];   // prolongator smoothing 4 / (3 lmax)
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) sval[p] = (col[p] == i ? 1.0 : 0.0) - f * val[p];
    const int32_t a = agg[i];
    p0c[i] = a >= 0 ? a : 0;
    p0v[i] = a >= 0 ? 1.0 : 0.0;
}

// ---- generic sparse product C = X Y, one wave per row of X ----------------------------------------------------------------
// PASS 0 counts the distinct columns of every row; PASS 1 (row offsets known) writes them sorted with their values.
// Pattern: the columns of the rows of Y that X's row names go into an LDS hash set, are compacted and sorted.  Values: driven by
// the products, not by lookups - every x_ik y_kj of the row is formed once, finds its output column in the sorted list in LDS and
// leaves its rounded value in a term table [entry of X's row][output column]; every output column then adds its terms in the
// order of X's row, starting from + 0.0.  So a value is the sequential sum of the separately rounded products, whatever the
// round size or the lane that formed a product (the term goes through LDS: nothing is contracted into an fma).
// The columns inside a row of Y are distinct (one writer per cell); neither X's nor Y's rows need ascend.
// flag |= 1: a row does not fit the hash table or has more than SLOTS / 2 distinct columns; it is written empty.
template <int PASS, int SLOTS>
__global__ void __launch_bounds__(256) k_spgemm(int64_t nx, const int32_t *__restrict__ xrp, const int32_t *__restrict__ xc, const double *__restrict__ xv,
                                                const int32_t *__restrict__ yrp, const int32_t *__restrict__ yc, const double *__restrict__ yv,
                                                int32_t *__restrict__ cnt, const int32_t *__restrict__ crp, int32_t *__restrict__ cc,
                                                double *__restrict__ cv, int32_t *flag) {   // PASS 1: crp has been clamped to the capacity of cc / cv (k_clamp_rowptr)
    __shared__ int32_t keys[4][SLOTS];
    __shared__ int32_t list[4][SLOTS];
    constexpr int kTerms = SLOTS < 512 ? 512 : 1024;   // cells of a wave's term table: a round takes kTerms / c entries of X (LDS per workgroup: 24 / 52 KB)
    __shared__ double terms[4][PASS == 1 ? kTerms : 1];
    __shared__ int32_t pstart[4][PASS == 1 ? 64 : 1], pys[4][PASS == 1 ? 64 : 1];   // per entry of the round: its first product, where its row of Y starts,
    __shared__ double pxv[4][PASS == 1 ? 64 : 1];                                   // its value
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + wave;
    if (row >= nx) return;                      // no block-wide barriers below: a wave works on its own tables
    int32_t *K = keys[wave], *L = list[wave];
    for (int sl = lane; sl < SLOTS; sl += 64) K[sl] = INT_MAX;
    wave_sync();
    const int32_t xs = xrp[row], xe = xrp[row + 1];
    bool overflow = false;
    for (int32_t p = xs + lane; p < xe; p += 64) {
        const int32_t k = xc[p];
        const int32_t ye = yrp[k + 1];
        for (int32_t q = yrp[k]; q < ye; ++q) {
            const int32_t j = yc[q];
            uint32_t h = ((uint32_t(j) * 2654435761u) >> 16) & (SLOTS - 1);
            bool placed = false;
            for (int probe = 0; probe < SLOTS; ++probe) {
                const int32_t old = atomicCAS(&K[h], INT_MAX, j);
                if (old == INT_MAX || old == j) { placed = true; break; }
                h = (h + 1) & (SLOTS - 1);
            }
            overflow |= !placed;
        }
    }
    wave_sync();
    // compact the occupied slots into the list (any order), count them
    int c = 0;
    for (int base = 0; base < SLOTS; base += 64) {
        const int32_t v = K[base + lane];
        const bool occ = v != INT_MAX;
        const uint64_t bal = __builtin_amdgcn_ballot_w64(occ);
        if (occ) L[c + __builtin_popcountll(bal & ((uint64_t(1) << lane) - 1))] = v;
        c += __builtin_popcountll(bal);
    }
    if (__builtin_amdgcn_ballot_w64(overflow) != 0 || c > SLOTS / 2) {
        if (lane == 0) atomicOr(flag, 1);
        c = 0;
    }
    if (PASS == 0) {
        if (lane == 0) cnt[row] = c;
        return;
    }
    if (c == 0) return;
    int m = 64;                                  // bitonic sort of the list padded to a power of two
    while (m < c) m <<= 1;
    for (int t = c + lane; t < m; t += 64) L[t] = INT_MAX;
    wave_sync();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < m / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int32_t a = L[lo], b = L[hi];
                if ((a > b) == up) { L[lo] = b; L[hi] = a; }
            }
            wave_sync();
        }
    const int64_t off = crp[row];
    const int room = int(crp[row + 1] - crp[row]);   // < c only when the product outgrew its arrays (flagged by k_clamp_rowptr): stay inside them
    if (c > room) c = room;
    if (c <= 0) return;
    // values, a round of up to npmax entries of X at a time: lane pp fetches entry pp and the bounds of its row of Y, a scan numbers
    // the round's products, and the lanes take the PRODUCTS (entry pp, entry q of that row): the product's output column t by a
    // search of the sorted list in LDS, its rounded value into cell (pp, t) of the term table - one writer per cell, the columns of
    // a row of Y being distinct; a column beyond a clamped list has no cell.  Then the lane of column t adds its cells in the order
    // of X's row and clears them: a term that does not exist is the + 0.0 of a cleared cell, the same sums as a serial walk.
    double *V = terms[wave];
    int32_t *PS = pstart[wave], *PY = pys[wave];
    double *PX = pxv[wave];
    constexpr int NACC = SLOTS / 128;            // output columns per lane: c <= SLOTS / 2
    double acc[NACC];
#pragma unroll
    for (int a = 0; a < NACC; ++a) acc[a] = 0.0;
    const int npmax = kTerms / c < 64 ? kTerms / c : 64;   // entries of X per round: >= 4 (512 slots) or 8 (c <= SLOTS / 2), one per lane at most
    for (int i = lane; i < c * npmax; i += 64) V[i] = 0.0;
    for (int32_t p0 = xs; p0 < xe; p0 += npmax) {
        const int np = (xe - p0 < npmax) ? int(xe - p0) : npmax;
        int32_t ys = 0, len = 0;
        double xval = 0.0;
        if (lane < np) {
            const int32_t k = xc[p0 + lane];
            xval = xv[p0 + lane];
            ys = yrp[k];
            len = yrp[k + 1] - ys;
        }
        int32_t incl = len;                      // products up to and including this lane's entry
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        const int32_t total = __shfl(incl, 63, 64);
        if (lane < np) { PS[lane] = incl - len; PY[lane] = ys; PX[lane] = xval; }
        wave_sync();                             // also: the cells cleared above / by the round before
        for (int32_t idx = lane; idx < total; idx += 64) {
            int lo = 1, hi = np;                 // pp = the last entry that starts at or before product idx (empty rows of Y start where the next one does)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (PS[mid] <= idx) lo = mid + 1; else hi = mid;
            }
            const int pp = lo - 1;
            const int32_t q = PY[pp] + (idx - PS[pp]);
            const int32_t j = yc[q];
            const double yval = yv[q];
            const int t = lower_bound_i32(L, 0, c, j);
            if (t < c && L[t] == j) V[pp * c + t] = PX[pp] * yval;
        }
        wave_sync();
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
            const int t = lane + 64 * a;
            if (t < c)
                for (int pp = 0; pp < np; ++pp) { acc[a] += V[pp * c + t]; V[pp * c + t] = 0.0; }
        }
    }
#pragma unroll
    for (int a = 0; a < NACC; ++a) {
        const int t = lane + 64 * a;
        if (t < c) { cc[off + t] = L[t]; cv[off + t] = acc[a]; }
    }
}

// row pointers of a product whose arrays were allocated by an upper bound, before the size is known on the host: anything
// beyond the capacity is cut off (rows stay inside the arrays, consumers never index past them) and flagged
__global__ void __launch_bounds__(256) k_clamp_rowptr(int64_t n, int32_t *__restrict__ rowptr, int32_t capacity, int32_t *flag) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int32_t v = rowptr[i];
    if (v > capacity) { rowptr[i] = capacity; if (i == n) atomicOr(flag, 2); }
}

// ---- transpose without a device-wide sort: count, scan, scatter in any order, then every row sorted by a wave in LDS --------
__global__ void __launch_bounds__(256) k_tr_count(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int32_t *__restrict__ cnt) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) atomicAdd(&cnt[col[p]], 1);
}
__global__ void __launch_bounds__(256) k_tr_fill(int64_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                 const int32_t *__restrict__ rrp, int32_t *__restrict__ cursor, int32_t *__restrict__ rc, double *__restrict__ rv) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
        const int32_t c = col[p];
        const int32_t at = rrp[c] + atomicAdd(&cursor[c], 1);
        rc[at] = int32_t(i);
        rv[at] = val[p];
    }
}
// Rows of R longer than MINLEN and up to MAXLEN entries, WAVES rows per workgroup (a wave sorts its row in LDS).  Two launches cover a
// level: <0, 512, 4> takes nearly every row; <512, 4096, 1> the few long ones (at 184 k vertices of a graded lattice mesh a coarse
// aggregate's smoothed prolongator column holds more than 512 entries: the hierarchy could not be built) - beyond 4096 flag 4.
constexpr int kTrMax = 512, kTrMaxLong = 4096;
template <int MINLEN, int MAXLEN, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_tr_sort(int64_t nr, const int32_t *__restrict__ rrp, int32_t *__restrict__ rc, double *__restrict__ rv, int32_t *flag) {
    __shared__ int32_t keys[WAVES][MAXLEN];
    __shared__ double vals[WAVES][MAXLEN];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = int64_t(blockIdx.x) * WAVES + wave;
    if (row >= nr) return;
    const int32_t rs = rrp[row], len = rrp[row + 1] - rs;
    if (len <= 1 || len <= MINLEN) return;
    if (len > MAXLEN) { if (lane == 0 && MAXLEN == kTrMaxLong) atomicOr(flag, 4); return; }
    int32_t *K = keys[wave];
    double *V = vals[wave];
    int m = 64;
    while (m < len) m <<= 1;
    for (int t = lane; t < m; t += 64) { K[t] = t < len ? rc[rs + t] : INT_MAX; V[t] = t < len ? rv[rs + t] : 0.0; }
    wave_sync();
    for (int size = 2; size <= m; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < m / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int32_t a = K[lo], b = K[hi];
                if ((a > b) == up) { K[lo] = b; K[hi] = a; const double x = V[lo]; V[lo] = V[hi]; V[hi] = x; }
            }
            wave_sync();
        }
    for (int t = lane; t < len; t += 64) { rc[rs + t] = K[t]; rv[rs + t] = V[t]; }
}

// How long R's rows are, for the lanes per row of the restriction: over[i] = rows with more than 16 << i entries (what 8 << i lanes
// take in one trip of row_product, two entries in flight per lane), i = 0 .. 2.  Integer counts: any order gives the same result.
__global__ void __launch_bounds__(256) k_row_classes(int64_t n, const int32_t *__restrict__ rowptr, int32_t *__restrict__ over) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int32_t len = i < n ? rowptr[i + 1] - rowptr[i] : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(len > (16 << c)));
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&over[c], cnt);
    }
}
// the narrowest group that takes 95 % of the rows in one trip (the rest pay a further trip each); 64 lanes is a whole wave
int lanes_for_rows(int64_t rows, const int32_t *over) {
    for (int c = 0; c < 3; ++c)
        if (int64_t(over[c]) * 20 <= rows) return 8 << c;
    return 64;
}

// ---- dense inverse of the coarsest operator: in-place Gauss-Jordan in LDS, no pivoting (symmetric positive definite) --------
__global__ void __launch_bounds__(256) k_dense_inverse(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ val, double *__restrict__ inv, int32_t *flag) {
    __shared__ double a[kAmgDenseMax * kAmgDenseMax];
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n; e += 256) a[e] = 0.0;
    __syncthreads();
    for (int i = tid; i < n; i += 256)
        for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) a[i * n + col[p]] = val[p];
    __syncthreads();
    for (int p = 0; p < n; ++p) {
        const double piv = a[p * n + p];
        if (!(piv > 0.0)) { if (tid == 0) atomicOr(flag, 2); return; }   // uniform: every thread reads the same entry
        const double ip = 1.0 / piv;
        __syncthreads();
        for (int j = tid; j < n; j += 256)
            if (j != p) a[p * n + j] *= ip;
        __syncthreads();
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, j = e - i * n;
            if (i != p && j != p) a[e] -= a[i * n + p] * a[p * n + j];
        }
        __syncthreads();
        for (int i = tid; i < n; i += 256)
            a[i * n + p] = (i == p) ? ip : -a[i * n + p] * ip;
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += 256) inv[e] = a[e];
}

template <class S, class D> __global__ void __launch_bounds__(256) k_convert(int64_t n, const S *__restrict__ src, D *__restrict__ dst) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = D(src[i]);
}

// ---- the cycle -------------------------------------------------------------------------------------------------------------
// Row operations: 8 lanes per row split its entries, every lane carries all K columns, the transposing reduction
// (wave_util.h) leaves column `mycol` of the row sum in lanes with `mine`.  The same device functions serve the one-launch-
// per-operation kernels of the large levels and the single-workgroup kernel that walks all small levels (k_amg_tail).
constexpr int kLpr = 8;

template <class T, int K, bool SCALE, int LPR = kLpr, class TX = T>
__device__ __forceinline__ void row_product(int32_t rs, int32_t re, int sub, const int32_t *__restrict__ col, const T *__restrict__ val,
                                            const T *__restrict__ dinv, const TX *__restrict__ x, T (&acc)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = T(0);
    for (int32_t p0 = rs + sub; p0 < re; p0 += 2 * LPR) {   // two passes of loads in flight
        int32_t j[2];
        T a[2], xv[2][K];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int32_t p = p0 + u * LPR;
            j[u] = -1; a[u] = T(0);
            if (p < re) { j[u] = col[p]; a[u] = val[p]; }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int c = 0; c < K; ++c) xv[u][c] = T(0);
            if (j[u] >= 0) {
                if (SCALE) a[u] *= dinv[j[u]];
                const TX *xr = x + int64_t(j[u]) * K;
#pragma unroll
                for (int c = 0; c < K; ++c) xv[u][c] = T(xr[c]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = fma(a[u], xv[u][c], acc[c]);   // spelled out: a sum must not depend on what the compiler contracts at this K
    }
    TReduce<K, LPR>::run(acc, sub);
}

// The same row sum from the fixed-width image of level 0 (AmgLevelT::ell_*, k_vblock_ell): a lane's kEllWidth / kLpr entries sit at an
// address known from the row number, so columns, values and the bounds of the row's further entries go out together and the
// gathers follow at once - two dependent round trips instead of three.  The padding of a short row is (row, 0): a gather that hits.
// A lane takes entries sub, sub + kLpr, ... in this order, as row_product does.
struct EllRow {
    int32_t j[kEllWidth / kLpr];
    int32_t rs, re;
};
template <class T> __device__ __forceinline__ EllRow ell_request(const AmgLevelT<T> &a, int64_t row, int sub, T (&v)[kEllWidth / kLpr]) {
    EllRow e;
    const int64_t eb = row * kEllWidth + sub;
#pragma unroll
    for (int u = 0; u < kEllWidth / kLpr; ++u) { e.j[u] = a.ell_col[eb + u * kLpr]; v[u] = a.ell_val[eb + u * kLpr]; }
    e.rs = a.ell_tail[2 * row]; e.re = a.ell_tail[2 * row + 1];
    return e;
}
template <class T, int K, bool SCALE, class TX>
__device__ __forceinline__ void ell_gather(const AmgLevelT<T> &a, const EllRow &e, T (&v)[kEllWidth / kLpr], const TX *__restrict__ x,
                                           T (&xv)[kEllWidth / kLpr][K]) {
#pragma unroll
    for (int u = 0; u < kEllWidth / kLpr; ++u) {
        if (SCALE) v[u] *= a.dinv[e.j[u]];
        const TX *xr = x + int64_t(e.j[u]) * K;
#pragma unroll
        for (int c = 0; c < K; ++c) xv[u][c] = T(xr[c]);
    }
}
template <class T, int K, bool SCALE, class TX>
__device__ __forceinline__ void ell_sum(const AmgLevelT<T> &a, const EllRow &e, const T (&v)[kEllWidth / kLpr], const T (&xv)[kEllWidth / kLpr][K], int sub,
                                        const TX *__restrict__ x, T (&acc)[K]) {
#pragma unroll
    for (int c = 0; c < K; ++c) acc[c] = T(0);
#pragma unroll
    for (int u = 0; u < kEllWidth / kLpr; ++u)
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = fma(v[u], xv[u][c], acc[c]);
    for (int32_t p = e.rs + sub; p < e.re; p += kLpr) {   // a row longer than the image: the usual case is none
        const int32_t j = a.col[p];
        T av = a.val[p];
        if (SCALE) av *= a.dinv[j];
        const TX *xr = x + int64_t(j) * K;
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = fma(av, T(xr[c]), acc[c]);
    }
    TReduce<K, kLpr>::run(acc, sub);
}
template <class T, int K, bool SCALE, class TX>
__device__ __forceinline__ void row_product_ell(const AmgLevelT<T> &a, int64_t row, int sub, const TX *__restrict__ x, T (&acc)[K]) {
    T v[kEllWidth / kLpr], xv[kEllWidth / kLpr][K];
    const EllRow e = ell_request<T>(a, row, sub, v);
    ell_gather<T, K, SCALE, TX>(a, e, v, x, xv);
    ell_sum<T, K, SCALE, TX>(a, e, v, xv, sub, x, acc);
}

struct Lane {
    int sub, mycol;
    bool mine;
};
template <int K, int LPR = kLpr> __device__ __forceinline__ Lane lane_of(int tid) {
    int idx[K], own[K];
    Lane l;
    l.sub = tid % LPR;
    towner_init<K, LPR>(idx, own, l.sub);
    l.mycol = idx[0];
    l.mine = own[0] != 0;
    return l;
}

// first half on a level: z = w D^-1 r (from zero), t = r - A z
template <class T, int K, class TR = T> __device__ __forceinline__ void op_pre(const AmgLevelT<T> &a, const TR *__restrict__ r, int64_t row, const Lane &ln) {
    T acc[K];
    row_product<T, K, true, kLpr, TR>(a.rowptr[row], a.rowptr[row + 1], ln.sub, a.col, a.val, a.dinv, r, acc);
    if (ln.mine) {
        const int64_t at = row * K + ln.mycol;
        const T w = T(a.omega), ri = T(r[at]);
        a.z[at] = w * a.dinv[row] * ri;
        a.t[at] = fma(-w, acc[0], ri);
    }
}
// r_next = R t
template <class T, int K, int LPR = kLpr> __device__ __forceinline__ void op_restrict(const AmgLevelT<T> &a, T *__restrict__ rn, int64_t row, const Lane &ln) {
    T acc[K];
    row_product<T, K, false, LPR>(a.r_rowptr[row], a.r_rowptr[row + 1], ln.sub, a.r_col, a.r_val, (const T *)nullptr, (const T *)a.t, acc);
    if (ln.mine) rn[row * K + ln.mycol] = acc[0];
}
// z += P z_next
template <class T, int K> __device__ __forceinline__ void op_prolong(const AmgLevelT<T> &a, const T *__restrict__ zn, int64_t row, const Lane &ln) {
    T acc[K];
    row_product<T, K, false>(a.p_rowptr[row], a.p_rowptr[row + 1], ln.sub, a.p_col, a.p_val, (const T *)nullptr, zn, acc);
    if (ln.mine) a.z[row * K + ln.mycol] += acc[0];
}
// second half: zout = z + w D^-1 (r - A z); LAST (finest level): zout / dinv is stored, the return value is dot + r * zout
template <class T, int K, bool LAST, class TR = T, bool ELL = false>
__device__ __forceinline__ double op_post(const AmgLevelT<T> &a, const TR *__restrict__ r, TR *__restrict__ zout, int64_t row, const Lane &ln, double dot = 0.0) {
    T acc[K];
    if constexpr (ELL) row_product_ell<T, K, false, T>(a, row, ln.sub, (const T *)a.z, acc);
    else row_product<T, K, false>(a.rowptr[row], a.rowptr[row + 1], ln.sub, a.col, a.val, (const T *)nullptr, (const T *)a.z, acc);
    if (ln.mine) {
        const int64_t at = row * K + ln.mycol;
        const TR rr = r[at];
        const T ri = T(rr), di = a.dinv[row];
        const T zn = fma(T(a.omega) * di, ri - acc[0], a.z[at]);
        zout[at] = TR(LAST ? zn / di : zn);
        dot = fma(double(rr), double(zn), dot);
    }
    return dot;
}

constexpr int kRpb = 256 / kLpr;   // rows per workgroup of the one-operation kernels

template <class T, int K, class TR>
__global__ void __launch_bounds__(256) k_amg_pre(AmgLevelT<T> a, const TR *__restrict__ r, const double *scal, int step) {
    if (amg_done(scal, step)) return;
    const Lane ln = lane_of<K>(threadIdx.x);
    const int64_t row = int64_t(blockIdx.x) * kRpb + threadIdx.x / kLpr;
    if (row < a.n) op_pre<T, K, TR>(a, r, row, ln);
}
// LPR lanes per row of R (AmgLevelT::r_lanes): 256 / LPR rows per workgroup
template <class T, int K, int LPR>
__global__ void __launch_bounds__(256) k_amg_restrict(AmgLevelT<T> a, int64_t n_next, T *__restrict__ rn, const double *scal, int step) {
    if (amg_done(scal, step)) return;
    const Lane ln = lane_of<K, LPR>(threadIdx.x);
    const int64_t row = int64_t(blockIdx.x) * (256 / LPR) + threadIdx.x / LPR;
    if (row < n_next) op_restrict<T, K, LPR>(a, rn, row, ln);
}
template <class T, int K>
__global__ void __launch_bounds__(256) k_amg_prolong(AmgLevelT<T> a, const T *__restrict__ zn, const double *scal, int step) {
    if (amg_done(scal, step)) return;
    const Lane ln = lane_of<K>(threadIdx.x);
    const int64_t row = int64_t(blockIdx.x) * kRpb + threadIdx.x / kLpr;
    if (row < a.n) op_prolong<T, K>(a, zn, row, ln);
}
// <r, z> partials of a workgroup of NW waves, one per column, in a fixed order: the lanes of a wave, then the waves
template <int K, int NW> __device__ __forceinline__ void post_partials(const Lane &ln, double dot, double *__restrict__ part) {
    __shared__ double smem[NW * K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double x = wave_sum((ln.mine && k == ln.mycol) ? dot : 0.0);
        if (lane == 0) smem[wave * K + k] = x;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = 0.0;
        for (int w = 0; w < NW; ++w) t += smem[w * K + threadIdx.x];
        part[blockIdx.x * K + threadIdx.x] = t;
    }
}
// (prolongation folded into this sweep - P z_next formed on the fly for the row and its neighbours - was measured: 24.7 us
// against 5.3 + 12 at 80 k rows, the inner loops over P's rows are chains of dependent loads)
template <class T, int K, bool LAST, int THREADS, class TR, bool ELL = false>
__global__ void __launch_bounds__(THREADS) k_amg_post(AmgLevelT<T> a, const TR *__restrict__ r, TR *__restrict__ zout,
                                                     double *__restrict__ part, const double *scal, int step) {
    if (amg_done(scal, step)) return;
    const Lane ln = lane_of<K>(threadIdx.x);
    constexpr int RPB = THREADS / kLpr;
    double dot = 0.0;
    for (int64_t row = int64_t(blockIdx.x) * RPB + threadIdx.x / kLpr; row < a.n; row += int64_t(gridDim.x) * RPB)
        dot = op_post<T, K, LAST, TR, ELL>(a, r, zout, row, ln, dot);
    if (LAST) post_partials<K, THREADS / 64>(ln, dot, part);
}

// The finest level's second half sweep on the fixed-width image: the same `nblocks` partial rows, but 256 threads per workgroup (a
// 1024-thread workgroup needs 16 free wave slots on one CU at once, beside the resident operator workgroups of the other
// contexts).  A workgroup walks its 128 rows as four row groups.  With the image no address depends on a load, so the requests of all
// four groups go out before any is used, then all their gathers: the four groups cost one chain of round trips, not four.
constexpr int kPostGroups = 4, kPostRows = kPostGroups * kRpb;
template <class T, int K, class TR>
__global__ void __launch_bounds__(256) k_amg_post_image(AmgLevelT<T> a, const TR *__restrict__ r, TR *__restrict__ zout, double *__restrict__ part,
                                                        const double *scal, int step) {
    if (amg_done(scal, step)) return;
    constexpr int NE = kEllWidth / kLpr;
    const Lane ln = lane_of<K>(threadIdx.x);
    double dot = 0.0;
    for (int64_t row0 = int64_t(blockIdx.x) * kPostRows + threadIdx.x / kLpr; row0 < a.n; row0 += int64_t(gridDim.x) * kPostRows) {
        int64_t row[kPostGroups];
        EllRow e[kPostGroups];
        T v[kPostGroups][NE], xv[kPostGroups][NE][K], zi[kPostGroups], di[kPostGroups];
        TR rr[kPostGroups];
#pragma unroll
        for (int g = 0; g < kPostGroups; ++g) {   // a group beyond the last row repeats the first one's reads and stores nothing
            row[g] = row0 + g * kRpb < a.n ? row0 + g * kRpb : row0;
            e[g] = ell_request<T>(a, row[g], ln.sub, v[g]);
            rr[g] = TR(0); zi[g] = T(0); di[g] = T(1);
            if (ln.mine) {
                const int64_t at = row[g] * K + ln.mycol;
                rr[g] = r[at]; zi[g] = a.z[at]; di[g] = a.dinv[row[g]];
            }
        }
#pragma unroll
        for (int g = 0; g < kPostGroups; ++g) ell_gather<T, K, false, T>(a, e[g], v[g], (const T *)a.z, xv[g]);
#pragma unroll
        for (int g = 0; g < kPostGroups; ++g) {
            T acc[K];
            ell_sum<T, K, false, T>(a, e[g], v[g], xv[g], ln.sub, (const T *)a.z, acc);
            if (ln.mine && row0 + g * kRpb < a.n) {
                const T zn = fma(T(a.omega) * di[g], T(rr[g]) - acc[0], zi[g]);
                zout[row[g] * K + ln.mycol] = TR(zn / di[g]);
                dot = fma(double(rr[g]), double(zn), dot);
            }
        }
    }
    post_partials<K, 4>(ln, dot, part);
}

template <class T, int K>
__device__ __forceinline__ void op_dense(int n, const T *__restrict__ inv, const T *__restrict__ r, T *__restrict__ z, int t) {
    const int row = t / K, c = t - row * K;
    T acc = T(0);
    for (int j = 0; j < n; ++j) acc += inv[j * n + row] * r[j * K + c];   // the inverse is symmetric: column = row, coalesced
    z[t] = acc;
}

// all small levels in ONE workgroup: pre / restrict down to the dense coarsest solve, prolong / post back up; the barriers of
// the workgroup stand in for the kernel boundaries (every vector goes through the L2, one CU, one L1)
constexpr int kTailLevels = 3;
constexpr int kTailRows = 128;     // levels of at most this many rows go into the tail kernel (the coarsest one always)
template <class T> struct AmgTailT {
    int levels;
    AmgLevelT<T> up;               // the level above the tail: its R and t feed the first restriction (R's rows are long: 16 to 64 lanes per row)
    AmgLevelT<T> lev[kTailLevels];
    const T *inv;
};
template <class T, int K, int LPR0>   // LPR0: lanes per row of the first restriction (the r_lanes of the level above the tail, 16 at least)
__global__ void __launch_bounds__(1024) k_amg_tail(AmgTailT<T> A, const double *scal, int step) {
    if (amg_done(scal, step)) return;
    const Lane ln = lane_of<K>(threadIdx.x);
    const int g = threadIdx.x / kLpr, ng = 1024 / kLpr;
    const int L = A.levels;
    {
        const Lane l0 = lane_of<K, LPR0>(threadIdx.x);
        for (int64_t row = threadIdx.x / LPR0; row < A.lev[0].n; row += 1024 / LPR0) op_restrict<T, K, LPR0>(A.up, A.lev[0].r, row, l0);
        __syncthreads();
    }
    for (int l = 0; l + 1 < L; ++l) {
        const AmgLevelT<T> &a = A.lev[l];
        for (int64_t row = g; row < a.n; row += ng) op_pre<T, K>(a, (const T *)a.r, row, ln);
        __syncthreads();
        const AmgLevelT<T> &b = A.lev[l + 1];
        for (int64_t row = g; row < b.n; row += ng) op_restrict<T, K>(a, b.r, row, ln);
        __syncthreads();
    }
    {
        const AmgLevelT<T> &c = A.lev[L - 1];
        for (int t = threadIdx.x; t < int(c.n) * K; t += 1024) op_dense<T, K>(int(c.n), A.inv, (const T *)c.r, c.z2, t);
        __syncthreads();
    }
    for (int l = L - 2; l >= 0; --l) {
        const AmgLevelT<T> &a = A.lev[l];
        const AmgLevelT<T> &b = A.lev[l + 1];
        for (int64_t row = g; row < a.n; row += ng) op_prolong<T, K>(a, (const T *)b.z2, row, ln);
        __syncthreads();
        for (int64_t row = g; row < a.n; row += ng) (void)op_post<T, K, false>(a, (const T *)a.r, a.z2, row, ln);
        __syncthreads();
    }
}

int grid_rows(int64_t n, int per_block) { return int((n + per_block - 1) / per_block); }

template <class T> bool level_image(const AmgLevelT<T> &a) { return a.ell_col && a.ell_tail && a.ell_val; }
// fn(int_c<LPR>): a kernel's lanes per row from the level's choice
template <int MIN = 8, class F> void for_lanes(int lanes, F &&fn) {
    if (lanes >= 64) fn(int_c<64>{});
    else if (lanes >= 32) fn(int_c<32>{});
    else if (lanes >= 16 || MIN >= 16) fn(int_c<16>{});
    else if constexpr (MIN < 16) fn(int_c<8>{});
}
#ifdef REMO_PROBES
template <class T> int restrict_lanes(const AmgLevelT<T> &a) { return g_tune.amg_r_lanes ? g_tune.amg_r_lanes : a.r_lanes; }
bool post_wide() { return g_tune.amg_post_wide != 0; }
#else
template <class T> int restrict_lanes(const AmgLevelT<T> &a) { return a.r_lanes; }
constexpr bool post_wide() { return false; }
#endif

// out[0 .. n] = exclusive prefix sums of cnt[0 .. n) (out[n] = total; cnt[n] must be addressable, its value does not matter);
// the temporary storage comes from the scratch end of the arena and is released by the caller's mark
void scan_counts(Arena &ar, hipStream_t s, int64_t n, const int32_t *cnt, int32_t *out) {
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, cnt, out, int32_t(0), size_t(n + 1), rocprim::plus<int32_t>(), s));
    void *tmp = ar.hi<char>(tb + 256);
    HIP_TRY(rocprim::exclusive_scan(tmp, tb, cnt, out, int32_t(0), size_t(n + 1), rocprim::plus<int32_t>(), s));
}

// one product C = X Y into arena memory: count, scan, (sync: size), fill.  Returns nnz(C); -1 when a row overflowed.
struct Csr {
    int64_t n = 0, nnz = 0;
    int32_t *rowptr = nullptr, *col = nullptr;
    double *val = nullptr;
};

// Products without a read-back.  The result arrays are allocated by an upper bound (`cap` entries), the row pointers come
// from the count pass and a scan on the device and are clamped to the capacity; overflowing hash tables (bit 1) or arrays
// (bit 2) raise the product's own flag slot, which the host reads at the NEXT point where it has to wait anyway.
// variant 1: a wave per row with 128 hash slots, 2: with 512; remembered per kind of matrix, level and product (process-wide;
// the meshes of a sweep look alike).  (Variant 0 was one LANE per row with a private sorted list of at most 32 columns for the
// short rows of S P0 and A P: 230 us per launch against 70 - private arrays with dynamic indices live in scratch memory; removed.)
template <int PASS>
void launch_product(int variant, hipStream_t s, const Csr &X, const Csr &Y, int32_t *cnt, const int32_t *crp, int32_t *cc, double *cv, int32_t *d_over) {
    if (variant <= 1)
        hipLaunchKernelGGL((k_spgemm<PASS, 128>), dim3(grid_rows(X.n, 4)), dim3(256), 0, s, X.n, X.rowptr, X.col, X.val, Y.rowptr, Y.col, Y.val, cnt, crp, cc, cv, d_over);
    else
        hipLaunchKernelGGL((k_spgemm<PASS, 512>), dim3(grid_rows(X.n, 4)), dim3(256), 0, s, X.n, X.rowptr, X.col, X.val, Y.rowptr, Y.col, Y.val, cnt, crp, cc, cv, d_over);
}

void spgemm_async(Arena &ar, bool permanent, hipStream_t s, const Csr &X, const Csr &Y, int64_t cap, int variant, int32_t *d_over, Csr &C) {
    if (cap > INT_MAX - 8) cap = INT_MAX - 8;
    C.n = X.n;
    C.nnz = cap;   // upper bound; the exact count is rowptr[n] on the device
    C.rowptr = permanent ? ar.lo<int32_t>(size_t(X.n) + 2) : ar.hi<int32_t>(size_t(X.n) + 2);
    int32_t *cnt = ar.hi<int32_t>(size_t(X.n) + 2);   // scratch of the level
    launch_product<0>(variant, s, X, Y, cnt, nullptr, nullptr, nullptr, d_over);
    scan_counts(ar, s, X.n, cnt, C.rowptr);
    hipLaunchKernelGGL(k_clamp_rowptr, dim3(grid_rows(X.n + 1, 256)), dim3(256), 0, s, X.n, C.rowptr, int32_t(cap), d_over);
    C.col = permanent ? ar.lo<int32_t>(size_t(cap) + 2) : ar.hi<int32_t>(size_t(cap) + 2);
    C.val = permanent ? ar.lo<double>(size_t(cap) + 2) : ar.hi<double>(size_t(cap) + 2);
    launch_product<1>(variant, s, X, Y, nullptr, C.rowptr, C.col, C.val, d_over);
}

std::atomic<int> g_product_hint[2][kAmgMaxLevels][3];   // [2D | 3D matrices][level][S P0, A P, R (A P)]; 0 / 1: 128 slots, 2: 512
std::atomic<int> g_ap_room[2];                          // log2 of the extra room of A P beyond 4 nnz(A) (0 .. 3)
constexpr int kFlagSlots = 64;                          // [0] setup flags, [8 + 3 level + product] product flags, [32 + 4 level + class] row classes of R
constexpr int kClassSlot = 32;
static_assert(8 + 3 * kAmgMaxLevels <= kClassSlot && kClassSlot + 4 * kAmgMaxLevels <= kFlagSlots, "flag slots overlap");

// REMO_AMG_DEBUG: per level the row lengths of A, P and R (minimum, median, 95 %, maximum) and the lanes chosen for R - a read-back
void print_row_lengths(hipStream_t s, const AmgT<double> &H) {
    auto stats = [&](const char *name, int l, const int32_t *d_rowptr, int64_t n) {
        if (!d_rowptr || n <= 0) return;
        std::vector<int32_t> rp(size_t(n) + 1);
        HIP_TRY(hipMemcpyAsync(rp.data(), d_rowptr, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<int32_t> len(static_cast<size_t>(n));
        for (int64_t i = 0; i < n; ++i) len[size_t(i)] = rp[size_t(i) + 1] - rp[size_t(i)];
        std::sort(len.begin(), len.end());
        fprintf(stderr, "amg level %d %s: %lld rows, entries per row min %d median %d 95 %% %d max %d\n", l, name, (long long)n, len.front(),
                len[size_t(n / 2)], len[size_t((n * 95) / 100)], len.back());
    };
    for (int l = 0; l < H.levels; ++l) {
        const AmgLevelT<double> &a = H.lev[l];
        stats("A", l, a.rowptr, a.n);
        if (l + 1 < H.levels) {
            stats("P", l, a.p_rowptr, a.n);
            stats("R", l, a.r_rowptr, H.lev[l + 1].n);
            fprintf(stderr, "amg level %d R: %d lanes per row\n", l, a.r_lanes);
        }
    }
}

// one attempt: 0 = built, 1 = a product outgrew its tables or arrays (the hints have been raised: try again), -1 = failed
int amg_build(Arena &ar, hipStream_t s, int hs, int64_t nv, const int32_t *rowptr, const int32_t *col, const double *val, int kmax, AmgT<double> &H,
              std::string &why) {
    H = AmgT<double>{};
    int32_t *d_flag = ar.lo<int32_t>(kFlagSlots);
    unsigned long long *d_bound = ar.lo<unsigned long long>(kAmgMaxLevels + 1);
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t) * kFlagSlots, s));
    HIP_TRY(hipMemsetAsync(d_bound, 0, sizeof(unsigned long long) * (kAmgMaxLevels + 1), s));
    int32_t h_flags[kFlagSlots] = {};
    int32_t h_nnz_a[kAmgMaxLevels] = {}, h_nnz_p[kAmgMaxLevels] = {};
    const int32_t *d_nnz_p[kAmgMaxLevels] = {};   // where the exact entry counts of the prolongators live on the device
    // looks at the flags read back so far; products of the levels below `upto`
    auto check = [&](int upto) -> int {
        int again = 0;   // the products first: a cut-off product leaves rows without a diagonal behind, which is then flagged as well
        for (int l = 0; l < upto; ++l)
            for (int p = 0; p < 3; ++p) {
                const int f = h_flags[8 + 3 * l + p];
                if (f == 0) continue;
                if (f & 1) {   // hash tables
                    if (g_product_hint[hs][l][p].load() >= 2) { why = "a product row with more than 256 distinct columns"; return -1; }
                    g_product_hint[hs][l][p].store(2);
                    again = 1;
                }
                if (f & 2) {   // arrays
                    if (p != 1 || g_ap_room[hs].load() >= 3) { why = "a product outgrew its arrays"; return -1; }
                    g_ap_room[hs].fetch_add(1);
                    again = 1;
                }
            }
        if (again) return 1;
        if (h_flags[0] != 0) {
            why = "setup raised flag " + std::to_string(h_flags[0]) + " (1 diagonal, 2 dense pivot, 4 a row of R beyond the LDS sort)";
            return -1;
        }
        return 0;
    };
    // level 0: compact copy of the leading block
    Csr A;
    A.n = nv;
    A.rowptr = ar.lo<int32_t>(size_t(nv) + 2);
    {
        const size_t mark = ar.hi_mark();
        int32_t *cnt = ar.hi<int32_t>(size_t(nv) + 2);
        hipLaunchKernelGGL((k_block_copy<0>), dim3(grid_rows(nv, 256)), dim3(256), 0, s, nv, rowptr, col, val, cnt, (const int32_t *)nullptr,
                           (int32_t *)nullptr, (double *)nullptr);
        scan_counts(ar, s, nv, cnt, A.rowptr);
        int32_t h = 0;
        HIP_TRY(hipMemcpyAsync(&h, A.rowptr + nv, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ar.hi_release(mark);
        if (h <= 0 || h == INT_MAX) { why = "empty vertex block"; return -1; }
        A.nnz = h;
        h_nnz_a[0] = h;
        A.col = ar.lo<int32_t>(size_t(h) + 2);
        A.val = ar.lo<double>(size_t(h) + 2);
        hipLaunchKernelGGL((k_block_copy<1>), dim3(grid_rows(nv, 256)), dim3(256), 0, s, nv, rowptr, col, val, (int32_t *)nullptr,
                           (const int32_t *)A.rowptr, A.col, A.val);
    }
    int L = 0;
    for (;;) {
        AmgLevelT<double> &lv = H.lev[L];
        const int64_t n = A.n;
        lv.n = n; lv.rowptr = A.rowptr; lv.col = A.col; lv.val = A.val;
        double *dinv = ar.lo<double>(size_t(n) + 2);
        lv.dinv = dinv;
        lv.z = ar.lo<double>(size_t(n) * kmax + 2);
        lv.z2 = ar.lo<double>(size_t(n) * kmax + 2);
        lv.t = ar.lo<double>(size_t(n) * kmax + 2);
        if (L > 0) lv.r = ar.lo<double>(size_t(n) * kmax + 2);
        const int g = grid_rows(n, 256);
        hipLaunchKernelGGL(k_level_diag, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, A.val, dinv, d_bound + L, d_flag);
        if (n <= kAmgDenseMax) {   // coarsest: dense inverse
            double *inv = ar.lo<double>(size_t(n) * n + 2);
            hipLaunchKernelGGL(k_dense_inverse, dim3(1), dim3(256), 0, s, int(n), A.rowptr, A.col, A.val, inv, d_flag);
            H.inv = inv;
            H.levels = L + 1;
            break;
        }
        if (L + 1 >= kAmgMaxLevels) { why = "too many levels"; return -1; }
        // ---- aggregation ----
        const size_t mark = ar.hi_mark();   // the scratch of a level is reused by the next one: the stream orders the kernels
        uint64_t *tup = ar.hi<uint64_t>(size_t(n) + 2), *m1 = ar.hi<uint64_t>(size_t(n) + 2);
        int32_t *isroot = ar.hi<int32_t>(size_t(n) + 2), *id = ar.hi<int32_t>(size_t(n) + 2);
        int32_t *agg1 = ar.hi<int32_t>(size_t(n) + 2), *agg = ar.hi<int32_t>(size_t(n) + 2);
        hipLaunchKernelGGL(k_mis_init, dim3(g), dim3(256), 0, s, n, tup);
        for (int it = 0; it < 10; ++it) {   // a fixed number of iterations, no read-back (460 of 80 k nodes are open after six, none after twelve); k_mis_finish settles stragglers
            hipLaunchKernelGGL(k_mis_max, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, tup, m1);
            hipLaunchKernelGGL(k_mis_update, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, tup, m1);
        }
        hipLaunchKernelGGL(k_mis_finish, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, tup, m1);
        hipLaunchKernelGGL(k_mis_flags, dim3(g), dim3(256), 0, s, n, m1, isroot);
        scan_counts(ar, s, n, isroot, id);
        hipLaunchKernelGGL(k_agg_near, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, m1, id, agg1);
        hipLaunchKernelGGL(k_agg_far, dim3(g), dim3(256), 0, s, n, A.rowptr, A.col, A.val, agg1, agg);
        // ---- the level's ONE wait: number of aggregates, spectrum bound, everything flagged so far, exact size of this level's matrix
        int32_t h_nc = 0;
        unsigned long long h_bound = 0;
        HIP_TRY(hipMemcpyAsync(&h_nc, id + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&h_bound, d_bound + L, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h_flags, d_flag, sizeof(int32_t) * kFlagSlots, hipMemcpyDeviceToHost, s));
        if (L > 0) HIP_TRY(hipMemcpyAsync(&h_nnz_a[L], A.rowptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const int verdict = check(L);
        if (verdict != 0) return verdict;
        double lmax;
        std::memcpy(&lmax, &h_bound, sizeof lmax);
        const int64_t nnz_a = h_nnz_a[L];
        if (getenv("REMO_AMG_DEBUG")) fprintf(stderr, "amg level %d: n %lld nnz %lld -> %d aggregates, lmax %.3f\n", L, (long long)n, (long long)nnz_a, h_nc, lmax);
        if (!(lmax > 0.0) || !std::isfinite(lmax) || nnz_a <= 0) { why = "level operator without a spectrum bound"; return -1; }
        lv.omega = 1.6 / lmax;
        lv.nnz = nnz_a;
        const int64_t nc = h_nc;
        if (nc <= 0 || nc * 10 > n * 8) { why = "no coarsening"; return -1; }
        // ---- P = (I - 4/(3 lmax) D^-1 A) P0: at most as many entries as A ----
        Csr S = A, P0;
        S.val = ar.hi<double>(size_t(nnz_a) + 2);
        P0.n = n; P0.nnz = n;
        P0.rowptr = ar.hi<int32_t>(size_t(n) + 2); P0.col = ar.hi<int32_t>(size_t(n) + 2); P0.val = ar.hi<double>(size_t(n) + 2);
        hipLaunchKernelGGL(k_smoothing_factor, dim3(grid_rows(n + 1, 256)), dim3(256), 0, s, n, A.rowptr, A.col, A.val, dinv, d_bound + L, S.val,
                           agg, P0.rowptr, P0.col, P0.val);
        int32_t *pf = d_flag + 8 + 3 * L;
        Csr P;
        spgemm_async(ar, true, s, S, P0, nnz_a, g_product_hint[hs][L][0].load(), pf + 0, P);
        lv.p_rowptr = P.rowptr; lv.p_col = P.col; lv.p_val = P.val;
        d_nnz_p[L] = P.rowptr + n;
        // ---- R = P^T: count the entries of every column, scan, scatter (any order), sort every row of R by its column = row of P ----
        Csr R;
        R.n = nc; R.nnz = nnz_a;
        R.rowptr = ar.lo<int32_t>(size_t(nc) + 2); R.col = ar.lo<int32_t>(size_t(nnz_a) + 2); R.val = ar.lo<double>(size_t(nnz_a) + 2);
        {
            int32_t *tcnt = ar.hi<int32_t>(size_t(nc) + 2), *cursor = ar.hi<int32_t>(size_t(nc) + 2);
            HIP_TRY(hipMemsetAsync(tcnt, 0, sizeof(int32_t) * (size_t(nc) + 2), s));
            HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(int32_t) * (size_t(nc) + 2), s));
            hipLaunchKernelGGL(k_tr_count, dim3(g), dim3(256), 0, s, n, P.rowptr, P.col, tcnt);
            scan_counts(ar, s, nc, tcnt, R.rowptr);
            hipLaunchKernelGGL(k_tr_fill, dim3(g), dim3(256), 0, s, n, P.rowptr, P.col, P.val, R.rowptr, cursor, R.col, R.val);
            hipLaunchKernelGGL((k_tr_sort<0, kTrMax, 4>), dim3(grid_rows(nc, 4)), dim3(256), 0, s, nc, R.rowptr, R.col, R.val, d_flag);
            hipLaunchKernelGGL((k_tr_sort<kTrMax, kTrMaxLong, 1>), dim3(grid_rows(nc, 1)), dim3(64), 0, s, nc, R.rowptr, R.col, R.val, d_flag);
            hipLaunchKernelGGL(k_row_classes, dim3(grid_rows(nc, 256)), dim3(256), 0, s, nc, R.rowptr, d_flag + kClassSlot + 4 * L);
        }
        lv.r_rowptr = R.rowptr; lv.r_col = R.col; lv.r_val = R.val;
        // ---- A' = R (A P): A P in scratch with room for (4 << room) nnz(A) entries, A' at most as many entries as A ----
        Csr AP, Ac;
        spgemm_async(ar, false, s, A, P, (nnz_a * 4) << g_ap_room[hs].load(), g_product_hint[hs][L][1].load(), pf + 1, AP);
        spgemm_async(ar, true, s, R, AP, nnz_a, g_product_hint[hs][L][2].load(), pf + 2, Ac);
        ar.hi_release(mark);
        A = Ac;
        A.n = nc;
        ++L;
    }
    // ---- the last wait: flags of the last level's products and of the dense inverse, exact sizes for the fp32 image ----
    HIP_TRY(hipMemcpyAsync(h_flags, d_flag, sizeof(int32_t) * kFlagSlots, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h_nnz_a[L], A.rowptr + A.n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    for (int l = 0; l < L; ++l) HIP_TRY(hipMemcpyAsync(&h_nnz_p[l], d_nnz_p[l], sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int verdict = check(L);
    if (verdict != 0) return verdict;
    H.lev[L].nnz = h_nnz_a[L];
    for (int l = 0; l < L; ++l) {
        H.lev[l].nnz_p = h_nnz_p[l];
        H.lev[l].r_lanes = lanes_for_rows(H.lev[l + 1].n, h_flags + kClassSlot + 4 * l);
    }
    if (getenv("REMO_AMG_DEBUG")) print_row_lengths(s, H);
    H.launches = 4 * (H.levels - 1);   // pre, restrict, prolong, post per level; the tail kernel stands for the last restriction + dense solve
    H.kmax = kmax;
    return 0;
}

}  // namespace

bool amg_setup(Arena &ar, hipStream_t s, int dim, int64_t nv, const int32_t *rowptr, const int32_t *col, const double *val, int kmax, AmgT<double> &H,
               std::string &why) {
    H = AmgT<double>{};
    if (nv <= kAmgDenseMax) { why = "vertex block too small"; return false; }
    const int hs = dim == 3 ? 1 : 0;   // what earlier batches taught about the products: per kind of matrix
    const size_t hi0 = ar.hi_mark(), lo0 = ar.lo_off;
    try {
        for (int attempt = 0; attempt < 6; ++attempt) {
            ar.hi_release(hi0);
            ar.lo_off = lo0;               // a repeated attempt reuses the memory of the failed one (the stream orders the kernels)
            const int rc = amg_build(ar, s, hs, nv, rowptr, col, val, kmax, H, why);
            ar.hi_release(hi0);
            if (rc == 0) return true;
            if (rc < 0) break;
        }
        if (why.empty()) why = "the products did not fit after several attempts";
        H = AmgT<double>{};
        ar.lo_off = lo0;                   // the fallback (polynomial) sees the arena as it was before the hierarchy was attempted
        return false;
    } catch (const std::exception &ex) {
        ar.hi_release(hi0);
        ar.lo_off = lo0;
        H = AmgT<double>{};
        why = ex.what();
        return false;
    }
}

void amg_debug_product(hipStream_t s, int slots, int64_t cap, int64_t nx, const int32_t *xrp, const int32_t *xc, const double *xv, int64_t ny,
                       const int32_t *yrp, const int32_t *yc, const double *yv, int32_t *crp, int32_t *cc, double *cv, int32_t *flags) {
    if (slots != 128 && slots != 512) throw std::runtime_error("amg_debug_product: 128 or 512 slots");
    if (nx < 1 || ny < 1 || nx > (1 << 24) || ny > (1 << 24) || cap < 1 || cap > (1 << 28)) throw std::runtime_error("amg_debug_product: sizes out of range");
    // the kernels trust their inputs: row pointers that ascend from 0, columns of X that name rows of Y
    auto ascending = [](const int32_t *rp, int64_t n) {
        if (rp[0] != 0) return false;
        for (int64_t i = 0; i < n; ++i)
            if (rp[i + 1] < rp[i]) return false;
        return rp[n] <= (1 << 28);
    };
    if (!ascending(xrp, nx) || !ascending(yrp, ny)) throw std::runtime_error("amg_debug_product: row pointers must ascend from 0");
    const size_t nnzx = size_t(xrp[nx]), nnzy = size_t(yrp[ny]);
    for (size_t p = 0; p < nnzx; ++p)
        if (xc[p] < 0 || xc[p] >= ny) throw std::runtime_error("amg_debug_product: a column of X names no row of Y");
    for (size_t q = 0; q < nnzy; ++q)
        if (yc[q] < 0 || yc[q] == INT_MAX) throw std::runtime_error("amg_debug_product: a column of Y out of range");
    const size_t ints = 2 * (size_t(nx) + size_t(ny) + 4) + nnzx + nnzy + 2 * size_t(nx) + size_t(cap) + 16 + kFlagSlots;
    const size_t bytes = 4 * ints + 8 * (nnzx + nnzy + size_t(cap) + 8) + 16 * size_t(nx) + (size_t(1) << 20);   // + the scan's storage, + 256 per array
    DeviceTemp tmp;
    Arena ar;
    ar.base = tmp.alloc<char>(bytes);
    ar.cap = bytes;
    HIP_TRY(hipMemsetAsync(ar.base, 0xFF, bytes, s));   // what the product does not write stays 0xFF
    Csr X, Y, C;
    auto put = [&](Csr &M, int64_t n, size_t nnz, const int32_t *rp, const int32_t *c, const double *v) {
        M.n = n; M.nnz = int64_t(nnz);
        M.rowptr = ar.lo<int32_t>(size_t(n) + 2); M.col = ar.lo<int32_t>(nnz + 2); M.val = ar.lo<double>(nnz + 2);
        HIP_TRY(hipMemcpyAsync(M.rowptr, rp, sizeof(int32_t) * (size_t(n) + 1), hipMemcpyHostToDevice, s));
        if (nnz) {
            HIP_TRY(hipMemcpyAsync(M.col, c, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(M.val, v, sizeof(double) * nnz, hipMemcpyHostToDevice, s));
        }
    };
    put(X, nx, nnzx, xrp, xc, xv);
    put(Y, ny, nnzy, yrp, yc, yv);
    int32_t *d_flag = ar.lo<int32_t>(kFlagSlots);
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t) * kFlagSlots, s));
    spgemm_async(ar, true, s, X, Y, cap, slots == 128 ? 1 : 2, d_flag, C);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(crp, C.rowptr, sizeof(int32_t) * (size_t(nx) + 1), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cc, C.col, sizeof(int32_t) * (size_t(cap) + 2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cv, C.val, sizeof(double) * (size_t(cap) + 2), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(flags, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

namespace {
template <class T>
void debug_row_ops(hipStream_t s, int op, int lanes, bool ell, int64_t n, int64_t nx, int k, const int32_t *rowptr, const int32_t *col, const double *val,
                   const double *dinv, double omega, const double *x, const double *r, int nblocks, int guard, void *out, void *out2) {
    const size_t nnz = size_t(rowptr[n]), nk = size_t(n) * k, nxk = size_t(nx) * k, cells = size_t(n) * kEllWidth + 8;
    const size_t bytes = 4 * (size_t(n) + 2 + nnz + 2 + cells + 2 * size_t(n) + 8) + 8 * (2 * nnz + 4 + size_t(n) + nxk + 4 * nk + 2 * cells) +
                         8 * (size_t(nblocks) * k + 3 * size_t(guard)) + 256 * 32;
    DeviceTemp tmp;
    Arena ar;
    ar.base = tmp.alloc<char>(bytes);
    ar.cap = bytes;
    HIP_TRY(hipMemsetAsync(ar.base, 0xFF, bytes, s));   // what the operation does not write stays 0xFF
    std::vector<std::vector<char>> keep;                // the converted host arrays live until the synchronisation below
    auto put = [&](auto tag, const double *src, size_t count) {   // a device array of `count` elements of the tag's type from host doubles
        using D = decltype(tag);
        D *d = ar.lo<D>(count + 2);
        keep.emplace_back(sizeof(D) * (count + 1));
        D *h = reinterpret_cast<D *>(keep.back().data());
        for (size_t i = 0; i < count; ++i) h[i] = D(src[i]);
        if (count) HIP_TRY(hipMemcpyAsync(d, h, sizeof(D) * count, hipMemcpyHostToDevice, s));
        return d;
    };
    int32_t *d_rp = ar.lo<int32_t>(size_t(n) + 2), *d_col = ar.lo<int32_t>(nnz + 2);
    HIP_TRY(hipMemcpyAsync(d_rp, rowptr, sizeof(int32_t) * (size_t(n) + 1), hipMemcpyHostToDevice, s));
    if (nnz) HIP_TRY(hipMemcpyAsync(d_col, col, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, s));
    AmgLevelT<T> a;
    a.n = n; a.nnz = int64_t(nnz); a.omega = omega;
    const T *d_val = put(T(0), val, nnz);
    a.rowptr = d_rp; a.col = d_col; a.val = d_val;
    if (op != 0) a.dinv = put(T(0), dinv, size_t(n));
    if (ell) {
        const double *d_val64 = put(double(0), val, nnz);
        int32_t *ecol = ar.lo<int32_t>(cells), *tail = ar.lo<int32_t>(size_t(n) * 2 + 8);
        T *ev = ar.lo<T>(cells);
        double *e64 = nullptr;
        float *e32 = nullptr;
        if constexpr (sizeof(T) == 8) e64 = ev; else e32 = ev;
        launch_vblock_ell(n, d_rp, d_col, d_val64, ecol, tail, e64, e32, s);
        a.ell_col = ecol; a.ell_tail = tail; a.ell_val = ev;
    }
    // the result arrays last, each with its guard behind it
    auto result = [&](auto tag, size_t count) { return ar.lo<decltype(tag)>(count + size_t(guard)); };
    auto fetch = [&](void *dst, const void *src, size_t elem, size_t count) {
        HIP_TRY(hipMemcpyAsync(dst, src, elem * (count + size_t(guard)), hipMemcpyDeviceToHost, s));
    };
    const double *scal = nullptr;
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (op == 0) {
            a.r_rowptr = d_rp; a.r_col = d_col; a.r_val = d_val;
            a.t = put(T(0), x, nxk);
            T *rn = result(T(0), nk);
            for_lanes(lanes, [&](auto lc) {
                constexpr int LPR = decltype(lc)::value;
                launch256(k_amg_restrict<T, K, LPR>, grid_rows(n, 256 / LPR), s, a, n, rn, scal, 0);
            });
            fetch(out, rn, sizeof(T), nk);
        } else if (op == 1) {
            const double *d_r = put(double(0), x, nk);
            a.z = result(T(0), nk); a.t = result(T(0), nk);
            launch256(k_amg_pre<T, K, double>, grid_rows(n, kRpb), s, a, d_r, scal, 0);
            fetch(out, a.z, sizeof(T), nk);
            fetch(out2, a.t, sizeof(T), nk);
        } else if (op == 2) {
            a.z = put(T(0), x, nk);
            const T *d_r = put(T(0), r, nk);
            T *zout = result(T(0), nk);
            launch256(k_amg_post<T, K, false, 256, T>, grid_rows(n, kRpb), s, a, d_r, zout, (double *)nullptr, scal, 0);
            fetch(out, zout, sizeof(T), nk);
        } else {
            a.z = put(T(0), x, nk);
            const double *d_r = put(double(0), r, nk);
            double *zout = result(double(0), nk), *part = result(double(0), size_t(nblocks) * k);
            if (ell) launch256(k_amg_post_image<T, K, double>, nblocks, s, a, d_r, zout, part, scal, 0);
            else hipLaunchKernelGGL((k_amg_post<T, K, true, 1024, double>), dim3(nblocks), dim3(1024), 0, s, a, d_r, zout, part, scal, 0);
            fetch(out, zout, sizeof(double), nk);
            fetch(out2, part, sizeof(double), size_t(nblocks) * k);
        }
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
}
}  // namespace

void amg_debug_row_ops(hipStream_t s, int op, int lanes, bool ell, bool fp32, int64_t n, int64_t nx, int k, const int32_t *rowptr, const int32_t *col,
                       const double *val, const double *dinv, double omega, const double *x, const double *r, int nblocks, int guard, void *out, void *out2) {
    if (op < 0 || op > 3) throw std::runtime_error("amg_debug_row_ops: op 0 .. 3");
    if (lanes != 8 && lanes != 16 && lanes != 32 && lanes != 64) throw std::runtime_error("amg_debug_row_ops: 8, 16, 32 or 64 lanes");
    if (op != 0 && lanes != 8) throw std::runtime_error("amg_debug_row_ops: the sweeps take 8 lanes per row");
    if (ell && op != 3) throw std::runtime_error("amg_debug_row_ops: only the finest level's second half sweep (op 3) reads the fixed-width image");
    if (n < 1 || nx < 1 || n > (1 << 22) || nx > (1 << 22) || k < 1 || k > 8 || guard < 0 || guard > 4096) throw std::runtime_error("amg_debug_row_ops: sizes out of range");
    if (op != 0 && nx != n) throw std::runtime_error("amg_debug_row_ops: a sweep needs a square matrix");
    if (op == 3 && (nblocks < 1 || nblocks > kMaxPartialBlocks / 2)) throw std::runtime_error("amg_debug_row_ops: workgroups out of range");
    if (op != 3) nblocks = 0;
    if (!x || (op != 0 && !dinv) || (op >= 2 && !r) || (op == 1 || op == 3 ? !out2 : false)) throw std::runtime_error("amg_debug_row_ops: an array is missing");
    // the kernels trust their inputs: row pointers that ascend from 0, columns that name rows of x
    if (rowptr[0] != 0) throw std::runtime_error("amg_debug_row_ops: row pointers must ascend from 0");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i] || rowptr[i + 1] > (1 << 26)) throw std::runtime_error("amg_debug_row_ops: row pointers must ascend from 0");
    for (int32_t p = 0; p < rowptr[n]; ++p)
        if (col[p] < 0 || col[p] >= nx) throw std::runtime_error("amg_debug_row_ops: a column names no row of x");
    if (fp32) debug_row_ops<float>(s, op, lanes, ell, n, nx, k, rowptr, col, val, dinv, omega, x, r, nblocks, guard, out, out2);
    else debug_row_ops<double>(s, op, lanes, ell, n, nx, k, rowptr, col, val, dinv, omega, x, r, nblocks, guard, out, out2);
}

void amg_to_float(Arena &ar, hipStream_t s, const AmgT<double> &in, int kmax, AmgT<float> &out) {
    auto conv = [&](const double *src, size_t count) {
        float *dst = ar.lo<float>(count + 4);
        hipLaunchKernelGGL((k_convert<double, float>), dim3(grid_rows(int64_t(count), 256)), dim3(256), 0, s, int64_t(count), src, dst);
        return (const float *)dst;
    };
    out = AmgT<float>{};
    out.levels = in.levels;
    out.launches = in.launches;
    out.kmax = kmax;
    for (int l = 0; l < in.levels; ++l) {
        const AmgLevelT<double> &a = in.lev[l];
        AmgLevelT<float> &b = out.lev[l];
        b.n = a.n; b.nnz = a.nnz; b.rowptr = a.rowptr; b.col = a.col; b.omega = a.omega;
        b.val = conv(a.val, size_t(a.nnz));
        b.dinv = conv(a.dinv, size_t(a.n));
        b.z = ar.lo<float>(size_t(a.n) * kmax + 4); b.z2 = ar.lo<float>(size_t(a.n) * kmax + 4); b.t = ar.lo<float>(size_t(a.n) * kmax + 4);
        if (l > 0) b.r = ar.lo<float>(size_t(a.n) * kmax + 4);
        if (l + 1 < in.levels) {
            b.p_rowptr = a.p_rowptr; b.p_col = a.p_col; b.r_rowptr = a.r_rowptr; b.r_col = a.r_col;
            b.nnz_p = a.nnz_p; b.r_lanes = a.r_lanes;
            b.p_val = conv(a.p_val, size_t(a.nnz_p));
            b.r_val = conv(a.r_val, size_t(a.nnz_p));
        }
    }
    const int64_t nc = in.lev[in.levels - 1].n;
    out.inv = conv(in.inv, size_t(nc * nc));
}

void amg_level0_image(Arena &ar, hipStream_t s, AmgT<double> &h64, bool want64, AmgT<float> *h32) {
    AmgLevelT<double> &a = h64.lev[0];
    if (h64.levels < 2 || a.n <= 0 || (!want64 && !h32)) return;
    const size_t cells = size_t(a.n) * kEllWidth + 8;
    int32_t *ecol = ar.lo<int32_t>(cells), *tail = ar.lo<int32_t>(size_t(a.n) * 2 + 8);
    double *e64 = want64 ? ar.lo<double>(cells) : nullptr;
    float *e32 = h32 ? ar.lo<float>(cells) : nullptr;
    launch_vblock_ell(a.n, a.rowptr, a.col, a.val, ecol, tail, e64, e32, s);   // level 0 is the compact block: every column is a vertex
    if (want64) { a.ell_col = ecol; a.ell_tail = tail; a.ell_val = e64; }
    if (h32) { AmgLevelT<float> &b = h32->lev[0]; b.ell_col = ecol; b.ell_tail = tail; b.ell_val = e32; }
}

template <class T, class TR> void launch_amg_cycle(const AmgT<T> &H, int k, int step, const TR *r, TR *cz, double *part, int nblocks, const double *scal, hipStream_t s) {
    const int L = H.levels;
    auto rows_grid = [&](int64_t n) { return int((n + kRpb - 1) / kRpb); };
    // the levels from `lt` on go into the single-workgroup kernel (always at least the coarsest one)
    int lt = L - 1;
    while (lt > 1 && H.lev[lt - 1].n <= kTailRows && L - (lt - 1) <= kTailLevels) --lt;
    const bool image = level_image(H.lev[0]);   // level 0's last sweep reads the fixed-width image if the builder made one
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        for (int l = 0; l < lt; ++l) {   // down
            const AmgLevelT<T> &a = H.lev[l], &b = H.lev[l + 1];
            if (l == 0) launch256(k_amg_pre<T, K, TR>, rows_grid(a.n), s, a, r, scal, step);   // (from the image: 8.9 us as from the CSR rows, profiles/cycle_rows_ab.txt)
            else launch256(k_amg_pre<T, K, T>, rows_grid(a.n), s, a, (const T *)a.r, scal, step);
            if (l + 1 < lt)
                for_lanes(restrict_lanes(a), [&](auto lc) {
                    constexpr int LPR = decltype(lc)::value;
                    launch256(k_amg_restrict<T, K, LPR>, grid_rows(b.n, 256 / LPR), s, a, b.n, b.r, scal, step);
                });
        }
        {
            AmgTailT<T> tail;
            tail.levels = L - lt;
            tail.up = H.lev[lt - 1];
            for (int l = lt; l < L; ++l) tail.lev[l - lt] = H.lev[l];
            tail.inv = H.inv;
            for_lanes<16>(restrict_lanes(tail.up), [&](auto lc) {
                hipLaunchKernelGGL((k_amg_tail<T, K, decltype(lc)::value>), dim3(1), dim3(1024), 0, s, tail, scal, step);
            });
        }
        for (int l = lt - 1; l >= 0; --l) {   // up
            const AmgLevelT<T> &a = H.lev[l], &b = H.lev[l + 1];
            hipLaunchKernelGGL((k_amg_prolong<T, K>), dim3(rows_grid(a.n)), dim3(256), 0, s, a, (const T *)b.z2, scal, step);
            if (l == 0 && image && !post_wide())   // the launch that leaves the partial sums is held to `nblocks` workgroups: 128 rows each
                launch256(k_amg_post_image<T, K, TR>, nblocks, s, a, r, cz, part, scal, step);
#ifdef REMO_PROBES
            else if (l == 0 && image)   // key 46: the image in 1024-thread workgroups, a row group each
                hipLaunchKernelGGL((k_amg_post<T, K, true, 1024, TR, true>), dim3(nblocks), dim3(1024), 0, s, a, r, cz, part, scal, step);
#endif
            else if (l == 0)
                hipLaunchKernelGGL((k_amg_post<T, K, true, 1024, TR, false>), dim3(nblocks), dim3(1024), 0, s, a, r, cz, part, scal, step);
            else
                hipLaunchKernelGGL((k_amg_post<T, K, false, 256, T>), dim3(rows_grid(a.n)), dim3(256), 0, s, a, (const T *)a.r, a.z2, (double *)nullptr, scal, step);
        }
    });
}

template void launch_amg_cycle<double, double>(const AmgT<double> &, int, int, const double *, double *, double *, int, const double *, hipStream_t);
template void launch_amg_cycle<float, float>(const AmgT<float> &, int, int, const float *, float *, double *, int, const double *, hipStream_t);
template void launch_amg_cycle<float, double>(const AmgT<float> &, int, int, const double *, double *, double *, int, const double *, hipStream_t);

}  // namespace remo
