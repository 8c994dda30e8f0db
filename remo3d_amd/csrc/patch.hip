// patch.hip — the patch operator (3D, remo_opts_t.op = 3): y = A x without the assembled matrix AND without a slab of element
// results.  Replaces the operator application inside CGSolver(a.mat, ...) (ngsolve_functions.py:50-51); same operator as the
// CSR product of the assembled matrix to rounding.
//
// The element list (sorted by smallest vertices, symbolic_gpu.hip: neighbours in the list are neighbours in the mesh) is cut into
// PATCHES of E consecutive tetrahedra, one 256-thread workgroup each: E = 256 / k for k right-hand sides, or twice that where a
// lane takes two elements (fp64 solves with k >= 3: ROUNDS = 2 below).  Counted on a batch of the headline sweep (370 568
// tetrahedra, 1 703 039 rows; tools/count_patch_rows.py, profiles/patch_two_rounds_ab.txt), distinct matrix rows per element
// instead of 20, and the share of a patch's rows that belong to no other patch:
//     E = 51: 8.45, 24 %     E = 85: 7.75, 30 %     E = 102: 7.53, 32 %
// (the largest patch has 559 / 859 / 994 rows).  Per patch (k_patch_apply):
//   1. every lane asks for the numbers of the rows it stages straight into REGISTERS (no row table in LDS, no barrier before the x
//      rows can be requested) and stages the x rows of the patch's distinct dofs in LDS - every row read once per patch;
//   2. lane (element, right-hand side) reads its 20 rows from LDS, runs the factorised reference tensors
//      (gen_elem_code.cpp: g = B x, h = c~ g, y = B^T h - 492 multiply-adds per column) and adds its 20 result rows into LDS
//      accumulators that REUSE the staging area (x lives in registers by then);
//   3. the accumulators leave as ONE linear copy, 16 bytes per lane and store, into the patch's own block of the slab Yb - every
//      row of the patch, also the rows no other patch touches (slot pboff[p] + m for local row m; blocks padded to 16 rows).
// y itself is written by whoever sums a row's slots in ascending patch order: the PCG's update launch (pcg_kernels.hip), or
// k_patch_reduce below (products outside the PCG, and remo_debug_tune key 22 = 0).
// HBM / L2 traffic per application: every patch reads its x rows once and writes them once to the slab, 1.84 (E = 51) or 1.64
// (E = 102) rows of k values per matrix row each way, plus 88 bytes per element, against
// 12 bytes per STORED ENTRY of the CSR product (48 entries per row).  The LDS accumulation uses ds_add_f64: the order of the adds
// inside a patch is not fixed, so results are reproducible to rounding (1e-16 relative per row), not bit for bit - the one kernel
// of the path for which that holds.
// Variants that were measured and removed (rows of one patch alone straight to y, a row-major slab, 512-thread workgroups,
// workgroups of a CU started one after the other): DESIGN.md section 8 keeps their figures.  The persistent forms live in patch_persist.inc (probe builds).
#include <hip/hip_runtime.h>
#include <limits.h>

#include <rocprim/device/device_scan.hpp>

#include "kernels.h"
#include "kutil.h"
#include "patch.h"
#include <stdexcept>
#include <type_traits>
#include "symbolic_gpu.h"
#include "wave_util.h"

#define REMO_ELEM_NS elem_tables_patch
#include "build/elem_apply.inc"

namespace remo {

namespace {

constexpr int kPatchDotBlocks = 32;                    // workgroups of k_patch_dot
constexpr uint32_t kSlotBits = 13;                      // element dof slots of a patch: E * 20 <= 4096 < 8192 (E <= 204: patch_elements_per_group)
constexpr uint64_t kNoRow = uint64_t(0x7FFFFFFF);      // constrained dof: sorts behind every row

// ---- tables ------------------------------------------------------------------------------------------------------------
// bcnt[r] = number of patches that touch row r (the row gets that many slots in the slab: every row goes through it, also the rows
// of one patch alone).  The adjacency of a row lists its elements in ascending order, so its patches ascend too.
__global__ void __launch_bounds__(256) k_patch_row_slots(int64_t n, int E, const int32_t *__restrict__ adjptr, const uint32_t *__restrict__ adj,
                                                         int32_t *__restrict__ bcnt) {
    const int64_t r = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r > n) return;
    int cnt = 0;
    if (r < n) {
        int32_t last = -1;
        for (int32_t a = adjptr[r]; a < adjptr[r + 1]; ++a) {
            const int32_t p = int32_t((adj[a] >> 5) / uint32_t(E));
            cnt += p != last;
            last = p;
        }
    }
    bcnt[r] = cnt;
}

// One workgroup per patch: sort the patch's (row, element dof slot) pairs in LDS, number the distinct rows 0 .. M - 1 in
// ascending order, and write
//   lidx[element dof]  local row (0xFFFF: constrained dof)
//   prow[p][m]         global row of local row m
//   pcount[p] = M      (raises flag bit 1 and records nothing beyond rows_cap if M > rows_cap)
//   pbcnt[p]           rows of the patch's block of the slab: one per row the tables hold (k_patch_slots numbers them)
__global__ void __launch_bounds__(256) k_patch_build(int64_t nt, int E, int rows_cap, int npad, const int32_t *__restrict__ eldof,
                                                     uint16_t *__restrict__ lidx, int32_t *__restrict__ pcount, int32_t *__restrict__ pbcnt,
                                                     int32_t *__restrict__ prow, int32_t *flag, int32_t *max_rows) {
    extern __shared__ uint64_t keys[];   // [npad]
    __shared__ int32_t cnts[256];
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x, e0 = p * E;
    const int ne = int(nt - e0 < E ? nt - e0 : E), nslots = ne * 20;
    for (int j = tid; j < npad; j += 256) {
        uint64_t k = ~uint64_t(0);
        if (j < nslots) {
            const int32_t r = eldof[e0 * 20 + j];
            k = ((r >= 0 ? uint64_t(uint32_t(r)) : kNoRow) << kSlotBits) | uint64_t(j);
        }
        keys[j] = k;
    }
    for (int size = 2; size <= npad; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < npad / 2; t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
            }
        }
    __syncthreads();
    const int per = npad / 256, j0 = tid * per;
    auto row_at = [&](int j) -> uint64_t { return keys[j] >> kSlotBits; };
    int heads = 0;
    for (int j = j0; j < j0 + per; ++j) {
        const uint64_t r = row_at(j);
        heads += (j < nslots && r < kNoRow && (j == 0 || row_at(j - 1) != r)) ? 1 : 0;
    }
    cnts[tid] = heads;
    __syncthreads();
    int before = 0, total = 0;
    for (int t = 0; t < 256; ++t) { const int c = cnts[t]; before += t < tid ? c : 0; total += c; }
    if (tid == 0) {
        pcount[p] = total;
        atomicMax(max_rows, total);
        if (total > rows_cap) atomicOr(flag, 1);
        // a patch's block of the slab begins on a 64-byte line in fp64 and fp32 storage alike (16 rows of k values): the linear
        // output phase then stores whole lines only
        pbcnt[p] = ((total < rows_cap ? total : rows_cap) + 15) & ~15;
    }
    int id = before - 1;     // local row of the most recent head at or before j
    for (int j = j0; j < j0 + per && j < nslots; ++j) {
        const uint64_t r = row_at(j);
        const int slot = int(keys[j] & ((uint64_t(1) << kSlotBits) - 1));
        if (r >= kNoRow) { lidx[e0 * 20 + slot] = 0xFFFF; continue; }
        const bool head = (j == 0 || row_at(j - 1) != r);
        id += head ? 1 : 0;
        lidx[e0 * 20 + slot] = uint16_t(id < 0xFFFF ? id : 0xFFFE);
        if (head && id < rows_cap) prow[p * rows_cap + id] = int32_t(r);
    }
}

// Constrained dofs read (and add into) a row of zeros behind the staged rows: local row = the largest row count of any patch,
// known once every patch is built (device-side value: no host round trip) - so the kernel needs no test per dof.
__global__ void __launch_bounds__(256) k_patch_zero_rows(int64_t nslots, uint16_t *__restrict__ lidx, const int32_t *__restrict__ max_rows) {
    const uint16_t z = uint16_t(max_rows[0] < 0xFFFF ? max_rows[0] : 0xFFFE);
    for (int64_t j = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; j < nslots; j += int64_t(gridDim.x) * blockDim.x)
        if (lidx[j] == 0xFFFF) lidx[j] = z;
}

// Slab slots.  The slab is PATCH-major: the rows of patch p own the slots pboff[p], pboff[p] + 1, ... in ascending row order,
// so a patch writes one contiguous block, and the rows of a block read by k_patch_reduce are neighbours too.  One workgroup per
// patch: pout[p][m] = pboff[p] + m = slot of local row m, and the row's list bslot[bptr[row] + rank of this patch among the
// patches of the row] = that slot.
__global__ void __launch_bounds__(256) k_patch_slots(int E, int rows_cap, const int32_t *__restrict__ pcount, const int32_t *__restrict__ pboff,
                                                     const int32_t *__restrict__ prow, int32_t *__restrict__ pout, const int32_t *__restrict__ adjptr,
                                                     const uint32_t *__restrict__ adj, const int32_t *__restrict__ bptr, int32_t *__restrict__ bslot,
                                                     int32_t *__restrict__ row4) {
    const int64_t p = blockIdx.x;
    const int mp = pcount[p] < rows_cap ? pcount[p] : rows_cap;
    for (int m = threadIdx.x; m < mp; m += 256) {
        const int32_t row = prow[p * rows_cap + m], slot = pboff[p] + m;
        int32_t last = -1, rank = 0;
        for (int32_t a = adjptr[row]; a < adjptr[row + 1]; ++a) {     // patches of the row ascend with its elements
            const int32_t q = int32_t((adj[a] >> 5) / uint32_t(E));
            if (q >= p) break;
            rank += q != last;
            last = q;
        }
        pout[p * rows_cap + m] = slot;
        bslot[bptr[row] + rank] = slot;
        // row4[row] = the row's first four slots side by side (-1: none; preset), so that the update launch finds them with ONE load
        // instead of two dependent ones; a row of five or more patches (vertex rows) keeps three there and -2 = "the rest is in bslot"
        const int32_t cnt = bptr[row + 1] - bptr[row];
        if (rank < 3 || (rank == 3 && cnt <= 4)) row4[int64_t(row) * 4 + rank] = slot;
        else if (rank == 3) row4[int64_t(row) * 4 + 3] = -2;
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ void lds_add(T *p, T v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One workgroup of 256 threads = one patch of E = 256 / K elements; lane = (element, right-hand side).
// The kernel is a chain of dependent memory round trips (tables -> x rows -> LDS -> ... -> stores) around ~1 us of arithmetic, so
// everything a lane will need from the tables is requested BEFORE the first wait - the patch's row count and first slab slot, the
// numbers of the rows it stages (in registers), the local rows of its element, the metric terms - which leaves two round trips:
// tables, then x.
// <x, A x> is summed element by element as g . h (g = B x, h = c~ g: x^T B^T c~ B x): complete when this launch ends, no second
// look at x.  MODE != 0: ablations for tools/probe_patch.py (wrong results on purpose): 1 = plain stores instead of the LDS
// atomics, 2 = no tensor arithmetic (y = x), 3 = nothing leaves the workgroup.
// LEAN: the register-lean order of phase 2 (five waves per SIMD instead of four in fp64): the gradient chain runs input by input
// straight from the staged rows in LDS (no x[20] in registers), BEFORE the staging area is recycled; the metric terms are asked for
// after it; the divergence chain hands every group of outputs to the LDS accumulators as soon as it is complete (no y[20]).
#ifndef REMO_LEAN_WAVES
#define REMO_LEAN_WAVES 5
#endif
// ROUNDS = 2 (fp64 storage, PatchTables::rounds): a patch holds 2 * (256 / K) elements and every lane takes TWO of them, one after
// the other, in its one column - element A from the first half of the patch's list, element B from the second (the spread of the
// lanes over runs applies inside each half).  The fixed cost of a patch (tables, staging round trip, clearing, rows out, barriers)
// is paid half as often and a patch of twice the elements has fewer rows per element (7.5 against 8.4 at size L: fewer slab rows
// written here and gathered by the update launch).  Order of phase 2: x of A -> y of A in registers and x of B read while the staged
// image is whole, THEN the image becomes the accumulators, y of A goes out, B is computed and goes out.  The lanes hold up to
// kPatchPasses2 staging passes (a patch of 2 * 51 elements has ~770 rows, 15 passes of 51; the largest ~1000).
constexpr int kPatchPasses2 = 20;
// TX = storage type of x, T = type of everything else.  TX = float with T = double (the PCG's fp32 search direction,
// PcgBuffersT::p32): phase 1 stages 4-byte values, the staged image in LDS is fp32 and a lane widens its twenty values as it reads
// them; the registers, <x, A x>, the accumulators and the slab are fp64 as with TX = T.
template <class T, int K, int MODE = 0, bool LEAN = false, int ROUNDS = 1, class TX = T>
__global__ void __launch_bounds__(kPatchBlock, (LEAN ? REMO_LEAN_WAVES : 1)) k_patch_apply(PatchTables tb, int rows, const TX *__restrict__ x, T *__restrict__ y, T *__restrict__ Yb,
                                                     double *__restrict__ ppart, const double *__restrict__ scal, int step, long long *__restrict__ stamps,
                                                     double *__restrict__ pbins) {
    static_assert(std::is_same<TX, T>::value || (std::is_same<TX, float>::value && std::is_same<T, double>::value && MODE == 0 && !LEAN),
                  "an x narrower than the rest: fp32 into the fp64 product, plain order");
    (void)y;     // (every row leaves through the slab; the argument keeps its place in the launch)
    // the "solve is over" word is asked for HERE but looked at when the row numbers are there (it travels with them, as a vector
    // load, so that no scalar load of the prologue queues behind a word another XCD wrote: one round trip instead of two)
    int done_word = 0;
    if (scal) done_word = load_as_vector(reinterpret_cast<const int *>(scal + kDoneSlot));
    // MODE 4: wave 0 of every workgroup leaves the clock at the phase boundaries (remo_debug_patch_phases)
#define REMO_STAMP(k) if constexpr (MODE == 4) { if (threadIdx.x == 0) stamps[(int64_t(blockIdx.x) << 3) + (k)] = __builtin_readcyclecounter(); }
    REMO_STAMP(0)
    constexpr int NL = K;
    static_assert(ROUNDS == 1 || (ROUNDS == 2 && MODE == 0 && !LEAN), "two rounds: the plain order of the product only");
    constexpr int U = ROUNDS == 2 ? kPatchPasses2 : kPatchPasses;   // loads in flight per lane: one trip over up to U * (256 / K) rows
    constexpr int BLK = kPatchBlock;
    constexpr int EK = BLK / K;                          // rows per pass of the staging / output phases
    constexpr uint32_t S = sizeof(T), SX = sizeof(TX);
    extern __shared__ double lds_raw[];
    TX *xs = reinterpret_cast<TX *>(lds_raw);            // [(rows + 2)][K]: x rows (TX), later the accumulators of y (double); row `rows` = zeros, row rows + 1 = slack
    __shared__ double smem[16 * K];
    const int tid = threadIdx.x;
    // workgroups b, b + 8, ... share an XCD and its L2: every XCD takes one contiguous eighth of the patches (neighbouring patches
    // share their boundary rows: the second reader finds them in that L2, and the slab rows of one matrix row are written through it)
    const int64_t per = (tb.npatch + 7) >> 3;
    const int64_t p = int64_t(blockIdx.x & 7) * per + int64_t(blockIdx.x >> 3);
    if (p >= tb.npatch) return;
    const int32_t *prow = tb.prow + p * tb.rows_cap;
    // the staging and output phases walk THIS patch's rows, not the largest patch's (`rows`: it sizes LDS and names the zero row): the
    // average patch has 0.6 of the rows of the largest, and a pass without rows still cost its instructions.  The number of passes
    // is a compile-time constant of the code that runs (a switch over 1 .. U: guards inside one unrolled loop keep the loads from
    // going out together and cost what the shorter walk saves); remo_debug_tune key 33 = 0: the largest patch's count for all
    const int el = tid / NL, c0 = tid - el * NL;
    const int32_t off_mask = tid < EK * K ? 0 : int32_t(0x80000000);   // or-ed into a row number: negative = no row for this lane
    // the patch's row count and the row numbers THIS lane stages (local rows el, el + EK, ...: the first U of them) are requested
    // together, straight into registers - no table in LDS, no barrier before the x rows can be asked for.  (The row count as a vector
    // load too: a scalar load would make every later scalar wait - kernel arguments, factor tables - wait for it.)
    const rsrc_t rpr = make_rsrc(prow, uint64_t(tb.rows_cap) * 4);
    int32_t r0[U];
    const int rows_own_v = load_as_vector(tb.pcount + p);
    const int slab0_v = load_as_vector(tb.pboff + p);     // first slab slot of the patch, wanted by the output phase
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int32_t t[1];
        buf_load<int32_t, 1>(rpr, off_mask == 0 ? uint32_t(el + EK * u) * 4u : kOutOfRange, t);
        r0[u] = t[0];
    }
    // the elements of a wave are taken from four runs of the patch's list instead of one (remo_debug_tune key 32: 0 = one run):
    // consecutive elements of the sorted list share their smallest vertices, i.e. they add into the same LDS rows in the same
    // instruction, which serialises - application 138.0 / 125.4 us against 141.3 / 128.2 at 443 k / 424 k tetrahedra.  Lane group el
    // takes element number (el >> 2) of run (el & 3); the runs have ceil((E - r) / 4) elements.
    // (R runs: lane group el takes element el / R of run el % R; run r has ceil((E - r) / R) elements and starts behind the runs before it:
    //  r * floor(E / R) + min(r, E % R))
    const int R = tb.spread > 1 ? tb.spread : 1;
    const int EL = ROUNDS == 2 ? (tb.E >> 1) : tb.E;      // elements per round: one per lane group
    const int run = el % R, base = EL / R, extra = EL % R;
    const int elp = R > 1 ? (run * base + (run < extra ? run : extra) + el / R) : el;
    const int64_t e = p * tb.E + elp;
    const bool active = el < EL && e < tb.nt;
    // two rounds: the lane's second element sits EL places further down the patch's list (a short last patch may have none)
    const int64_t eB = e + EL;
    const bool activeB = ROUNDS == 2 && el < EL && eB < tb.nt;
    uint32_t li[10];
    double cm[6];
#pragma unroll
    for (int q = 0; q < 10; ++q) li[q] = 0u;
#pragma unroll
    for (int q = 0; q < 6; ++q) cm[q] = 0.0;
    // 1a. the element's own data (local rows, metric terms) is asked for BEHIND the row numbers: it is wanted much later, loads
    // return in order, and the wait in front of the x rows then covers the row numbers only.
    // (buffer loads: a lane without an element hands over an offset out of range instead of branching around the loads - with a branch
    // the compiler's count of loads in flight is the smaller one of the two paths, and every later wait for a row number would wait for
    // these, the slowest loads of the prologue, too)
    const rsrc_t rli = make_rsrc(tb.lidx, uint64_t(tb.nt) * 40), rcm = make_rsrc(tb.C, uint64_t(tb.nt) * 48);
    buf_load<uint32_t, 10>(rli, active ? uint32_t(e) * 40u : kOutOfRange, li);   // 40-byte records: 8-byte aligned
    if constexpr (!(LEAN && MODE != 2)) buf_load<double, 6>(rcm, active ? uint32_t(e) * 48u : kOutOfRange, cm);   // metric terms (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
    uint32_t liB[ROUNDS == 2 ? 10 : 1];
    double cmB[ROUNDS == 2 ? 6 : 1];
    if constexpr (ROUNDS == 2) {
#pragma unroll
        for (int q = 0; q < 10; ++q) liB[q] = 0u;
#pragma unroll
        for (int q = 0; q < 6; ++q) cmB[q] = 0.0;
        buf_load<uint32_t, 10>(rli, activeB ? uint32_t(eB) * 40u : kOutOfRange, liB);
        buf_load<double, 6>(rcm, activeB ? uint32_t(eB) * 48u : kOutOfRange, cmB);
    }
    const int rows_own = __builtin_amdgcn_readfirstlane(rows_own_v);
    if (__builtin_amdgcn_readfirstlane(done_word) != 0 && __builtin_amdgcn_readfirstlane(done_word) <= step) return;   // (solve_done; uniform)
    const int rows_p = (tb.trim && rows_own < rows) ? rows_own : rows;
    const int npass = (rows_p + EK - 1) / EK;
    REMO_STAMP(1)
    // 1b. stage the patch's x rows, ONE VALUE per lane and load: in pass u lane (el, c0) takes column c0 of local row el + EK u
    // (EK = 256 / K rows per pass), i.e. value tid + EK K u of the staged image - neighbouring lanes read neighbouring addresses
    // inside a row and across consecutive rows (a patch's rows come in a few runs of consecutive matrix rows), no division per
    // value, and ALL loads of a lane are in flight together (U passes; the phase is one memory round trip, not one per pass: a
    // round trip is ~2-5 k clocks here, the arithmetic of a whole patch ~4 k).  Buffer loads with the hardware range check: a lane
    // without a row hands over an offset beyond the descriptor (no request, no branch); its LDS store goes to the slack row.
    // 24-bit multiplies: rows and slots are below 2^24 (checked by the caller).  Row `rows` is the zero row constrained dofs read.
    const rsrc_t rx = make_rsrc(x, uint64_t(tb.n) * K * SX);
    const uint32_t slack = uint32_t((rows + 1) * K + c0);
#define REMO_PASSES_UP_TO_12(fn)                                                                                          \
        case 1: fn(std::integral_constant<int, 1>{}, 0); break;   case 2: fn(std::integral_constant<int, 2>{}, 0); break;   \
        case 3: fn(std::integral_constant<int, 3>{}, 0); break;   case 4: fn(std::integral_constant<int, 4>{}, 0); break;   \
        case 5: fn(std::integral_constant<int, 5>{}, 0); break;   case 6: fn(std::integral_constant<int, 6>{}, 0); break;   \
        case 7: fn(std::integral_constant<int, 7>{}, 0); break;   case 8: fn(std::integral_constant<int, 8>{}, 0); break;   \
        case 9: fn(std::integral_constant<int, 9>{}, 0); break;   case 10: fn(std::integral_constant<int, 10>{}, 0); break; \
        case 11: fn(std::integral_constant<int, 11>{}, 0); break; case 12: fn(std::integral_constant<int, 12>{}, 0); break;
#define REMO_PASSES(fn)                                                                                                   \
    if constexpr (ROUNDS == 2) {                                                                                          \
        switch (npass) {                                                                                                  \
            REMO_PASSES_UP_TO_12(fn)                                                                                      \
            case 13: fn(std::integral_constant<int, 13>{}, 0); break; case 14: fn(std::integral_constant<int, 14>{}, 0); break; \
            case 15: fn(std::integral_constant<int, 15>{}, 0); break; case 16: fn(std::integral_constant<int, 16>{}, 0); break; \
            case 17: fn(std::integral_constant<int, 17>{}, 0); break; case 18: fn(std::integral_constant<int, 18>{}, 0); break; \
            case 19: fn(std::integral_constant<int, 19>{}, 0); break; case 20: fn(std::integral_constant<int, 20>{}, 0); break; \
            default:                                                                                                      \
                for (int m0 = 0; m0 < rows_p; m0 += U * EK) fn(std::integral_constant<int, U>{}, m0);                     \
        }                                                                                                                 \
    } else {                                                                                                              \
        switch (npass) {                                                                                                  \
            REMO_PASSES_UP_TO_12(fn)                                                                                      \
            default:                                                                                                      \
                for (int m0 = 0; m0 < rows_p; m0 += U * EK) fn(std::integral_constant<int, U>{}, m0);                     \
        }                                                                                                                 \
    }
    static_assert(kPatchPasses == 12 && kPatchPasses2 == 20, "REMO_PASSES lists the cases 1 .. U");
    // the row numbers come from registers (a patch with more than U passes of rows - the largest few of a batch - asks for the
    // numbers of its later chunks when it gets there)
    auto stage = [&](auto np_c, int m0) {
        constexpr int NP = decltype(np_c)::value;
        int32_t r[NP];
        TX v[NP][1];
        if (m0 == 0) {
#pragma unroll
            for (int u = 0; u < NP; ++u) r[u] = r0[u];
        } else {
#pragma unroll
            for (int u = 0; u < NP; ++u) {
                int32_t t[1];
                buf_load<int32_t, 1>(rpr, off_mask == 0 ? uint32_t(m0 + el + EK * u) * 4u : kOutOfRange, t);
                r[u] = t[0];
            }
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) r[u] = (off_mask == 0 && m0 + el + EK * u < rows_own) ? r[u] : -1;
#pragma unroll
        for (int u = 0; u < NP; ++u)
            buf_load<TX, 1>(rx, r[u] >= 0 ? __umul24(uint32_t(r[u]), K * SX) + uint32_t(c0) * SX : kOutOfRange, v[u]);
#pragma unroll
        for (int u = 0; u < NP; ++u) xs[r[u] >= 0 ? uint32_t((m0 + el + EK * u) * K + c0) : slack] = v[u][0];
    };
    REMO_PASSES(stage)
    if (tid < 2 * K) xs[rows * K + tid] = TX(0);
    __syncthreads();
    REMO_STAMP(2)
    // 2. my element, my column
    double d0 = 0.0;
    double *ya = lds_raw;
#define REMO_PATCH_L(i) ((li[(i) >> 1] >> (16 * ((i) & 1))) & 0xFFFFu)      /* local row of dof i; constrained dofs: the zero row (k_patch_zero_rows) */
    if constexpr (LEAN && MODE != 2) {
        typedef const T __attribute__((address_space(4))) *ctab_t;
        ctab_t tgi = (ctab_t)ElemTables2<T>::grad_in(), tdo = (ctab_t)ElemTables2<T>::div_out();
        if constexpr (sizeof(T) == 8) { asm volatile("" : "+s"(tgi)); asm volatile("" : "+s"(tdo)); }
        T g[30];
#define REMO_PATCH_XL(i) xs[REMO_PATCH_L(i) * K + c0]
        // (lanes without an element read row 0 and drop the result.)  Scheduling barriers between the blocks of the chain: fp32
        // (factors are literals) 72 registers with them, 88 without; fp64 (factors arrive by scalar loads) must not wait per block
#define REMO_BAR_ON __builtin_amdgcn_sched_barrier(0);
#define REMO_BAR_OFF
        if constexpr (sizeof(T) == 4) { REMO_ELEM_GRAD_IN(T, REMO_PATCH_XL, g, tgi, REMO_BAR_ON) }
        else { REMO_ELEM_GRAD_IN(T, REMO_PATCH_XL, g, tgi, REMO_BAR_OFF) }
#undef REMO_PATCH_XL
        // (pin the chain HERE: its results are used only behind the barriers, inside a branch, and the compiler would sink the
        // arithmetic there - keeping all twenty x values and every factor alive across the barriers)
#pragma unroll
        for (int j = 0; j < 30; ++j) asm volatile("" : "+v"(g[j]));
        __builtin_amdgcn_sched_barrier(0);                   // the metric terms are NOT wanted in registers during the chain above
        if (active) {
            const double *ce = tb.C + e * 6;                 // in flight while the workgroup meets at the two barriers below
#pragma unroll
            for (int q = 0; q < 6; ++q) cm[q] = ce[q];
        }
        __syncthreads();    // every lane has read its x values: the staging area becomes the accumulators
        REMO_STAMP(3)
        for (int j = 2 * tid; j < rows_p * K; j += 2 * BLK) { ya[j] = 0.0; ya[j + 1] = 0.0; }     // (16 bytes per lane; an odd count clears one value of the next row: unused, or the zero row)
        if (tid < K) ya[rows * K + tid] = 0.0;
        __syncthreads();
        REMO_STAMP(4)
        if (active) {
            const T c11 = T(cm[0]), c12 = T(cm[1]), c13 = T(cm[2]), c22 = T(cm[3]), c23 = T(cm[4]), c33 = T(cm[5]);
            T dd = T(0);
#pragma unroll
            for (int m = 0; m < 10; ++m) {     // h = c~ g, in place; g . h on the way
                const T g1 = g[m], g2 = g[10 + m], g3 = g[20 + m];
                const T h1 = c11 * g1 + c12 * g2 + c13 * g3, h2 = c12 * g1 + c22 * g2 + c23 * g3, h3 = c13 * g1 + c23 * g2 + c33 * g3;
                dd += g1 * h1 + g2 * h2 + g3 * h3;
                g[m] = h1; g[10 + m] = h2; g[20 + m] = h3;
            }
            d0 = double(dd);
            if constexpr (sizeof(T) == 8) {      // fp64: the local rows are fetched again (an L1 / L2 hit) rather than held through h = c~ g
                const uint32_t *pl2 = reinterpret_cast<const uint32_t *>(tb.lidx + e * 20);
#pragma unroll
                for (int q = 0; q < 10; ++q) li[q] = __builtin_nontemporal_load(pl2 + q);
            }
#define REMO_PATCH_EMIT(i, v) { if constexpr (MODE == 1) ya[REMO_PATCH_L(i) * K + c0] = double(v); else lds_add(ya + REMO_PATCH_L(i) * K + c0, double(v)); }
            if constexpr (sizeof(T) == 4) { REMO_ELEM_DIV_OUT(T, g, tdo, REMO_PATCH_EMIT, REMO_BAR_ON) }
            else { REMO_ELEM_DIV_OUT(T, g, tdo, REMO_PATCH_EMIT, REMO_BAR_OFF) }
#undef REMO_PATCH_EMIT
#undef REMO_BAR_ON
#undef REMO_BAR_OFF
        }
    } else if constexpr (ROUNDS == 2) {
        typedef const T __attribute__((address_space(4))) *ctab_t;
        ctab_t tgrad = (ctab_t)ElemTables<T>::grad(), tdiv = (ctab_t)ElemTables<T>::div();
        if constexpr (sizeof(T) == 8) { asm volatile("" : "+s"(tgrad)); asm volatile("" : "+s"(tdiv)); }
        // y = B^T c~ B x of one element in this lane's column; returns g . h
        auto element = [&](const T (&xe)[20], const double (&ce)[6], T (&ye)[20]) -> double {
            const T c11 = T(ce[0]), c12 = T(ce[1]), c13 = T(ce[2]), c22 = T(ce[3]), c23 = T(ce[4]), c33 = T(ce[5]);
            T g[30];
            REMO_ELEM_GRAD(T, xe, g, tgrad)
            T dd = T(0);
#pragma unroll
            for (int m = 0; m < 10; ++m) {     // h = c~ g, in place; g . h on the way
                const T g1 = g[m], g2 = g[10 + m], g3 = g[20 + m];
                const T h1 = c11 * g1 + c12 * g2 + c13 * g3, h2 = c12 * g1 + c22 * g2 + c23 * g3, h3 = c13 * g1 + c23 * g2 + c33 * g3;
                dd += g1 * h1 + g2 * h2 + g3 * h3;
                g[m] = h1; g[10 + m] = h2; g[20 + m] = h3;
            }
            REMO_ELEM_DIV(T, g, ye, tdiv)
            return double(dd);
        };
        // the local rows of an element are read a second time for its accumulation (an L1 / L2 hit), as in the one-round order
        auto emit = [&](int64_t ee, const T (&ye)[20]) {
            uint32_t lq[10];
            const uint32_t *pl2 = reinterpret_cast<const uint32_t *>(tb.lidx + ee * 20);
#pragma unroll
            for (int q = 0; q < 10; ++q) lq[q] = __builtin_nontemporal_load(pl2 + q);
#pragma unroll
            for (int i = 0; i < 20; ++i) lds_add(ya + ((lq[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) * K + c0, double(ye[i]));
        };
        // element A: its x values and its whole result; element B: its x values - all while the staged image is whole
        T yA[20], xB[20];
        double dA = 0.0;
        if (active) {
            T xA[20];
#pragma unroll
            for (int i = 0; i < 20; ++i) xA[i] = T(xs[REMO_PATCH_L(i) * K + c0]);
            dA = element(xA, cm, yA);
            // (pin the result HERE: it is used behind the barriers, and the compiler would sink the arithmetic there)
#pragma unroll
            for (int i = 0; i < 20; ++i) asm volatile("" : "+v"(yA[i]));
        }
        if (activeB) {
#pragma unroll
            for (int i = 0; i < 20; ++i) xB[i] = T(xs[((liB[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) * K + c0]);
        }
        __syncthreads();        // every lane holds what it wants of the image: the staging area becomes the accumulators
        REMO_STAMP(3)
        for (int j = 2 * tid; j < rows_p * K; j += 2 * BLK) { ya[j] = 0.0; ya[j + 1] = 0.0; }
        if (tid < K) ya[rows * K + tid] = 0.0;
        __syncthreads();
        REMO_STAMP(4)
        if (active) emit(e, yA);
        d0 = dA;
        if (activeB) {
            T yB[20];
            d0 += element(xB, cmB, yB);
            emit(eB, yB);
        }
    } else {
    T xv[20];
    if (active) {
#pragma unroll
        for (int i = 0; i < 20; ++i) xv[i] = T(xs[REMO_PATCH_L(i) * K + c0]);
    }
    __syncthreads();        // every lane holds its x values: the staging area becomes the accumulators
    REMO_STAMP(3)
    // the accumulators are fp64 whatever T is: ds_add_f32 runs at about a lane per clock on this chip (measured: 204 of the 304 us
    // of the fp32 kernel at 443 k tetrahedra were its 20 atomics per lane; ds_add_f64 costs 4 us there)
    for (int j = 2 * tid; j < rows_p * K; j += 2 * BLK) { ya[j] = 0.0; ya[j + 1] = 0.0; }     // (16 bytes per lane; an odd count clears one value of the next row: unused, or the zero row)
    if (tid < K) ya[rows * K + tid] = 0.0;
    __syncthreads();
    REMO_STAMP(4)
    if (active) {
        const T c11 = T(cm[0]), c12 = T(cm[1]), c13 = T(cm[2]), c22 = T(cm[3]), c23 = T(cm[4]), c33 = T(cm[5]);
        T g[30], yv[20];
        if constexpr (MODE == 2) {
#pragma unroll
            for (int i = 0; i < 20; ++i) yv[i] = xv[i] * c11;
        } else {
            // fp64: ONE base address of each factor table in scalar registers (left to itself the compiler forms the address anew,
            // three scalar instructions, before each of its 48 s_load_dwordx16)
            typedef const T __attribute__((address_space(4))) *ctab_t;
            ctab_t tgrad = (ctab_t)ElemTables<T>::grad(), tdiv = (ctab_t)ElemTables<T>::div();
            if constexpr (sizeof(T) == 8) { asm volatile("" : "+s"(tgrad)); asm volatile("" : "+s"(tdiv)); }
            REMO_ELEM_GRAD(T, xv, g, tgrad)
            T dd = T(0);
#pragma unroll
            for (int m = 0; m < 10; ++m) {     // h = c~ g, in place; g . h on the way
                const T g1 = g[m], g2 = g[10 + m], g3 = g[20 + m];
                const T h1 = c11 * g1 + c12 * g2 + c13 * g3, h2 = c12 * g1 + c22 * g2 + c23 * g3, h3 = c13 * g1 + c23 * g2 + c33 * g3;
                dd += g1 * h1 + g2 * h2 + g3 * h3;
                g[m] = h1; g[10 + m] = h2; g[20 + m] = h3;
            }
            d0 = double(dd);
            REMO_ELEM_DIV(T, g, yv, tdiv)
        }
        // the local rows are read a second time for the accumulation (an L1 / L2 hit) instead of being held in ten registers
        // through the tensor arithmetic: that is the difference between three and four waves per SIMD in fp64
        {
            const uint32_t *pl2 = reinterpret_cast<const uint32_t *>(tb.lidx + e * 20);
#pragma unroll
            for (int q = 0; q < 10; ++q) li[q] = __builtin_nontemporal_load(pl2 + q);
        }
#pragma unroll
        for (int i = 0; i < 20; ++i) {
            const uint32_t l = REMO_PATCH_L(i);
            if constexpr (MODE == 1) ya[l * K + c0] = double(yv[i]);
            else lds_add(ya + l * K + c0, double(yv[i]));
        }
    }
    }
#undef REMO_PATCH_L
    __syncthreads();
    REMO_STAMP(5)
    // 3. the accumulators -> the patch's block of the slab, one linear copy: value j of the image to value j of the block.  The block has
    // its own buffer descriptor (64-bit base, the patch's rows as its range): small offsets, no limit on the slab's size, and the
    // hardware drops what lies behind the patch's last row
    if (MODE != 3) {
        // 16 bytes per lane and store (two fp64 / four fp32 values; the accumulators come out of LDS 16 bytes at a time as well): half
        // the store instructions of a value per lane.  A store that straddles the end of the block loses its dwords beyond it
        // (buffer stores of several dwords are range-checked dword by dword).
        constexpr int VEC = 16 / int(S);
        const rsrc_t rp = make_rsrc(Yb + int64_t(__builtin_amdgcn_readfirstlane(slab0_v)) * K, uint64_t(rows_own) * K * S);
        auto put = [&](auto np_c, int m0) {
            constexpr int NP = decltype(np_c)::value;
            constexpr int NQ = (NP * EK * K + VEC * BLK - 1) / (VEC * BLK);      // NP passes of EK rows = NP EK K values from value m0 K on
            T v[NQ][VEC];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int j = m0 * K + VEC * (tid + BLK * q);                     // (behind the patch's rows: whatever LDS holds, never stored)
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[q][i] = T(ya[j + i]);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) buf_store<T, VEC>(rp, uint32_t(m0 * K + VEC * (tid + BLK * q)) * S, v[q]);
        };
        REMO_PASSES(put)
    }
    REMO_STAMP(6)
    if (ppart) {
        double dot[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] = (c == c0) ? d0 : 0.0;
        const double mine = block_sum_column<K>(dot, smem);     // (not block_sum + pick: that went through scratch memory, kutil.h)
        if (tid < K) {
            // pbins: straight into the consumer's rows (kPqBins of them, patches p, p + kPqBins, ... share one; return-less atomic
            // adds performed at the memory side, complete when the launch ends) instead of a row per patch that a launch folds
            if (pbins) (void)__hip_atomic_fetch_add(pbins + (p % kPqBins) * K + tid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else ppart[p * K + tid] = mine;
        }
    }
    REMO_STAMP(7)
#undef REMO_STAMP
#undef REMO_PASSES
#undef REMO_PASSES_UP_TO_12
}

// y = for every row the sum of its slab slots (one per patch that touches it) in ascending patch order.  DOT: the patches' <x, A x> are folded
// into <= 1024 partial rows for the consumer (every workgroup takes a fixed subset: deterministic given the patches' sums).
template <class T, int K, bool DOT>
__global__ void __launch_bounds__(256) k_patch_reduce(int64_t n, int64_t npatch, const int32_t *__restrict__ bptr, const int32_t *__restrict__ bslot,
                                                      const T *__restrict__ Yb,
                                                      T *__restrict__ y, const double *__restrict__ ppart,
                                                      double *__restrict__ part, const double *__restrict__ scal, int step) {
    if (scal && solve_done(scal, step)) return;
    const int64_t stride = int64_t(gridDim.x) * blockDim.x;
    for (int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; row < n; row += stride) {
        const int32_t b0 = bptr[row], b1 = bptr[row + 1];
        if (b1 <= b0) continue;
        T acc[K];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = T(0);
        for (int32_t s0 = b0; s0 < b1; s0 += 2) {     // two slots in flight (a row has 2-4), ascending patches
            T v0[K], v1[K];
            const bool second = s0 + 1 < b1;
            const int64_t a0 = bslot[s0], a1 = second ? bslot[s0 + 1] : 0;
#pragma unroll
            for (int c = 0; c < K; ++c) v0[c] = Yb[a0 * K + c];
#pragma unroll
            for (int c = 0; c < K; ++c) v1[c] = second ? Yb[a1 * K + c] : T(0);
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = (acc[c] + v0[c]) + v1[c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) y[row * K + c] = acc[c];
    }
    if (DOT) {
        double dot[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] = 0.0;
        for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < npatch; p += stride)
#pragma unroll
            for (int c = 0; c < K; ++c) dot[c] += ppart[p * K + c];
        __shared__ double smem[16 * K];
        block_sum<K>(dot, smem);
        if (threadIdx.x < K) part[blockIdx.x * K + threadIdx.x] = pick<K>(dot, threadIdx.x);
    }
}

// <x, A x> of the patches folded into <= 1024 partial rows for the consumer (every workgroup takes a fixed subset): what
// k_patch_reduce<DOT> does at its end, alone - for the PCG, whose update launch sums the shared rows itself
template <int K>
__global__ void __launch_bounds__(256) k_patch_dot(int64_t npatch, const double *__restrict__ ppart, double *__restrict__ part,
                                                   const double *__restrict__ scal, int step) {
    if (scal && solve_done(scal, step)) return;
    double dot[K];
#pragma unroll
    for (int c = 0; c < K; ++c) dot[c] = 0.0;
    for (int64_t p = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; p < npatch; p += int64_t(gridDim.x) * blockDim.x)
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] += ppart[p * K + c];
    __shared__ double smem[16 * K];
    block_sum<K>(dot, smem);
    if (threadIdx.x < K) part[blockIdx.x * K + threadIdx.x] = pick<K>(dot, threadIdx.x);
}

long long *g_patch_stamps = nullptr;   // mode 4: device buffer [grid][8] of phase time stamps (remo_debug_patch_phases)

}  // namespace

void set_patch_stamps(long long *buf) { g_patch_stamps = buf; }

#ifdef REMO_PROBES
#include "patch_persist.inc"     // keys 34 and 35: k_patch_apply_p / k_patch_apply_r and launch_patch_persistent
#endif

// one lane per (element, right-hand side) and round; at most 204 elements (the table builder sorts 20 slots per element in 32 KB of LDS)
constexpr int kPatchMaxElements = 204;   // 204 x 20 slots sort in 4096 LDS keys (and fit the 13-bit slot field of a key)
// rounds of a patch: two where 2 * (256 / kmax) elements fit the table builder (kmax >= 3)
int patch_rounds(int kmax, int wanted) { return (wanted >= 2 && 2 * (kPatchBlock / (kmax > 0 ? kmax : 1)) <= kPatchMaxElements) ? 2 : 1; }
int patch_elements_per_group(int kmax, int rounds) {
    const int e = rounds * (kPatchBlock / (kmax > 0 ? kmax : 1));
    return e < kPatchMaxElements ? e : kPatchMaxElements;
}

size_t patch_arena_bytes(int64_t nt, int64_t n_max, int kmax) {
    size_t most = 0;
    for (int rounds = 1; rounds <= 2; ++rounds) {      // whichever the batch gets (a batch that falls back to one round reuses the room)
        const int E = patch_elements_per_group(kmax, patch_rounds(kmax, rounds));
        const int64_t npatch = (nt + E - 1) / E;
        const int64_t cap = int64_t(E) * 20;
        const size_t b = size_t(nt) * 40 + size_t(npatch) * (16 + 12 * size_t(cap)) + size_t(n_max + 2) * 8 + size_t(n_max + 1) * 16 + size_t(npatch) * 8 * 8 + (1 << 20);
        most = b > most ? b : most;
    }
    return most;
}

// Everything is enqueued on s; flag_and_max (device, two ints) must be read by the caller after its next synchronisation:
// [0] != 0 -> a patch has more distinct rows than the tables hold (the caller builds tables of one round instead of two, or, with
// one round, falls back to another operator), [1] = the largest row count (sizes the kernel's LDS).
void build_patch_tables(Arena &ar, hipStream_t s, const DeviceSymbolic &sy, const double *C, int kmax, int rounds, PatchTables &out, int32_t *flag_and_max) {
    out = PatchTables{};
    const int64_t nt = sy.nt, n = sy.nfree;
    rounds = patch_rounds(kmax, rounds);
    const int E = patch_elements_per_group(kmax, rounds);
    out.rounds = rounds;
    // rows a patch may hold: what fits the LDS budget of one workgroup (48 KB of k-wide fp64 rows), at most every dof distinct
    int rows_cap = int((48 * 1024) / (size_t(kmax) * 8)) - 2;
    if (rows_cap > E * 20) rows_cap = E * 20;
    int npad = 256;
    while (npad < E * 20) npad <<= 1;
    out.nt = nt; out.n = n; out.E = E; out.rows_cap = rows_cap; out.spread = g_tune.patch_spread; out.trim = g_tune.patch_trim;
    // constants, kept for the layout of the kernels' by-value argument (kernels.h): threads per workgroup, every row through the slab, no stagger
    out.block = kPatchBlock; out.all_slab = 1; out.stagger = 0;
    out.npatch = (nt + E - 1) / E;
    out.C = C;
    uint16_t *lidx = ar.lo<uint16_t>(size_t(nt) * 20 + 8);
    int32_t *pcount = ar.lo<int32_t>(size_t(out.npatch) + 1);
    int32_t *prow = ar.lo<int32_t>(size_t(out.npatch) * rows_cap + 1);
    int32_t *pout = ar.lo<int32_t>(size_t(out.npatch) * rows_cap + 1);
    int32_t *bptr = ar.lo<int32_t>(size_t(n) + 2);
    out.nslot_cap = out.npatch * int64_t(rows_cap) < nt * 20 ? out.npatch * int64_t(rows_cap) : nt * 20;
    int32_t *bslot = ar.lo<int32_t>(size_t(out.nslot_cap) + 2);
    int32_t *row4 = ar.lo<int32_t>(size_t(n) * 4 + 4);
    (void)hipMemsetAsync(row4, 0xFF, sizeof(int32_t) * size_t(n) * 4, s);
    const size_t mark = ar.hi_mark();
    int32_t *bcnt = ar.hi<int32_t>(size_t(n) + 2);
    int32_t *pboff = ar.lo<int32_t>(size_t(out.npatch) + 2);
    int32_t *pbcnt = ar.hi<int32_t>(size_t(out.npatch) + 2);
    (void)hipMemsetAsync(flag_and_max, 0, 3 * sizeof(int32_t), s);
    (void)hipMemsetAsync(prow, 0xFF, sizeof(int32_t) * (size_t(out.npatch) * rows_cap + 1), s);   // -1 behind a patch's last row
    (void)hipMemsetAsync(pbcnt + out.npatch, 0, sizeof(int32_t), s);
    hipLaunchKernelGGL(k_patch_row_slots, dim3(int((n + 1 + 255) / 256)), dim3(256), 0, s, n, E, sy.adjptr, sy.adj, bcnt);
    hipLaunchKernelGGL(k_patch_build, dim3(int(out.npatch)), dim3(256), size_t(npad) * 8, s, nt, E, rows_cap, npad, sy.eldof, lidx, pcount, pbcnt,
                       prow, flag_and_max, flag_and_max + 1);
    size_t tb1 = 0, tb2 = 0;
    (void)rocprim::exclusive_scan(nullptr, tb1, bcnt, bptr, int32_t(0), size_t(n + 1), rocprim::plus<int32_t>(), s);
    (void)rocprim::exclusive_scan(nullptr, tb2, pbcnt, pboff, int32_t(0), size_t(out.npatch + 1), rocprim::plus<int32_t>(), s);
    void *tmp = ar.hi<char>((tb1 > tb2 ? tb1 : tb2) + 256);
    (void)rocprim::exclusive_scan(tmp, tb1, bcnt, bptr, int32_t(0), size_t(n + 1), rocprim::plus<int32_t>(), s);
    (void)rocprim::exclusive_scan(tmp, tb2, pbcnt, pboff, int32_t(0), size_t(out.npatch + 1), rocprim::plus<int32_t>(), s);
    hipLaunchKernelGGL(k_patch_zero_rows, dim3(1024), dim3(256), 0, s, nt * 20, lidx, (const int32_t *)(flag_and_max + 1));
    hipLaunchKernelGGL(k_patch_slots, dim3(int(out.npatch)), dim3(256), 0, s, E, rows_cap, (const int32_t *)pcount, (const int32_t *)pboff, (const int32_t *)prow, pout,
                       sy.adjptr, sy.adj, (const int32_t *)bptr, bslot, row4);
    (void)hipMemcpyAsync(flag_and_max + 2, pboff + out.npatch, sizeof(int32_t), hipMemcpyDeviceToDevice, s);   // slab slots in use (blocks padded to 16 rows)
    ar.hi_release(mark);     // the stream orders later users of this scratch behind these launches
    out.lidx = lidx; out.pcount = pcount; out.prow = prow; out.pout = pout; out.pboff = pboff; out.row4 = row4; out.bptr = bptr; out.bslot = bslot;
}

template <class T, int K> static void patch_dispatch(const CsrViewT<T> &A, const T *x, T *y, double *part, const double *scal, int step, int nb, hipStream_t s, bool defer) {
    const PatchOpT<T> &P = *A.patch;
    const PatchTables &tb = P.t;
    const int64_t per = (tb.npatch + 7) / 8;
    double *pp = part ? P.ppart : nullptr;
    double *bins = (part && defer && P.dot_bins) ? part + (step & 1) * (kPqBins * 8) : nullptr;
    auto launch = [&](auto kernel) {
        const size_t bytes = patch_lds_bytes(P.lds_rows, K);   // staged rows, later fp64 accumulators
        hipLaunchKernelGGL(kernel, dim3(int(per * 8)), dim3(kPatchBlock), bytes, s, tb, P.lds_rows, x, y, P.Yb, pp, scal, step, g_patch_stamps, bins);
    };
    bool launched = false;
#ifdef REMO_PROBES      // persistent forms, ablations (wrong results on purpose), the phase probe, the other arithmetic order: tools/ builds only (make probes)
    const int mode = g_tune.patch_mode, lean = g_tune.patch_lean;
    launched = launch_patch_persistent<T, K>(P, mode, g_patch_stamps, x, y, pp, scal, step, bins, s);
    if constexpr (K == 5) {     // ablations and the phase probe (tools/probe_patch.py); one-round tables only
        if (!launched && tb.rounds == 1 && mode >= 1 && mode <= 3 + (g_patch_stamps ? 1 : 0)) {
            launched = true;
            if (mode == 1) launch(k_patch_apply<T, 5, 1>);
            else if (mode == 2) launch(k_patch_apply<T, 5, 2>);
            else if (mode == 3) launch(k_patch_apply<T, 5, 3>);
            else launch(k_patch_apply<T, 5, 4>);
        }
    }
    // remo_debug_tune key 26: the register-lean order of the kernel's arithmetic phase (k_patch_apply LEAN): -1 = in fp32 storage only
    // (default), 0 = never, 1 = always.  fp32: 72-80 registers against 104 at first (111 against 124 us at 443 k tetrahedra); once the
    // staging / output phases had their pass count as a compile-time constant the plain order needed 67 registers by itself and was
    // level at 443 k tetrahedra (87 against 90 us) but not on the batches of the headline sweep (370 k / 320 k: 86 against 77 us, solve
    // 158.3 against 153.1 ms per four batches): lean stays the fp32 default.  fp64: 96 registers with spills, five waves: 160 against 156 us.
    if (!launched && tb.rounds == 1 && ((lean == 1) != (sizeof(T) == 4)) && lean >= 0) {     // the other order than the product's
        if (sizeof(T) == 4) launch(k_patch_apply<T, K, 0>); else launch(k_patch_apply<T, K, 0, true>);
        launched = true;
    }
#endif
    // the product: plain order in fp64 (124 registers, four waves per SIMD; two rounds: 146 registers, three waves - a size-L batch's
    // 40 KB of LDS allow three workgroups per CU anyway), register-lean order in fp32 storage (seven)
    if (!launched) {
        if constexpr (sizeof(T) == 4) {
            if (tb.rounds != 1) throw std::logic_error("patch operator: tables of two rounds in fp32 storage (they are built for fp64 solves only)");
            launch(k_patch_apply<T, K, 0, true>);
        } else {
            if (tb.rounds == 2) launch(k_patch_apply<T, K, 0, false, 2>);
            else launch(k_patch_apply<T, K, 0>);
        }
    }
    if (bins) return;     // the patches have added their sums into the update launch's rows themselves
    if (part && defer) {
        // (a few workgroups: the rows of `part` behind them stay zero - cleared by the solver once per solve)
        hipLaunchKernelGGL(k_patch_dot<K>, dim3(nb < kPatchDotBlocks ? nb : kPatchDotBlocks), dim3(256), 0, s, tb.npatch, (const double *)P.ppart, part, scal, step);
        return;
    }
    if (part) hipLaunchKernelGGL((k_patch_reduce<T, K, true>), dim3(nb), dim3(256), 0, s, A.n, tb.npatch, tb.bptr, tb.bslot, (const T *)P.Yb, y, (const double *)P.ppart, part, scal, step);
    else hipLaunchKernelGGL((k_patch_reduce<T, K, false>), dim3(nb), dim3(256), 0, s, A.n, tb.npatch, tb.bptr, tb.bslot, (const T *)P.Yb, y, (const double *)nullptr, part, scal, step);
}

template <class T> void launch_patch_spmm(const CsrViewT<T> &A, int k, const T *x, T *y, double *part, const double *scal, int nb, hipStream_t s, int step, bool defer) {
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; patch_dispatch<T, K>(A, x, y, part, scal, step, nb, s, defer); });
}
// The PCG's product with the search direction in fp32 storage (PcgBuffersT::p32): the shared rows stay in the slab (defer_q), the
// patches' <p, A p> go where launch_patch_spmm puts them.  The tables' own kernel or none: a batch the patch operator does not take
// never gets an fp32 direction (batch_run.hip set_launch_shape).
template <int K> static void patch_dispatch_x32(const CsrViewT<double> &A, const float *x, double *part, const double *scal, int step, int nb, hipStream_t s) {
    const PatchOpT<double> &P = *A.patch;
    const PatchTables &tb = P.t;
    const int64_t per = (tb.npatch + 7) / 8;
    double *bins = P.dot_bins ? part + (step & 1) * (kPqBins * 8) : nullptr;
    const size_t bytes = patch_lds_bytes(P.lds_rows, K);
    if (tb.rounds == 2)
        hipLaunchKernelGGL((k_patch_apply<double, K, 0, false, 2, float>), dim3(int(per * 8)), dim3(kPatchBlock), bytes, s, tb, P.lds_rows, x, (double *)nullptr, P.Yb, P.ppart, scal, step, (long long *)nullptr, bins);
    else
        hipLaunchKernelGGL((k_patch_apply<double, K, 0, false, 1, float>), dim3(int(per * 8)), dim3(kPatchBlock), bytes, s, tb, P.lds_rows, x, (double *)nullptr, P.Yb, P.ppart, scal, step, (long long *)nullptr, bins);
    if (!bins) hipLaunchKernelGGL(k_patch_dot<K>, dim3(nb < kPatchDotBlocks ? nb : kPatchDotBlocks), dim3(256), 0, s, tb.npatch, (const double *)P.ppart, part, scal, step);
}

void launch_patch_spmm_x32(const CsrViewT<double> &A, int k, const float *x, double *part, const double *scal, int nb, hipStream_t s, int step) {
    if (!patch_applies(A, k) || !part) throw std::logic_error("patch operator on an fp32 direction: no patch tables for this batch");
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; patch_dispatch_x32<K>(A, x, part, scal, step, nb, s); });
}

template void launch_patch_spmm<double>(const CsrViewT<double> &, int, const double *, double *, double *, const double *, int, hipStream_t, int, bool);
template void launch_patch_spmm<float>(const CsrViewT<float> &, int, const float *, float *, double *, const double *, int, hipStream_t, int, bool);

}  // namespace remo
