// patch_persist.inc — the two PERSISTENT forms of the patch kernel: measured, parity-green, not faster (DESIGN.md section 8).
// Included once by patch.hip, at namespace scope behind k_patch_apply, in builds with -DREMO_PROBES only (make probes: tools/ and
// tests/test_gpu_parity.py::test_persistent_patch_kernel_is_the_same_operator); the product library holds none of it.
// patch.hip sees one function of this file: launch_patch_persistent (at its end).

namespace {

// ---- apply, persistent form --------------------------------------------------------------------------------------------------
// The kernel above is a chain of dependent memory round trips per workgroup: row tables, then x rows, then arithmetic, then stores;
// four workgroups per CU overlap each other's waits only partly (a workgroup spent 11 k of its 27 k cycles waiting for the two trips).
// Here a workgroup is PERSISTENT: it walks a contiguous run of patches (XCD-contiguous like the launch above), and everything patch
// i + 1 needs - its x rows, its row tables (i + 2: the row numbers are the addresses of the x rows), local indices and metric terms of
// its elements - travels while patch i is being computed, by LDS-DMA (`global_load_lds_dword`: per-lane global address, consecutive LDS
// words; no registers hold the data, so the arithmetic phase keeps its register budget):
//   LDS: two row images of (R + 1) k-wide fp64 rows (the image of patch i becomes its accumulators once its values are in
//        registers, the other one fills with patch i + 1), three slots of row numbers, two of slab slots, two of element data.
//   per patch: [zero row] barrier | issue the DMA of patch i + 1 (and the row numbers of i + 2) | x values into registers | barrier |
//        clear accumulators | barrier | tensor chains + ds_add_f64 | s_waitcnt vmcnt(0) (the DMA issued a whole arithmetic phase ago
//        and the stores of patch i - 1) | barrier | rows out (y or slab) - no wait on memory anywhere but that one, long satisfied.
// <x, A x> is kept in a register across the patches of the workgroup and leaves it once, at the end.
// R = the batch's largest row count; the image is sized by it, so two (small patches: three) workgroups share a CU's 160 KB.
#ifndef REMO_STAMP_WAVE
#define REMO_STAMP_WAVE 0        /* which wave of a persistent workgroup reports its phase clocks (probe builds) */
#endif
typedef const void __attribute__((address_space(1))) *dma_src_t;
typedef void __attribute__((address_space(3))) *dma_dst_t;

inline size_t patch_lds_bytes_p(int R, int K, int E) {
    const size_t Rp = size_t((R + 63) & ~63);
    return size_t(2) * size_t(R + 1) * size_t(K) * 8 + 5 * Rp * 4 + 2 * (size_t(E) * 40 + size_t(E) * 48) + 64;
}

// Workgroup barrier that waits for this wave's LDS operations only.  __syncthreads() is fence + barrier, and the fence drains the
// vector-memory counter too (`s_waitcnt vmcnt(0) lgkmcnt(0)` in the ISA): inside the persistent loop that would wait, at the first
// barrier of a patch, for the stores of the patch before it and, at the second, for the LDS-DMA just issued for the next one -
// exactly the two round trips the loop exists to hide (measured: 7.5 k of 20.6 k clock ticks per patch sat in that first barrier).
// Data that crosses the barrier here lives in LDS (ordered by lgkmcnt(0)); what the DMA brings is ordered by the explicit
// `s_waitcnt vmcnt(0)` before barrier B3; nothing a wave stores to global memory is read by another wave of the launch.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class T, int K, bool STAMP = false>
__global__ void __launch_bounds__(256, 2) k_patch_apply_p(PatchTables tb, int R, const T *__restrict__ x, T *__restrict__ y, T *__restrict__ Yb,
                                                          double *__restrict__ ppart, const double *__restrict__ scal, int step, double *__restrict__ pbins,
                                                          long long *__restrict__ stamps) {
    if (scal && solve_done(scal, step)) return;
    // STAMP (probe builds, remo_debug_patch_phases): wave 0 sums the clock ticks of every phase over the workgroup's patches
    long long ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tk = 0;
#define REMO_PH(k) if constexpr (STAMP) { const long long now_ = __builtin_readcyclecounter(); ph[k] += now_ - tk; tk = now_; }
    constexpr int BLK = 256, EK = BLK / K, U = kPatchPasses;
    constexpr uint32_t S = sizeof(T);
    constexpr int DPR = int(K * S / 4);                  // 4-byte words of a staged row
    extern __shared__ double lds_raw[];
    __shared__ double smem[16 * K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Rp = (R + 63) & ~63;
    const int E = tb.E;
    double *const Xb0 = lds_raw, *const Xb1 = lds_raw + size_t(R + 1) * K;
    int32_t *const trow0 = reinterpret_cast<int32_t *>(lds_raw + size_t(2) * size_t(R + 1) * K);   // [3][Rp]
    int32_t *const tout0 = trow0 + 3 * Rp;                                                          // [2][Rp]
    uint32_t *const eli0 = reinterpret_cast<uint32_t *>(tout0 + 2 * Rp);                             // [2][E * 10]: local rows, two per word
    double *const ecm0 = reinterpret_cast<double *>(eli0 + 2 * E * 10);                             // [2][E * 6]: metric terms
    // this workgroup's run of patches: XCD b & 7 owns one contiguous eighth of the list (neighbouring patches share boundary rows:
    // the second reader finds them in that L2), its workgroups contiguous runs of the eighth
    const int64_t per = (tb.npatch + 7) >> 3;
    const int64_t xb = int64_t(blockIdx.x & 7) * per, xe = (xb + per < tb.npatch) ? xb + per : tb.npatch;
    const int64_t cnt = xe > xb ? xe - xb : 0;
    const int64_t nwx = int64_t(gridDim.x >> 3), w = int64_t(blockIdx.x >> 3);
    const int64_t share = cnt / nwx, extra = cnt % nwx;
    const int64_t p0_ = xb + w * share + (w < extra ? w : extra);
    // (patch numbers in scalar registers: the row counts of the patches ahead are then scalar loads - a vector load here would be waited
    // for on the spot, together with every store still in flight)
    const int p0 = __builtin_amdgcn_readfirstlane(int(p0_)), p1 = __builtin_amdgcn_readfirstlane(int(p0_ + share + (w < extra ? 1 : 0)));
    if (p0 >= p1) return;                                 // (the whole workgroup)

    // `ndw` consecutive 4-byte words from src to LDS at dst (both wave-uniform), 64 words per wave instruction
    auto dma_copy = [&](const uint32_t *src, uint32_t *dst, int ndw) {
        for (int t = wave; t * 64 < ndw; t += 4) {
            const int j = t * 64 + lane;
            if (j < ndw) __builtin_amdgcn_global_load_lds((dma_src_t)(src + j), (dma_dst_t)(dst + t * 64), 4, 0, 0);
        }
    };
    // the same in 16-byte pieces (1 KB per wave instruction) for sources and destinations aligned to 16 bytes; the tail in 4-byte words
    auto dma_copy16 = [&](const uint32_t *src, uint32_t *dst, int ndw) {
        const int n16 = ndw >> 2;
        for (int t = wave; t * 64 < n16; t += 4) {
            const int j = t * 64 + lane;
            if (j < n16) __builtin_amdgcn_global_load_lds((dma_src_t)(src + 4 * j), (dma_dst_t)(dst + t * 256), 16, 0, 0);
        }
        const int tail = ndw & 3;
        if (wave == 3 && lane < tail) __builtin_amdgcn_global_load_lds((dma_src_t)(src + 4 * n16 + lane), (dma_dst_t)(dst + 4 * n16), 4, 0, 0);
    };
    // the k-wide x rows named by rowtab[0 .. rows) into the image X: word d of the image = word d % DPR of row rowtab[d / DPR].
    // The row numbers of UN pieces are read from LDS together, then the UN pieces leave back to back: one piece at a time, its row
    // number's LDS latency in front of every instruction, cost a wave ~300 clock ticks per piece (7 k ticks per patch: measured)
    auto dma_rows = [&](const int32_t *rowtab, double *X, int rows) {
        const int ndw = rows * DPR;
        const uint32_t *xw = reinterpret_cast<const uint32_t *>(x);
        constexpr int UN = 6;
        for (int t0 = wave; t0 * 64 < ndw; t0 += 4 * UN) {
            uint32_t r[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int d = (t0 + 4 * u) * 64 + lane;
                const int m = int(uint32_t(d) / uint32_t(DPR));
                r[u] = uint32_t(rowtab[m < rows ? m : rows - 1]);
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int t = t0 + 4 * u, d = t * 64 + lane;
                if (d < ndw) {
                    const int m = int(uint32_t(d) / uint32_t(DPR));
                    const uint32_t rr = r[u] < uint32_t(tb.n) ? r[u] : 0u;     // (never out of range by construction; a source address must not depend on that)
                    __builtin_amdgcn_global_load_lds((dma_src_t)(xw + size_t(rr) * DPR + (d - m * DPR)),
                                                     (dma_dst_t)(reinterpret_cast<uint32_t *>(X) + t * 64), 4, 0, 0);
                }
            }
        }
    };
    auto dma_elem = [&](int p, int slot) {
        const int64_t e0 = int64_t(p) * E;
        const int ne = int(tb.nt - e0 < E ? tb.nt - e0 : E);
        dma_copy(reinterpret_cast<const uint32_t *>(tb.lidx + e0 * 20), eli0 + slot * E * 10, ne * 10);
        dma_copy16(reinterpret_cast<const uint32_t *>(tb.C + e0 * 6), reinterpret_cast<uint32_t *>(ecm0 + slot * E * 6), ne * 12);
    };
    const bool tab16 = (tb.rows_cap & 3) == 0;          // a patch's tables start on 16 bytes
    auto dma_tab = [&](const uint32_t *src, uint32_t *dst, int n) { if (tab16) dma_copy16(src, dst, n); else dma_copy(src, dst, n); };
    auto prow_of = [&](int p) { return reinterpret_cast<const uint32_t *>(tb.prow + int64_t(p) * tb.rows_cap); };
    auto pout_of = [&](int p) { return reinterpret_cast<const uint32_t *>(tb.pout + int64_t(p) * tb.rows_cap); };
    auto clampR = [&](int c) { return c < R ? c : R; };

    // (the row counts through the constant address space: invariant during the launch, so the loads are scalar loads even behind stores)
    typedef const int32_t __attribute__((address_space(4))) *cint_t;
    const cint_t pcnt = (cint_t)tb.pcount;
    int rows_cur = clampR(pcnt[p0]);
    int rows_nxt = (p0 + 1 < p1) ? clampR(pcnt[p0 + 1]) : 0;
    // prologue: tables of the first two patches and the element data of the first, then the first patch's rows (the only exposed trips)
    dma_tab(prow_of(p0), reinterpret_cast<uint32_t *>(trow0), rows_cur);
    dma_tab(pout_of(p0), reinterpret_cast<uint32_t *>(tout0), rows_cur);
    if (p0 + 1 < p1) dma_tab(prow_of(p0 + 1), reinterpret_cast<uint32_t *>(trow0 + Rp), rows_nxt);
    dma_elem(p0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    dma_rows(trow0, Xb0, rows_cur);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    const int el = tid / K, c0 = tid - el * K;
    const int32_t off_mask = tid < EK * K ? 0 : int32_t(0x80000000);
    const int Rr = tb.spread > 1 ? tb.spread : 1;
    const int run = el % Rr, rbase = E / Rr, rextra = E % Rr;
    const int elp = Rr > 1 ? (run * rbase + (run < rextra ? run : rextra) + el / Rr) : el;
    const rsrc_t ry = make_rsrc(y, uint64_t(tb.n) * K * S), rb = make_rsrc(Yb, uint64_t(tb.nslot_cap) * K * S);
    // y and the slab are two ranges of one arena: when both fit one buffer descriptor (4 GB of byte offsets) a value needs ONE store
    // instruction with the destination chosen by offset, not two of which the hardware drops one - the output phase is bound by the
    // ISSUE of its stores (the waves of a workgroup queue behind each other in it)
    const char *const lo_ = reinterpret_cast<const char *>(y) < reinterpret_cast<const char *>(Yb) ? reinterpret_cast<const char *>(y) : reinterpret_cast<const char *>(Yb);
    const uint64_t y_off64 = uint64_t(reinterpret_cast<const char *>(y) - lo_), b_off64 = uint64_t(reinterpret_cast<const char *>(Yb) - lo_);
    const uint64_t span = (y_off64 + uint64_t(tb.n) * K * S > b_off64 + uint64_t(tb.nslot_cap) * K * S) ? y_off64 + uint64_t(tb.n) * K * S : b_off64 + uint64_t(tb.nslot_cap) * K * S;
    const bool one_desc = span < 0xFFFFF000ull;
    const rsrc_t rboth = make_rsrc(lo_, one_desc ? span : 0);
    const uint32_t y_off = uint32_t(y_off64), b_off = uint32_t(b_off64);
    double d0 = 0.0;
    int slot3 = 0;                                        // slot of the current patch's row numbers (patch number mod 3, without the division)
    for (int p = p0; p < p1; ++p) {
        const int it = p - p0;
        double *const Xc = (it & 1) ? Xb1 : Xb0, *const Xn = (it & 1) ? Xb0 : Xb1;
        T *const xs = reinterpret_cast<T *>(Xc);
        const int s1 = slot3 == 2 ? 0 : slot3 + 1, s2 = s1 == 2 ? 0 : s1 + 1;
        int32_t *const trow_c = trow0 + slot3 * Rp, *const trow_n = trow0 + s1 * Rp, *const trow_nn = trow0 + s2 * Rp;
        int32_t *const tout_c = tout0 + (it & 1) * Rp, *const tout_n = tout0 + ((it + 1) & 1) * Rp;
        const int rows_nn = (p + 2 < p1) ? clampR(pcnt[p + 2]) : 0;           // (a scalar load: wanted at the next turn)
        if constexpr (STAMP) tk = __builtin_readcyclecounter();
        if (tid < K) xs[R * K + tid] = T(0);              // the row constrained dofs read
        if constexpr (STAMP) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); REMO_PH(9) }      // (probe: this wave's own LDS / scalar operations, apart from the barrier)
        lds_barrier();                                   // B0: X(p) is in LDS (every wave waited for its pieces); the other image and the oldest table slots are free
        REMO_PH(0)                                          // barrier B0
        if (p + 1 < p1) {
            dma_rows(trow_n, Xn, rows_nxt);
            dma_tab(pout_of(p + 1), reinterpret_cast<uint32_t *>(tout_n), rows_nxt);
            dma_elem(p + 1, (it + 1) & 1);
        }
        if (p + 2 < p1) dma_tab(prow_of(p + 2), reinterpret_cast<uint32_t *>(trow_nn), rows_nn);
        REMO_PH(1)                                          // DMA issue
        const int64_t e = int64_t(p) * E + elp;
        const bool active = el < E && e < tb.nt;
        const uint32_t *const eli = eli0 + (it & 1) * E * 10 + elp * 10;
        const double *const ecm = ecm0 + (it & 1) * E * 6 + elp * 6;
        uint32_t li[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) li[q] = active ? eli[q] : 0u;
#define REMO_PATCH_L(i) ((li[(i) >> 1] >> (16 * ((i) & 1))) & 0xFFFFu)
        T xv[20];
#pragma unroll
        for (int i = 0; i < 20; ++i) xv[i] = xs[REMO_PATCH_L(i) * K + c0];
        REMO_PH(2)                                          // x values into registers
        lds_barrier();                                   // B1: every lane holds its x values: the image becomes the accumulators
        REMO_PH(3)
        double *const ya = Xc;
        for (int j = tid; j < rows_cur * K; j += BLK) ya[j] = 0.0;
        if (tid < K) ya[R * K + tid] = 0.0;
        lds_barrier();                                   // B2
        REMO_PH(4)                                          // clearing + B2
        if (active) {
            double cm[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) cm[q] = ecm[q];
            const T c11 = T(cm[0]), c12 = T(cm[1]), c13 = T(cm[2]), c22 = T(cm[3]), c23 = T(cm[4]), c33 = T(cm[5]);
            T g[30], yv[20];
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
            d0 += double(dd);
            REMO_ELEM_DIV(T, g, yv, tdiv)
#pragma unroll
            for (int i = 0; i < 20; ++i) lds_add(ya + REMO_PATCH_L(i) * K + c0, double(yv[i]));
        }
#undef REMO_PATCH_L
        REMO_PH(5)                                          // tensor chains + LDS accumulation
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of patch p + 1 (issued an arithmetic phase ago) and its stores of patch p - 1
        REMO_PH(6)                                          // wait for the DMA / older stores
        lds_barrier();                                   // B3: accumulators complete; X(p + 1), tables and element data of p + 1 in LDS
        REMO_PH(7)
        auto rows_out = [&](auto one_c) {
            constexpr bool ONE_STORE = decltype(one_c)::value;
            auto put = [&](auto np_c, int m0) {
                constexpr int NP = decltype(np_c)::value;
                int32_t r[NP], o[NP];
                T v[NP][1];
#pragma unroll
                for (int u = 0; u < NP; ++u) {
                    const int m = m0 + el + EK * u;
                    const bool in = m < rows_cur;
                    r[u] = (in ? trow_c[m] : -1) | off_mask; o[u] = in ? tout_c[m] : -1;
                    v[u][0] = T(ya[(in ? m : 0) * K + c0]);
                }
#pragma unroll
                for (int u = 0; u < NP; ++u) {
                    if constexpr (ONE_STORE) {      // ONE store per value: y and the slab through one descriptor (base = the lower of the two)
                        const bool have = r[u] >= 0;
                        const uint32_t off = o[u] < 0 ? y_off + __umul24(uint32_t(r[u]), K * S) : b_off + __umul24(uint32_t(o[u]), K * S);
                        buf_store<T, 1>(rboth, have ? off + uint32_t(c0) * S : kOutOfRange, v[u]);
                    } else {                        // one of the two stores of a value is out of range: dropped by the hardware, no branch
                        const bool have = r[u] >= 0;
                        buf_store<T, 1>(ry, (have && o[u] < 0) ? __umul24(uint32_t(r[u]), K * S) + uint32_t(c0) * S : kOutOfRange, v[u]);
                        buf_store<T, 1>(rb, (have && o[u] >= 0) ? __umul24(uint32_t(o[u]), K * S) + uint32_t(c0) * S : kOutOfRange, v[u]);
                    }
                }
            };
            const int npass = (rows_cur + EK - 1) / EK;
            switch (npass) {
                case 1: put(std::integral_constant<int, 1>{}, 0); break;   case 2: put(std::integral_constant<int, 2>{}, 0); break;
                case 3: put(std::integral_constant<int, 3>{}, 0); break;   case 4: put(std::integral_constant<int, 4>{}, 0); break;
                case 5: put(std::integral_constant<int, 5>{}, 0); break;   case 6: put(std::integral_constant<int, 6>{}, 0); break;
                case 7: put(std::integral_constant<int, 7>{}, 0); break;   case 8: put(std::integral_constant<int, 8>{}, 0); break;
                case 9: put(std::integral_constant<int, 9>{}, 0); break;   case 10: put(std::integral_constant<int, 10>{}, 0); break;
                case 11: put(std::integral_constant<int, 11>{}, 0); break; case 12: put(std::integral_constant<int, 12>{}, 0); break;
                default:
                    for (int m0 = 0; m0 < rows_cur; m0 += U * EK) put(std::integral_constant<int, U>{}, m0);
            }
        };
        if (one_desc) rows_out(std::true_type{}); else rows_out(std::false_type{});
        REMO_PH(8)                                          // rows out
        rows_cur = rows_nxt; rows_nxt = rows_nn;
        slot3 = s1;
    }
    if constexpr (STAMP) {
        if (tid == 64 * REMO_STAMP_WAVE) {
            for (int k = 0; k < 10; ++k) stamps[int64_t(blockIdx.x) * 12 + k] = ph[k];
            stamps[int64_t(blockIdx.x) * 12 + 10] = p1 - p0;
        }
    }
#undef REMO_PH
    if (ppart) {
        double dot[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] = (c == c0) ? d0 : 0.0;
        const double mine = block_sum_column<K>(dot, smem);
        if (tid < K) {
            if (pbins) (void)__hip_atomic_fetch_add(pbins + (blockIdx.x % kPqBins) * K + tid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else ppart[int64_t(p0) * K + tid] = mine;
        }
        if (!pbins)      // one row of sums per PATCH is what the folding launches read: this workgroup's other patches contribute zero
            for (int64_t j = tid; j < int64_t(p1 - p0 - 1) * K; j += BLK) ppart[int64_t(p0 + 1) * K + j] = 0.0;
    }
}

// ---- apply, persistent form with the prefetch through REGISTERS ----------------------------------------------------------------
// Same idea as k_patch_apply_p - a workgroup walks a run of patches and fetches patch i + 1 while it computes patch i - with
// what the LDS-DMA version taught: the DMA instructions cost a wave ~240 ticks each to issue (25 per patch) and the second row
// image halves the workgroups per CU.  Here the next patch's x rows are ordinary buffer loads into registers (one value per lane and
// pass, up to 12 in flight: 24 VGPRs in fp64), issued before the tensor chains and written into the ONE row image once the
// current patch's results have been read out of it; row tables travel the same way one patch further ahead, the element's local
// rows and metric terms are requested behind the chains (their registers are free then) for the next turn.  LDS: one image + two
// slots of tables (~32 KB: the register budget - three waves per SIMD - decides the residency, not LDS).  Barriers wait for LDS
// only (lds_barrier): a wave never waits for memory except where the compiler counts the loads it needs next.
inline size_t patch_lds_bytes_r(int R, int K, int E) {
    const size_t Rp = size_t((R + 255) & ~255);
    return size_t(R + 2) * size_t(K) * 8 + 4 * Rp * 4 + size_t(E) * 88 + 64;
}

template <class T, int K, bool STAMP = false>
__global__ void __launch_bounds__(256, 3) k_patch_apply_r(PatchTables tb, int R, const T *__restrict__ x, T *__restrict__ y, T *__restrict__ Yb,
                                                          double *__restrict__ ppart, const double *__restrict__ scal, int step, double *__restrict__ pbins,
                                                          long long *__restrict__ stamps) {
    if (scal && solve_done(scal, step)) return;
    long long ph[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tk = 0;
#define REMO_PH(k) if constexpr (STAMP) { const long long now_ = __builtin_readcyclecounter(); ph[k] += now_ - tk; tk = now_; }
    constexpr int BLK = 256, EK = BLK / K, U = kPatchPasses, TJ = 4;     // TJ table words per lane: up to 1024 rows
    constexpr uint32_t S = sizeof(T);
    extern __shared__ double lds_raw[];
    __shared__ double smem[16 * K];
    const int tid = threadIdx.x;
    const int Rp = (R + 255) & ~255;
    const int E = tb.E;
    double *const ya = lds_raw;                                          // [(R + 2)][K] fp64 accumulators; the same bytes hold the x image (T) before
    T *const xs = reinterpret_cast<T *>(lds_raw);
    int32_t *const trow0 = reinterpret_cast<int32_t *>(lds_raw + size_t(R + 2) * K);   // [2][Rp]
    int32_t *const tout0 = trow0 + 2 * Rp;                                              // [2][Rp]
    double *const ecm = reinterpret_cast<double *>(tout0 + 2 * Rp);                    // [E][6] metric terms of the current patch's elements
    uint32_t *const eli = reinterpret_cast<uint32_t *>(ecm + size_t(E) * 6);           // [E][10] their local rows, two per word
    const int64_t per = (tb.npatch + 7) >> 3;
    const int64_t xb = int64_t(blockIdx.x & 7) * per, xe = (xb + per < tb.npatch) ? xb + per : tb.npatch;
    const int64_t cnt = xe > xb ? xe - xb : 0;
    const int64_t nwx = int64_t(gridDim.x >> 3), w = int64_t(blockIdx.x >> 3);
    const int64_t share = cnt / nwx, extra = cnt % nwx;
    const int64_t p0_ = xb + w * share + (w < extra ? w : extra);
    const int p0 = __builtin_amdgcn_readfirstlane(int(p0_)), p1 = __builtin_amdgcn_readfirstlane(int(p0_ + share + (w < extra ? 1 : 0)));
    if (p0 >= p1) return;                                 // (the whole workgroup)
    typedef const int32_t __attribute__((address_space(4))) *cint_t;
    const cint_t pcnt = (cint_t)tb.pcount;
    auto clampR = [&](int c) { return c < R ? c : R; };

    const int el = tid / K, c0 = tid - el * K;
    const int32_t off_mask = tid < EK * K ? 0 : int32_t(0x80000000);
    const int Rr = tb.spread > 1 ? tb.spread : 1;
    const int run = el % Rr, rbase = E / Rr, rextra = E % Rr;
    const int elp = Rr > 1 ? (run * rbase + (run < rextra ? run : rextra) + el / Rr) : el;
    const bool has_el = el < E;
    const rsrc_t rx = make_rsrc(x, uint64_t(tb.n) * K * S);
    const rsrc_t ry = make_rsrc(y, uint64_t(tb.n) * K * S), rb = make_rsrc(Yb, uint64_t(tb.nslot_cap) * K * S);
    const rsrc_t rpr = make_rsrc(tb.prow, uint64_t(tb.npatch) * uint64_t(tb.rows_cap) * 4), rpo = make_rsrc(tb.pout, uint64_t(tb.npatch) * uint64_t(tb.rows_cap) * 4);

    // this lane's table words of patch p (rows tid + 256 j): range-checked buffer loads, nothing beyond the patch's rows is requested
    auto load_tables = [&](int p, int rows, int32_t (&tr)[TJ], int32_t (&to)[TJ]) {
        const uint32_t base = uint32_t(p) * uint32_t(tb.rows_cap);
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int m = tid + 256 * j;
            const uint32_t off = m < rows ? (base + uint32_t(m)) * 4u : kOutOfRange;
            tr[j] = int32_t(__builtin_amdgcn_raw_buffer_load_b32(rpr, off, 0, 0));
            to[j] = int32_t(__builtin_amdgcn_raw_buffer_load_b32(rpo, off, 0, 0));
        }
    };
    auto store_tables = [&](int slot, int rows, const int32_t (&tr)[TJ], const int32_t (&to)[TJ]) {
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int m = tid + 256 * j;
            if (m < rows) { trow0[slot * Rp + m] = tr[j]; tout0[slot * Rp + m] = to[j]; }
        }
    };
    // x values of the patch whose row numbers are in table slot `slot`: pass u = row el + EK u, this lane's column
    auto load_x = [&](int slot, int rows, T (&xr)[U]) {
        const int32_t *const tr = trow0 + slot * Rp;
        int el_l = el;
        asm volatile("" : "+v"(el_l));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = el_l + EK * u;
            int32_t r = -1;
            if (u * EK < rows) r = (m < rows ? tr[m] : -1) | off_mask;
            T v[1];
            buf_load<T, 1>(rx, r >= 0 ? __umul24(uint32_t(r), K * S) + uint32_t(c0) * S : kOutOfRange, v);
            xr[u] = v[0];
        }
    };
    auto store_x = [&](int rows, const T (&xr)[U]) {
        int el_s = el;
        asm volatile("" : "+v"(el_s));                   // (no loop-invariant addresses held across the patch loop: see the read-out of the results)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = el_s + EK * u;
            if (m < rows && off_mask == 0) xs[m * K + c0] = xr[u];
        }
    };
    // local rows and metric terms of this lane's element of patch p into registers (lanes of an element ask for the same words)
    auto load_elem = [&](int p, uint32_t (&li)[10], double (&cm)[6]) {
        const int64_t e = int64_t(p) * E + elp;
        const bool active = has_el && e < tb.nt;
#pragma unroll
        for (int q = 0; q < 10; ++q) li[q] = 0u;
#pragma unroll
        for (int q = 0; q < 6; ++q) cm[q] = 0.0;
        if (active) {
            const uint32_t *pl = reinterpret_cast<const uint32_t *>(tb.lidx + e * 20);
#pragma unroll
            for (int q = 0; q < 10; ++q) li[q] = pl[q];
            const double *ce = tb.C + e * 6;
#pragma unroll
            for (int q = 0; q < 6; ++q) cm[q] = ce[q];
        }
    };
    // ... and from registers into the workgroup's LDS copy (the k lanes of an element write the same words): they are wanted three
    // times per patch - x values, metric contraction, accumulation - and would otherwise sit in 22 registers through the tensor chains
    auto park_elem = [&](const uint32_t (&li)[10], const double (&cm)[6]) {
        if (has_el && c0 == 0) {
#pragma unroll
            for (int q = 0; q < 10; ++q) eli[elp * 10 + q] = li[q];
#pragma unroll
            for (int q = 0; q < 6; ++q) ecm[elp * 6 + q] = cm[q];
        }
    };

    int rows_cur = clampR(pcnt[p0]);
    int rows_nxt = (p0 + 1 < p1) ? clampR(pcnt[p0 + 1]) : 0;
    // in flight across the loop's back edge: the NEXT patch's element data and row tables (requested behind the tensor chains)
    uint32_t li_n[10];
    double cm_n[6];
    int32_t tr_n[TJ], to_n[TJ];
    {   // prologue: the first patch's tables, rows and element data (the only exposed round trips), the second patch's tables on their way
        int32_t tr[TJ], to[TJ];
        load_tables(p0, rows_cur, tr, to);
        load_elem(p0, li_n, cm_n);
        load_tables(p0 + 1 < p1 ? p0 + 1 : p0, rows_nxt, tr_n, to_n);
        store_tables(0, rows_cur, tr, to);
        __syncthreads();
        T xr[U];
        load_x(0, rows_cur, xr);
        store_x(rows_cur, xr);
    }
    double d0 = 0.0;
    for (int p = p0; p < p1; ++p) {
        const int it = p - p0, sc = it & 1, sn = sc ^ 1;
        const int32_t *const trow_c = trow0 + sc * Rp, *const tout_c = tout0 + sc * Rp;
        const int rows_nn = (p + 2 < p1) ? clampR(pcnt[p + 2]) : 0;
        if constexpr (STAMP) tk = __builtin_readcyclecounter();
        if (tid < K) xs[R * K + tid] = T(0);              // the row constrained dofs read
        park_elem(li_n, cm_n);                           // element data of patch p (requested a patch ago)
        store_tables(sn, rows_nxt, tr_n, to_n);          // tables of patch p + 1 into the slot patch p - 1 has left
        lds_barrier();                                   // B0: the image holds X(p), slot sc the tables of p, slot sn those of p + 1
        REMO_PH(0)
        const int64_t e = int64_t(p) * E + elp;
        const bool active = has_el && e < tb.nt;
        const uint32_t *const my_li = eli + (has_el ? elp : 0) * 10;
        const double *const my_cm = ecm + (has_el ? elp : 0) * 6;
        T xv[20];
        {
            uint32_t li[10];
#pragma unroll
            for (int q = 0; q < 10; ++q) li[q] = my_li[q];
#define REMO_PATCH_L(i) ((li[(i) >> 1] >> (16 * ((i) & 1))) & 0xFFFFu)
#pragma unroll
            for (int i = 0; i < 20; ++i) xv[i] = xs[REMO_PATCH_L(i) * K + c0];
        }
        REMO_PH(2)
        lds_barrier();                                   // B1: every lane holds its x values: the image becomes the accumulators
        REMO_PH(3)
        for (int j = tid; j < rows_cur * K; j += BLK) ya[j] = 0.0;
        if (tid < K) ya[R * K + tid] = 0.0;
        lds_barrier();                                   // B2
        REMO_PH(4)
        typedef const T __attribute__((address_space(4))) *ctab_t;
        T g[30];
#pragma unroll
        for (int j = 0; j < 30; ++j) g[j] = T(0);
        if (active) {
            ctab_t tgrad = (ctab_t)ElemTables<T>::grad();
            if constexpr (sizeof(T) == 8) asm volatile("" : "+s"(tgrad));
            REMO_ELEM_GRAD(T, xv, g, tgrad)
        }
        // patch p + 1's x values are requested HERE, between the two tensor chains: the twenty x values of this patch are dead, the
        // thirty gradients alive - the point of lowest register pressure that still leaves the loads half the arithmetic phase, two
        // barriers and the read-out of the results to arrive (nothing is requested behind the run's last patch: rows_nxt = 0)
#pragma unroll
        for (int j = 0; j < 30; ++j) asm volatile("" : "+v"(g[j]));      // (the first chain is complete here, not sunk behind the loads)
        T xr[U];
        load_x(sn, rows_nxt, xr);
        REMO_PH(1)
        if (active) {
            T yv[20];
            ctab_t tdiv = (ctab_t)ElemTables<T>::div();
            if constexpr (sizeof(T) == 8) asm volatile("" : "+s"(tdiv));
            {
                const T c11 = T(my_cm[0]), c12 = T(my_cm[1]), c13 = T(my_cm[2]), c22 = T(my_cm[3]), c23 = T(my_cm[4]), c33 = T(my_cm[5]);
                T dd = T(0);
#pragma unroll
                for (int m = 0; m < 10; ++m) {     // h = c~ g, in place; g . h on the way
                    const T g1 = g[m], g2 = g[10 + m], g3 = g[20 + m];
                    const T h1 = c11 * g1 + c12 * g2 + c13 * g3, h2 = c12 * g1 + c22 * g2 + c23 * g3, h3 = c13 * g1 + c23 * g2 + c33 * g3;
                    dd += g1 * h1 + g2 * h2 + g3 * h3;
                    g[m] = h1; g[10 + m] = h2; g[20 + m] = h3;
                }
                d0 += double(dd);
            }
            REMO_ELEM_DIV(T, g, yv, tdiv)
            uint32_t li[10];
#pragma unroll
            for (int q = 0; q < 10; ++q) li[q] = my_li[q];
#pragma unroll
            for (int i = 0; i < 20; ++i) lds_add(ya + REMO_PATCH_L(i) * K + c0, double(yv[i]));
#undef REMO_PATCH_L
        }
        REMO_PH(5)
        // the next patch's element data and the row tables of the one after it: requested here, behind the chains (their registers
        // are free now), parked in LDS at the top of the next turn
        load_elem(p + 1 < p1 ? p + 1 : p, li_n, cm_n);
        load_tables(p + 2 < p1 ? p + 2 : p, rows_nn, tr_n, to_n);
        lds_barrier();                                   // B3: accumulators complete
        REMO_PH(6)
        // results of patch p out of LDS into registers (the image is about to receive patch p + 1), stored after that
        int32_t orow[U], oslot[U];
        T ov[U];
        const int npass = (rows_cur + EK - 1) / EK;
        // (the LDS addresses of the passes are loop invariants; hoisted out of the patch loop they would sit in a dozen registers through
        // the tensor chains - i.e. in scratch, and a scratch reload waits for every load still in flight: formed anew from an opaque copy)
        int el_o = el;
        asm volatile("" : "+v"(el_o));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            orow[u] = -1; oslot[u] = -1; ov[u] = T(0);
            if (u < npass) {
                const int m = el_o + EK * u;
                const bool in = m < rows_cur;
                orow[u] = (in ? trow_c[m] : -1) | off_mask; oslot[u] = in ? tout_c[m] : -1;
                ov[u] = T(ya[(in ? m : 0) * K + c0]);
            }
        }
        lds_barrier();                                   // B4: every lane has its results: the image is free
        REMO_PH(7)
        store_x(rows_nxt, xr);                           // X(p + 1) (the compiler waits for exactly these loads: what was requested after them stays in flight)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < npass) {                             // one of the two stores of a value is out of range: dropped by the hardware, no branch
                const bool have = orow[u] >= 0;
                T v[1] = {ov[u]};
                buf_store<T, 1>(ry, (have && oslot[u] < 0) ? __umul24(uint32_t(orow[u]), K * S) + uint32_t(c0) * S : kOutOfRange, v);
                buf_store<T, 1>(rb, (have && oslot[u] >= 0) ? __umul24(uint32_t(oslot[u]), K * S) + uint32_t(c0) * S : kOutOfRange, v);
            }
        }
        REMO_PH(8)
        rows_cur = rows_nxt; rows_nxt = rows_nn;
    }
    if constexpr (STAMP) {
        if (tid == 64 * REMO_STAMP_WAVE) {
            for (int k = 0; k < 10; ++k) stamps[int64_t(blockIdx.x) * 12 + k] = ph[k];
            stamps[int64_t(blockIdx.x) * 12 + 10] = p1 - p0;
        }
    }
#undef REMO_PH
    if (ppart) {
        double dot[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dot[c] = (c == c0) ? d0 : 0.0;
        const double mine = block_sum_column<K>(dot, smem);
        if (tid < K) {
            if (pbins) (void)__hip_atomic_fetch_add(pbins + (blockIdx.x % kPqBins) * K + tid, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else ppart[int64_t(p0) * K + tid] = mine;
        }
        if (!pbins)
            for (int64_t j = tid; j < int64_t(p1 - p0 - 1) * K; j += BLK) ppart[int64_t(p0 + 1) * K + j] = 0.0;
    }
}

}  // namespace

// remo_debug_tune key 34: 1 = persistent workgroups with LDS-DMA prefetch of the next patch, 2 = the same with the prefetch through
// registers, 0 = one workgroup per patch (default).
// Measured at size L (370 k tetrahedra, k = 5, fp64; profiles/r04_h_*): the persistent form is parity-green and removes every wait on
// memory from the loop (the wait before barrier B3 costs 8 clock ticks) but takes 138 us per application against 112: its LDS (two
// row images + tables: 65 KB) leaves two workgroups per CU, a wave spends 5.9 k of its 18.7 k ticks per patch ISSUING the ~25 LDS-DMA
// instructions of the next patch (4-byte pieces - 40-byte rows do not tile into 16-byte ones - cost ~240 ticks each), and the tensor
// chains (7.5 k) are bound by the fp64 rate whenever the CU's two workgroups are in them together.  With two contexts on the GPU the
// two forms give the same points/s (115.9 against 115.3).  Kept for that record and as the starting point of a version with
// 16-byte-tiled rows; not the default.
//
// Launches the persistent form key 34 asks for, if it can run this batch (mode: key 21, stamps: g_patch_stamps of patch.hip), on key 35's
// workgroups per XCD where that is fewer than stay resident; false: nothing was launched and k_patch_apply takes the application.  per = patches per XCD.
template <class T, int K>
static bool launch_patch_persistent(const PatchOpT<T> &P, int mode, long long *stamps, const T *x, T *y, double *pp2, const double *scal, int step,
                                    double *bins, hipStream_t s) {
    const PatchTables &tb = P.t;
    const int64_t per = (tb.npatch + 7) / 8;
    if (mode != 0 && mode != 4) return false;
    if (tb.rounds != 1) return false;      // the persistent forms take one element per lane
    const int form = g_tune.patch_persist, wgs_per_xcd = g_tune.patch_wgs_per_xcd;
    if (form == 2 && P.lds_rows <= kPatchPasses * (256 / K) && P.lds_rows <= 1024) {
        // persistent form with the prefetch through registers: three workgroups per CU by its registers (LDS would allow four or five)
        const size_t bytes = patch_lds_bytes_r(P.lds_rows, K, tb.E);
        int wpc = int((160 * 1024) / (bytes + 16 * K * 8 + 1024));
        if (wpc > 3) wpc = 3;
        if (wpc >= 1 && bytes <= 64 * 1024 - 2048) {
            int64_t nwx = int64_t(32) * wpc;
            if (wgs_per_xcd > 0 && wgs_per_xcd < nwx) nwx = wgs_per_xcd;
            if (nwx > per) nwx = per;
            if (nwx < 1) nwx = 1;
            if (stamps && K == 5)
                hipLaunchKernelGGL((k_patch_apply_r<T, K, true>), dim3(int(nwx * 8)), dim3(256), bytes, s, tb, P.lds_rows, x, y, P.Yb, pp2, scal, step, bins, stamps);
            else
                hipLaunchKernelGGL((k_patch_apply_r<T, K>), dim3(int(nwx * 8)), dim3(256), bytes, s, tb, P.lds_rows, x, y, P.Yb, pp2, scal, step, bins, (long long *)nullptr);
            return true;
        }
    }
    if (form == 1) {
        // persistent form: as many workgroups as stay resident (LDS: two row images + tables per workgroup), 32 CUs per XCD
        const size_t bytes = patch_lds_bytes_p(P.lds_rows, K, tb.E);
        const size_t lds_cu = 160 * 1024, per_wg = bytes + 16 * K * 8 + 1024;
        int wpc = int(lds_cu / per_wg);
        if (wpc > 4) wpc = 4;
        if (wpc >= 1 && bytes <= 150 * 1024) {
            static bool attr_ok[2][9] = {};
            auto kernel = k_patch_apply_p<T, K>;
            bool &ok = attr_ok[sizeof(T) == 4 ? 1 : 0][K];
            if (!ok) ok = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(150 * 1024)) == hipSuccess;
            if (ok) {
                int64_t nwx = int64_t(32) * wpc;
                if (wgs_per_xcd > 0 && wgs_per_xcd < nwx) nwx = wgs_per_xcd;
                if (nwx > per) nwx = per;
                if (nwx < 1) nwx = 1;
                if (stamps && K == 5) {
                    auto ks = k_patch_apply_p<T, K, true>;
                    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ks), hipFuncAttributeMaxDynamicSharedMemorySize, int(150 * 1024));
                    hipLaunchKernelGGL(ks, dim3(int(nwx * 8)), dim3(256), bytes, s, tb, P.lds_rows, x, y, P.Yb, pp2, scal, step, bins, stamps);
                } else
                    hipLaunchKernelGGL(kernel, dim3(int(nwx * 8)), dim3(256), bytes, s, tb, P.lds_rows, x, y, P.Yb, pp2, scal, step, bins, (long long *)nullptr);
                return true;
            }
        }
    }
    return false;
}
