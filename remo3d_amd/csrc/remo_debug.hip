// remo_debug.hip — the probes of include/remo3d_hip_debug.h: bandwidth / clock / XCD / grid-barrier measurements, the phase clocks
// of the patch kernel (probe builds), and remo_debug_tune with the tuning state it writes.
#include <limits.h>

#include <algorithm>
#include <vector>

#include "../../include/remo3d_hip_debug.h"
#include "remo_internal.h"
#include "patch.h"

using namespace remo;

namespace remo {
Tune g_tune;
}

extern "C" {

namespace {
__global__ void __launch_bounds__(256) k_stream_read(const double2 *__restrict__ x, int64_t n2, double *__restrict__ out) {
    double a = 0.0, b = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n2; i += int64_t(gridDim.x) * blockDim.x) {
        const double2 v = x[i];
        a += v.x; b += v.y;
    }
    a += b;
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * 4 + (threadIdx.x >> 6)] = a;
}
// scattered 16-byte reads from a 2 MiB buffer (resident in every XCD's 4 MiB L2 after the first touch): the L2 -> L1 -> lane path
// the SpMM's x gather lives on
__global__ void __launch_bounds__(256) k_l2_gather(const double2 *__restrict__ x, uint32_t mask, int iters, double *__restrict__ out) {
    uint32_t idx = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
    double a = 0.0;
    for (int i = 0; i < iters; ++i) {
        const double2 v = x[idx & mask];
        a += v.x + v.y;
        idx = idx * 1664525u + 1013904223u;
    }
    if (a == 1.2345e300) out[0] = a;
}

// a chain of dependent fp32 multiply-adds per wave, one wave per SIMD-sized slice of the chip: its rate follows the shader clock
__global__ void __launch_bounds__(64) k_clock_probe(int iters, float *__restrict__ out) {
    float a = float(threadIdx.x) * 1e-3f;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 16; ++u) a = __builtin_fmaf(a, 0.999999f, 0.5f);
    }
    if (a == 123.456f) out[blockIdx.x] = a;
}
}  // namespace

int remo_debug_cache_gather(remo_ctx_t *ctx, int64_t bytes, double *gbs) {
    if (!ctx || !gbs || bytes < (1 << 20) || bytes > (int64_t(1) << 32) || (bytes & (bytes - 1)) != 0) return REMO_ERR_ARG;   // a power of two
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const int64_t n2 = bytes / 16;   // 16-byte elements
        DeviceTemp tmp;
        double *a = tmp.alloc<double>(size_t(n2) * 2), *o = tmp.alloc<double>(8);
        HIP_TRY(hipMemsetAsync(a, 0, size_t(n2) * 16, ctx->stream));
        const int blocks = 4096, iters = 64;
        float best = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
            hipLaunchKernelGGL(k_l2_gather, dim3(blocks), dim3(256), 0, ctx->stream, reinterpret_cast<const double2 *>(a), uint32_t(n2 - 1), iters, o);
            HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
            if (ms < best) best = ms;
        }
        *gbs = double(blocks) * 256.0 * iters * 16.0 / (double(best) * 1e6);
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_debug_clock(remo_ctx_t *ctx, double *gfma_per_wave) {
    if (!ctx || !gfma_per_wave) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        DeviceTemp tmp;
        float *o = tmp.alloc<float>(1024);
        const int iters = 1 << 16;   // x 16 dependent multiply-adds
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) {
            HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
            hipLaunchKernelGGL(k_clock_probe, dim3(1024), dim3(64), 0, ctx->stream, iters, o);
            HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
            if (ms < best) best = ms;
        }
        *gfma_per_wave = double(iters) * 16.0 / (double(best) * 1e6);
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

namespace {
// which XCD (accelerator die) a workgroup runs on: hardware register XCC_ID (id 20, 4 bits) - the SpMM's row schedule assumes
// workgroup b runs on XCD b mod 8
__global__ void __launch_bounds__(64) k_xcc_probe(int32_t *__restrict__ out) {
    const int32_t id = __builtin_amdgcn_s_getreg((3 << 11) | 20);
    if (threadIdx.x == 0) out[blockIdx.x] = id;
}
}  // namespace

int remo_debug_xcc(remo_ctx_t *ctx, int32_t *out, int32_t nblocks) {
    if (!ctx || !out || nblocks < 1 || nblocks > 65536) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        DeviceTemp tmp;
        int32_t *d = tmp.alloc<int32_t>(nblocks);
        hipLaunchKernelGGL(k_xcc_probe, dim3(nblocks), dim3(64), 0, ctx->stream, d);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(hipMemcpy(out, d, sizeof(int32_t) * nblocks, hipMemcpyDeviceToHost));
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_debug_device(remo_ctx_t *ctx, int64_t *out8) {
    if (!ctx || !out8) return REMO_ERR_ARG;
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, ctx->device) != hipSuccess) return fail(ctx, REMO_ERR_DEVICE, "hipGetDeviceProperties failed");
    out8[0] = pr.multiProcessorCount;
    out8[1] = pr.clockRate;          // kHz
    out8[2] = pr.memoryClockRate;    // kHz
    out8[3] = pr.memoryBusWidth;
    out8[4] = pr.l2CacheSize;
    out8[5] = int64_t(pr.totalGlobalMem >> 20);
    out8[6] = pr.maxSharedMemoryPerMultiProcessor;
    out8[7] = pr.asicRevision;
    return REMO_OK;
}

int remo_debug_stream(remo_ctx_t *ctx, int64_t bytes, double *read_gbs, double *copy_gbs) {
    if (!ctx || bytes < (1 << 20)) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const int64_t n = bytes / 16 * 2;
        DeviceTemp tmp;
        double *a = tmp.alloc<double>(n), *b = tmp.alloc<double>(n), *o = tmp.alloc<double>(4096 * 4);
        HIP_TRY(hipMemsetAsync(a, 0, sizeof(double) * n, ctx->stream));
        HIP_TRY(hipMemsetAsync(b, 0, sizeof(double) * n, ctx->stream));
        float best_r = 1e30f, best_c = 1e30f;
        for (int rep = 0; rep < 6; ++rep) {
            HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
            hipLaunchKernelGGL(k_stream_read, dim3(4096), dim3(256), 0, ctx->stream, reinterpret_cast<const double2 *>(a), n / 2, o);
            HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
            HIP_TRY(hipMemcpyAsync(b, a, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            float r = 0, c = 0;
            (void)hipEventElapsedTime(&r, ctx->ev[0], ctx->ev[1]);
            (void)hipEventElapsedTime(&c, ctx->ev[1], ctx->ev[2]);
            if (r < best_r) best_r = r;
            if (c < best_c) best_c = c;
        }
        if (read_gbs) *read_gbs = double(n) * 8.0 / (double(best_r) * 1e6);
        if (copy_gbs) *copy_gbs = 2.0 * double(n) * 8.0 / (double(best_c) * 1e6);
        if (bytes <= (int64_t(192) << 20) && read_gbs) {   // a buffer that fits the 256 MB Infinity Cache: re-read it back to back
            float best = 1e30f;
            for (int rep = 0; rep < 6; ++rep) {
                hipLaunchKernelGGL(k_stream_read, dim3(4096), dim3(256), 0, ctx->stream, reinterpret_cast<const double2 *>(a), n / 2, o);   // refill
                HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
                for (int k = 0; k < 4; ++k)
                    hipLaunchKernelGGL(k_stream_read, dim3(4096), dim3(256), 0, ctx->stream, reinterpret_cast<const double2 *>(a), n / 2, o);
                HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                float r = 0;
                (void)hipEventElapsedTime(&r, ctx->ev[0], ctx->ev[1]);
                if (r < best) best = r;
            }
            *read_gbs = 4.0 * double(n) * 8.0 / (double(best) * 1e6);
        }
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_debug_grid_barrier(remo_ctx_t *ctx, int32_t nblocks, int32_t nbar, double *out3) {
    if (!ctx || !out3 || nblocks < 1 || nblocks > 2048 || nbar < 1 || nbar > 100000) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        DeviceTemp tmp;
        unsigned *counter = tmp.alloc<unsigned>(16);
        float *buf = tmp.alloc<float>(size_t(nblocks) * 256);
        int *fail_flag = reinterpret_cast<int *>(counter) + 4, *mismatch = reinterpret_cast<int *>(counter) + 8;
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        float ms = 0.f;
        for (int rep = 0; rep < 2; ++rep) {     // the second run is the measurement
            HIP_TRY(hipMemsetAsync(counter, 0, 64, ctx->stream));
            HIP_TRY(hipMemsetAsync(buf, 0, sizeof(float) * size_t(nblocks) * 256, ctx->stream));
            HIP_TRY(hipEventRecord(e0, ctx->stream));
            launch_barrier_probe(nblocks, nbar, counter, fail_flag, buf, mismatch, ctx->stream);
            HIP_TRY(hipEventRecord(e1, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        }
        int h[12];
        HIP_TRY(hipMemcpy(h, counter, sizeof h, hipMemcpyDeviceToHost));
        out3[0] = 1e3 * double(ms) / (2.0 * nbar);    // two barriers per iteration
        out3[1] = h[4]; out3[2] = h[8];
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return REMO_OK;
    } catch (const std::exception &e) {
        return fail(ctx, REMO_ERR_DEVICE, e.what());
    }
}

#ifdef REMO_PROBES
namespace {
// What the two phase probes of the patch kernel share: 5 columns of pseudo-random x, a stamp buffer, and the operator of the
// batch's last run in fp64 or as the fp32 instantiation on the same tables (vectors reinterpreted: timing only).
struct PatchProbe {
    static constexpr int k = 5;
    remo_ctx *ctx;
    remo_batch *b;
    bool fp32;
    DeviceTemp tmp;
    double *dx, *dy;
    long long *st;
    size_t stamp_words;
    int nb;
    CsrViewT<float> A32;
    PatchOpT<float> P32;
    PatchProbe(remo_ctx *ctx_, remo_batch *b_, bool fp32_, size_t stamp_words_)
        : ctx(ctx_), b(b_), fp32(fp32_), stamp_words(stamp_words_), A32{b_->A.n, 0, nullptr, nullptr, nullptr}, P32(patch_view32(b_->patch64)) {
        const int64_t n = b->A.n;
        dx = tmp.alloc<double>(n * k + 2);
        dy = tmp.alloc<double>(n * k + 2);
        st = tmp.alloc<long long>(stamp_words);
        std::vector<double> hx(size_t(n) * k);
        for (size_t i = 0; i < hx.size(); ++i) hx[i] = double((i * 2654435761u) % 1000) * 1e-3 - 0.5;
        HIP_TRY(hipMemcpy(dx, hx.data(), sizeof(double) * hx.size(), hipMemcpyHostToDevice));
        HIP_TRY(hipMemset(st, 0, sizeof(long long) * stamp_words));
        nb = spmv_grid(n, choose_lanes_per_row(n, b->A.nnz));
        A32.patch = &P32; A32.vertex_block_only = true;
    }
    void once() {
        if (fp32) launch_spmm(A32, k, reinterpret_cast<const float *>(dx), reinterpret_cast<float *>(dy), nullptr, nullptr, nb, ctx->stream);
        else launch_spmm(b->A, k, dx, dy, nullptr, nullptr, nb, ctx->stream);
    }
    void stamped_runs() {     // three applications that leave their phase stamps (patch mode 4)
        set_patch_stamps(st); g_tune.patch_mode = 4;
        for (int rep = 0; rep < 3; ++rep) once();
        g_tune.patch_mode = 0; set_patch_stamps(nullptr);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    double timed_us() {       // the whole application (apply + reduce launches), microseconds per application
        once();
        HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        for (int rep = 0; rep < 10; ++rep) once();
        HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
        return 1e3 * double(ms) / 10.0;
    }
    std::vector<long long> stamps() {
        std::vector<long long> h(stamp_words);
        HIP_TRY(hipMemcpy(h.data(), st, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
        return h;
    }
};

// the argument errors both probes answer with (REMO_OK: go on)
int patch_probe_check(remo_ctx *ctx, remo_batch *b) {
    if (!b->has_system || b->run_id != ctx->run_id || !b->A.patch) return fail(ctx, REMO_ERR_ARG, "the last run on this batch did not use the patch operator");
    if (b->patch64.t.rounds != 1) return fail(ctx, REMO_ERR_ARG, "the batch's patch tables hold two elements per lane: set remo_debug_tune key 40 to 1 and run the batch again");
    if (PatchProbe::k * b->patch64.t.E > kPatchBlock) return fail(ctx, REMO_ERR_ARG, "the batch's patch tables are laid out for fewer than 5 columns");
    return REMO_OK;
}
}  // namespace
#endif

int remo_debug_patch_phases(remo_ctx_t *ctx, remo_batch_t *b, int32_t fp32, double *out16) {
    if (!ctx || !b || !out16) return REMO_ERR_ARG;
#ifndef REMO_PROBES
    (void)fp32;
    return fail(ctx, REMO_ERR_ARG, "remo_debug_patch_phases: the library was built without -DREMO_PROBES (make -C remo3d_amd/csrc probes)");
#else
    if (int rc = patch_probe_check(ctx, b)) return rc;
    // (this probe is about the one-workgroup-per-patch form; remo_debug_patch_phases_p is the persistent one's: key 34 is put back on every way out)
    struct PersistOff { int was = g_tune.patch_persist; PersistOff() { g_tune.patch_persist = 0; } ~PersistOff() { g_tune.patch_persist = was; } } persist_off;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const int64_t grid = (b->patch64.t.npatch + 7) / 8 * 8;
        std::vector<long long> h;
        {
            PatchProbe pr(ctx, b, fp32 != 0, size_t(grid) * 8);
            pr.stamped_runs();
            for (int mode = 0; mode <= 3; ++mode) {     // the ablation modes 0 .. 3
                g_tune.patch_mode = mode;
                out16[10 + mode] = pr.timed_us();
            }
            g_tune.patch_mode = 0;
            h = pr.stamps();
        }
        for (int i = 0; i < 10; ++i) out16[i] = 0.0;
        long long lo = LLONG_MAX, hi = 0;
        int64_t cnt = 0;
        for (int64_t w = 0; w < grid; ++w) {
            const long long *s8 = h.data() + w * 8;
            if (s8[0] == 0 || s8[7] == 0) continue;
            for (int q = 0; q < 7; ++q) out16[q] += double(s8[q + 1] - s8[q]);
            out16[7] += double(s8[7] - s8[0]);
            lo = std::min(lo, s8[0]); hi = std::max(hi, s8[7]);
            ++cnt;
        }
        for (int q = 0; q < 8; ++q) out16[q] /= double(cnt > 0 ? cnt : 1);
        out16[8] = double(hi - lo);     // first start to last end, clock ticks
        out16[9] = double(cnt);
        return REMO_OK;
    } catch (const std::exception &ex) {
        g_tune.patch_mode = 0; set_patch_stamps(nullptr);
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
#endif
}

int remo_debug_patch_phases_p(remo_ctx_t *ctx, remo_batch_t *b, int32_t fp32, double *out16) {
    if (!ctx || !b || !out16) return REMO_ERR_ARG;
#ifndef REMO_PROBES
    (void)fp32;
    return fail(ctx, REMO_ERR_ARG, "remo_debug_patch_phases_p: the library was built without -DREMO_PROBES (make -C remo3d_amd/csrc probes)");
#else
    if (int rc = patch_probe_check(ctx, b)) return rc;
    const int64_t slots = 8192;      // workgroups the stamp buffer holds
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        std::vector<long long> h;
        double us = 0.0;
        {
            PatchProbe pr(ctx, b, fp32 != 0, size_t(slots) * 12);
            pr.stamped_runs();
            us = pr.timed_us();
            h = pr.stamps();
        }
        for (int i = 0; i < 16; ++i) out16[i] = 0.0;
        double patches = 0, wgs = 0, longest = 0;
        for (int64_t w = 0; w < slots; ++w) {
            const long long *s12 = h.data() + w * 12;
            if (s12[10] <= 0) continue;
            double tot = 0;
            for (int q = 0; q < 10; ++q) { out16[q] += double(s12[q]); tot += double(s12[q]); }
            patches += double(s12[10]); wgs += 1; longest = std::max(longest, tot);
        }
        for (int q = 0; q < 10; ++q) out16[q] /= (patches > 0 ? patches : 1);     // clock ticks per patch, phase by phase
        out16[10] = patches; out16[11] = wgs; out16[12] = longest; out16[13] = us;
        return REMO_OK;
    } catch (const std::exception &ex) {
        g_tune.patch_mode = 0; set_patch_stamps(nullptr);
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
#endif
}

int remo_debug_direction_forms(remo_ctx_t *ctx, int64_t n, int64_t nv, int32_t k, int32_t grid, int32_t step, double tol2, const double *r,
                               const float *p, const double *z, const double *dinv, const double *part_even, const double *part_odd,
                               int32_t nb_rz, const double *scal48, float *p_flat, float *p_row, double *scal_flat, double *scal_row) {
    if (!ctx || n < 1 || nv < 0 || nv > n || k < 1 || k > 8 || grid < 1 || grid > kMaxPartialBlocks || step < 0 || nb_rz < 0 || nb_rz > kMaxPartialBlocks ||
        !r || !p || !dinv || (nv > 0 && !z) || !part_even || !part_odd || !scal48 || !p_flat || !p_row || !scal_flat || !scal_row)
        return REMO_ERR_ARG;
    if (uint64_t(n) * uint64_t(k) * 8 >= 0xFFFFF000ull) return fail(ctx, REMO_ERR_ARG, "remo_debug_direction_forms: n k sizeof(double) must stay below 4 GB (the flat form's range)");
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t N = size_t(n) * k, NV = size_t(nv) * k, NP = size_t(nb_rz > 0 ? nb_rz : 1) * k;
        DeviceTemp tmp;
        double *dr = tmp.alloc<double>(N), *dz = tmp.alloc<double>(NV + 2), *dd = tmp.alloc<double>(n), *dpart = tmp.alloc<double>(2 * NP),
               *dscal = tmp.alloc<double>(48);
        float *dp = tmp.alloc<float>(N);
        HIP_TRY(hipMemcpy(dr, r, sizeof(double) * N, hipMemcpyHostToDevice));
        if (NV) HIP_TRY(hipMemcpy(dz, z, sizeof(double) * NV, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(dd, dinv, sizeof(double) * n, hipMemcpyHostToDevice));
        if (nb_rz > 0) {
            HIP_TRY(hipMemcpy(dpart, part_even, sizeof(double) * NP, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dpart + NP, part_odd, sizeof(double) * NP, hipMemcpyHostToDevice));
        }
        for (int form = 1; form >= 0; --form) {      // the flat form, then the row form, each from the caller's p and scalars
            HIP_TRY(hipMemcpy(dp, p, sizeof(float) * N, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(dscal, scal48, sizeof(double) * 48, hipMemcpyHostToDevice));
            launch_direction_form(form != 0, grid, n, nv, k, step, tol2, nb_rz, dpart + ((step + 1) & 1) * NP, dscal, dr, dp, dd, dz, ctx->stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipMemcpy(form ? p_flat : p_row, dp, sizeof(float) * N, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(form ? scal_flat : scal_row, dscal, sizeof(double) * 48, hipMemcpyDeviceToHost));
        }
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_debug_product(remo_ctx_t *ctx, int32_t slots, int64_t cap, int64_t nx, const int32_t *xrp, const int32_t *xc, const double *xv,
                       int64_t ny, const int32_t *yrp, const int32_t *yc, const double *yv, int32_t *crp, int32_t *cc, double *cv,
                       int32_t *flags) {
    if (!ctx || !xrp || !xc || !xv || !yrp || !yc || !yv || !crp || !cc || !cv || !flags) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        amg_debug_product(ctx->stream, slots, cap, nx, xrp, xc, xv, ny, yrp, yc, yv, crp, cc, cv, flags);
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_debug_row_ops(remo_ctx_t *ctx, int32_t op, int32_t lanes, int32_t reading, int32_t fp32, int64_t n, int64_t nx, int32_t k, const int32_t *rowptr,
                       const int32_t *col, const double *val, const double *dinv, double omega, const double *x, const double *r, int32_t nblocks,
                       int32_t guard, void *out, void *out2) {
    if (!ctx || !rowptr || !col || !val || !x || !out || (reading != 0 && reading != 1)) return REMO_ERR_ARG;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        amg_debug_row_ops(ctx->stream, op, lanes, reading == 1, fp32 != 0, n, nx, k, rowptr, col, val, dinv, omega, x, r, nblocks, guard, out, out2);
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

#ifdef REMO_PROBES
namespace {
// remo_debug_vector_heads: the stamp rows of both launches while the probe is on.  One buffer for the process, on the device of the context
// that switched the probe on (the kernels' g_vec_stamps is that device's symbol): a probe for one context at a time, as the header says.
long long *g_vec_stamp_buf = nullptr;
}
#endif

int remo_debug_vector_heads(remo_ctx_t *ctx, int32_t on, double *out8) {
    if (!ctx || (!on && !out8)) return REMO_ERR_ARG;
#ifndef REMO_PROBES
    return fail(ctx, REMO_ERR_ARG, "remo_debug_vector_heads: the library was built without -DREMO_PROBES (make -C remo3d_amd/csrc probes)");
#else
    const size_t words = size_t(2) * kMaxPartialBlocks * 4;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (on) {
            if (!g_vec_stamp_buf) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&g_vec_stamp_buf), sizeof(long long) * words));
            HIP_TRY(hipMemset(g_vec_stamp_buf, 0, sizeof(long long) * words));
            set_vector_stamps(g_vec_stamp_buf);
            return REMO_OK;
        }
        set_vector_stamps(nullptr);
        for (int i = 0; i < 8; ++i) out8[i] = 0.0;
        if (!g_vec_stamp_buf) return REMO_OK;
        std::vector<long long> h(words);
        HIP_TRY(hipMemcpy(h.data(), g_vec_stamp_buf, sizeof(long long) * words, hipMemcpyDeviceToHost));
        HIP_TRY(hipFree(g_vec_stamp_buf));
        g_vec_stamp_buf = nullptr;
        for (int which = 0; which < 2; ++which) {
            double head = 0, whole = 0, share = 0, cnt = 0;
            for (int w = 0; w < kMaxPartialBlocks; ++w) {
                const long long *s4 = h.data() + (size_t(which) * kMaxPartialBlocks + w) * 4;
                if (s4[0] == 0 || s4[2] <= s4[0]) continue;
                head += double(s4[1] - s4[0]); whole += double(s4[2] - s4[0]);
                share += double(s4[1] - s4[0]) / double(s4[2] - s4[0]);
                cnt += 1;
            }
            const double c = cnt > 0 ? cnt : 1;
            out8[4 * which] = head / c; out8[4 * which + 1] = whole / c; out8[4 * which + 2] = share / c; out8[4 * which + 3] = cnt;
        }
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
#endif
}

namespace {
// the keys of remo_debug_tune: the switch a key writes (tune.h has its meaning and default) and, where a switch holds a few values only,
// how the caller's value is stored
struct TuneKey {
    int key;
    int Tune::*field;
    int (*stored)(int) = nullptr;
};
const TuneKey kTuneKeys[] = {
    // Keys that force ONE OF THE PRODUCT'S OWN PATHS - a choice the library makes by size or dimension, forced so that a small test
    // mesh reaches the code a large batch runs; every setting gives the same operator / preconditioner to rounding: always there.
    {3, &Tune::spmm_mapping},
    {6, &Tune::square},
    {9, &Tune::fold_first},
    {13, &Tune::compact},
    {15, &Tune::chain32},
    {16, &Tune::amg},
    {17, &Tune::amg32},
    {18, &Tune::element_order},
    {22, &Tune::defer_q},
    {24, &Tune::ell},
    {25, &Tune::x_in_direction},
    {29, &Tune::slab_masked},
    {30, &Tune::flat_direction},
    {31, &Tune::tile_update},
    {39, &Tune::x_ev},
    {40, &Tune::patch_rounds, [](int v) { return v == 1 ? 1 : 2; }},      // (patch_rounds tests >= 2: anything but 1 asks for two)
    {41, &Tune::p32},
    {42, &Tune::pairs_fused},
    {43, &Tune::pair_ev_bytes},
#ifdef REMO_PROBES
    // Keys of rejected experiments and ablations (some give wrong results on purpose): tools/ builds only (make probes)
    {0, &Tune::spmm_variant},
    {1, &Tune::spmm_lpr},
    {2, &Tune::spmm_threads},
    {4, &Tune::spmm_grid},
    {5, &Tune::spmm_mode},
    {7, &Tune::sq_lanes},
    {8, &Tune::row_pattern},
    {21, &Tune::patch_mode},
    {26, &Tune::patch_lean},
    {27, &Tune::slab_ahead},
    {28, &Tune::dot_bins},
    {32, &Tune::patch_spread},
    {33, &Tune::patch_trim},
    {34, &Tune::patch_persist, [](int v) { return (v == 1 || v == 2) ? v : 0; }},
    {35, &Tune::patch_wgs_per_xcd, [](int v) { return v > 0 ? v : 0; }},
    {36, &Tune::extra_apply},
    {44, &Tune::amg_r_lanes, [](int v) { return (v == 8 || v == 16 || v == 32 || v == 64) ? v : 0; }},
    {45, &Tune::amg_image},
    {46, &Tune::amg_post_wide},
#endif
};
}  // namespace

int remo_debug_tune(int32_t key, int32_t value) {
    for (const TuneKey &t : kTuneKeys)
        if (t.key == key) {
            g_tune.*t.field = t.stored ? t.stored(value) : value;
            return 0;
        }
    return -1;      // no such key, or not in this build
}

int remo_debug_sens_timing(remo_ctx_t *ctx, double *out2) {
    if (!ctx || !out2) return REMO_ERR_ARG;
    out2[0] = ctx->sens_ms;
    out2[1] = ctx->sens_bytes;
    return REMO_OK;
}

int remo_debug_sens_group_timing(remo_ctx_t *ctx, double *out4) {
    if (!ctx || !out4) return REMO_ERR_ARG;
    for (int i = 0; i < 4; ++i) out4[i] = ctx->sens_group_ms[i];
    return REMO_OK;
}

int remo_debug_field_timing(remo_ctx_t *ctx, double *out2) {
    if (!ctx || !out2) return REMO_ERR_ARG;
    out2[0] = ctx->field_ms[0];
    out2[1] = ctx->field_ms[1];
    return REMO_OK;
}

int remo_debug_pairs_timing(remo_ctx_t *ctx, double *out2) {
    if (!ctx || !out2) return REMO_ERR_ARG;
    out2[0] = ctx->pair_ms[0];
    out2[1] = ctx->pair_ms[1];
    return REMO_OK;
}

int remo_debug_pair_groups_timing(remo_ctx_t *ctx, double *out4) {
    if (!ctx || !out4) return REMO_ERR_ARG;
    for (int i = 0; i < 4; ++i) out4[i] = ctx->pair_group_ms[i];
    return REMO_OK;
}

int remo_debug_point_location(remo_ctx_t *ctx) { return ctx ? ctx->point_location : REMO_ERR_ARG; }
int remo_debug_direction_bytes(remo_ctx_t *ctx) { return ctx ? ctx->direction_bytes : REMO_ERR_ARG; }
int remo_debug_secondary_timing(remo_ctx_t *ctx, double *ms) {
    if (!ctx || !ms) return REMO_ERR_ARG;
    *ms = ctx->sec_ms;
    return REMO_OK;
}

}  // extern "C"
