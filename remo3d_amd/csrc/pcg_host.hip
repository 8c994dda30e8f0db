// pcg_host.hip — host side of the PCG: the launch loop of one solve (the host stays a few steps ahead of the device and watches
// the progress records the kernels write into mapped memory) and the mixed-precision mode's outer cycle.
#include <atomic>
#include <cmath>
#include <cstring>
#include <thread>
#include <type_traits>

#include "pcg_host.h"
#include "warm.h"

namespace remo {

namespace {

// fp64 side of a mixed-precision inner solve: where the residual replacements read and write
struct RefineHooks {
    const CsrView *A64 = nullptr;
    const double *f64 = nullptr;
    double *x64 = nullptr, *q64 = nullptr;
    double factor2 = 1e-6;   // replace once <Cr,r> of some column has dropped by this factor since the last replacement
    int replacements = 0;
};

// One PCG solve in storage type T.  tol2: relative target on <Cr,r> (w.r.t. this solve's own start);
// floor: optional absolute per-column floor of <Cr,r> (mixed mode: the outer target).  rz_first /
// rz_last return <Cr,r> at the start and at the end.
template <class T>
ChunkResult run_pcg_t(remo_ctx *ctx, const CsrViewT<T> &A, int k, const T *d_f, PcgBuffersT<T> &buf, double tol2, const double *floor,
                      int maxit, int check, int time_kernels, remo_stats_t *st, size_t &ev_used, double *rz_first, double *rz_last,
                      RefineHooks *hooks = nullptr) {
    ChunkResult res;
    bool replace_next = false, have_ref = false;
    double rz_ref[REMO_MAX_RHS] = {0};
    hipStream_t s = ctx->stream;
    if (check <= 0) check = 10;
    for (int i = 0; i < ctx->progress_len; ++i) ctx->progress[i].step = -1;
    std::atomic_thread_fence(std::memory_order_seq_cst);
    HIP_TRY(hipMemsetAsync(buf.rz0, 0, kScalarSlots * sizeof(double), s));   // forwarded totals + done flag + floor
    if (buf.defer_q) HIP_TRY(hipMemsetAsync(buf.part_pq, 0, sizeof(double) * kMaxPartialBlocks * 8, s));   // the patch operator's dot launch fills only its first rows
    if (floor) {
        std::memcpy(ctx->floor_stage, floor, sizeof(double) * REMO_MAX_RHS);
        HIP_TRY(hipMemcpyAsync(buf.rz0 + 5 * 8, ctx->floor_stage, sizeof(double) * REMO_MAX_RHS, hipMemcpyHostToDevice, s));
    }
    launch_pcg_init(A, k, d_f, buf, s);
    volatile int32_t *done_step = &ctx->progress[ctx->progress_len - 1].step;
    int step = 0;
    bool done = false;
    // q = A p (+ partials of <p, A p>) of the step; a search direction in fp32 storage (PcgBuffersT::p32) has the patch operator's own kernel
    auto apply = [&]() {
        if constexpr (std::is_same<T, double>::value) {
            if (buf.p32) {
                launch_patch_spmm_x32(A, k, (const float *)buf.p32, buf.part_pq, (const double *)buf.rz0, buf.nb_spmv, s, step);
                return;
            }
        }
        launch_spmm(A, k, (const T *)buf.p, buf.q, buf.part_pq, (const double *)buf.rz0, buf.nb_spmv, s, step, buf.defer_q);
    };
    for (; step < maxit && !done;) {
        // time_kernels = k: every k-th SpMM launch is bracketed with events (a bracket costs the stream ~1.5 us)
        if (time_kernels > 0 && (step % time_kernels) == (time_kernels / 2) && ev_used + 2 <= ctx->spmv_ev.size()) {
            HIP_TRY(hipEventRecord(ctx->spmv_ev[ev_used], s));
            apply();
            HIP_TRY(hipEventRecord(ctx->spmv_ev[ev_used + 1], s));
            ev_used += 2;
        } else {
            apply();
        }
#ifdef REMO_PROBES
        for (int extra = 0; extra < g_tune.extra_apply && buf.p; ++extra)      // (idempotent: the same q and slab again, no dot products)
            launch_spmm(A, k, (const T *)buf.p, buf.q, (double *)nullptr, (const double *)buf.rz0, buf.nb_spmv, s, step, false);
#endif
        bool replaced = false;
        if constexpr (std::is_same<T, float>::value) {
            if (hooks && replace_next) {
                launch_pcg_replace(A, *hooks->A64, k, step, tol2, buf, hooks->f64, hooks->x64, hooks->q64, s);
                hooks->replacements += 1;
                replace_next = false;
                replaced = true;
            }
        }
        if (!replaced) launch_pcg_update(A, k, step, tol2, buf, s);
        launch_pcg_direction(A, k, step, tol2, buf, s, !replaced);
        ++step;
        if (*done_step >= 0) { done = true; break; }   // the device froze every column: the queued launches are no-ops
        if (step % check == 0) {
            // stay one check interval ahead of the device (a step is ~10 launches, ~30 us of host time
            // against ~150 us on the device); the wait also ends when the "done" record appears
            const int target = step - check;
            if (target >= 0) {
                volatile int32_t *flag = &ctx->progress[target % (ctx->progress_len - 1)].step;
                const double t0 = now_ms();
                int spins = 0;
                while (*flag != target && *done_step < 0) {
                    if (++spins > 64) {
                        std::this_thread::yield();
                        if (now_ms() - t0 > 2000.0) {
                            HIP_TRY(hipStreamSynchronize(s));
                            if (*flag != target && *done_step < 0) throw std::runtime_error("PCG progress record not visible to the host");
                        }
                    }
                }
                std::atomic_thread_fence(std::memory_order_acquire);
                if (*done_step >= 0) { done = true; break; }
                const PcgProgress &pr = ctx->progress[target % (ctx->progress_len - 1)];
                for (int c = 0; c < k; ++c)
                    if (!std::isfinite(pr.rz[c])) { res.finite = false; done = true; }
                if (hooks) {   // schedule a residual replacement when the (lagged) history has dropped far enough
                    if (!have_ref) {
                        for (int c = 0; c < k; ++c) rz_ref[c] = pr.rz[c];
                        have_ref = true;
                    } else {
                        bool hit = false;
                        for (int c = 0; c < k; ++c)
                            if (rz_ref[c] > 0.0 && pr.rz[c] > 0.0 && pr.rz[c] <= hooks->factor2 * rz_ref[c]) hit = true;
                        if (hit) {
                            replace_next = true;
                            for (int c = 0; c < k; ++c) rz_ref[c] = pr.rz[c];
                        }
                    }
                }
            }
        }
    }
    launch_pcg_final(k, step, buf, s);
    HIP_TRY(hipStreamSynchronize(s));
    std::atomic_thread_fence(std::memory_order_acquire);
    const PcgProgress &dn = ctx->progress[ctx->progress_len - 1];
    const int last = (dn.step >= 0) ? dn.step : step;   // index of the record that holds the final <Cr,r>
    const PcgProgress &fin = (dn.step >= 0) ? dn : ctx->progress[step % (ctx->progress_len - 1)];
    res.steps = (dn.step >= 0) ? dn.step : step;
    const PcgProgress &p0 = (last == 0) ? fin : ctx->progress[0];
    res.converged = true;
    for (int c = 0; c < k; ++c) {
        res.iters[c] = last;
        const double r0 = p0.rz[c];
        const double thr = std::max(tol2 * r0, floor ? floor[c] : 0.0);
        for (int i = 0; i <= last; ++i) {
            const PcgProgress &pr = (i == last) ? fin : ctx->progress[i % (ctx->progress_len - 1)];
            if (i != last && pr.step != i) continue;
            if (!std::isfinite(pr.rz[c])) res.finite = false;
            if (!(pr.rz[c] > thr)) { res.iters[c] = i; break; }
        }
        const double rl = fin.rz[c];
        res.relres[c] = (r0 > 0.0) ? std::sqrt(rl / r0) : 0.0;
        if (rl > thr) res.converged = false;
        if (!std::isfinite(rl)) res.finite = false;
        if (rz_first) rz_first[c] = r0;
        if (rz_last) rz_last[c] = rl;
    }
    if (st) st->pcg_steps += res.steps;
    return res;
}

}  // namespace

ChunkResult run_pcg(remo_ctx *ctx, const CsrView &A, int k, const double *d_f, PcgBuffers &buf, const remo_opts_t &o,
                    remo_stats_t *st, size_t &ev_used) {
    return run_pcg_t<double>(ctx, A, k, d_f, buf, o.rtol * o.rtol, nullptr, o.maxsteps, o.check_every, o.time_kernels, st, ev_used, nullptr,
                             nullptr);
}

// Warm start: the shape of the mixed mode's outer cycle below, once, in fp64.  The stopping threshold is the one the cold solve
// would have used, rtol^2 <C f, f> of THIS system and preconditioner: one PCG step on A d = f publishes <C f, f> as its step-0 record
// (its x is discarded: the solve below starts from zero again).  Then q = A x_prev (launch_spmm as the mixed mode calls it: the
// patch operator's shared rows are folded, not left in the slab), f' = f - q, and the unchanged PCG from zero on A d = f' with no
// relative target (tol2 = 0) and that threshold as the absolute per-column floor (kFloorSlot: read by the update and the direction
// launch (pcg_kernels.hip pcg_update_head, pcg_direction_head) alike, whatever the storage type; the host's iters / converged
// accounting takes max(tol2 r0, floor)).  A chunk
// whose f' is below the floor freezes every column in the update launch of step 0: zero steps.
ChunkResult run_pcg_warm(remo_ctx *ctx, const CsrView &A, int k, double *d_f, PcgBuffers &buf, double *x_prev, const remo_opts_t &o,
                         remo_stats_t *st, size_t &ev_used) {
    hipStream_t s = ctx->stream;
    const double tol2 = o.rtol * o.rtol;
    double rzf[REMO_MAX_RHS] = {0}, floor[REMO_MAX_RHS] = {0}, last[REMO_MAX_RHS] = {0};
    ChunkResult probe = run_pcg_t<double>(ctx, A, k, d_f, buf, tol2, nullptr, 1, o.check_every, 0, st, ev_used, rzf, nullptr);
    if (!probe.finite) return probe;
    for (int c = 0; c < k; ++c) floor[c] = tol2 * rzf[c];
    launch_spmm(A, k, (const double *)x_prev, buf.q, (double *)nullptr, (const double *)nullptr, buf.nb_spmv, s);
    launch_warm_residual(A.n, k, d_f, buf.q, s);
    ChunkResult out = run_pcg_t<double>(ctx, A, k, d_f, buf, 0.0, floor, o.maxsteps, o.check_every, o.time_kernels, st, ev_used, nullptr, last);
    launch_warm_add(A.n, k, buf.x, x_prev, s);
    for (int c = 0; c < k; ++c) out.relres[c] = rzf[c] > 0.0 ? std::sqrt(last[c] / rzf[c]) : 0.0;
    out.steps += probe.steps;
    HIP_TRY(hipStreamSynchronize(s));
    return out;
}

// Mixed precision (BASELINE config 5): PCG runs in fp32 storage (matrix values, vectors,
// preconditioner; scalars fp64) and its residual is refreshed from fp64 as it goes.  Every time <Cr,r>
// of a column has dropped by `inner_digits` decimal digits, the step's update is replaced by
//   x64 += x32, x32 = 0, r32 = float(f - A64 x64)            (launch_pcg_replace)
// while the search direction and the scalars carry on (residual replacement: the Krylov process is NOT
// restarted, which restart-style refinement pays for with 30-60 % more steps on these matrices).
// When the recurrence says converged, an outer cycle re-measures the TRUE residual in fp64; the solve
// ends with a cycle whose START already meets the target (normally the second one, at the cost of one
// fp64 SpMM and one inner step).  <Cr,r> is measured with the fp32 preconditioner.
ChunkResult run_pcg_mixed(remo_ctx *ctx, const CsrView &A, int k, const double *d_f, PcgBuffers &buf, MixedBuffers &mx, const remo_opts_t &o,
                          remo_stats_t *st, size_t &ev_used) {
    hipStream_t s = ctx->stream;
    const int64_t nk = A.n * k;
    const double tol2 = o.rtol * o.rtol;
    const int digits = o.inner_digits > 0 ? std::min(o.inner_digits, 5) : 3;   // fp32 recurrences do not hold more than ~5 digits
    const double tol2_in = std::pow(10.0, -2.0 * digits);
    ChunkResult out;
    out.converged = false;
    for (int c = 0; c < REMO_MAX_RHS; ++c) { out.iters[c] = 0; out.relres[c] = 0.0; }
    double rz0g[REMO_MAX_RHS] = {0}, floor[REMO_MAX_RHS] = {0}, first[REMO_MAX_RHS], last[REMO_MAX_RHS];
    HIP_TRY(hipMemsetAsync(buf.x, 0, sizeof(double) * nk, s));
    int total = 0;
    const int max_cycles = 40;
    for (int cycle = 0; cycle < max_cycles; ++cycle) {
        if (cycle == 0) {
            launch_mixed_residual(nk, d_f, nullptr, mx.f32, s);
        } else {
            launch_spmm(A, k, (const double *)buf.x, buf.q, (double *)nullptr, (const double *)nullptr, buf.nb_spmv, s);
            launch_mixed_residual(nk, d_f, buf.q, mx.f32, s);
        }
        const int budget = std::max(1, o.maxsteps - total);
        RefineHooks hooks;
        hooks.A64 = &A; hooks.f64 = d_f; hooks.x64 = buf.x; hooks.q64 = buf.q; hooks.factor2 = tol2_in;
        ChunkResult in = run_pcg_t<float>(ctx, mx.A32, k, mx.f32, mx.b32, 0.5 * tol2, cycle ? floor : nullptr, budget, o.check_every,
                                          o.time_kernels, st, ev_used, first, last, &hooks);
        if (st) st->refinement_cycles += hooks.replacements;
        if (cycle == 0)
            for (int c = 0; c < k; ++c) { rz0g[c] = first[c]; floor[c] = 0.5 * tol2 * rz0g[c]; }   // inner target: 0.7 of the outer one in norm
        out.finite = out.finite && in.finite;
        if (!in.finite) break;
        bool met = true;
        for (int c = 0; c < k; ++c) {
            out.relres[c] = rz0g[c] > 0.0 ? std::sqrt(first[c] / rz0g[c]) : 0.0;   // TRUE residual at the start of this cycle
            if (first[c] > tol2 * rz0g[c]) met = false;
        }
        if (met) { out.converged = true; break; }   // nothing to add: every column was frozen at step 0
        launch_mixed_accumulate(nk, buf.x, mx.b32.x, 0, s);
        total += in.steps;
        for (int c = 0; c < k; ++c) out.iters[c] += in.iters[c];
        if (st) st->refinement_cycles += 1;
        if (total >= o.maxsteps) break;
    }
    out.steps = total;
    HIP_TRY(hipStreamSynchronize(s));
    return out;
}

}  // namespace remo
