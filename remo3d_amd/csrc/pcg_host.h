// pcg_host.h — host side of the PCG (pcg_host.hip): the launch loop of one solve, its wait on the mapped progress records, and
// the mixed-precision mode's outer cycle with residual replacement.
#pragma once
#include "remo_internal.h"

namespace remo {

struct ChunkResult {
    int steps = 0;
    bool converged = false;
    bool finite = true;
    int iters[REMO_MAX_RHS];
    double relres[REMO_MAX_RHS];
};

// the fp32 image of a solve for the mixed mode's inner solver (batch_run.hip mixed_buffers)
struct MixedBuffers {
    CsrViewT<float> A32{};
    PcgBuffersT<float> b32{};
    float *f32 = nullptr;
};

// one chunk of k right-hand sides in fp64 / with the fp32 inner solver; both end with the stream drained
ChunkResult run_pcg(remo_ctx *ctx, const CsrView &A, int k, const double *d_f, PcgBuffers &buf, const remo_opts_t &o, remo_stats_t *st,
                    size_t &ev_used);
ChunkResult run_pcg_mixed(remo_ctx *ctx, const CsrView &A, int k, const double *d_f, PcgBuffers &buf, MixedBuffers &mx, const remo_opts_t &o,
                          remo_stats_t *st, size_t &ev_used);

// Warm-started chunk (remo_solve_batch_sens_warm): x_prev holds the previous call's solutions of these k columns.  d_f is
// overwritten with f - A x_prev; buf.x ends as x_prev + d, and so does x_prev.  warm.h
ChunkResult run_pcg_warm(remo_ctx *ctx, const CsrView &A, int k, double *d_f, PcgBuffers &buf, double *x_prev, const remo_opts_t &o,
                         remo_stats_t *st, size_t &ev_used);

}  // namespace remo
