// warm.h — remo_warm_t: the solutions of one remo_solve_batch_sens_warm call kept on the device for the next one (warm.hip), and
// the two stream kernels of a warm chunk.
#pragma once
#include "remo_internal.h"

// One device allocation (plain hipMalloc, grow-only) with the forward and adjoint solutions of the last successful call in the layout
// of Sens::block (batch_run.hip).  Tied to a device, not to a context.
struct remo_warm {
    int device = 0;
    double *d = nullptr;
    size_t cap = 0;             // doubles allocated
    bool filled = false;
    int32_t used_last = 0;      // the last call that was handed this object started from its solutions
    // what the stored solutions belong to (compared for memory safety only: a stale guess costs steps, never accuracy)
    int dim = 0, condense = 0, n_rhs = 0, n_fun = 0;
    int64_t n_nodes = 0, n_elems = 0, n_bfacets = 0, n_free = 0;
};

namespace remo {

// doubles of a warm object for n rows: Sens::block's layout (adjoint part on a 32-double boundary) + the slack of a taken vector
inline size_t warm_doubles(int64_t n, int n_rhs, int n_fun) { return (size_t(n) * size_t(n_rhs) + 31) / 32 * 32 + size_t(n) * size_t(n_fun) + 64; }
bool warm_matches(const remo_warm *w, const remo_batch *b, int condense, int64_t n_free);
void warm_reserve(remo_warm *w, size_t doubles);                                          // grow-only; growing loses the contents
void warm_label(remo_warm *w, const remo_batch *b, int condense, int64_t n_free);         // the object now holds this batch's solutions

int stream_grid(int64_t n);   // kernels.hip
// f -= q over n rows of k columns (the residual of the previous solutions: f' = f - A x_prev)
void launch_warm_residual(int64_t n, int k, double *f, const double *q, hipStream_t s);
// x = x_prev + d where d lies in x; the sum goes to x (what the contraction reads) and to x_prev (the warm object), one pass
void launch_warm_add(int64_t n, int k, double *x, double *x_prev, hipStream_t s);

}  // namespace remo
