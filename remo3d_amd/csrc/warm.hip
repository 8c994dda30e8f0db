// warm.hip — remo_warm_t (include/remo3d_hip.h): the solutions of a remo_solve_batch_sens_warm call kept on the device, so that
// the next call on nearly the same conductivities solves for a correction instead of starting every column from zero
// (pcg_host.hip run_pcg_warm), and the two stream kernels of that correction.
#include <cstring>
#include <type_traits>

#include "warm.h"

namespace remo {

bool warm_matches(const remo_warm *w, const remo_batch *b, int condense, int64_t n_free) {
    return w->filled && w->d && w->dim == b->dim && w->n_nodes == b->nv && w->n_elems == b->nt && w->n_bfacets == b->nbf && w->condense == condense &&
           w->n_free == n_free && w->n_rhs == b->n_rhs && w->n_fun == (b->sens ? b->sens->n_fun : 0) && warm_doubles(n_free, w->n_rhs, w->n_fun) <= w->cap;
}

void warm_reserve(remo_warm *w, size_t doubles) {
    if (doubles <= w->cap) return;
    w->filled = false;
    if (w->d) HIP_TRY(hipFree(w->d));
    w->d = nullptr;
    w->cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&w->d), sizeof(double) * doubles));
    w->cap = doubles;
}

void warm_label(remo_warm *w, const remo_batch *b, int condense, int64_t n_free) {
    w->dim = b->dim; w->n_nodes = b->nv; w->n_elems = b->nt; w->n_bfacets = b->nbf; w->condense = condense;
    w->n_free = n_free; w->n_rhs = b->n_rhs; w->n_fun = b->sens ? b->sens->n_fun : 0;
    w->filled = true;
}

// Streams over n K doubles.  K even: 16 bytes per lane and access (the blocks start on 64-byte boundaries: taken buffers, and
// chunks of n * REMO_MAX_RHS doubles inside them); K odd: 8 bytes.  Grid-stride, no LDS, nothing indexed at run time.
template <int K> struct WarmVec {
    static constexpr int V = (K % 2 == 0) ? 2 : 1;
    using type = typename std::conditional<V == 2, double2, double>::type;
};
__device__ __forceinline__ double vsub(double a, double b) { return a - b; }
__device__ __forceinline__ double2 vsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double vadd(double a, double b) { return a + b; }
__device__ __forceinline__ double2 vadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

template <int K>
__global__ void __launch_bounds__(256) k_warm_residual(int64_t n, double *__restrict__ f, const double *__restrict__ q) {
    using V = typename WarmVec<K>::type;
    const int64_t m = n * K / WarmVec<K>::V;
    V *fv = reinterpret_cast<V *>(f);
    const V *qv = reinterpret_cast<const V *>(q);
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) fv[i] = vsub(fv[i], qv[i]);
}

template <int K>
__global__ void __launch_bounds__(256) k_warm_add(int64_t n, double *__restrict__ x, double *__restrict__ x_prev) {
    using V = typename WarmVec<K>::type;
    const int64_t m = n * K / WarmVec<K>::V;
    V *xv = reinterpret_cast<V *>(x), *pv = reinterpret_cast<V *>(x_prev);
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < m; i += int64_t(gridDim.x) * blockDim.x) {
        const V sum = vadd(pv[i], xv[i]);
        xv[i] = sum;
        pv[i] = sum;
    }
}

// (the warm object is sized by the caller's k: a k outside 1 .. REMO_MAX_RHS is an error here, not a launch with K = 8)
static void warm_check_k(int k) {
    if (k < 1 || k > REMO_MAX_RHS) throw std::runtime_error("warm start: more columns than REMO_MAX_RHS");
}

void launch_warm_residual(int64_t n, int k, double *f, const double *q, hipStream_t s) {
    if (n <= 0) return;
    warm_check_k(k);
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        hipLaunchKernelGGL(k_warm_residual<K>, dim3(stream_grid(n * k / WarmVec<K>::V)), dim3(256), 0, s, n, f, q);
    });
}

void launch_warm_add(int64_t n, int k, double *x, double *x_prev, hipStream_t s) {
    if (n <= 0) return;
    warm_check_k(k);
    for_k(k, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        hipLaunchKernelGGL(k_warm_add<K>, dim3(stream_grid(n * k / WarmVec<K>::V)), dim3(256), 0, s, n, x, x_prev);
    });
}

}  // namespace remo

using namespace remo;

extern "C" {

remo_warm_t *remo_warm_create(int device_id) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e);
        return nullptr;
    }
    if (device_id < 0 || device_id >= ndev) {
        g_create_error = "device_id out of range";
        return nullptr;
    }
    remo_warm *w = new remo_warm();
    w->device = device_id;
    return w;
}

void remo_warm_destroy(remo_warm_t *w) {
    if (!w) return;
    if (w->d) {
        (void)hipSetDevice(w->device);
        (void)hipFree(w->d);
    }
    delete w;
}

void remo_warm_clear(remo_warm_t *w) {
    if (!w) return;
    w->filled = false;
    w->used_last = 0;
}

int remo_warm_info(const remo_warm_t *w, int64_t *n_free, int32_t *n_cols, int64_t *bytes, int32_t *used_last) {
    if (!w) return REMO_ERR_ARG;
    if (n_free) *n_free = w->filled ? w->n_free : 0;
    if (n_cols) *n_cols = w->filled ? w->n_rhs + w->n_fun : 0;
    if (bytes) *bytes = int64_t(w->cap * sizeof(double));
    if (used_last) *used_last = w->used_last;
    return REMO_OK;
}

}  // extern "C"
