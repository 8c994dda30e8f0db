// remo_internal.h — what the translation units behind the C ABI share: the context and batch objects, error plumbing and a holder
// for temporary device memory (the process-wide tuning state of remo_debug_tune: tune.h, through kernels.h).  Not installed, not a public header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/remo3d_hip.h"
#include "kernels.h"
#include "amg.h"
#include "symbolic_gpu.h"

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) {                                                                        \
            char buf__[512];                                                                            \
            snprintf(buf__, sizeof buf__, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            throw std::runtime_error(buf__);                                                            \
        }                                                                                               \
    } while (0)

namespace remo {

inline double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// what remo_last_error(NULL) returns: why the last remo_ctx_create / remo_host_symbolic of this thread failed (remo_api.hip)
extern thread_local std::string g_create_error;

// Symmetric positive definite (leading principal minors > 0) and finite: the upper triangle of one material's tensor (remo_host.cpp)
bool tensor_ok(int dim, const double *S);

// Temporary device memory of one entry point, freed when the holder leaves scope (normal and error path alike).  hipFree
// synchronises the device: the holder's scope ends where the call has drained its stream.
struct DeviceTemp {
    std::vector<void *> held;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp &) = delete;
    ~DeviceTemp() { for (void *p : held) (void)hipFree(p); }
    template <class T> T *alloc(size_t count) {
        held.push_back(nullptr);
        HIP_TRY(hipMalloc(&held.back(), sizeof(T) * count));
        return static_cast<T *>(held.back());
    }
};

// the fp32 instantiation of a patch operator on the same tables: the slab and the partial sums are scratch of one application, so
// both storage types share them (dot_bins is the applying solve's to set)
inline PatchOpT<float> patch_view32(const PatchOpT<double> &p) {
    return PatchOpT<float>{p.t, reinterpret_cast<float *>(p.Yb), p.ppart, p.lds_rows};
}

}  // namespace remo

struct remo_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    remo::Arena ar;
    double *d_M2 = nullptr, *d_M3 = nullptr, *d_M2q = nullptr;   // reference tensors: exact 2D / 3D, 2D by the degree-4 rule
    double *d_B3 = nullptr;                  // factors of the 3D tensors (ref_factors3) for the sensitivity contraction, uploaded by its first use
    double sens_ms = 0.0, sens_bytes = 0.0;  // last remo_solve_batch_sens: HIP-event time and algorithmic bytes of the contraction launches (remo_debug_sens_timing)
    double sens_group_ms[4] = {};            // last remo_solve_batch_sens_groups: group order; with time_kernels also the material pass, the per-element pass and the group sums, each over all functionals (remo_debug_sens_group_timing)
    double pair_ms[2] = {};                  // last job with pairs: HIP-event time of the pair pass (element launches + reduction) and its launch count (remo_debug_pairs_timing)
    double pair_group_ms[4] = {};            // last job with pair_n_group > 0: HIP-event time of the group order; of the per-element launches and of the group sums (apart only with time_kernels, else both in [1]); the number of slices (remo_debug_pair_groups_timing)
    double field_ms[2] = {};                 // last remo_solve_batch_field / remo_batch_field: HIP-event time of the location of the points and of the evaluation launches (remo_debug_field_timing)
    hipEvent_t fev[4] = {};                  // their events, created by the first use
    double sec_ms = 0.0;                     // last remo_batch_run with remo_job_secondary_t.secondary: HIP-event time of the load-vector launches, all chunks (remo_debug_secondary_timing)
    int point_location = 0;                  // last remo_batch_run: 0 = axis kernels, 1 = cell grid (remo_debug_point_location)
    int direction_bytes = 0;                 // last remo_batch_run: bytes per stored value of the PCG's search direction, 4 or 8 (remo_debug_direction_bytes)
    remo::PcgProgress *progress = nullptr;  // mapped, coherent host memory
    remo::PcgProgress *progress_dev = nullptr;
    int progress_len = 0;
    int32_t *d_err = nullptr;
    hipEvent_t ev[8] = {};
    std::vector<hipEvent_t> spmv_ev;
    uint64_t run_id = 0;  // the arena holds the system / solution of the batch that ran last
    // input pool of the one-shot entry (remo_solve_batch): the mesh arrays of the batch in hand, grow-only - a sweep of thousands of
    // batches then makes no hipMalloc / hipFree per batch (hipFree synchronises the whole device, i.e. the other contexts' streams)
    char *in_pool = nullptr;
    size_t in_cap = 0;
    double floor_stage[REMO_MAX_RHS] = {};   // host staging of the mixed mode's <Cr,r> floors (outlives the async copy)

    template <class T> T *take(size_t count) { return ar.lo<T>(count); }
    void reserve(size_t bytes) {
        ar.reset();
        if (bytes <= ar.cap) return;
        HIP_TRY(hipStreamSynchronize(stream));
        if (ar.base) HIP_TRY(hipFree(ar.base));
        ar.base = nullptr;
        ar.cap = 0;
        const size_t want = remo::align_up(bytes + bytes / 4, 4096);  // the top-down end must stay aligned too
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ar.base), want));
        ar.cap = want;
    }
    void ensure_progress(int len) {
        if (len <= progress_len) return;
        if (progress) HIP_TRY(hipHostFree(progress));
        progress = nullptr;
        progress_len = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&progress), sizeof(remo::PcgProgress) * size_t(len),
                              hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&progress_dev), progress, 0));
        progress_len = len;
    }
};

// What remo_solve_batch_sens adds to a batch: linear functionals J_j = sum_i w[i] u_rhs[j](p[i]) and where their values and
// derivatives go (host pointers of the caller, valid for the duration of the call only).  The points are the batch's fun_p.
struct remo_sens_request {
    int n_fun = 0;
    const int32_t *fun_rhs = nullptr, *fun_ptr = nullptr;
    const double *fun_w = nullptr;
    double *J_out = nullptr, *dJ_out = nullptr;
    // remo_solve_batch_sens_groups: the caller's group of every element (host array, checked by the entry) and where the sums go
    int32_t n_group = 0;
    const int32_t *group = nullptr;
    double *dJg_out = nullptr;
    // remo_job_error_t.err: error estimates of the functionals (errest.h), with a grouping of their own (checked by the entry)
    bool err = false;
    int32_t err_n_group = 0;
    const int32_t *err_group = nullptr;
    double *err_out = nullptr, *errg_out = nullptr;
};

// What remo_solve_batch_field adds to a batch: points of the mesh, the right-hand sides whose solution is read there and where the
// values go (host pointers of the caller, valid for the duration of the call only; every output may be NULL).
struct remo_field_request {
    int64_t n_pts = 0;
    const double *pts = nullptr;          // [n_pts * dim]
    int32_t n_frhs = 0;
    const int32_t *field_rhs = nullptr;   // [n_frhs], each in [0, n_rhs)
    double *u = nullptr, *grad = nullptr, *J = nullptr;
    int32_t *elem = nullptr;
};

// What remo_job_pairs_t adds to a batch: pairs of right-hand sides (a, b) and where -u_a^T (dA/dsigma) u_b goes (host pointers of the
// caller, checked by the entry, valid for the duration of the call only).  A batch with pairs has a `sens` request too (n_fun may be
// 0): the forward solutions stay in the arena for the pass (pairs.h).
struct remo_pairs_request {
    int n_pair = 0;
    const int32_t *pair_a = nullptr, *pair_b = nullptr;
    double *dP_out = nullptr;
    // remo_job_pair_groups_t: the caller's group of every element (host array, checked by the entry) and where the sums per (pair, group) go
    int32_t n_group = 0;
    const int32_t *group = nullptr;
    double *dPg_out = nullptr;
};

struct remo_warm;   // warm.h

struct remo_batch {
    int dim = 0;
    int64_t nv = 0, nt = 0, nbf = 0;
    int n_mat = 0;
    int sigma_comp = 1;      // doubles per material in d_sigma: 1 = scalar; 3 (2D) / 6 (3D) = upper triangle of a tensor (remo_solve_batch_tensor)
    // points: per chunk [sources..., evals...]
    int n_rhs = 0;
    std::vector<int32_t> src_ptr, eval_ptr;
    std::vector<double> src_p, src_I, eval_p;   // points: dim coordinates each; the axis entries store (0, .., z)
    std::vector<double> fun_p;                  // the points of `sens`'s functionals, likewise
    // resident device inputs (everything the path reads is in HBM before remo_batch_run)
    double *d_coords = nullptr, *d_sigma = nullptr;
    int32_t *d_mat = nullptr, *d_conn = nullptr, *d_bconn = nullptr;
    uint8_t *d_bdir = nullptr;
    bool pooled = false;     // the six arrays live in the context's input pool (remo_solve_batch): not freed with the batch
    const remo_sens_request *sens = nullptr;   // remo_solve_batch_sens: adjoint solves + contraction after the forward solves (batch_run.hip)
    const remo_pairs_request *pairs = nullptr; // remo_job_pairs_t: derivatives of u_a(x_b) for pairs of forward columns, one element pass (batch_run.hip, pairs.hip)
    remo_warm *warm = nullptr;                 // remo_solve_batch_sens_warm: where the solutions of the previous call are, and where these go (warm.h)
    const remo_field_request *field = nullptr; // remo_solve_batch_field: the solution at arbitrary points, chunk by chunk (batch_run.hip, field.hip)
    // remo_job_secondary_t.secondary: the secondary-potential formulation (secondary.h) - element rule, sphere of the primary field and the
    // background conductivity of every right-hand side as the entry resolved it
    bool secondary = false;
    int sec_quad = 0;
    double sec_radius = 0.0;
    std::vector<double> sec_sigma0;
    bool eval_only = false;  // remo_solve_batch: nothing reads the solution after the run but the evaluation points (PcgBuffersT::x_ev)
    // last system (pointers into the context arena; valid until the next run on the context)
    bool has_system = false;
    remo::DeviceSymbolic sym;
    remo::CsrView A{};
    double *d_val = nullptr, *d_dinv = nullptr;
    double *d_x = nullptr, *d_C = nullptr;  // solution block [n][k_last] and metric terms of the last run
    double *d_f = nullptr;                  // load vectors [n][k_last] of the last chunk
    remo::PatchOpT<double> patch64{};       // patch operator of the last run (remo_opts_t.op = 3), pointers into the arena
    remo::PatchOpT<float> patch32{};
    remo::AmgT<double> amg64{};             // multigrid hierarchy of the vertex block of the last run (arena)
    remo::AmgT<float> amg32{};
    int k_last = 0;
    // the axis points of the last chunk (arena): what the recovery of a condensed cell bubble reads (remo_batch_field)
    const int32_t *d_prhs_last = nullptr, *d_found_last = nullptr;
    const double *d_pI_last = nullptr, *d_fint_last = nullptr;
    int nq_last = 0;
    const double *d_M_last = nullptr;       // reference tensors of the last run (remo_opts_t.quadrature)
    uint64_t run_id = 0;
    std::vector<double> u_out;
};

namespace remo {

inline int fail(remo_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// A batch's mesh with metric terms C[nt][NTERM] and reference tensors M as the element kernels read it (elem_access.h): a view, valid
// while the batch's numbering (pointers into the context's arena) is
inline ElemMesh elem_mesh(const remo_batch *b, const double *C, const double *M) {
    const DeviceSymbolic &sy = b->sym;
    ElemMesh em;
    em.dim = b->dim; em.condense = sy.condense; em.nt = b->nt;
    em.coords = b->d_coords; em.conn = sy.conn; em.mat = b->d_mat; em.eperm = sy.eperm;
    em.sigma = b->d_sigma; em.sigma_comp = b->sigma_comp; em.n_mat = b->n_mat;
    em.eldof = sy.eldof; em.C = C; em.M = M;
    em.adjptr = sy.adjptr; em.adj = sy.adj;
    return em;
}

// The host checks of a batch's mesh, conductivities, sources and evaluation points: everything that is refused before any device
// work (remo_api.hip).  full: src_p / eval_p hold dim coordinates per point (the job entries) and are checked for finiteness here;
// else they hold axis positions z, and a bad one is found when the points are located.
int check_batch_args(remo_ctx *ctx, const remo_mesh_t *mesh, const remo_job_t &j, bool full);

}  // namespace remo
