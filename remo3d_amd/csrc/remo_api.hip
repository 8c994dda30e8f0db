// remo_api.hip — the C ABI of include/remo3d_hip.h: context, resident batches (creation, one-shot solves, fetch) and the
// inspection entries that read a batch's last system.  remo_batch_run itself is batch_run.hip; the probes are remo_debug.hip,
// the CPU hooks remo_host.cpp.  remo_batch_field / remo_batch_eval launch their element kernels with resident_mesh: the ElemMesh view
// (elem_access.h) of the batch's last system, built by the same elem_mesh as the run's.
#include <limits.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "remo_internal.h"
#include "fem_p3.h"
#include "field.h"
#include "warm.h"
#include "secondary.h"

using namespace remo;

namespace remo {
thread_local std::string g_create_error;
}

// n points as the batch keeps them, dim coordinates each: from full coordinates (full) or from axis positions z, (0, .., z)
static void store_points(std::vector<double> &to, const double *from, int n, int dim, bool full) {
    if (n <= 0) { to.clear(); return; }
    if (full) { to.assign(from, from + size_t(n) * dim); return; }
    to.assign(size_t(n) * dim, 0.0);
    for (int q = 0; q < n; ++q) to[size_t(q) * dim + dim - 1] = from[q];
}

// the host checks of batch_create (remo_internal.h).  j.tensor: sigma holds n_mat upper triangles instead of n_mat scalars
int remo::check_batch_args(remo_ctx *ctx, const remo_mesh_t *mesh, const remo_job_t &j, bool full) {
    if (!ctx) return REMO_ERR_ARG;
    const bool tensor = j.tensor != 0;
    if (!mesh || !j.sigma || j.n_mat <= 0 || j.n_rhs <= 0 || !j.src_ptr || !j.eval_ptr)
        return fail(ctx, REMO_ERR_ARG, "null or empty argument");
    if (mesh->dim != 2 && mesh->dim != 3) return fail(ctx, REMO_ERR_ARG, "dim must be 2 or 3");
    if (mesh->n_nodes <= 0 || mesh->n_elems <= 0 || !mesh->coords || !mesh->conn || !mesh->mat)
        return fail(ctx, REMO_ERR_ARG, "empty mesh");
    if (mesh->n_bfacets < 0 || (mesh->n_bfacets > 0 && (!mesh->bconn || !mesh->bdirichlet)))
        return fail(ctx, REMO_ERR_ARG, "boundary arrays missing");
    if (mesh->n_nodes >= (int64_t(1) << 31) || mesh->n_elems >= (int64_t(1) << 27)) return fail(ctx, REMO_ERR_ARG, "mesh too large");
    if (j.src_ptr[0] != 0 || j.eval_ptr[0] != 0) return fail(ctx, REMO_ERR_ARG, "src_ptr / eval_ptr must start at 0");
    for (int k = 0; k < j.n_rhs; ++k)
        if (j.src_ptr[k + 1] < j.src_ptr[k] || j.eval_ptr[k + 1] < j.eval_ptr[k]) return fail(ctx, REMO_ERR_ARG, "src_ptr / eval_ptr not monotone");
    if ((j.src_ptr[j.n_rhs] > 0 && (!j.src_p || !j.src_I)) || (j.eval_ptr[j.n_rhs] > 0 && !j.eval_p)) return fail(ctx, REMO_ERR_ARG, "point arrays missing");
    const int dim = mesh->dim;
    for (int64_t i = 0; i < mesh->n_nodes * dim; ++i)
        if (!std::isfinite(mesh->coords[i])) return fail(ctx, REMO_ERR_MESH, "non-finite coordinate");
    if (full) {   // the job entries: before any device work
        for (int64_t i = 0; i < int64_t(j.src_ptr[j.n_rhs]) * dim; ++i)
            if (!std::isfinite(j.src_p[i])) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
        for (int64_t i = 0; i < int64_t(j.eval_ptr[j.n_rhs]) * dim; ++i)
            if (!std::isfinite(j.eval_p[i])) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
    }
    const int ncomp = tensor ? ((dim == 2) ? 3 : 6) : 1;
    if (tensor) {
        for (int i = 0; i < j.n_mat; ++i)
            if (!tensor_ok(dim, j.sigma + size_t(i) * ncomp))
                return fail(ctx, REMO_ERR_ARG, "sigma_tensor of material " + std::to_string(i) + " is not finite and positive definite");
    } else {
        for (int i = 0; i < j.n_mat; ++i)
            if (!(j.sigma[i] > 0.0) || !std::isfinite(j.sigma[i])) return fail(ctx, REMO_ERR_ARG, "sigma must be positive and finite");
    }
    return REMO_OK;
}


extern "C" {


int remo_abi_version(void) { return REMO_ABI_VERSION; }

void remo_opts_default(remo_opts_t *o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->preconditioner = 1;  // remo3d.py:82 default "multigrid" => best available
    o->condense = 1;        // remo3d.py:83
    o->maxsteps = 1000;     // ngsolve_functions.py:50
    o->check_every = 5;
    o->rtol = 1e-8;         // NGSolve CGSolver default precision
    o->time_kernels = 0;
    o->coarse_degree = 0;   // 0 = by dimension and size (remo_batch_run): e.g. Chebyshev(5) on [lmax/90, lmax] at 1e4 vertices in 3D
    o->coarse_ratio = 0;
    o->coarse = 0;          // by dimension: multigrid cycle on the vertex block in 2D, Chebyshev polynomial in 3D
}

remo_ctx_t *remo_ctx_create(int device_id) {
    remo_ctx *ctx = nullptr;
    try {
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
        ctx = new remo_ctx();
        ctx->device = device_id;
        HIP_TRY(hipSetDevice(device_id));
        HIP_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        for (auto &ev : ctx->ev) HIP_TRY(hipEventCreate(&ev));
        const double *m2 = ref_tables(2), *m3 = ref_tables(3);
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_M2), sizeof(double) * 9 * 100));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_M3), sizeof(double) * 6 * 400));
        HIP_TRY(hipMemcpy(ctx->d_M2, m2, sizeof(double) * 9 * 100, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(ctx->d_M3, m3, sizeof(double) * 6 * 400, hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_M2q), sizeof(double) * 9 * 100));
        HIP_TRY(hipMemcpy(ctx->d_M2q, ref_tables2_rule4(), sizeof(double) * 9 * 100, hipMemcpyHostToDevice));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_err), sizeof(int32_t)));
        ctx->ensure_progress(1024 + 2);
        return ctx;
    } catch (const std::exception &ex) {
        g_create_error = ex.what();
        delete ctx;
        return nullptr;
    }
}

void remo_ctx_destroy(remo_ctx_t *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    for (auto &ev : ctx->spmv_ev) hipEventDestroy(ev);
    for (auto &ev : ctx->ev)
        if (ev) hipEventDestroy(ev);
    for (auto &ev : ctx->fev)
        if (ev) hipEventDestroy(ev);
    if (ctx->ar.base) hipFree(ctx->ar.base);
    if (ctx->in_pool) hipFree(ctx->in_pool);
    if (ctx->d_M2) hipFree(ctx->d_M2);
    if (ctx->d_M3) hipFree(ctx->d_M3);
    if (ctx->d_M2q) hipFree(ctx->d_M2q);
    if (ctx->d_B3) hipFree(ctx->d_B3);
    if (ctx->d_err) hipFree(ctx->d_err);
    if (ctx->progress) hipHostFree(ctx->progress);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *remo_last_error(remo_ctx_t *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// The head of a job - conductivities, sources, evaluation points - checked and uploaded.  full: src_p / eval_p are full coordinates
// (the job entries), else axis positions z (every other entry, through axis_job).  pooled: the inputs go into the context's pool.
static int batch_create(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, bool full, remo_batch_t **out, bool pooled) {
    if (!ctx) return REMO_ERR_ARG;
    if (!out) return fail(ctx, REMO_ERR_ARG, "null or empty argument");
    if (int rc = check_batch_args(ctx, mesh, j, full)) return rc;
    const int dim = mesh->dim, nb = dim + 1;
    const int ncomp = j.tensor ? ((dim == 2) ? 3 : 6) : 1;
    remo_batch *b = nullptr;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        b = new remo_batch();
        b->dim = dim; b->nv = mesh->n_nodes; b->nt = mesh->n_elems; b->nbf = mesh->n_bfacets; b->n_mat = j.n_mat;
        b->sigma_comp = ncomp;
        b->n_rhs = j.n_rhs;
        b->src_ptr.assign(j.src_ptr, j.src_ptr + j.n_rhs + 1);
        b->eval_ptr.assign(j.eval_ptr, j.eval_ptr + j.n_rhs + 1);
        store_points(b->src_p, j.src_p, j.src_ptr[j.n_rhs], dim, full);
        if (j.src_ptr[j.n_rhs] > 0) b->src_I.assign(j.src_I, j.src_I + j.src_ptr[j.n_rhs]);
        store_points(b->eval_p, j.eval_p, j.eval_ptr[j.n_rhs], dim, full);
        hipStream_t s = ctx->stream;
        b->pooled = pooled;
        size_t pool_at = 0;
        if (pooled) {     // one grow-only device buffer per context holds the inputs of the batch in hand
            const size_t need = align_up(sizeof(double) * size_t(b->nv) * dim) + align_up(sizeof(int32_t) * size_t(b->nt) * nb) + align_up(sizeof(int32_t) * size_t(b->nt)) +
                                align_up(sizeof(double) * size_t(j.n_mat) * ncomp) + align_up(sizeof(int32_t) * size_t(b->nbf) * dim + 4) + align_up(size_t(b->nbf) + 4) + 4096;
            if (need > ctx->in_cap) {
                HIP_TRY(hipStreamSynchronize(s));
                if (ctx->in_pool) HIP_TRY(hipFree(ctx->in_pool));
                ctx->in_pool = nullptr; ctx->in_cap = 0;
                const size_t want = align_up(need + need / 4, 4096);
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->in_pool), want));
                ctx->in_cap = want;
            }
        }
        auto up = [&](auto **dst, const auto *src, size_t count) {
            using T = std::remove_const_t<std::remove_pointer_t<decltype(src)>>;
            if (pooled) {
                *dst = reinterpret_cast<T *>(ctx->in_pool + pool_at);
                pool_at += align_up(sizeof(T) * (count ? count : 1));
            } else {
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(dst), sizeof(T) * (count ? count : 1)));
            }
            if (count) HIP_TRY(hipMemcpyAsync(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice, s));
        };
        up(&b->d_coords, mesh->coords, size_t(b->nv) * dim);
        up(&b->d_conn, mesh->conn, size_t(b->nt) * nb);
        up(&b->d_mat, mesh->mat, size_t(b->nt));
        up(&b->d_sigma, j.sigma, size_t(j.n_mat) * ncomp);
        up(&b->d_bconn, mesh->bconn, size_t(b->nbf) * dim);
        up(&b->d_bdir, mesh->bdirichlet, size_t(b->nbf));
        HIP_TRY(hipStreamSynchronize(s));
        b->u_out.assign(size_t(j.eval_ptr[j.n_rhs]), std::nan(""));
        *out = b;
        return REMO_OK;
    } catch (const std::exception &ex) {
        remo_batch_destroy(ctx, b);
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

// The head of an argument-list entry as a job (scalar conductivities; the _tensor entries set j.tensor): src_p / eval_p hold its axis
// positions z, so the job goes on with full = false.  The entries add the members of their parts by name.
static remo_job_t axis_job(int32_t n_mat, const double *sigma, int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                           const int32_t *eval_ptr, const double *eval_z, double *u_out) {
    remo_job_t j;
    std::memset(&j, 0, sizeof j);
    j.size = sizeof j;
    j.n_mat = n_mat; j.sigma = sigma;
    j.n_rhs = n_rhs; j.src_ptr = src_ptr; j.src_p = src_z; j.src_I = src_I;
    j.eval_ptr = eval_ptr; j.eval_p = eval_z; j.u_out = u_out;
    return j;
}

int remo_batch_create(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                      const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                      const double *eval_z, remo_batch_t **out) {
    return batch_create(ctx, mesh, axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, nullptr), false, out, false);
}

int remo_batch_create_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                             const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                             const double *eval_z, remo_batch_t **out) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, nullptr);
    j.tensor = 1;
    return batch_create(ctx, mesh, j, false, out, false);
}

void remo_batch_destroy(remo_ctx_t *ctx, remo_batch_t *b) {
    if (!b) return;
    if (ctx) (void)hipSetDevice(ctx->device);
    if (!b->pooled)
    for (void *p : {(void *)b->d_coords, (void *)b->d_mat, (void *)b->d_sigma, (void *)b->d_conn, (void *)b->d_bconn, (void *)b->d_bdir})
        if (p) (void)hipFree(p);
    delete b;
}

int remo_batch_fetch(remo_ctx_t *ctx, remo_batch_t *b, double *u_out) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || (!u_out && !b->u_out.empty())) return fail(ctx, REMO_ERR_ARG, "null argument");
    if (!b->u_out.empty()) std::memcpy(u_out, b->u_out.data(), sizeof(double) * b->u_out.size());
    return REMO_OK;
}

// every output the job names: NaN, elem_f -1 (sizes from the job's own counts; arrays that cannot be sized are left alone)
static void job_nan_fill(const remo_mesh_t *mesh, const remo_job_t &j) {
    const int dim = (mesh && mesh->dim == 2) ? 2 : 3;
    const size_t ncomp = (j.tensor && mesh) ? ((dim == 2) ? 3 : 6) : 1;   // (no mesh: the call is refused, and nothing sizes a triangle)
    auto fill = [](double *a, size_t n) { for (size_t i = 0; a && i < n; ++i) a[i] = std::nan(""); };
    if (j.eval_ptr && j.n_rhs > 0 && j.eval_ptr[j.n_rhs] > 0) fill(j.u_out, size_t(j.eval_ptr[j.n_rhs]));
    if (j.n_fun > 0) {
        fill(j.J_out, size_t(j.n_fun));
        if (j.n_mat > 0) fill(j.dJ_out, size_t(j.n_fun) * size_t(j.n_mat) * ncomp);
        if (j.n_group > 0) fill(j.dJg_out, size_t(j.n_fun) * size_t(j.n_group) * ncomp);
    }
    if (j.n_pts > 0) {
        const size_t nv = (j.n_frhs > 0) ? size_t(j.n_pts) * size_t(j.n_frhs) : 0;
        fill(j.u_f, nv); fill(j.grad_f, nv * dim); fill(j.J_f, nv * dim);
        for (int32_t i = 0; j.elem_f && i < j.n_pts; ++i) j.elem_f[i] = -1;
    }
}

// The parts of a one-shot call that its ENTRY names (not its counts: remo_solve_batch_sens with n_fun = 0 is a sens call).  A warm
// object and the secondary formulation need no flag: j.warm, and the `sec` of solve_one.
enum : unsigned { kFun = 1, kGroups = 2, kField = 4 };

// the functionals of a job (and its groups), on the host arrays, before any device work
static int check_functionals(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, unsigned parts, bool full) {
    if (parts & kGroups) {
        if (j.n_group < 1 || !j.group) return fail(ctx, REMO_ERR_ARG, "n_group must be at least 1 and group must be given");
        if (!mesh || mesh->n_elems <= 0) return fail(ctx, REMO_ERR_ARG, "empty mesh");
        if (j.n_fun > 0 && !j.dJg_out) return fail(ctx, REMO_ERR_ARG, "dJg_out missing");
        for (int64_t e = 0; e < mesh->n_elems; ++e)
            if (j.group[e] < -1 || j.group[e] >= j.n_group) return fail(ctx, REMO_ERR_ARG, "group id of element " + std::to_string(e) + " outside [-1, n_group)");
    }
    if (j.n_fun < 0 || (j.n_fun > 0 && (!j.fun_rhs || !j.fun_ptr || !j.J_out || !j.dJ_out))) return fail(ctx, REMO_ERR_ARG, "functional arrays missing");
    if (j.n_fun <= 0) return REMO_OK;
    if (j.fun_ptr[0] != 0) return fail(ctx, REMO_ERR_ARG, "fun_ptr must start at 0");
    for (int f = 0; f < j.n_fun; ++f) {
        if (j.fun_ptr[f + 1] < j.fun_ptr[f]) return fail(ctx, REMO_ERR_ARG, "fun_ptr not monotone");
        if (j.fun_rhs[f] < 0 || j.fun_rhs[f] >= j.n_rhs) return fail(ctx, REMO_ERR_ARG, "fun_rhs names no right-hand side of the batch");
    }
    const int nq = j.fun_ptr[j.n_fun];
    if (nq > 0 && (!j.fun_p || !j.fun_w)) return fail(ctx, REMO_ERR_ARG, "functional arrays missing");
    for (int q = 0; q < nq; ++q)
        if (!std::isfinite(j.fun_w[q])) return fail(ctx, REMO_ERR_ARG, "non-finite functional weight");
    if (full && mesh && (mesh->dim == 2 || mesh->dim == 3))
        for (int64_t i = 0; i < int64_t(nq) * mesh->dim; ++i)
            if (!std::isfinite(j.fun_p[i])) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
    return REMO_OK;
}

// the error estimates of a job (remo_job_error_t), likewise: what they do not combine with, and their grouping
static int check_error(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_error_t &e, unsigned parts, const remo_opts_t *opts) {
    if (e.err != 0 && e.err != 1) return fail(ctx, REMO_ERR_ARG, "remo_job_error_t.err must be 0 or 1");
    if (e.err == 0) return REMO_OK;
    if (j.n_fun <= 0) return fail(ctx, REMO_ERR_ARG, "remo_job_error_t.err estimates the error of functionals: n_fun must be at least 1");
    if (e.sec.secondary) return fail(ctx, REMO_ERR_ARG, "remo_job_error_t.err does not combine with the secondary formulation");
    if (parts & kField) return fail(ctx, REMO_ERR_ARG, "remo_job_error_t.err does not combine with field points");
    if (opts && opts->precision == 1) return fail(ctx, REMO_ERR_ARG, "the error estimates are formed from fp64 solutions: remo_opts_t.precision = 1 (mixed) is not supported with remo_job_error_t.err");
    if (!e.err_out) return fail(ctx, REMO_ERR_ARG, "err_out missing");
    if (e.err_n_group < 0) return fail(ctx, REMO_ERR_ARG, "err_n_group must not be negative");
    if (e.err_n_group > 0) {
        if (!e.err_group || !e.errg_out) return fail(ctx, REMO_ERR_ARG, "err_n_group > 0 needs err_group and errg_out");
        if (!mesh || mesh->n_elems <= 0) return fail(ctx, REMO_ERR_ARG, "empty mesh");
        for (int64_t t = 0; t < mesh->n_elems; ++t)
            if (e.err_group[t] < -1 || e.err_group[t] >= e.err_n_group) return fail(ctx, REMO_ERR_ARG, "err_group id of element " + std::to_string(t) + " outside [-1, err_n_group)");
    }
    return REMO_OK;
}

// err_out / errg_out as a negative return leaves them
static void error_nan_fill(const remo_job_t &j, const remo_job_error_t &e) {
    if (e.err == 0 || j.n_fun <= 0) return;
    for (int32_t i = 0; e.err_out && i < j.n_fun; ++i) e.err_out[i] = std::nan("");
    if (e.errg_out && e.err_n_group > 0)
        for (size_t i = 0; i < size_t(j.n_fun) * size_t(e.err_n_group); ++i) e.errg_out[i] = std::nan("");
}

// the pairs of a job (remo_job_pairs_t), likewise: what they do not combine with, and their indices
static int check_pairs(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_pair_groups_t &xg, unsigned parts,
                       const remo_opts_t *opts) {
    const remo_job_pairs_t &x = xg.pairs;
    if (x.n_pair < 0) return fail(ctx, REMO_ERR_ARG, "n_pair must not be negative");
    if (x.pair_reserved != 0) return fail(ctx, REMO_ERR_ARG, "remo_job_pairs_t.pair_reserved must be 0");
    if (xg.pair_n_group < 0) return fail(ctx, REMO_ERR_ARG, "pair_n_group must not be negative");
    if (xg.pair_group_reserved != 0) return fail(ctx, REMO_ERR_ARG, "remo_job_pair_groups_t.pair_group_reserved must be 0");
    if (xg.pair_n_group > 0) {
        if (x.n_pair == 0) return fail(ctx, REMO_ERR_ARG, "pair_n_group > 0 needs pairs: n_pair must be at least 1");
        if (!xg.pair_group || !xg.dPg_out) return fail(ctx, REMO_ERR_ARG, "pair_n_group > 0 needs pair_group and dPg_out");
        if (!mesh || mesh->n_elems <= 0) return fail(ctx, REMO_ERR_ARG, "empty mesh");
        for (int64_t t = 0; t < mesh->n_elems; ++t)
            if (xg.pair_group[t] < -1 || xg.pair_group[t] >= xg.pair_n_group)
                return fail(ctx, REMO_ERR_ARG, "pair_group id of element " + std::to_string(t) + " outside [-1, pair_n_group)");
    }
    if (x.n_pair == 0) return REMO_OK;
    if (!x.pair_a || !x.pair_b || !x.dP_out) return fail(ctx, REMO_ERR_ARG, "n_pair > 0 needs pair_a, pair_b and dP_out");
    if (x.err.sec.secondary) return fail(ctx, REMO_ERR_ARG, "pairs do not combine with the secondary formulation");
    if (parts & kField) return fail(ctx, REMO_ERR_ARG, "pairs do not combine with field points");
    if (j.warm) return fail(ctx, REMO_ERR_ARG, "pairs do not combine with a warm object");
    if (opts && opts->precision == 1) return fail(ctx, REMO_ERR_ARG, "the pair derivatives are formed from fp64 solutions: remo_opts_t.precision = 1 (mixed) is not supported with n_pair > 0");
    for (int32_t p = 0; p < x.n_pair; ++p)
        if (x.pair_a[p] < 0 || x.pair_a[p] >= j.n_rhs || x.pair_b[p] < 0 || x.pair_b[p] >= j.n_rhs)
            return fail(ctx, REMO_ERR_ARG, "pair " + std::to_string(p) + " names no right-hand side of the batch");
    return REMO_OK;
}

// dP_out and dPg_out as a negative return leaves them
static void pairs_nan_fill(const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_pair_groups_t &xg) {
    const remo_job_pairs_t &x = xg.pairs;
    if (x.n_pair <= 0) return;
    const size_t ncomp = (j.tensor && mesh) ? ((mesh->dim == 2) ? 3 : 6) : 1;
    if (x.dP_out && j.n_mat > 0)
        for (size_t i = 0; i < size_t(x.n_pair) * size_t(j.n_mat) * ncomp; ++i) x.dP_out[i] = std::nan("");
    if (xg.dPg_out && xg.pair_n_group > 0)
        for (size_t i = 0; i < size_t(x.n_pair) * size_t(xg.pair_n_group) * ncomp; ++i) xg.dPg_out[i] = std::nan("");
}

// the field points of a job, likewise
static int check_field(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_opts_t *opts) {
    if (j.n_pts < 0 || j.n_frhs < 0 || (j.n_pts > 0 && !j.pts) || (j.n_frhs > 0 && !j.field_rhs)) return fail(ctx, REMO_ERR_ARG, "field points or field_rhs missing");
    if (j.n_pts >= (1 << 28)) return fail(ctx, REMO_ERR_ARG, "too many field points");
    for (int f = 0; f < j.n_frhs; ++f)
        if (j.field_rhs[f] < 0 || j.field_rhs[f] >= j.n_rhs) return fail(ctx, REMO_ERR_ARG, "field_rhs names no right-hand side of the batch");
    if (opts && opts->precision == 1)
        return fail(ctx, REMO_ERR_ARG, "field sections are formed from the fp64 solution: remo_opts_t.precision = 1 (mixed) is not supported by remo_solve_batch_field");
    if (mesh && (mesh->dim == 2 || mesh->dim == 3))
        for (int64_t i = 0; i < int64_t(j.n_pts) * mesh->dim; ++i)
            if (!std::isfinite(j.pts[i])) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
    return REMO_OK;
}

// Every one-shot call: outputs NaN, the checks of the named parts (theirs first, the batch's own in batch_create), the batch with its
// inputs in the context's pool (no hipMalloc / hipFree per batch), the parts attached - batch_run.hip solves the adjoint columns of
// the functionals after the forward ones and contracts them (sens.hip), locates the field points once and reads every chunk's solutions
// there (field.hip), builds the load vector of the secondary formulation (secondary.hip) - run, fetch, destroy.
// full: src_p / eval_p / fun_p are full coordinates (remo_solve_job), else axis positions z (the remo_solve_batch* entries).
static int solve_one(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_secondary_t *sec, unsigned parts, bool full,
                     const remo_opts_t *opts, remo_stats_t *stats, const remo_job_error_t *est = nullptr, const remo_job_pair_groups_t *prs = nullptr) {
    if (!ctx) return REMO_ERR_ARG;
    // whatever goes wrong below, the object does not keep solutions of an earlier call (remo_batch_run labels it again on success)
    struct WarmGuard {
        remo_warm *w;
        int rc = REMO_ERR_ARG;
        ~WarmGuard() { if (w && rc < 0) remo_warm_clear(w); }
    } guard{j.warm};
    if (j.warm) j.warm->used_last = 0;
    if (j.warm && !sec && j.warm->device != ctx->device) return fail(ctx, REMO_ERR_ARG, "the warm object belongs to another device than the context");
    job_nan_fill(mesh, j);
    if (est) error_nan_fill(j, *est);
    if (prs) pairs_nan_fill(mesh, j, *prs);
    std::vector<double> sigma0;
    int rc = est ? check_error(ctx, mesh, j, *est, parts, opts) : REMO_OK;
    if (rc == REMO_OK && prs) rc = check_pairs(ctx, mesh, j, *prs, parts, opts);
    if (rc != REMO_OK) return rc;
    rc = sec ? resolve_secondary(ctx, mesh, j, *sec, opts, sigma0) : REMO_OK;   // (refuses every other part, a warm object included)
    if (rc == REMO_OK && (parts & kFun)) rc = check_functionals(ctx, mesh, j, parts, full);
    if (rc == REMO_OK && (parts & kField)) rc = check_field(ctx, mesh, j, opts);
    remo_batch_t *b = nullptr;
    if (rc == REMO_OK) rc = batch_create(ctx, mesh, j, full, &b, true);
    if (rc != REMO_OK) return rc;
    const bool groups = parts & kGroups;
    remo_sens_request sens{j.n_fun, j.fun_rhs, j.fun_ptr, j.fun_w, j.J_out, j.dJ_out, groups ? j.n_group : 0, groups ? j.group : nullptr, groups ? j.dJg_out : nullptr};
    const remo_field_request field{j.n_pts, j.pts, j.n_frhs, j.field_rhs, j.u_f, j.grad_f, j.J_f, j.elem_f};
    if (parts & kFun) {
        store_points(b->fun_p, j.fun_p, j.n_fun > 0 ? j.fun_ptr[j.n_fun] : 0, b->dim, full);
        if (est && est->err) {
            sens.err = true;
            sens.err_n_group = est->err_n_group;
            sens.err_group = est->err_n_group > 0 ? est->err_group : nullptr;
            sens.err_out = est->err_out; sens.errg_out = est->errg_out;
        }
        b->sens = &sens;
        b->warm = j.warm;
    }
    remo_pairs_request pairs;
    if (prs) {
        pairs.n_pair = prs->pairs.n_pair; pairs.pair_a = prs->pairs.pair_a; pairs.pair_b = prs->pairs.pair_b; pairs.dP_out = prs->pairs.dP_out;
        if (prs->pair_n_group > 0) { pairs.n_group = prs->pair_n_group; pairs.group = prs->pair_group; pairs.dPg_out = prs->dPg_out; }
    }
    if (pairs.n_pair > 0) b->pairs = &pairs;   // (the entry has made a job with pairs a kFun job: the forward solutions stay for the pass)
    if (parts & kField) b->field = &field;
    if (sec) attach_secondary(b, *sec, sigma0);
    b->eval_only = true;
    rc = remo_batch_run(ctx, b, opts, stats);
    if (rc >= 0 && j.u_out) remo_batch_fetch(ctx, b, j.u_out);
    if (rc < 0) job_nan_fill(mesh, j);
    if (rc < 0 && est) error_nan_fill(j, *est);
    if (rc < 0 && prs) pairs_nan_fill(mesh, j, *prs);
    remo_batch_destroy(ctx, b);
    guard.rc = rc;
    return rc;
}

// ---- the entries with an argument list: each is remo_solve_job with axis positions z and the parts its name says ------------------------
int remo_solve_batch(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                     const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                     const double *eval_z, double *u_out, const remo_opts_t *opts, remo_stats_t *stats) {
    return solve_one(ctx, mesh, axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out), nullptr, 0, false, opts, stats);
}

int remo_solve_batch_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                            const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                            const double *eval_z, double *u_out, const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.tensor = 1;
    return solve_one(ctx, mesh, j, nullptr, 0, false, opts, stats);
}

static void set_functionals(remo_job_t &j, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                            double *J_out, double *dJ_out) {
    j.n_fun = n_fun; j.fun_rhs = fun_rhs; j.fun_ptr = fun_ptr; j.fun_p = fun_z; j.fun_w = fun_w;
    j.J_out = J_out; j.dJ_out = dJ_out;
}

int remo_solve_batch_sens(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                          const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                          const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                          const double *fun_z, const double *fun_w, double *J_out, double *dJ_out, const remo_opts_t *opts,
                          remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    return solve_one(ctx, mesh, j, nullptr, kFun, false, opts, stats);
}

int remo_solve_batch_sens_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                                 const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                                 const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                                 const double *fun_z, const double *fun_w, double *J_out, double *dJ_out, const remo_opts_t *opts,
                                 remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.tensor = 1;
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    return solve_one(ctx, mesh, j, nullptr, kFun, false, opts, stats);
}

int remo_solve_batch_sens_warm(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                               const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                               const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                               const double *fun_z, const double *fun_w, double *J_out, double *dJ_out, remo_warm_t *warm,
                               const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    j.warm = warm;
    return solve_one(ctx, mesh, j, nullptr, kFun, false, opts, stats);
}

int remo_solve_batch_sens_warm_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                                      const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                                      const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                                      const double *fun_z, const double *fun_w, double *J_out, double *dJ_out, remo_warm_t *warm,
                                      const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.tensor = 1;
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    j.warm = warm;
    return solve_one(ctx, mesh, j, nullptr, kFun, false, opts, stats);
}

int remo_solve_batch_sens_groups(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                                 const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                                 const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                                 const double *fun_z, const double *fun_w, int32_t n_group, const int32_t *group, double *J_out, double *dJ_out,
                                 double *dJg_out, const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    j.n_group = n_group; j.group = group; j.dJg_out = dJg_out;
    return solve_one(ctx, mesh, j, nullptr, kFun | kGroups, false, opts, stats);
}

int remo_solve_batch_sens_groups_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                                        const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                                        const double *eval_z, double *u_out, int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr,
                                        const double *fun_z, const double *fun_w, int32_t n_group, const int32_t *group, double *J_out,
                                        double *dJ_out, double *dJg_out, const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.tensor = 1;
    set_functionals(j, n_fun, fun_rhs, fun_ptr, fun_z, fun_w, J_out, dJ_out);
    j.n_group = n_group; j.group = group; j.dJg_out = dJg_out;
    return solve_one(ctx, mesh, j, nullptr, kFun | kGroups, false, opts, stats);
}

int remo_solve_batch_field(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma, int32_t n_rhs,
                           const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                           const double *eval_z, double *u_out, int32_t n_pts, const double *pts, int32_t n_frhs, const int32_t *field_rhs,
                           double *u_f, double *grad_f, double *J_f, int32_t *elem_f, const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.n_pts = n_pts; j.pts = pts; j.n_frhs = n_frhs; j.field_rhs = field_rhs;
    j.u_f = u_f; j.grad_f = grad_f; j.J_f = J_f; j.elem_f = elem_f;
    return solve_one(ctx, mesh, j, nullptr, kField, false, opts, stats);
}

int remo_solve_batch_field_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor, int32_t n_rhs,
                                  const int32_t *src_ptr, const double *src_z, const double *src_I, const int32_t *eval_ptr,
                                  const double *eval_z, double *u_out, int32_t n_pts, const double *pts, int32_t n_frhs,
                                  const int32_t *field_rhs, double *u_f, double *grad_f, double *J_f, int32_t *elem_f, const remo_opts_t *opts,
                                  remo_stats_t *stats) {
    remo_job_t j = axis_job(n_mat, sigma_tensor, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z, u_out);
    j.tensor = 1;
    j.n_pts = n_pts; j.pts = pts; j.n_frhs = n_frhs; j.field_rhs = field_rhs;
    j.u_f = u_f; j.grad_f = grad_f; j.J_f = J_f; j.elem_f = elem_f;
    return solve_one(ctx, mesh, j, nullptr, kField, false, opts, stats);
}

// remo_solve_job / remo_batch_create_job: the job as this library knows it - the caller's leading `size` bytes, the rest zero.
static int read_job(remo_ctx_t *ctx, const remo_job_t *job, remo_job_t &j, remo_job_pair_groups_t &x) {
    if (!ctx) return REMO_ERR_ARG;
    if (!job) return fail(ctx, REMO_ERR_ARG, "null job");
    const size_t size = job->size;
    if (size < offsetof(remo_job_t, n_fun)) return fail(ctx, REMO_ERR_ARG, "remo_job_t.size is smaller than the part every job has (through u_out)");
    std::memset(&j, 0, sizeof j);
    std::memset(&x, 0, sizeof x);
    std::memcpy(&x, job, std::min(size, sizeof x));   // remo_job_pair_groups_t begins with a remo_job_pairs_t, that with a remo_job_error_t, that with a remo_job_secondary_t, that with a remo_job_t: one layout, five lengths
    j = x.pairs.err.sec.job;
    const unsigned char *raw = reinterpret_cast<const unsigned char *>(job);
    for (size_t i = sizeof x; i < size; ++i)   // a newer caller: what this library does not know must not be asked for
        if (raw[i]) return fail(ctx, REMO_ERR_ARG, "remo_job_t.size is larger than this library's struct and the tail is not zero");
    if (j.tensor != 0 && j.tensor != 1) return fail(ctx, REMO_ERR_ARG, "remo_job_t.tensor must be 0 or 1");
    return REMO_OK;
}

int remo_solve_job(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t *job, const remo_opts_t *opts, remo_stats_t *stats) {
    remo_job_t j;
    remo_job_pair_groups_t xg;
    int rc = read_job(ctx, job, j, xg);
    const remo_job_pairs_t &xp = xg.pairs;
    const remo_job_error_t &xe = xp.err;
    const remo_job_secondary_t &x = xe.sec;
    const bool pairs = rc == REMO_OK && xp.n_pair > 0;   // (a job with pairs is a job with functionals, n_fun = 0 included: its solutions stay)
    const bool fun = rc == REMO_OK && (j.n_fun != 0 || pairs), field = rc == REMO_OK && (j.n_pts != 0 || j.n_frhs != 0);
    if (rc == REMO_OK && fun && field) rc = fail(ctx, REMO_ERR_ARG, "field points together with functionals: two calls");
    if (rc == REMO_OK && !fun && (j.n_group != 0 || j.warm)) rc = fail(ctx, REMO_ERR_ARG, "groups or a warm object without functionals");
    if (rc == REMO_OK && x.secondary != 0 && x.secondary != 1) rc = fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.secondary must be 0 or 1");
    if (rc != REMO_OK) {
        if (ctx && job && job->size >= offsetof(remo_job_t, n_fun)) {   // a job that could be read: its outputs as the entries leave them on an error
            job_nan_fill(mesh, j);
            error_nan_fill(j, xe);
            pairs_nan_fill(mesh, j, xg);
            if (j.warm) remo_warm_clear(j.warm);
        }
        return rc;
    }
    const unsigned parts = (fun ? kFun : 0) | (j.n_group != 0 ? kGroups : 0) | (field ? kField : 0);
    if (xe.err != 0 && !fun) {   // (with functionals solve_one checks the members beside the other parts)
        job_nan_fill(mesh, j);
        return check_error(ctx, mesh, j, xe, parts, opts);
    }
    return solve_one(ctx, mesh, j, x.secondary ? &x : nullptr, parts, true, opts, stats, &xe, &xg);
}

int remo_batch_create_job(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t *job, remo_batch_t **out) {
    remo_job_t j;
    remo_job_pair_groups_t xg;
    if (int rc = read_job(ctx, job, j, xg)) return rc;
    const remo_job_pairs_t &xp = xg.pairs;
    const remo_job_error_t &xe = xp.err;
    if (xg.pair_n_group > 0) return fail(ctx, REMO_ERR_ARG, "remo_job_pair_groups_t.pair_n_group needs the solutions of a one-shot job: a resident batch keeps none (remo_solve_job)");
    const remo_job_secondary_t &x = xe.sec;
    if (xp.n_pair > 0) return fail(ctx, REMO_ERR_ARG, "remo_job_pairs_t.n_pair needs the solutions of a one-shot job: a resident batch keeps none (remo_solve_job)");
    if (xe.err != 0) return fail(ctx, REMO_ERR_ARG, "remo_job_error_t.err needs functionals: a resident batch has none (remo_solve_job)");
    if (x.secondary != 0 && x.secondary != 1) return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.secondary must be 0 or 1");
    std::vector<double> sigma0;
    if (x.secondary)   // (the batch entries read the sources and the evaluation points only: the other parts of the job must be empty here too)
        if (int rc = resolve_secondary(ctx, mesh, j, x, nullptr, sigma0)) return rc;
    const int rc = batch_create(ctx, mesh, j, true, out, false);
    if (rc == REMO_OK && x.secondary) attach_secondary(*out, x, sigma0);
    return rc;
}

// the system of a batch's last run, still resident, as the element kernels read it: what remo_batch_field / remo_batch_eval evaluate on
static ElemMesh resident_mesh(const remo_ctx_t *ctx, const remo_batch_t *b) {
    return elem_mesh(b, b->d_C, b->d_M_last ? b->d_M_last : ((b->dim == 2) ? ctx->d_M2 : ctx->d_M3));
}

int remo_batch_field(remo_ctx_t *ctx, remo_batch_t *b, int32_t rhs, int32_t n_pts, const double *pts, double *u, double *grad, double *J,
                     int32_t *elem) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || n_pts < 0 || (n_pts > 0 && !pts) || n_pts >= (1 << 28)) return fail(ctx, REMO_ERR_ARG, "bad argument");
    const int dim = b->dim;
    for (int32_t i = 0; i < n_pts; ++i) {
        if (u) u[i] = std::nan("");
        if (elem) elem[i] = -1;
        for (int d = 0; d < dim; ++d) {
            if (grad) grad[size_t(i) * dim + d] = std::nan("");
            if (J) J[size_t(i) * dim + d] = std::nan("");
        }
    }
    if (b->secondary) return fail(ctx, REMO_ERR_ARG, "remo_batch_field reads u_h alone: not available on a batch of the secondary formulation");
    if (!b->has_system || b->run_id != ctx->run_id || b->k_last <= 0 || b->n_rhs > REMO_MAX_RHS || !b->d_x)
        return fail(ctx, REMO_ERR_ARG, "no resident solution for this batch (another batch ran on the context since)");
    if (rhs < 0 || rhs >= b->k_last) return fail(ctx, REMO_ERR_ARG, "rhs index out of range");
    for (int64_t i = 0; i < int64_t(n_pts) * dim; ++i)
        if (!std::isfinite(pts[i])) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
    if (n_pts == 0) return REMO_OK;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const DeviceSymbolic &sy = b->sym;
        const size_t np = size_t(n_pts);
        const FieldGrid grid = field_grid(dim, n_pts, pts);
        const size_t sort_bytes = field_sort_bytes(n_pts, grid.ncell), loc_bytes = field_locate_bytes(n_pts, b->nt, grid.ncell, sort_bytes);
        DeviceTemp tmp;
        double *d_pts = tmp.alloc<double>(np * dim), *d_out = tmp.alloc<double>(np * (1 + 2 * dim));
        int32_t *d_found = tmp.alloc<int32_t>(np * 2), *d_elem = d_found + np;
        const FieldLocate loc = field_locate_carve(tmp.alloc<char>(loc_bytes), n_pts, b->nt, grid.ncell, sort_bytes);
        for (hipEvent_t &e : ctx->fev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventRecord(ctx->fev[0], s));
        HIP_TRY(hipMemcpyAsync(d_pts, pts, sizeof(double) * np * dim, hipMemcpyHostToDevice, s));
        field_locate(dim, b->nt, b->d_coords, sy.conn, n_pts, d_pts, grid, loc, d_found, s);
        launch_field_elem(n_pts, d_found, sy.eperm, d_elem, s);
        HIP_TRY(hipEventRecord(ctx->fev[1], s));
        FieldCols cols;
        cols.n = 1; cols.col[0] = rhs; cols.slot[0] = 0;
        const PointLoads src{b->d_prhs_last, b->d_pI_last, b->d_found_last, b->d_fint_last, b->nq_last};
        double *d_u = d_out, *d_grad = d_out + np, *d_J = d_grad + np * dim;
        HIP_TRY(hipEventRecord(ctx->fev[2], s));
        launch_field_eval(resident_mesh(ctx, b), n_pts, d_pts, d_found, b->k_last, b->d_x, cols, src, d_u, d_grad, d_J, s);
        HIP_TRY(hipEventRecord(ctx->fev[3], s));
        if (u) HIP_TRY(hipMemcpyAsync(u, d_u, sizeof(double) * np, hipMemcpyDeviceToHost, s));
        if (grad) HIP_TRY(hipMemcpyAsync(grad, d_grad, sizeof(double) * np * dim, hipMemcpyDeviceToHost, s));
        if (J) HIP_TRY(hipMemcpyAsync(J, d_J, sizeof(double) * np * dim, hipMemcpyDeviceToHost, s));
        if (elem) HIP_TRY(hipMemcpyAsync(elem, d_elem, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->fev[0], ctx->fev[1]); ctx->field_ms[0] = ms;
        (void)hipEventElapsedTime(&ms, ctx->fev[2], ctx->fev[3]); ctx->field_ms[1] = ms;
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_batch_eval(remo_ctx_t *ctx, remo_batch_t *b, int32_t rhs, int32_t npts, const double *z, double *u_out) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || !z || !u_out || npts <= 0) return fail(ctx, REMO_ERR_ARG, "bad argument");
    for (int i = 0; i < npts; ++i) u_out[i] = std::nan("");
    if (b->secondary) return fail(ctx, REMO_ERR_ARG, "remo_batch_eval reads u_h alone: not available on a batch of the secondary formulation");
    if (!b->has_system || b->run_id != ctx->run_id || b->k_last <= 0 || b->n_rhs > REMO_MAX_RHS)
        return fail(ctx, REMO_ERR_ARG, "no resident solution for this batch (another batch ran on the context since)");
    if (rhs < 0 || rhs >= b->k_last) return fail(ctx, REMO_ERR_ARG, "rhs index out of range");
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const DeviceSymbolic &sy = b->sym;
        const int dim = b->dim, N = (dim == 2) ? 10 : 20;
        const size_t bytes = size_t(npts) * (sizeof(double) * (4 + N) + sizeof(int32_t) * 2) + 1024;
        DeviceTemp tmp;
        char *scratch = tmp.alloc<char>(bytes);
        double *d_z = reinterpret_cast<double *>(scratch), *d_I = d_z + npts, *d_phi = d_I + npts, *d_fint = d_phi + size_t(npts) * N, *d_out = d_fint + npts;
        int32_t *d_rhs = reinterpret_cast<int32_t *>(d_out + npts), *d_found = d_rhs + npts;
        std::vector<int32_t> h_rhs(npts, rhs), h_found(npts, INT_MAX);
        HIP_TRY(hipMemsetAsync(scratch, 0, bytes, s));   // strengths 0 (evaluation points), no bubble loads
        HIP_TRY(hipMemsetAsync(ctx->d_err, 0, sizeof(int32_t), s));
        HIP_TRY(hipMemcpyAsync(d_z, z, sizeof(double) * npts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_rhs, h_rhs.data(), sizeof(int32_t) * npts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_found, h_found.data(), sizeof(int32_t) * npts, hipMemcpyHostToDevice, s));
        for (int q0 = 0; q0 < npts; q0 += kMaxPoints)
            launch_locate(dim, b->nt, b->d_coords, sy.conn, std::min(kMaxPoints, npts - q0), d_z + q0, d_found + q0, s);
        launch_point_shapes(dim, npts, d_z, d_found, b->d_coords, sy.conn, d_phi, ctx->d_err, s);
        launch_eval(resident_mesh(ctx, b), npts, d_rhs, d_I, d_found, d_phi, b->k_last, b->d_x, d_fint, d_out, s);
        int32_t h_err = 0;
        HIP_TRY(hipMemcpyAsync(u_out, d_out, sizeof(double) * npts, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&h_err, ctx->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_err & 2) return fail(ctx, REMO_ERR_POINT, "evaluation point outside the mesh");
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_batch_get_system(remo_ctx_t *ctx, remo_batch_t *b, int32_t *rowptr, int32_t *col, double *val, double *dinv,
                          int32_t *freeid) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || !b->has_system || b->run_id != ctx->run_id) return fail(ctx, REMO_ERR_ARG, "no assembled system on this batch (run it first)");
    if (b->A.vertex_block_only && (rowptr || col || val))
        return fail(ctx, REMO_ERR_ARG, "the last run assembled only the diagonal and the P1 block (remo_opts_t.assemble): run with assemble = 1 to inspect the matrix");
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const DeviceSymbolic &sy = b->sym;
        if (rowptr) HIP_TRY(hipMemcpy(rowptr, sy.rowptr, sizeof(int32_t) * (sy.nfree + 1), hipMemcpyDeviceToHost));
        if (col) HIP_TRY(hipMemcpy(col, sy.col, sizeof(int32_t) * sy.nnz, hipMemcpyDeviceToHost));
        if (freeid) HIP_TRY(hipMemcpy(freeid, sy.freeid, sizeof(int32_t) * sy.ndof, hipMemcpyDeviceToHost));
        if (val) {   // plain CSR order for the caller: undo the interleaving of the edge-pair rows
            std::vector<double> raw(size_t(sy.nnz));
            std::vector<int32_t> rp(size_t(sy.nfree) + 1);
            HIP_TRY(hipMemcpy(raw.data(), b->d_val, sizeof(double) * sy.nnz, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(rp.data(), sy.rowptr, sizeof(int32_t) * (sy.nfree + 1), hipMemcpyDeviceToHost));
            std::memcpy(val, raw.data(), sizeof(double) * sy.nnz);
            for (int64_t r = b->A.pair_begin; r + 1 < b->A.pair_end; r += 2) {
                const int32_t rs = rp[r], len = rp[r + 1] - rp[r];
                for (int32_t e = 0; e < len; ++e) { val[rs + e] = raw[rs + 2 * e]; val[rs + len + e] = raw[rs + 2 * e + 1]; }
            }
        }
        if (dinv) HIP_TRY(hipMemcpy(dinv, b->d_dinv, sizeof(double) * sy.nfree, hipMemcpyDeviceToHost));
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_batch_get_vectors(remo_ctx_t *ctx, remo_batch_t *b, double *x, double *f, int32_t *k_out) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || !b->has_system || b->run_id != ctx->run_id || b->k_last <= 0) return fail(ctx, REMO_ERR_ARG, "no resident solution on this batch (run it first)");
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const size_t bytes = sizeof(double) * size_t(b->A.n) * size_t(b->k_last);
        if (x) HIP_TRY(hipMemcpy(x, b->d_x, bytes, hipMemcpyDeviceToHost));
        if (f) HIP_TRY(hipMemcpy(f, b->d_f, bytes, hipMemcpyDeviceToHost));
        if (k_out) *k_out = b->k_last;
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}


int remo_batch_apply_coarse(remo_ctx_t *ctx, remo_batch_t *b, int32_t k, const double *r, double *z, int32_t fp32, int64_t *nv_out) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || !b->has_system || b->run_id != ctx->run_id || k < 1 || k > REMO_MAX_RHS) return fail(ctx, REMO_ERR_ARG, "bad argument");
    if (b->amg64.levels < 2 || (fp32 && b->amg32.levels < 2)) return fail(ctx, REMO_ERR_ARG, "the last run on this batch built no multigrid hierarchy");
    if (k > b->amg64.kmax) return fail(ctx, REMO_ERR_ARG, "more columns than the hierarchy's level vectors hold (the batch's right-hand sides per chunk)");
    const int64_t nv = b->amg64.lev[0].n;
    if (nv_out) *nv_out = nv;
    if (!r || !z) return REMO_OK;
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        DeviceTemp tmp;
        double *dr = tmp.alloc<double>(nv * k + 2), *dz = tmp.alloc<double>(nv * k + 2), *dpart = tmp.alloc<double>(kMaxPartialBlocks * 8);
        HIP_TRY(hipMemcpy(dr, r, sizeof(double) * nv * k, hipMemcpyHostToDevice));
        const int nb = cheb_grid(nv);
        if (fp32) launch_amg_cycle<float, double>(b->amg32, k, 0, (const double *)dr, dz, dpart, nb, (const double *)nullptr, ctx->stream);
        else launch_amg_cycle<double, double>(b->amg64, k, 0, (const double *)dr, dz, dpart, nb, (const double *)nullptr, ctx->stream);
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        std::vector<double> dinv(static_cast<size_t>(nv));
        HIP_TRY(hipMemcpy(z, dz, sizeof(double) * nv * k, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dinv.data(), b->d_dinv, sizeof(double) * nv, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < nv; ++i)
            for (int c = 0; c < k; ++c) z[i * k + c] *= dinv[static_cast<size_t>(i)];   // the cycle stores z / dinv for the direction launch
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

int remo_batch_spmv(remo_ctx_t *ctx, remo_batch_t *b, int32_t k, const double *x, double *y, int32_t reps, double *ms_avg) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b || !b->has_system || b->run_id != ctx->run_id || !x || !y || k < 1 || k > REMO_MAX_RHS || reps < 1)
        return fail(ctx, REMO_ERR_ARG, "bad argument");
    if (b->A.vertex_block_only && !patch_applies(b->A, k))
        return fail(ctx, REMO_ERR_ARG, "the last run assembled no matrix and its patch tables hold fewer columns than asked for (remo_opts_t.assemble = 1 keeps the matrix)");
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const int64_t n = b->A.n;
        DeviceTemp tmp;
        double *dx = tmp.alloc<double>(n * k + 2), *dy = tmp.alloc<double>(n * k);  // dx: 16 bytes of slack for chunk loads
        HIP_TRY(hipMemcpy(dx, x, sizeof(double) * n * k, hipMemcpyHostToDevice));
        const int nb = spmv_grid(n, choose_lanes_per_row(n, b->A.nnz));
        launch_spmm(b->A, k, dx, dy, nullptr, nullptr, nb, ctx->stream);  // warm-up
        HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        for (int r = 0; r < reps; ++r) launch_spmm(b->A, k, dx, dy, nullptr, nullptr, nb, ctx->stream);
        HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]);
        if (ms_avg) *ms_avg = double(ms) / reps;
        HIP_TRY(hipMemcpy(y, dy, sizeof(double) * n * k, hipMemcpyDeviceToHost));
        return REMO_OK;
    } catch (const std::exception &ex) {
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}

}  // extern "C"
