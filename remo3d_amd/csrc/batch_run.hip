// batch_run.hip — remo_batch_run: the host orchestration of one batch (numbering -> upload -> assembly -> multi-RHS PCG ->
// evaluation) as a list of stages.  The orchestration mirrors the inner loop of remo3d/workers/worker.py:100-134 with one
// difference the reference leaves on the table: the matrix of a batch is assembled once and all its
// right-hand sides are solved together.
//
// The context's arena is a bump allocator: the addresses of a batch follow from the ORDER of the ctx->take calls (and of
// build_patch_tables / amg_setup / amg_to_float, which take from it too).  The stages below keep one order; arena_estimate names
// the buffers term by term so that the two can be compared by eye.
// The element passes (metric terms, loads, evaluation, sensitivities, pairs, field, error estimates, secondary loads) are launched with
// ONE view of the batch's mesh and system, System::em (ElemMesh, elem_access.h; elem_mesh of remo_internal.h fills it in take_system).
#include <limits.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "pcg_host.h"
#include "patch.h"
#include "sens.h"
#include "pairs.h"
#include "field.h"
#include "warm.h"
#include "secondary.h"
#include "errest.h"

using namespace remo;

namespace {

std::mutex g_solve_mutex;   // remo_opts_t.serialize_solves

// the handles every stage reads
struct Run {
    remo_ctx *ctx;
    remo_batch *b;
    const remo_opts_t &o;
    remo_stats_t *st;
    hipStream_t s;
    int dim, N, NT;   // local dofs and metric terms per element
};

// ---- options ----------------------------------------------------------------------------------------------------------------
int checked_opts(remo_ctx *ctx, const remo_opts_t *opts_in, remo_opts_t &o) {
    if (opts_in) o = *opts_in; else remo_opts_default(&o);
    if (o.maxsteps <= 0 || !(o.rtol > 0.0)) return fail(ctx, REMO_ERR_ARG, "maxsteps and rtol must be positive");
    if (o.coarse < 0 || o.coarse > 3) return fail(ctx, REMO_ERR_ARG, "remo_opts_t.coarse must be 0 (by dimension), 1 (polynomial), 2 (multigrid cycle) or 3 (cycle, else polynomial)");
    if (o.op != 0 && o.op != 2 && o.op != 3)
        return fail(ctx, REMO_ERR_ARG, "remo_opts_t.op must be 0 (default), 2 (CSR product) or 3 (patch operator); 1, the round-2 element-wise operator, left the library with ABI 7");
    return REMO_OK;
}

// ---- points of all RHS, chunk by chunk: [sources..., evals...] --------------------------------------------------------------
struct Points {
    int dim = 0;
    std::vector<double> P, I;                           // P: dim coordinates per point
    std::vector<double> z;                              // on_axis: the last coordinate of every point, what launch_locate reads
    std::vector<int32_t> rhs, chunk_begin, eval_slot;   // eval_slot: u_out index or -1
    std::vector<std::pair<int32_t, int32_t>> fun_reads; // remo_solve_batch_sens: (point, index into fun_p) of the points the functionals read
    int forward_chunks = 0;                             // chunks [0, forward_chunks) are the batch's right-hand sides, the rest adjoint columns
    std::vector<int32_t> found_init;                    // INT_MAX per point: what launch_locate starts from
    bool on_axis = true;                                // every lateral coordinate is exactly 0: k_locate / k_point_shapes, else field_locate
    FieldGrid grid{};                                   // !on_axis: the cell grid of the points and what their location needs
    size_t sort_bytes = 0, locate_bytes = 0;
    int n() const { return int(I.size()); }
};

Points gather_points(const remo_batch *b) {
    Points p;
    const int dim = p.dim = b->dim;
    auto add = [&](const std::vector<double> &from, int q, double I, int rhs, int slot) {
        p.P.insert(p.P.end(), from.begin() + size_t(q) * dim, from.begin() + size_t(q + 1) * dim);
        p.I.push_back(I); p.rhs.push_back(rhs); p.eval_slot.push_back(slot);
    };
    for (int c0 = 0; c0 < b->n_rhs; c0 += REMO_MAX_RHS) {
        p.chunk_begin.push_back(int32_t(p.n()));
        const int c1 = std::min(b->n_rhs, c0 + REMO_MAX_RHS);
        for (int r = c0; r < c1; ++r)
            for (int q = b->src_ptr[r]; q < b->src_ptr[r + 1]; ++q) add(b->src_p, q, b->src_I[q], r - c0, -1);
        for (int r = c0; r < c1; ++r)
            for (int q = b->eval_ptr[r]; q < b->eval_ptr[r + 1]; ++q) add(b->eval_p, q, 0.0, r - c0, q);
        if (const remo_sens_request *sn = b->sens)   // J_j = sum_i w_i u(p_i): the functionals' points are read like evaluation points
            for (int j = 0; j < sn->n_fun; ++j)
                if (sn->fun_rhs[j] >= c0 && sn->fun_rhs[j] < c1)
                    for (int q = sn->fun_ptr[j]; q < sn->fun_ptr[j + 1]; ++q) {
                        p.fun_reads.emplace_back(int32_t(p.n()), q);
                        add(b->fun_p, q, 0.0, sn->fun_rhs[j] - c0, -1);
                    }
    }
    p.forward_chunks = int(p.chunk_begin.size());
    if (const remo_sens_request *sn = b->sens)   // adjoint right-hand sides g_j = sum_i w_i phi(p_i): the same points as sources of strength w_i
        for (int a0 = 0; a0 < sn->n_fun; a0 += REMO_MAX_RHS) {
            p.chunk_begin.push_back(int32_t(p.n()));
            for (int j = a0; j < std::min(sn->n_fun, a0 + REMO_MAX_RHS); ++j)
                for (int q = sn->fun_ptr[j]; q < sn->fun_ptr[j + 1]; ++q) add(b->fun_p, q, sn->fun_w[q], j - a0, -1);
        }
    p.chunk_begin.push_back(int32_t(p.n()));
    p.found_init.assign(size_t(p.n()), INT_MAX);
    for (int q = 0; q < p.n(); ++q)
        for (int k = 0; k + 1 < dim; ++k)
            if (p.P[size_t(q) * dim + k] != 0.0) p.on_axis = false;
    if (p.on_axis) {
        p.z.resize(size_t(p.n()));
        for (int q = 0; q < p.n(); ++q) p.z[size_t(q)] = p.P[size_t(q) * dim + dim - 1];
    }
    return p;
}

// host part of the location of points off the axis (field.hip): the cell grid over their box and the bytes of its buffers
void plan_point_location(const remo_batch *b, Points &p) {
    if (p.on_axis || p.n() == 0) return;
    p.grid = field_grid(p.dim, p.n(), p.P.data());
    p.sort_bytes = field_sort_bytes(p.n(), p.grid.ncell);
    p.locate_bytes = field_locate_bytes(p.n(), b->nt, p.grid.ncell, p.sort_bytes);
}

// ---- what the batch will build, and the arena it needs ------------------------------------------------------------------------
struct Plan {
    int kmax = 0;                       // right-hand sides per chunk
    bool x_ev_only = false;             // no x, only the values the evaluation points read (PcgBuffersT::x_ev)
    bool p32 = false;                   // ... and, if the operator turns out to be the patch operator, the search direction in fp32 storage (PcgBuffersT::p32)
    bool want_patch = false, want_amg = false;
    int64_t vertex_block_above = -1;    // build_symbolic_gpu: element count above which only the P1 block gets a pattern
    size_t field_bytes = 0;             // remo_solve_batch_field: everything field_take takes (Field::bytes)
    size_t point_locate_bytes = 0;      // points off the axis: their coordinates beyond z and the buffers of field_locate (take_points)
    size_t secondary_bytes = 0;         // remo_job_secondary_t.secondary: everything take_secondary takes (Secondary::bytes)
    size_t arena_bytes = 0;
};

// pairs one per-element launch takes: what the budget of element values holds (remo_debug_tune key 43), one at least
int pair_ev_pairs(int64_t nt, int ncomp, int n_pair) {
    const size_t budget = g_tune.pair_ev_bytes > 0 ? size_t(g_tune.pair_ev_bytes) : kPairEvBytes;
    const size_t per_pair = size_t(std::max<int64_t>(nt, 1)) * size_t(ncomp) * 8;
    return int(std::max<size_t>(1, std::min<size_t>({budget / per_pair, size_t(std::max(n_pair, 1)), size_t(kPairEvMaxPairs)})));
}

// Upper bounds of everything the stages take, in the order they take it (the vertex solver's share: VertexSolverBuilder::arena_bytes).
// (Generous in places and meant to stay as it is: reserve() only ever grows the arena.)
size_t arena_estimate(const remo_batch *b, const remo_opts_t &o, const Plan &p, int npts) {
    const int dim = b->dim, N = (dim == 2) ? 10 : 20, NT = (dim == 2) ? 9 : 6;
    const int64_t nt = b->nt, nv = b->nv;
    const size_t kmax = size_t(p.kmax);
    const int64_t ndof_max = nv + (dim == 2 ? 7 : 16) * nt, nnz_max = nt * int64_t(N) * N;
    size_t need = symbolic_gpu_arena_bytes(dim, nv, nt, b->nbf);    // numbering: DeviceSymbolic and its scratch
    need += size_t(nt) * NT * 8;                                     // d_C
    need += size_t(nnz_max) * 8;                                     // d_val
    need += size_t(ndof_max) * 8 * (1 + 5 * kmax);                   // d_dinv; d_f, x, r, p, q
    if (p.want_patch)   // tables + slab (upper bound: a row per element dof, and every patch's block padded to 16 rows)
        need += patch_arena_bytes(nt, ndof_max, p.kmax) + (size_t(nt) * 21 + 64) * kmax * 8;
    need += size_t(kMaxPartialBlocks) * 8 * 8 * 3;                   // part_pq, part_rz (rz0, d_bound and the flags ride on the slack below)
    need += size_t(npts) * (N + 8) * 8;                              // d_pz, d_pI, d_prhs, d_found, d_phi, d_fint, d_out
    need += p.point_locate_bytes;                                    // off the axis: d_pz holds dim coordinates; the location's buffers
    need += p.secondary_bytes;                                       // secondary formulation: d_rule, d_src, d_ptr, d_fe, d_fbub
    need += p.field_bytes;                                           // field sections: d_pts, d_found, d_elem, d_u, d_grad, d_J and the location's buffers
    need += (1 << 20);                                               // alignment of every take + the small buffers
    if (p.x_ev_only) {   // slots + values instead of x
        need -= size_t(ndof_max) * 8 * kmax;                         // x, one of the five vectors above
        // (p.p32: the direction takes half its room; the other half stays in the estimate for the fp64 vector set_launch_shape takes
        // instead where the patch operator does not run after all)
        need += size_t(npts + 1) * N * 16;                           // d_ev_at, d_x_ev
    }
    need += VertexSolverBuilder::arena_bytes(dim, nv, kmax, p.want_amg, o.precision == 1);   // the vertex solver's vectors and images, fp32 ones included
    if (b->sens) {   // every forward and adjoint solution stays (sens_take), and the contraction's partial sums
        const size_t ncomp = size_t(b->sigma_comp);
        need += size_t(ndof_max) * 8 * size_t(b->n_rhs + b->sens->n_fun);                                 // keep
        need += size_t(b->sens->n_fun) * size_t(b->n_mat) * ncomp * 8 * (size_t(sens_grid(nt)) + 1);     // part, d_dJ
        if (b->sens->group) {   // sums per group of elements (sens_take)
            const size_t ng = size_t(b->sens->n_group);
            need += size_t(nt) * 4 * 5 + (ng + 2) * 4;                                                    // d_group, keys_in, ids, keys, perm; off
            need += sens_group_sort_bytes(nt, b->sens->n_group) + 256;                                    // rocPRIM's temporary storage
            need += size_t(nt) * ncomp * 8 + size_t(sens_group_chunks(nt)) * 2 * ncomp * 8;               // ev (one functional at a time), cpart
            need += size_t(b->sens->n_fun) * ng * ncomp * 8 + 16 * 256;                                   // d_dJg (+ the alignment of these takes)
        }
        if (b->sens->err) {   // error estimates (err_take)
            need += size_t(nt) * 8 * size_t(b->n_rhs + b->sens->n_fun) + 256;                             // eta2: a slab of nt per forward and adjoint column
            need += size_t(nt) * 8 + size_t(b->sens->n_fun) * 8 * (size_t(sens_grid(nt)) + 1) + 8 * 256;  // ev; part, d_E; d_rule (+ the alignment of these takes)
            if (b->sens->err_group) {   // the second group ordering
                const size_t ng = size_t(b->sens->err_n_group);
                need += size_t(nt) * 4 * 5 + (ng + 2) * 4;                                                // d_group, keys_in, ids, keys, perm; off
                need += sens_group_sort_bytes(nt, b->sens->err_n_group) + 256;                            // rocPRIM's temporary storage
                need += size_t(sens_group_chunks(nt)) * 2 * 8 + size_t(b->sens->n_fun) * ng * 8 + 16 * 256;   // cpart, d_Eg
            }
        }
    }
    if (b->pairs)   // pair derivatives (pairs_take): slots; part, d_dP (+ the alignment of these takes)
        need += size_t(b->pairs->n_pair) * 8 + size_t(b->pairs->n_pair) * size_t(b->n_mat) * size_t(b->sigma_comp) * 8 * (size_t(pair_grid(nt)) + 1) + 4 * 256;
    if (b->pairs && b->pairs->n_group > 0) {   // ... per group of elements: the ordering of their own, one slice's element values, every pair's sums
        const size_t ng = size_t(b->pairs->n_group), ncomp = size_t(b->sigma_comp), npair = size_t(b->pairs->n_pair);
        const size_t slice = size_t(pair_ev_pairs(nt, b->sigma_comp, b->pairs->n_pair));
        need += npair * 8;                                                                            // gslots
        need += size_t(nt) * 4 * 5 + (ng + 2) * 4;                                                    // d_group, keys_in, ids, keys, perm; off
        need += sens_group_sort_bytes(nt, b->pairs->n_group) + 256;                                   // rocPRIM's temporary storage
        need += slice * (size_t(nt) * ncomp * 8 + size_t(sens_group_chunks(nt)) * 2 * ncomp * 8);     // ev, cpart of a slice
        need += npair * ng * ncomp * 8 + 16 * 256;                                                    // d_dPg (+ the alignment of these takes)
    }
    if (o.precision == 1) {   // fp32 copies of the matrix values and of every PCG vector (mixed_buffers)
        need += size_t(nnz_max) * 4;                                 // v32
        need += size_t(ndof_max) * 4 * (1 + 5 * kmax);               // dinv32; x, r, p, q, f32
    }
    return need;
}

Plan plan_batch(const remo_batch *b, const remo_opts_t &o, const Points &pts, size_t field_bytes, size_t secondary_bytes) {
    Plan p;
    const int dim = b->dim, npts = pts.n();
    p.field_bytes = field_bytes;
    p.secondary_bytes = secondary_bytes;
    p.point_locate_bytes = pts.on_axis ? 0 : align_up(size_t(npts + 1) * dim * 8) + align_up(pts.locate_bytes);
    p.kmax = std::min<int>(std::max(b->n_rhs, b->sens ? b->sens->n_fun : 0), REMO_MAX_RHS);   // the adjoint columns run through the same buffers
    // one-shot fp64 solve: no x, only the values the evaluation points read (PcgBuffersT::x_ev); the debug forms of the update
    // (key 25 = 0 writes x there) and the mixed mode's refinement (x64 += x32) need the whole block
    // (field sections read whole element vectors at points that are only located on the device: the whole block, as with sensitivities)
    p.x_ev_only = b->eval_only && !b->sens && !b->field && g_tune.x_ev && g_tune.x_in_direction && o.precision == 0;
    // the patch operator is 3D only; a 2D batch always runs on the CSR product, whatever `op` says
    p.want_patch = dim == 3 && (o.op == 3 || o.op == 0);
    // on that path and the patch operator the search direction is stored in fp32 (remo_debug_tune key 41; whole-x solves, i.e.
    // keys 39 = 0 and 25 = 0, keep fp64): nothing but the direction launch, the operator's staging and the x_ev slots reads it
    p.p32 = p.x_ev_only && p.want_patch && g_tune.p32 && g_tune.defer_q;
    p.want_amg = o.preconditioner != 0 && g_tune.amg != 1 &&
                 (g_tune.amg == 2 || o.coarse == 2 || o.coarse == 3 || (o.coarse == 0 && dim == 2 && o.coarse_degree <= 0));   // coarse = 0: an explicit degree asks for the polynomial
    // patch operator batches above 200 k tetrahedra (assemble = 2: any size) number only the P1 block of the matrix
    p.vertex_block_above = (p.want_patch && o.assemble != 1) ? (o.assemble == 2 ? 0 : 200000) : -1;
    p.arena_bytes = arena_estimate(b, o, p, npts);
    return p;
}

// ---- dof numbering + CSR pattern (device) --------------------------------------------------------------------------------------
int number_dofs(const Run &r, const Plan &plan, double t_start) {
    remo_batch *b = r.b;
    remo_stats_t *st = r.st;
    std::string err;
    DeviceSymbolic &sy = b->sym;
    int rc = build_symbolic_gpu(r.ctx->ar, r.s, r.dim, b->nv, b->nt, b->d_conn, b->nbf, b->d_bconn, b->d_bdir, r.o.condense != 0, r.ctx->d_err, sy, err,
                                plan.vertex_block_above);
    if (rc != REMO_OK) return fail(r.ctx, rc, err);
    st->ms_symbolic = now_ms() - t_start;
    st->n_dof = sy.ndof; st->n_free = sy.nfree; st->nnz = sy.vertex_block_only ? 0 : sy.nnz; st->n_edges = sy.ne; st->n_faces = sy.nf;
    st->n_rhs = b->n_rhs;
    return REMO_OK;
}

// ---- the system: metric terms, matrix values, Jacobi factors, load vectors -----------------------------------------------------
struct System {
    int64_t n = 0;            // free dofs
    bool lite = false;        // only the P1 block has a pattern: the operator is the patch operator
    double *d_C = nullptr, *d_val = nullptr, *d_dinv = nullptr, *d_f = nullptr;
    const double *d_M = nullptr;              // reference tensors (remo_opts_t.quadrature)
    int64_t pair_begin = 0, pair_end = 0;     // edge-dof rows: consecutive pairs with identical patterns, values interleaved
    ElemMesh em;                              // mesh and system as the element kernels read them (elem_mesh): take_system fills it with the rest
    CsrView view(const DeviceSymbolic &sy) const { return CsrView{n, sy.nnz, sy.rowptr, sy.col, d_val}; }
};

System take_system(const Run &r, const Plan &plan) {
    const DeviceSymbolic &sy = r.b->sym;
    System sys;
    sys.n = sy.nfree;
    sys.lite = sy.vertex_block_only;
    sys.d_C = r.ctx->take<double>(r.b->nt * r.NT);
    sys.d_val = r.ctx->take<double>(sy.nnz + 2);   // + 16 bytes: the SpMM reads single rows' values as 16-byte pairs (CsrViewT)
    sys.d_dinv = r.ctx->take<double>(sys.n);
    sys.d_f = r.ctx->take<double>(sys.n * plan.kmax);
    sys.d_M = (r.dim == 2) ? (r.o.quadrature == 1 ? r.ctx->d_M2q : r.ctx->d_M2) : r.ctx->d_M3;
    sys.em = elem_mesh(r.b, sys.d_C, sys.d_M);   // once per run: no stage sees a System without its view
    return sys;
}

void assemble_system(const Run &r, System &sys) {
    remo_batch *b = r.b;
    const DeviceSymbolic &sy = b->sym;
    const int dim = r.dim;
    b->d_M_last = sys.d_M;
    if (sys.em.tensor())
        launch_metric_terms_tensor(sys.em, r.ctx->d_err, r.s);
    else
        launch_metric_terms(sys.em, r.ctx->d_err, r.s);
    if (sys.lite) {   // values of the P1 block (the generic row walk over the vertex rows: their columns are vertex dofs, other local dofs
                      // of an element fall behind the row's last column and are dropped) + the Jacobi factors of every other row
        launch_assemble(dim, sy.condense, sy.nvfree, 0, 0, sy.rowptr, sy.col, sy.adjptr, sy.adj, sy.eldof, sys.d_C, sys.d_M, sys.d_val, sys.d_dinv, r.s);
        launch_diag_rows(dim, sy.nvfree, sys.n, sy.adjptr, sy.adj, sys.d_C, sys.d_M, sys.d_dinv, r.s);
    } else {
        if (sy.nvefree > sy.nvfree && ((sy.nvefree - sy.nvfree) & 1) == 0) { sys.pair_begin = sy.nvfree; sys.pair_end = sy.nvefree; }
        launch_assemble(dim, sy.condense, sys.n, sys.pair_begin, sys.pair_end, sy.rowptr, sy.col, sy.adjptr, sy.adj, sy.eldof, sys.d_C, sys.d_M, sys.d_val,
                        sys.d_dinv, r.s);
    }
}

// ---- the solve's buffers and its preconditioner's shape ------------------------------------------------------------------------
void take_pcg_buffers(const Run &r, const Plan &plan, const System &sys, PcgBuffers &buf) {
    remo_ctx *ctx = r.ctx;
    const int64_t n = sys.n;
    const int kmax = plan.kmax;
    buf.x = plan.x_ev_only ? nullptr : ctx->take<double>(n * kmax);
    buf.r = ctx->take<double>(n * kmax);
    if (plan.p32) buf.p32 = ctx->take<float>(n * kmax + 4);      // (set_launch_shape takes the fp64 vector instead where the patch operator does not run)
    else buf.p = ctx->take<double>(n * kmax);
    buf.q = ctx->take<double>(n * kmax);
    buf.dinv = sys.d_dinv;
    buf.part_pq = ctx->take<double>(kMaxPartialBlocks * 8);
    buf.part_rz = ctx->take<double>(kMaxPartialBlocks * 8 * 2);
    buf.rz0 = ctx->take<double>(kScalarSlots);
}

// progress records of the PCG and the event pool of remo_opts_t.time_kernels (host objects of the context, grown on demand)
void prepare_progress(const Run &r, PcgBuffers &buf) {
    remo_ctx *ctx = r.ctx;
    ctx->ensure_progress(r.o.maxsteps + 3);
    buf.progress = ctx->progress_dev;
    buf.progress_len = ctx->progress_len;
    if (r.o.time_kernels && ctx->spmv_ev.size() < 8192) {
        const size_t old = ctx->spmv_ev.size();
        ctx->spmv_ev.resize(8192);
        for (size_t i = old; i < ctx->spmv_ev.size(); ++i) HIP_TRY(hipEventCreate(&ctx->spmv_ev[i]));
    }
}

// ---- the points on the device: upload, location, shape values ------------------------------------------------------------------
struct DevicePoints {
    int npts = 0;
    double *d_pz = nullptr, *d_pI = nullptr;
    int32_t *d_prhs = nullptr, *d_found = nullptr;
    double *d_phi = nullptr, *d_fint = nullptr, *d_out = nullptr;
    int64_t *d_ev_at = nullptr;   // x_ev_only: slots and values of the solution the points read
    double *d_x_ev = nullptr;
    FieldLocate loc{};            // points off the axis: d_pz holds dim coordinates per point, and the buffers of field_locate
    bool full = false;            // d_pz holds dim coordinates per point (points off the axis), else z alone
};

DevicePoints take_points(const Run &r, const Plan &plan, const Points &pts) {
    remo_ctx *ctx = r.ctx;
    const int npts = pts.n();
    DevicePoints p;
    p.npts = npts;
    p.full = !pts.on_axis;
    p.d_pz = ctx->take<double>(pts.on_axis ? size_t(npts + 1) : size_t(npts + 1) * r.dim); p.d_pI = ctx->take<double>(npts + 1);
    p.d_prhs = ctx->take<int32_t>(npts + 1); p.d_found = ctx->take<int32_t>(npts + 1);
    p.d_phi = ctx->take<double>(size_t(npts + 1) * r.N); p.d_fint = ctx->take<double>(npts + 1); p.d_out = ctx->take<double>(npts + 1);
    p.d_ev_at = plan.x_ev_only ? ctx->take<int64_t>(size_t(npts + 1) * r.N) : nullptr;
    p.d_x_ev = plan.x_ev_only ? ctx->take<double>(size_t(npts + 1) * r.N) : nullptr;
    if (!pts.on_axis && npts > 0) p.loc = field_locate_carve(ctx->take<char>(pts.locate_bytes), npts, r.b->nt, pts.grid.ncell, pts.sort_bytes);
    return p;
}

void upload_points(const Run &r, const Points &pts, const DevicePoints &dp) {
    const int npts = dp.npts;
    HIP_TRY(hipMemsetAsync(r.ctx->d_err, 0, sizeof(int32_t), r.s));
    if (npts > 0) {
        if (pts.on_axis) HIP_TRY(hipMemcpyAsync(dp.d_pz, pts.z.data(), sizeof(double) * npts, hipMemcpyHostToDevice, r.s));
        else HIP_TRY(hipMemcpyAsync(dp.d_pz, pts.P.data(), sizeof(double) * size_t(npts) * r.dim, hipMemcpyHostToDevice, r.s));
        HIP_TRY(hipMemcpyAsync(dp.d_pI, pts.I.data(), sizeof(double) * npts, hipMemcpyHostToDevice, r.s));
        HIP_TRY(hipMemcpyAsync(dp.d_prhs, pts.rhs.data(), sizeof(int32_t) * npts, hipMemcpyHostToDevice, r.s));
        HIP_TRY(hipMemcpyAsync(dp.d_found, pts.found_init.data(), sizeof(int32_t) * npts, hipMemcpyHostToDevice, r.s));
    }
}

// point location + shapes (all points at once).  Points on the axis: the element pass over the axis' elements; a batch with a
// point off it: all its points through the cell grid of the field sections (same tie rule, same tolerances).
void locate_points(const Run &r, const Points &pts, const DevicePoints &dp) {
    const remo_batch *b = r.b;
    const DeviceSymbolic &sy = b->sym;
    r.ctx->point_location = pts.on_axis ? 0 : 1;
    if (dp.npts <= 0) return;
    if (!pts.on_axis) {
        field_locate(r.dim, b->nt, b->d_coords, sy.conn, dp.npts, dp.d_pz, pts.grid, dp.loc, dp.d_found, r.s);
        launch_point_shapes_at(r.dim, dp.npts, dp.d_pz, dp.d_found, b->d_coords, sy.conn, dp.d_phi, r.ctx->d_err, r.s);
        return;
    }
    for (int q0 = 0; q0 < dp.npts; q0 += kMaxPoints)
        launch_locate(r.dim, b->nt, b->d_coords, sy.conn, std::min(kMaxPoints, dp.npts - q0), dp.d_pz + q0, dp.d_found + q0, r.s);
    launch_point_shapes(r.dim, dp.npts, dp.d_pz, dp.d_found, b->d_coords, sy.conn, dp.d_phi, r.ctx->d_err, r.s);
}

// ---- secondary-potential formulation: the load vector is an element integral instead of point values (secondary.hip) ----------------
struct Secondary {
    bool on = false;
    int nq = 0, chunks = 0;
    double R = 0.0;
    SecSources host;              // the sources of every chunk, column by column, with I / (4 pi sigma0) and sigma0
    std::vector<double> rule;     // element rule [nq][dim + 2]
    double *d_rule = nullptr, *d_src = nullptr, *d_fe = nullptr, *d_fbub = nullptr;
    int32_t *d_ptr = nullptr;
    size_t fe_count(const remo_batch *b, int kmax) const { return size_t(b->nt) * (b->dim == 2 ? 10 : 20) * size_t(kmax); }
    size_t bytes(const remo_batch *b, int kmax) const {   // of take_secondary, every take rounded up
        if (!on) return 0;
        return align_up(rule.size() * 8) + align_up(host.src.size() * 8 + 8) + align_up(host.ptr.size() * 4) + align_up(fe_count(b, kmax) * 8) +
               align_up(size_t(b->nt) * size_t(kmax) * 8);
    }
};

// host part: the rule and the source records.  An evaluation point on a source of its own right-hand side has no primary potential.
int plan_secondary(remo_ctx *ctx, const remo_batch *b, Secondary &sec) {
    if (!b->secondary) return REMO_OK;
    const int dim = b->dim;
    const double pi4 = 12.566370614359172953850573533118;
    sec.on = true;
    sec.R = b->sec_radius;
    const int n = b->sec_quad > 0 ? b->sec_quad : kSecQuadDefault;
    sec.rule = sec_rule(dim, n);
    sec.nq = int(sec.rule.size() / size_t(dim + 2));
    for (int c0 = 0; c0 < b->n_rhs; c0 += REMO_MAX_RHS, ++sec.chunks)
        for (int c = 0; c <= REMO_MAX_RHS; ++c) {
            sec.host.ptr.push_back(int32_t(sec.host.n()));
            const int r = c0 + c;
            if (c == REMO_MAX_RHS || r >= b->n_rhs) continue;
            for (int q = b->src_ptr[r]; q < b->src_ptr[r + 1]; ++q) {
                if (b->src_I[q] == 0.0) continue;   // zero strengths are skipped, as in k_build_rhs
                const double *a = &b->src_p[size_t(q) * dim];
                for (int e = b->eval_ptr[r]; e < b->eval_ptr[r + 1]; ++e) {
                    double d2 = 0.0, a2 = 0.0;
                    for (int k = 0; k < dim; ++k) { const double d = b->eval_p[size_t(e) * dim + k] - a[k]; d2 += d * d; a2 += a[k] * a[k]; }
                    if (std::sqrt(d2) <= 1e-9 * (1.0 + std::sqrt(a2)))
                        return fail(ctx, REMO_ERR_POINT, "secondary formulation: an evaluation point lies on a source of its right-hand side");
                }
                const double rec[kSecSrc] = {a[0], a[1], dim == 3 ? a[2] : 0.0, b->src_I[q] / (pi4 * b->sec_sigma0[size_t(r)]), b->sec_sigma0[size_t(r)]};
                sec.host.src.insert(sec.host.src.end(), rec, rec + kSecSrc);
            }
        }
    return REMO_OK;
}

void take_secondary(const Run &r, const Plan &plan, Secondary &sec) {
    if (!sec.on) return;
    remo_ctx *ctx = r.ctx;
    sec.d_rule = ctx->take<double>(sec.rule.size());
    sec.d_src = ctx->take<double>(sec.host.src.size() + 1);
    sec.d_ptr = ctx->take<int32_t>(sec.host.ptr.size());
    sec.d_fe = ctx->take<double>(sec.fe_count(r.b, plan.kmax));
    sec.d_fbub = ctx->take<double>(size_t(r.b->nt) * size_t(plan.kmax));
}

void upload_secondary(const Run &r, const Secondary &sec) {
    if (!sec.on) return;
    HIP_TRY(hipMemcpyAsync(sec.d_rule, sec.rule.data(), sizeof(double) * sec.rule.size(), hipMemcpyHostToDevice, r.s));
    if (!sec.host.src.empty()) HIP_TRY(hipMemcpyAsync(sec.d_src, sec.host.src.data(), sizeof(double) * sec.host.src.size(), hipMemcpyHostToDevice, r.s));
    HIP_TRY(hipMemcpyAsync(sec.d_ptr, sec.host.ptr.data(), sizeof(int32_t) * sec.host.ptr.size(), hipMemcpyHostToDevice, r.s));
}

// a source in or on an element whose conductivity differs from its sigma0 makes the integrand singular: bit 4 of the error flag,
// read back with the batch's one synchronisation
void check_secondary_sources(const Run &r, const System &sys, const Secondary &sec) {
    if (!sec.on) return;
    launch_sec_check(sys.em, sec.host.n(), sec.d_src, r.ctx->d_err, r.s);
}

// the load vectors of one chunk (d_f is the chunk's): element vectors, then the rows' sums in ascending element order
void build_secondary_rhs(const Run &r, const System &sys, const Secondary &sec, int chunk, int k) {
    const DeviceSymbolic &sy = r.b->sym;
    launch_sec_elements(sys.em, sec.d_rule, sec.nq, sec.d_src, sec.d_ptr + size_t(chunk) * (REMO_MAX_RHS + 1), k, sec.R, sec.d_fe, sec.d_fbub, r.s);
    launch_sec_gather(r.dim, sys.n, k, sy.adjptr, sy.adj, sec.d_fe, sys.d_f, r.s);
}

// ---- field sections: points anywhere in the mesh, located once per batch; every chunk's solutions are read there while they exist ----
struct Field {
    int64_t n = 0;          // points
    int n_frhs = 0;
    FieldGrid grid{};
    size_t sort_bytes = 0, locate_bytes = 0;
    double *d_pts = nullptr, *d_u = nullptr, *d_grad = nullptr, *d_J = nullptr;
    int32_t *d_found = nullptr, *d_elem = nullptr;
    FieldLocate loc{};
    float ms_locate = 0.f, ms_eval = 0.f;
    size_t values() const { return size_t(n) * size_t(n_frhs); }
    size_t bytes(int dim) const {   // of field_take, every take rounded up
        if (n <= 0) return 0;
        return align_up(size_t(n) * dim * 8) + 2 * align_up(size_t(n) * 4) + align_up(values() * 8 + 8) + 2 * align_up(values() * dim * 8 + 8) + align_up(locate_bytes);
    }
};

// host part: the cell grid of the points and what the location needs
Field field_plan(const remo_batch *b) {
    Field f;
    const remo_field_request *rq = b->field;
    if (!rq || rq->n_pts <= 0) return f;
    f.n = rq->n_pts;
    f.n_frhs = rq->n_frhs;
    f.grid = field_grid(b->dim, f.n, rq->pts);
    f.sort_bytes = field_sort_bytes(f.n, f.grid.ncell);
    f.locate_bytes = field_locate_bytes(f.n, b->nt, f.grid.ncell, f.sort_bytes);
    return f;
}

void field_take(const Run &r, Field &f) {
    if (f.n <= 0) return;
    remo_ctx *ctx = r.ctx;
    f.d_pts = ctx->take<double>(size_t(f.n) * r.dim);
    f.d_found = ctx->take<int32_t>(size_t(f.n)); f.d_elem = ctx->take<int32_t>(size_t(f.n));
    f.d_u = ctx->take<double>(f.values() + 1); f.d_grad = ctx->take<double>(f.values() * r.dim + 1); f.d_J = ctx->take<double>(f.values() * r.dim + 1);
    f.loc = field_locate_carve(ctx->take<char>(f.locate_bytes), f.n, r.b->nt, f.grid.ncell, f.sort_bytes);
    for (hipEvent_t &e : ctx->fev)
        if (!e) HIP_TRY(hipEventCreate(&e));
}

void field_locate_points(const Run &r, Field &f) {
    if (f.n <= 0) return;
    const remo_batch *b = r.b;
    HIP_TRY(hipEventRecord(r.ctx->fev[0], r.s));
    HIP_TRY(hipMemcpyAsync(f.d_pts, b->field->pts, sizeof(double) * size_t(f.n) * r.dim, hipMemcpyHostToDevice, r.s));
    field_locate(r.dim, b->nt, b->d_coords, b->sym.conn, f.n, f.d_pts, f.grid, f.loc, f.d_found, r.s);
    launch_field_elem(f.n, f.d_found, b->sym.eperm, f.d_elem, r.s);
    HIP_TRY(hipEventRecord(r.ctx->fev[1], r.s));
}

// the columns of chunk `chunk` (right-hand sides c0 .. c0 + k - 1, solution in x[n][k]) that field_rhs names, into their slots
void field_eval_chunk(const Run &r, const System &sys, const DevicePoints &dp, const double *x, Field &f, int c0, int k, int q0, int nq) {
    if (f.n <= 0 || f.n_frhs <= 0) return;
    const remo_batch *b = r.b;
    const PointLoads src{dp.d_prhs + q0, dp.d_pI + q0, dp.d_found + q0, dp.d_fint + q0, nq};
    FieldCols cols;
    bool any = false;
    auto flush = [&]() {
        if (cols.n == 0) return;
        if (!any) HIP_TRY(hipEventRecord(r.ctx->fev[2], r.s));
        any = true;
        launch_field_eval(sys.em, f.n, f.d_pts, f.d_found, k, x, cols, src, f.d_u, f.d_grad, f.d_J, r.s);
        cols.n = 0;
    };
    for (int j = 0; j < f.n_frhs; ++j) {
        const int rhs = b->field->field_rhs[j];
        if (rhs < c0 || rhs >= c0 + k) continue;
        cols.col[cols.n] = rhs - c0; cols.slot[cols.n] = j;
        if (++cols.n == REMO_MAX_RHS) flush();   // (a right-hand side named more than once)
    }
    flush();
    if (!any) return;
    HIP_TRY(hipEventRecord(r.ctx->fev[3], r.s));
    HIP_TRY(hipEventSynchronize(r.ctx->fev[3]));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, r.ctx->fev[2], r.ctx->fev[3]);
    f.ms_eval += ms;
}

void field_fetch(const Run &r, Field &f) {
    const remo_field_request *rq = r.b->field;
    if (f.n <= 0) return;
    hipStream_t s = r.s;
    if (rq->elem) HIP_TRY(hipMemcpyAsync(rq->elem, f.d_elem, sizeof(int32_t) * size_t(f.n), hipMemcpyDeviceToHost, s));
    if (f.values() > 0) {
        if (rq->u) HIP_TRY(hipMemcpyAsync(rq->u, f.d_u, sizeof(double) * f.values(), hipMemcpyDeviceToHost, s));
        if (rq->grad) HIP_TRY(hipMemcpyAsync(rq->grad, f.d_grad, sizeof(double) * f.values() * r.dim, hipMemcpyDeviceToHost, s));
        if (rq->J) HIP_TRY(hipMemcpyAsync(rq->J, f.d_J, sizeof(double) * f.values() * r.dim, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipEventElapsedTime(&f.ms_locate, r.ctx->fev[0], r.ctx->fev[1]);
    r.ctx->field_ms[0] = f.ms_locate;
    r.ctx->field_ms[1] = f.ms_eval;
}

// ---- the patch tables, enqueued right after the vertex block's images.  The read-back lands in this struct: it must stay where it is until the synchronisation.
struct PatchBuild {
    PatchTables ptab{};
    int32_t h_patch[3] = {1, 0, 0};     // overflow flag, largest patch, slab slots
    int32_t *d_pflag = nullptr;         // device side of h_patch
    size_t patch_mark = 0;              // arena mark in front of the tables (patch_tables_one_round)
    PatchBuild() = default; PatchBuild(const PatchBuild &) = delete;
};

// patch operator (patch.hip): its tables are built beside the assembly; their overflow flag and largest patch come
// back with the other small read-backs
// Two elements per lane (remo_debug_tune key 40) in fp64 storage; the mixed mode's fp32 kernel takes one, and it runs on these tables.
void patch_tables_enqueue(const Run &r, const Plan &plan, const System &sys, PatchBuild &pb) {
    if (!plan.want_patch) return;
    pb.d_pflag = r.ctx->take<int32_t>(4);
    pb.patch_mark = r.ctx->ar.lo_mark();      // nothing else is taken before the synchronisation: patch_tables_one_round may build them again here
    build_patch_tables(r.ctx->ar, r.s, r.b->sym, sys.d_C, plan.kmax, r.o.precision == 0 ? g_tune.patch_rounds : 1, pb.ptab, pb.d_pflag);
    HIP_TRY(hipMemcpyAsync(pb.h_patch, pb.d_pflag, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, r.s));
}

// Right after the synchronisation, before anything else is taken from the arena: a batch whose largest patch of two rounds holds
// more rows than the tables or the kernel's LDS do (pb.h_patch: the flag and the row count the build left on the device) gets
// tables of one round in the same place - the patch operator stays, and the batch waits once more.
void patch_tables_one_round(const Run &r, const Plan &plan, const System &sys, PatchBuild &pb) {
    if (!plan.want_patch || pb.ptab.rounds == 1) return;
    if (pb.h_patch[0] == 0 && patch_lds_bytes(pb.h_patch[1], plan.kmax) <= kPatchLdsLimit) return;
    r.ctx->ar.lo_release(pb.patch_mark);
    build_patch_tables(r.ctx->ar, r.s, r.b->sym, sys.d_C, plan.kmax, 1, pb.ptab, pb.d_pflag);
    HIP_TRY(hipMemcpyAsync(pb.h_patch, pb.d_pflag, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, r.s));
    HIP_TRY(hipStreamSynchronize(r.s));
}

// ---- the operator: patch operator or CSR product --------------------------------------------------------------------------------
// Leaves the system on the batch (b->A and the pointers the inspection entries read).
int choose_operator(const Run &r, const Plan &plan, const System &sys, const PcgBuffers &buf, PatchBuild &pb, bool &patch_op) {
    remo_ctx *ctx = r.ctx;
    remo_batch *b = r.b;
    const DeviceSymbolic &sy = b->sym;
    const int64_t n = sys.n;
    const int kmax = plan.kmax;
    PatchTables &ptab = pb.ptab;
    const int32_t *h_patch = pb.h_patch;
    b->A = sys.view(sy);
    b->A.pair_begin = sys.pair_begin; b->A.pair_end = sys.pair_end;
    b->A.vertex_block_only = sys.lite;
    // (the patch kernel's buffer descriptor addresses x with 32-bit byte offsets: beyond 4 GB the CSR product stays; every patch
    // addresses its own block of the slab through a descriptor of its own, so the slab is not bound by this)
    const bool x_fits = uint64_t(n) * uint64_t(kmax) * 8 < 0xFFFFF000ull;
    // patch operator: asked for, or (op = 0) whenever its tables fit; a patch with more distinct rows than the tables hold
    // (an element list without locality) sends op = 0 on to the CSR product and fails op = 3
    // (the kernel forms byte offsets of rows and slab slots with 24-bit multiplies and 32-bit buffer offsets)
    const size_t patch_lds = patch_lds_bytes(h_patch[1], kmax);   // what k_patch_apply asks for (kernels.hip patch_applies)
    const bool patch_ok = plan.want_patch && h_patch[0] == 0 && h_patch[1] > 0 && x_fits && n < (int64_t(1) << 24) && h_patch[2] < 0x7FFFFFF0 && patch_lds <= kPatchLdsLimit;
    if (sys.lite && !patch_ok) return fail(ctx, REMO_ERR_ARG, "only the P1 block was assembled but the patch operator cannot run on this batch: rerun with remo_opts_t.assemble = 1");
    if (r.o.op == 3 && r.dim == 3 && !patch_ok) return fail(ctx, REMO_ERR_ARG, "patch operator: a patch of the element list touches more distinct rows than its tables hold (or the mesh is too large)");
    patch_op = patch_ok;
    r.st->op_used = patch_op ? 3 : 0;
    r.st->patch_rounds = patch_op ? ptab.rounds : 0;
    r.st->assembled = sys.lite ? 2 : 1;
    if (patch_op) {
        ptab.nslot_cap = h_patch[2] > 0 ? h_patch[2] : 1;     // the slab holds the slots in use
        b->patch64 = PatchOpT<double>{ptab, ctx->take<double>(size_t(ptab.nslot_cap) * size_t(kmax) + 8), ctx->take<double>(size_t(ptab.npatch) * 8 + 8), h_patch[1]};
        b->A.patch = &b->patch64;
    }
    b->d_val = sys.d_val;
    b->d_dinv = sys.d_dinv;
    b->d_x = buf.x;
    b->d_f = sys.d_f;
    b->d_C = sys.d_C;
    b->k_last = 0;
    b->has_system = true;
    return REMO_OK;
}

// grids of the PCG's launches and the forms of its update / direction launches
void set_launch_shape(const Run &r, const Plan &plan, const System &sys, bool patch_op, PcgBuffers &buf) {
    remo_batch *b = r.b;
    const int lpr = choose_lanes_per_row(sys.n, b->sym.nnz);
    buf.nb_spmv = spmv_grid(sys.n, lpr);
    buf.nb_vec = vec_grid(sys.n);
    buf.defer_q = patch_op && g_tune.defer_q && !vertex_first_folds(buf.vs);     // the update launch sums the shared rows of q = A p itself
    buf.x_in_direction = g_tune.x_in_direction != 0;
    buf.pq_bins = buf.defer_q && g_tune.dot_bins != 0;
    if (patch_op) b->patch64.dot_bins = buf.pq_bins;
    // the fp32 search direction needs the patch operator with its shared rows left in the slab (no update form that reads p row by
    // row, no CSR product): anything else - op = 0 on a mesh the tables do not take, a folded Chebyshev step - gets its fp64 vector now
    if (buf.p32 && !(patch_op && buf.defer_q && buf.x_in_direction)) {
        buf.p32 = nullptr;
        buf.p = r.ctx->take<double>(sys.n * plan.kmax);
    }
    r.ctx->direction_bytes = (buf.p32 || r.o.precision == 1) ? 4 : 8;     // (mixed mode: the inner solver's vectors are fp32, p among them)
}

// ---- mixed precision: the same solve in fp32 storage ----------------------------------------------------------------------------
// Derived from the fp64 description: what does not depend on the storage type is copied, the fp32 vectors are taken from the arena
// and the value arrays converted (the vertex solver's: VertexSolverBuilder::to_float).
MixedBuffers mixed_buffers(const Run &r, const Plan &plan, const System &sys, const PcgBuffers &buf, const VertexSolverBuilder &vsb, bool patch_op) {
    remo_ctx *ctx = r.ctx;
    remo_batch *b = r.b;
    hipStream_t s = r.s;
    const DeviceSymbolic &sy = b->sym;
    const size_t nk = size_t(sys.n) * plan.kmax;
    MixedBuffers mx;
    float *v32 = ctx->take<float>(size_t(sy.nnz) + 2);   // same slack as d_val
    float *dinv32 = ctx->take<float>(size_t(sys.n));
    launch_to_float(sy.nnz, sys.d_val, v32, s);
    launch_to_float(sys.n, sys.d_dinv, dinv32, s);
    mx.A32 = CsrViewT<float>{sys.n, sy.nnz, sy.rowptr, sy.col, v32};
    mx.A32.pair_begin = b->A.pair_begin; mx.A32.pair_end = b->A.pair_end; mx.A32.vertex_block_only = sys.lite;
    PcgBuffersT<float> &f = mx.b32;
    f.x = ctx->take<float>(nk); f.r = ctx->take<float>(nk);
    f.p = ctx->take<float>(nk + 4); f.q = ctx->take<float>(nk);
    mx.f32 = ctx->take<float>(nk);
    f.dinv = dinv32;
    f.part_pq = buf.part_pq; f.part_rz = buf.part_rz; f.rz0 = buf.rz0;
    f.progress = buf.progress; f.progress_len = buf.progress_len;
    f.nb_spmv = buf.nb_spmv; f.nb_vec = buf.nb_vec;
    f.vs = vsb.to_float(ctx->ar, s, buf.vs, v32, b->amg32);
    // the forms of the update / direction launches are the fp64 solve's (set_launch_shape; to_float says why they cannot differ)
    f.defer_q = buf.defer_q; f.x_in_direction = buf.x_in_direction; f.pq_bins = buf.pq_bins;
    if (patch_op) {
        b->patch32 = patch_view32(b->patch64);
        b->patch32.dot_bins = f.pq_bins;
        mx.A32.patch = &b->patch32;
    }
    return mx;
}

// ---- one chunk of right-hand sides: loads, PCG, evaluation ----------------------------------------------------------------------
struct RunTotals {
    int ret = REMO_OK;
    size_t ev_used = 0;               // events of remo_opts_t.time_kernels
    float ms_solve = 0.f, ms_eval = 0.f;
};

// x_prev != nullptr: the chunk's columns of the previous call (remo_warm_t) - the solve starts from them (run_pcg_warm)
int solve_chunk(const Run &r, const Plan &plan, const System &sys, const DevicePoints &dp, PcgBuffers &buf, MixedBuffers *mx, int k, int q0, int nq,
                std::vector<double> &h_out, RunTotals &tot, double *x_prev = nullptr, const Secondary *sec = nullptr, int chunk = 0) {
    remo_ctx *ctx = r.ctx;
    remo_batch *b = r.b;
    remo_stats_t *st = r.st;
    hipStream_t s = r.s;
    const DeviceSymbolic &sy = b->sym;
    const int dim = r.dim, N = r.N;
    HIP_TRY(hipEventRecord(ctx->ev[4], s));
    HIP_TRY(hipMemsetAsync(sys.d_f, 0, sizeof(double) * sys.n * k, s));
    if (sec) {   // secondary formulation: no point values in f, no bubble loads of single sources
        if (nq > 0) HIP_TRY(hipMemsetAsync(dp.d_fint + q0, 0, sizeof(double) * nq, s));
        build_secondary_rhs(r, sys, *sec, chunk, k);
    } else if (nq > 0)
        launch_build_rhs(sys.em, nq, dp.d_prhs + q0, dp.d_pI + q0, dp.d_found + q0, dp.d_phi + size_t(q0) * N, k, sys.d_f, dp.d_fint + q0, s);
    if (plan.x_ev_only) {   // the slots of this chunk's points (k and the columns change with the chunk)
        launch_eval_slots(sys.em, nq, dp.d_prhs + q0, dp.d_found + q0, k, dp.d_ev_at, s);
        if (nq > 0) HIP_TRY(hipMemsetAsync(dp.d_x_ev, 0, sizeof(double) * size_t(nq) * N, s));
        buf.x_ev_at = dp.d_ev_at; buf.x_ev = dp.d_x_ev; buf.x_ev_n = nq * N;
    }
    HIP_TRY(hipEventRecord(ctx->ev[5], s));
    ChunkResult cr = mx ? run_pcg_mixed(ctx, b->A, k, sys.d_f, buf, *mx, r.o, st, tot.ev_used)
                        : (x_prev ? run_pcg_warm(ctx, b->A, k, sys.d_f, buf, x_prev, r.o, st, tot.ev_used) : run_pcg(ctx, b->A, k, sys.d_f, buf, r.o, st, tot.ev_used));
    HIP_TRY(hipEventRecord(ctx->ev[6], s));
    if (nq > 0)
        launch_eval(sys.em, nq, dp.d_prhs + q0, dp.d_pI + q0, dp.d_found + q0, dp.d_phi + size_t(q0) * N, k, buf.x, dp.d_fint + q0, dp.d_out + q0, s, buf.x_ev,
                    (sec && sy.condense) ? sec->d_fbub : nullptr);
    if (sec && nq > 0)   // u = u_s + u_p at the evaluation points
        launch_sec_add_primary(dim, nq, dp.d_prhs + q0, dp.d_pI + q0, dp.d_pz + size_t(q0) * (dp.full ? dim : 1), !dp.full,
                               sec->d_src, sec->d_ptr + size_t(chunk) * (REMO_MAX_RHS + 1), sec->R, dp.d_out + q0, s);
    HIP_TRY(hipEventRecord(ctx->ev[7], s));
    if (nq > 0) HIP_TRY(hipMemcpyAsync(h_out.data() + q0, dp.d_out + q0, sizeof(double) * nq, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float e1 = 0, e2 = 0, e3 = 0;
    (void)hipEventElapsedTime(&e1, ctx->ev[4], ctx->ev[5]);
    (void)hipEventElapsedTime(&e2, ctx->ev[5], ctx->ev[6]);
    (void)hipEventElapsedTime(&e3, ctx->ev[6], ctx->ev[7]);
    tot.ms_eval += e1 + e3;
    if (sec) ctx->sec_ms += e1;
    tot.ms_solve += e2;
    if (!cr.finite) return fail(ctx, REMO_ERR_NUMERIC, "non-finite residual in PCG");
    b->k_last = k;
    b->d_prhs_last = dp.d_prhs + q0; b->d_pI_last = dp.d_pI + q0; b->d_found_last = dp.d_found + q0; b->d_fint_last = dp.d_fint + q0; b->nq_last = nq;
    if (!cr.converged) tot.ret = REMO_NOT_CONVERGED;
    for (int c = 0; c < k; ++c) {
        st->iterations[c] = cr.iters[c];
        st->relres[c] = cr.relres[c];
        st->max_iterations = std::max(st->max_iterations, cr.iters[c]);
    }
    return REMO_OK;
}

// ---- sensitivities: where the solutions stay, and the contraction ----------------------------------------------------------------
// Chunk c of the forward columns lies at keep + n * REMO_MAX_RHS * c as a block [n][k_c]; the adjoint chunks follow the n * n_rhs
// forward values in the same way.
struct Sens {
    double *keep = nullptr, *part = nullptr, *d_dJ = nullptr;
    int grid = 0, nmc = 0;
    // groups of elements: the caller's array, the sort's input and output, the segment offsets, one functional's element values,
    // the chunk sums of long segments, and every functional's sums
    int32_t *d_group = nullptr, *ids = nullptr, *perm = nullptr, *off = nullptr;
    uint32_t *keys_in = nullptr, *keys = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    double *ev = nullptr, *cpart = nullptr, *d_dJg = nullptr;
    double *block(int64_t n, int n_rhs, bool adjoint, int chunk) const {   // (the adjoint part starts on a 256-byte boundary like every taken buffer)
        return keep + (adjoint ? (size_t(n) * n_rhs + 31) / 32 * 32 : size_t(0)) + size_t(n) * REMO_MAX_RHS * chunk;
    }
};

Sens sens_take(const Run &r, const System &sys) {
    const remo_batch *b = r.b;
    Sens sn;
    sn.grid = sens_grid(b->nt);
    sn.nmc = b->n_mat * b->sigma_comp;
    sn.keep = r.ctx->take<double>(size_t(sys.n) * size_t(b->n_rhs + b->sens->n_fun) + 64);
    sn.part = r.ctx->take<double>(size_t(b->sens->n_fun) * sn.grid * sn.nmc + 1);
    sn.d_dJ = r.ctx->take<double>(size_t(b->sens->n_fun) * sn.nmc + 1);
    if (b->sens->group) {
        const size_t nt = size_t(b->nt), ng = size_t(b->sens->n_group);
        sn.d_group = r.ctx->take<int32_t>(nt); sn.keys_in = r.ctx->take<uint32_t>(nt); sn.ids = r.ctx->take<int32_t>(nt);
        sn.keys = r.ctx->take<uint32_t>(nt); sn.perm = r.ctx->take<int32_t>(nt);
        sn.off = r.ctx->take<int32_t>(ng + 2);
        sn.sort_bytes = sens_group_sort_bytes(b->nt, b->sens->n_group);
        sn.sort_tmp = r.ctx->take<char>(sn.sort_bytes + 256);
        sn.ev = r.ctx->take<double>(nt * size_t(b->sigma_comp));
        sn.cpart = r.ctx->take<double>(size_t(sens_group_chunks(b->nt)) * 2 * size_t(b->sigma_comp));
        sn.d_dJg = r.ctx->take<double>(size_t(b->sens->n_fun) * ng * size_t(b->sigma_comp) + 1);
    }
    return sn;
}

// the tables sens_element / pair_moments read: 2D the reference tensors of the run, 3D their factors, uploaded by the first use
const double *sens_tables(const Run &r, const System &sys) {
    remo_ctx *ctx = r.ctx;
    if (r.dim == 3 && !ctx->d_B3) {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_B3), sizeof(double) * 600));
        HIP_TRY(hipMemcpyAsync(ctx->d_B3, ref_factors3(), sizeof(double) * 600, hipMemcpyHostToDevice, r.s));
    }
    return (r.dim == 3) ? ctx->d_B3 : sys.d_M;
}

// dJ_j/d(component of material m) = -lambda_j^T A_m u_rhs(j): one pass over the elements per functional, then the workgroups' sums
// With groups: the elements are ordered by group once, then per functional the material pass as before (dJ_out has the bits of
// remo_solve_batch_sens), the per-element pass into the one ev buffer, and the sums of its segments.
void sens_contract(const Run &r, const System &sys, const DevicePoints &dp, const Points &pts, const Sens &sn, std::vector<double> &h_dJ) {
    remo_ctx *ctx = r.ctx;
    const remo_batch *b = r.b;
    const remo_sens_request *rq = b->sens;
    const DeviceSymbolic &sy = b->sym;
    hipStream_t s = r.s;
    const double *tab = sens_tables(r, sys);
    const PointLoads pl{dp.d_prhs, dp.d_pI, dp.d_found, dp.d_fint, 0};   // the whole batch's points: the columns name their own ranges
    const bool groups = rq->group != nullptr && rq->n_fun > 0;
    const bool split_times = groups && r.o.time_kernels != 0;   // one synchronisation per functional: measuring runs only
    const size_t ngc = size_t(rq->n_group) * size_t(b->sigma_comp);
    for (double &m : ctx->sens_group_ms) m = 0.0;
    if (groups) {
        HIP_TRY(hipEventRecord(ctx->ev[6], s));
        HIP_TRY(hipMemcpyAsync(sn.d_group, rq->group, sizeof(int32_t) * size_t(b->nt), hipMemcpyHostToDevice, s));
        sens_group_order(b->nt, sn.d_group, sy.eperm, rq->n_group, sn.keys_in, sn.ids, sn.keys, sn.perm, sn.off, sn.sort_tmp, sn.sort_bytes, s);
        HIP_TRY(hipEventRecord(ctx->ev[7], s));
        HIP_TRY(hipEventSynchronize(ctx->ev[7]));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]);
        ctx->sens_group_ms[0] = ms;
    }
    hipEvent_t tev[4] = {};
    if (split_times)
        for (hipEvent_t &e : tev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ctx->ev[4], s));
    for (int j = 0; j < rq->n_fun; ++j) {
        if (split_times) HIP_TRY(hipEventRecord(tev[0], s));
        const int cf = rq->fun_rhs[j] / REMO_MAX_RHS, ca = j / REMO_MAX_RHS, fa = pts.forward_chunks + ca;
        SensColumns col;
        col.xu = sn.block(sys.n, b->n_rhs, false, cf); col.ku = std::min(b->n_rhs - cf * REMO_MAX_RHS, REMO_MAX_RHS); col.cu = rq->fun_rhs[j] % REMO_MAX_RHS;
        col.xl = sn.block(sys.n, b->n_rhs, true, ca); col.kl = std::min(rq->n_fun - ca * REMO_MAX_RHS, REMO_MAX_RHS); col.cl = j % REMO_MAX_RHS;
        col.qu0 = pts.chunk_begin[cf]; col.nqu = pts.chunk_begin[cf + 1] - col.qu0;
        col.ql0 = pts.chunk_begin[fa]; col.nql = pts.chunk_begin[fa + 1] - col.ql0;
        launch_sens_contract(sys.em, tab, col, pl, sn.part + size_t(j) * sn.grid * sn.nmc, s);
        if (!groups) continue;
        if (split_times) HIP_TRY(hipEventRecord(tev[1], s));
        launch_sens_contract(sys.em, tab, col, pl, sn.ev, s, true);
        if (split_times) HIP_TRY(hipEventRecord(tev[2], s));
        launch_sens_group_sum(b->sigma_comp, b->nt, rq->n_group, sn.keys, sn.perm, sn.off, sn.ev, sn.cpart, sn.d_dJg + size_t(j) * ngc, s);
        if (split_times) {
            HIP_TRY(hipEventRecord(tev[3], s));
            HIP_TRY(hipEventSynchronize(tev[3]));
            for (int k = 0; k < 3; ++k) {
                float e = 0;
                (void)hipEventElapsedTime(&e, tev[k], tev[k + 1]);
                ctx->sens_group_ms[1 + k] += e;
            }
        }
    }
    for (hipEvent_t e : tev)
        if (e) (void)hipEventDestroy(e);
    launch_sens_reduce(rq->n_fun, sn.grid, sn.nmc, sn.part, sn.d_dJ, s);
    HIP_TRY(hipEventRecord(ctx->ev[5], s));
    h_dJ.assign(size_t(rq->n_fun) * sn.nmc, std::nan(""));
    if (!h_dJ.empty()) HIP_TRY(hipMemcpyAsync(h_dJ.data(), sn.d_dJ, sizeof(double) * h_dJ.size(), hipMemcpyDeviceToHost, s));
    if (groups) HIP_TRY(hipMemcpyAsync(rq->dJg_out, sn.d_dJg, sizeof(double) * size_t(rq->n_fun) * ngc, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]);
    ctx->sens_ms = ms;
    // per functional: the x rows of both columns once (8 n each), and per element its dof numbers, vertices, material and (2D) metric terms
    ctx->sens_bytes = double(rq->n_fun) * (16.0 * double(sys.n) + double(b->nt) * (4.0 * r.N + 4.0 * (r.dim + 1) + 4.0 + (r.dim == 2 ? 8.0 * r.NT : 0.0)));
}

// ---- pair derivatives (pairs.hip): dP_p = -u_a^T (dA/dsigma) u_b for pairs of forward columns ------------------------------------------
struct Pairs {
    int32_t *d_slots = nullptr;   // two staged-column slots per pair, in the order the launches take the pairs
    double *part = nullptr, *d_dP = nullptr;
    int grid = 0, nmc = 0;
    // remo_job_pair_groups_t: the slots of the per-element launches, the group ordering (buffers of its own, as ErrEst has), the
    // element values and chunk sums of one slice of `slice` pairs, and every pair's sums
    int32_t *d_gslots = nullptr;
    int32_t *d_group = nullptr, *ids = nullptr, *perm = nullptr, *off = nullptr;
    uint32_t *keys_in = nullptr, *keys = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    int slice = 0;
    double *ev = nullptr, *cpart = nullptr, *d_dPg = nullptr;
};

Pairs pairs_take(const Run &r) {
    const remo_batch *b = r.b;
    const size_t np = size_t(b->pairs->n_pair);
    Pairs pr;
    pr.grid = pair_grid(b->nt);
    pr.nmc = b->n_mat * b->sigma_comp;
    pr.d_slots = r.ctx->take<int32_t>(2 * np);
    pr.part = r.ctx->take<double>(np * pr.grid * pr.nmc + 1);
    pr.d_dP = r.ctx->take<double>(np * pr.nmc + 1);
    if (b->pairs->n_group > 0) {
        const size_t nt = size_t(b->nt), ng = size_t(b->pairs->n_group), ncomp = size_t(b->sigma_comp);
        pr.slice = pair_ev_pairs(b->nt, b->sigma_comp, b->pairs->n_pair);
        pr.d_gslots = r.ctx->take<int32_t>(2 * np);
        pr.d_group = r.ctx->take<int32_t>(nt); pr.keys_in = r.ctx->take<uint32_t>(nt); pr.ids = r.ctx->take<int32_t>(nt);
        pr.keys = r.ctx->take<uint32_t>(nt); pr.perm = r.ctx->take<int32_t>(nt);
        pr.off = r.ctx->take<int32_t>(ng + 2);
        pr.sort_bytes = sens_group_sort_bytes(b->nt, b->pairs->n_group);
        pr.sort_tmp = r.ctx->take<char>(pr.sort_bytes + 256);
        pr.ev = r.ctx->take<double>(size_t(pr.slice) * nt * ncomp);
        pr.cpart = r.ctx->take<double>(size_t(pr.slice) * size_t(sens_group_chunks(b->nt)) * 2 * ncomp);
        pr.d_dPg = r.ctx->take<double>(np * ng * ncomp + 1);
    }
    return pr;
}

// The pairs that join chunk ca with chunk cb go together: both blocks are staged once per element.  A launch keeps at most
// kPairSliceAcc accumulators (always one pair), so a chunk pair with many pairs or materials takes several.  The launches take the
// pairs in an order of their own; dP_out gets them back in the caller's.
// With groups (remo_job_pair_groups_t) the same partition is walked once more, sliced by the bytes of element values a launch may
// write: per slice one per-element launch and one batched group sum; dPg_out gets its rows back in the caller's order too.
void pairs_contract(const Run &r, const System &sys, const DevicePoints &dp, const Points &pts, const Sens &sn, const Pairs &pr) {
    remo_ctx *ctx = r.ctx;
    const remo_batch *b = r.b;
    const remo_pairs_request *rq = b->pairs;
    const DeviceSymbolic &sy = b->sym;
    hipStream_t s = r.s;
    const double *tab = sens_tables(r, sys);
    const PointLoads pl{dp.d_prhs, dp.d_pI, dp.d_found, dp.d_fint, 0};   // the whole batch's points: the columns name their own ranges
    const int np = rq->n_pair, nchunk = pts.forward_chunks;
    struct Launch { PairColumns pc; int first, count; };
    // the launches of the (chunk, chunk) partition with at most per_launch pairs each; order[i]: the caller's index of the pair at
    // position i (the same for every per_launch: a set's pairs stay in the caller's order)
    auto partition = [&](int per_launch, std::vector<Launch> &launches, std::vector<int32_t> &order, std::vector<int32_t> &slots) {
        for (int ca = 0; ca < nchunk; ++ca)
            for (int cb = ca; cb < nchunk; ++cb) {
                std::vector<int32_t> mine;
                for (int p = 0; p < np; ++p) {
                    const int a = rq->pair_a[p] / REMO_MAX_RHS, c = rq->pair_b[p] / REMO_MAX_RHS;
                    if (std::min(a, c) == ca && std::max(a, c) == cb) mine.push_back(p);
                }
                for (size_t i0 = 0; i0 < mine.size(); i0 += size_t(per_launch)) {
                    Launch L{};
                    L.first = int(order.size());
                    L.count = int(std::min(mine.size() - i0, size_t(per_launch)));
                    const int chunks[2] = {ca, cb};
                    for (int i = 0; i < 2; ++i) {
                        L.pc.x[i] = sn.block(sys.n, b->n_rhs, false, chunks[i]);
                        L.pc.k[i] = std::min(b->n_rhs - chunks[i] * REMO_MAX_RHS, REMO_MAX_RHS);
                        L.pc.q0[i] = pts.chunk_begin[chunks[i]];
                        L.pc.nq[i] = pts.chunk_begin[chunks[i] + 1] - L.pc.q0[i];
                    }
                    int slot_of[kPairMaxCols];
                    std::fill(slot_of, slot_of + kPairMaxCols, -1);
                    for (int i = 0; i < L.count; ++i) {
                        const int p = mine[i0 + size_t(i)];
                        order.push_back(p);
                        for (const int rhs : {rq->pair_a[p], rq->pair_b[p]}) {
                            const int key = ((rhs / REMO_MAX_RHS == ca) ? 0 : 8) + rhs % REMO_MAX_RHS;   // block and column (ca == cb: block 0)
                            if (slot_of[key] < 0) { slot_of[key] = L.pc.ncol; L.pc.col[L.pc.ncol++] = int8_t(key); }
                            slots.push_back(slot_of[key]);
                        }
                    }
                    launches.push_back(L);
                }
            }
    };
    std::vector<Launch> launches;
    std::vector<int32_t> order, slots;
    partition(std::max(1, kPairSliceAcc / std::max(1, pr.nmc)), launches, order, slots);
    HIP_TRY(hipEventRecord(ctx->ev[4], s));
    const bool fused = g_tune.pairs_fused != 0;
    const int grid = fused ? pr.grid : sens_grid(b->nt);   // (sens_grid <= pair_grid: part holds either)
    size_t n_launch = launches.size();
    if (fused) {
        HIP_TRY(hipMemcpyAsync(pr.d_slots, slots.data(), sizeof(int32_t) * slots.size(), hipMemcpyHostToDevice, s));
        for (const Launch &L : launches)
            launch_pair_contract(sys.em, tab, L.pc, L.count, pr.d_slots + 2 * size_t(L.first), pl, grid, pr.part + size_t(L.first) * grid * pr.nmc, s);
    } else {   // remo_debug_tune key 42 = 0: every pair as a functional whose adjoint column is the forward column a
        n_launch = size_t(np);
        for (int i = 0; i < np; ++i) {
            const int a = rq->pair_a[order[size_t(i)]], c = rq->pair_b[order[size_t(i)]], ca = a / REMO_MAX_RHS, cc = c / REMO_MAX_RHS;
            SensColumns col;
            col.xu = sn.block(sys.n, b->n_rhs, false, cc); col.ku = std::min(b->n_rhs - cc * REMO_MAX_RHS, REMO_MAX_RHS); col.cu = c % REMO_MAX_RHS;
            col.xl = sn.block(sys.n, b->n_rhs, false, ca); col.kl = std::min(b->n_rhs - ca * REMO_MAX_RHS, REMO_MAX_RHS); col.cl = a % REMO_MAX_RHS;
            col.qu0 = pts.chunk_begin[cc]; col.nqu = pts.chunk_begin[cc + 1] - col.qu0;
            col.ql0 = pts.chunk_begin[ca]; col.nql = pts.chunk_begin[ca + 1] - col.ql0;
            launch_sens_contract(sys.em, tab, col, pl, pr.part + size_t(i) * grid * pr.nmc, s);
        }
    }
    launch_sens_reduce(np, grid, pr.nmc, pr.part, pr.d_dP, s);
    HIP_TRY(hipEventRecord(ctx->ev[5], s));
    std::vector<double> h(size_t(np) * pr.nmc);
    HIP_TRY(hipMemcpyAsync(h.data(), pr.d_dP, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < np; ++i) std::memcpy(rq->dP_out + size_t(order[size_t(i)]) * pr.nmc, h.data() + size_t(i) * pr.nmc, sizeof(double) * pr.nmc);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]);
    ctx->pair_ms[0] = ms;
    ctx->pair_ms[1] = double(n_launch);
    for (double &m : ctx->pair_group_ms) m = 0.0;
    if (rq->n_group <= 0) return;
    // ---- per group of elements (remo_job_pair_groups_t): the material launches above stay what they are (dP_out keeps its bits); the
    // moments are formed once more by per-element launches, sliced by the bytes of ev, each followed by one batched group sum
    const size_t ngc = size_t(rq->n_group) * size_t(b->sigma_comp), evs = size_t(b->nt) * size_t(b->sigma_comp);
    HIP_TRY(hipEventRecord(ctx->ev[6], s));
    HIP_TRY(hipMemcpyAsync(pr.d_group, rq->group, sizeof(int32_t) * size_t(b->nt), hipMemcpyHostToDevice, s));
    sens_group_order(b->nt, pr.d_group, sy.eperm, rq->n_group, pr.keys_in, pr.ids, pr.keys, pr.perm, pr.off, pr.sort_tmp, pr.sort_bytes, s);
    HIP_TRY(hipEventRecord(ctx->ev[7], s));
    std::vector<Launch> slices;
    std::vector<int32_t> gorder, gslots;
    partition(pr.slice, slices, gorder, gslots);
    HIP_TRY(hipMemcpyAsync(pr.d_gslots, gslots.data(), sizeof(int32_t) * gslots.size(), hipMemcpyHostToDevice, s));
    const bool split_times = r.o.time_kernels != 0;   // one synchronisation per slice: measuring runs only
    hipEvent_t tev[3] = {};
    if (split_times)
        for (hipEvent_t &e : tev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ctx->ev[4], s));
    for (const Launch &L : slices) {
        if (split_times) HIP_TRY(hipEventRecord(tev[0], s));
        launch_pair_contract(sys.em, tab, L.pc, L.count, pr.d_gslots + 2 * size_t(L.first), pl, pr.grid, pr.ev, s, true);
        if (split_times) HIP_TRY(hipEventRecord(tev[1], s));
        launch_sens_group_sum_batch(b->sigma_comp, b->nt, rq->n_group, pr.keys, pr.perm, pr.off, pr.ev, pr.cpart, pr.d_dPg + size_t(L.first) * ngc, L.count,
                                    int64_t(evs), int64_t(ngc), s);
        if (split_times) {
            HIP_TRY(hipEventRecord(tev[2], s));
            HIP_TRY(hipEventSynchronize(tev[2]));
            for (int k = 0; k < 2; ++k) {
                float e = 0;
                (void)hipEventElapsedTime(&e, tev[k], tev[k + 1]);
                ctx->pair_group_ms[1 + k] += e;
            }
        }
    }
    for (hipEvent_t e : tev)
        if (e) (void)hipEventDestroy(e);
    HIP_TRY(hipEventRecord(ctx->ev[5], s));
    std::vector<double> hg(size_t(np) * ngc);
    HIP_TRY(hipMemcpyAsync(hg.data(), pr.d_dPg, sizeof(double) * hg.size(), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < np; ++i) std::memcpy(rq->dPg_out + size_t(gorder[size_t(i)]) * ngc, hg.data() + size_t(i) * ngc, sizeof(double) * ngc);
    (void)hipEventElapsedTime(&ms, ctx->ev[6], ctx->ev[7]);
    ctx->pair_group_ms[0] = ms;
    if (!split_times) {
        (void)hipEventElapsedTime(&ms, ctx->ev[4], ctx->ev[5]);
        ctx->pair_group_ms[1] = ms;
    }
    ctx->pair_group_ms[3] = double(slices.size());
}

// ---- error estimates of the functionals (errest.hip) ------------------------------------------------------------------------------
// eta2: column c of the forward solutions at eta2 + nt * c, adjoint column j at eta2 + nt * (n_rhs + j)
struct ErrEst {
    double *d_rule = nullptr, *eta2 = nullptr, *ev = nullptr, *part = nullptr, *d_E = nullptr;
    int grid = 0;
    int32_t *d_group = nullptr, *ids = nullptr, *perm = nullptr, *off = nullptr;
    uint32_t *keys_in = nullptr, *keys = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_bytes = 0;
    double *cpart = nullptr, *d_Eg = nullptr;
};

ErrEst err_take(const Run &r) {
    const remo_batch *b = r.b;
    const remo_sens_request *rq = b->sens;
    const size_t nt = size_t(b->nt);
    ErrEst e;
    e.grid = sens_grid(b->nt);
    e.d_rule = r.ctx->take<double>(ErrRule<3>::NTAB);
    e.eta2 = r.ctx->take<double>(nt * size_t(b->n_rhs + rq->n_fun));
    e.ev = r.ctx->take<double>(nt);
    e.part = r.ctx->take<double>(size_t(rq->n_fun) * e.grid + 1);
    e.d_E = r.ctx->take<double>(size_t(rq->n_fun) + 1);
    if (rq->err_group) {
        const size_t ng = size_t(rq->err_n_group);
        e.d_group = r.ctx->take<int32_t>(nt); e.keys_in = r.ctx->take<uint32_t>(nt); e.ids = r.ctx->take<int32_t>(nt);
        e.keys = r.ctx->take<uint32_t>(nt); e.perm = r.ctx->take<int32_t>(nt);
        e.off = r.ctx->take<int32_t>(ng + 2);
        e.sort_bytes = sens_group_sort_bytes(b->nt, rq->err_n_group);
        e.sort_tmp = r.ctx->take<char>(e.sort_bytes + 256);
        e.cpart = r.ctx->take<double>(size_t(sens_group_chunks(b->nt)) * 2);
        e.d_Eg = r.ctx->take<double>(size_t(rq->n_fun) * ng + 1);
    }
    HIP_TRY(hipMemcpyAsync(e.d_rule, err_rule(r.dim), sizeof(double) * (r.dim == 2 ? ErrRule<2>::NTAB : ErrRule<3>::NTAB), hipMemcpyHostToDevice, r.s));
    return e;
}

// eta_e^2 of the k columns of a chunk (solution in x[n][k]) into the slabs from column `slab0` on, while the chunk's solutions are there
void err_facets_chunk(const Run &r, const System &sys, const DevicePoints &dp, const double *x, const ErrEst &e, int slab0, int k, int q0, int nq) {
    const PointLoads src{dp.d_prhs + q0, dp.d_pI + q0, dp.d_found + q0, dp.d_fint + q0, nq};
    launch_error_facets(sys.em, e.d_rule, k, x, src, e.eta2 + size_t(r.b->nt) * size_t(slab0), r.s);
}

// E_j and the group sums of every functional, in the fixed orders of the sensitivity sums
void err_combine(const Run &r, const ErrEst &e) {
    const remo_batch *b = r.b;
    const remo_sens_request *rq = b->sens;
    hipStream_t s = r.s;
    const size_t nt = size_t(b->nt), ng = size_t(rq->err_n_group);
    const bool groups = rq->err_group != nullptr;
    if (groups) {
        HIP_TRY(hipMemcpyAsync(e.d_group, rq->err_group, sizeof(int32_t) * nt, hipMemcpyHostToDevice, s));
        sens_group_order(b->nt, e.d_group, b->sym.eperm, rq->err_n_group, e.keys_in, e.ids, e.keys, e.perm, e.off, e.sort_tmp, e.sort_bytes, s);
    }
    for (int j = 0; j < rq->n_fun; ++j) {
        launch_error_combine(b->nt, e.eta2 + nt * size_t(rq->fun_rhs[j]), e.eta2 + nt * size_t(b->n_rhs + j), groups ? e.ev : nullptr, e.part + size_t(j) * e.grid, s);
        if (groups) launch_sens_group_sum(1, b->nt, rq->err_n_group, e.keys, e.perm, e.off, e.ev, e.cpart, e.d_Eg + size_t(j) * ng, s);
    }
    launch_sens_reduce(rq->n_fun, e.grid, 1, e.part, e.d_E, s);
    HIP_TRY(hipMemcpyAsync(rq->err_out, e.d_E, sizeof(double) * size_t(rq->n_fun), hipMemcpyDeviceToHost, s));
    if (groups && ng > 0) HIP_TRY(hipMemcpyAsync(rq->errg_out, e.d_Eg, sizeof(double) * size_t(rq->n_fun) * ng, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
}

// ---- events -> remo_stats_t -----------------------------------------------------------------------------------------------------
void fill_timing_stats(const Run &r, const Plan &plan, const System &sys, bool mixed, bool patch_op, const RunTotals &tot) {
    remo_ctx *ctx = r.ctx;
    remo_stats_t *st = r.st;
    hipStream_t s = r.s;
    const DeviceSymbolic &sy = r.b->sym;
    const int64_t n = sys.n;
    const int kmax = plan.kmax;
    float m = 0;
    (void)hipEventElapsedTime(&m, ctx->ev[0], ctx->ev[1]); st->ms_h2d = m;
    (void)hipEventElapsedTime(&m, ctx->ev[1], ctx->ev[2]); st->ms_assemble = m;
    (void)hipEventElapsedTime(&m, ctx->ev[2], ctx->ev[3]); st->ms_eval = m + tot.ms_eval;
    st->ms_solve = tot.ms_solve;
    st->spmv_bytes = mixed ? 8.0 * double(sy.nnz) + 4.0 * double(n) + 8.0 * double(kmax) * double(n)   // fp32 values and vectors
                           : 12.0 * double(sy.nnz) + 4.0 * double(n) + 16.0 * double(kmax) * double(n);
    if (patch_op)   // the patch operator reads no stored entries: x and y once (k columns) + 40 bytes of local indices and 48 of metric terms per element
        st->spmv_bytes = (mixed ? 8.0 : 16.0) * double(kmax) * double(n) + 88.0 * double(r.b->nt);
    if (r.o.time_kernels) {
        // what an event bracket measures beyond the enclosed kernel: an empty pair on the same stream
        float overhead = 1e30f;
        for (int rep = 0; rep < 16; ++rep) {
            HIP_TRY(hipEventRecord(ctx->ev[0], s));
            HIP_TRY(hipEventRecord(ctx->ev[1], s));
            HIP_TRY(hipEventSynchronize(ctx->ev[1]));
            float e = 0;
            (void)hipEventElapsedTime(&e, ctx->ev[0], ctx->ev[1]);
            if (e < overhead) overhead = e;
        }
        if (!(overhead < 1e29f) || overhead < 0.f) overhead = 0.f;
        double sum = 0, raw = 0;
        for (size_t i = 0; i + 1 < tot.ev_used; i += 2) {
            float e = 0;
            (void)hipEventElapsedTime(&e, ctx->spmv_ev[i], ctx->spmv_ev[i + 1]);
            raw += e;
            sum += (e > overhead) ? double(e - overhead) : 0.0;
        }
        st->spmv_ms = sum;
        st->spmv_ms_raw = raw;
        st->event_overhead_ms = overhead;
        st->spmv_launches = int64_t(tot.ev_used / 2);
    }
}

}  // namespace

extern "C" int remo_batch_run(remo_ctx_t *ctx, remo_batch_t *b, const remo_opts_t *opts_in, remo_stats_t *st) {
    if (!ctx) return REMO_ERR_ARG;
    if (!b) return fail(ctx, REMO_ERR_ARG, "null batch");
    remo_opts_t o;
    if (int rc = checked_opts(ctx, opts_in, o)) return rc;
    remo_stats_t local;
    if (!st) st = &local;
    std::memset(st, 0, sizeof *st);
    std::fill(b->u_out.begin(), b->u_out.end(), std::nan(""));
    if (b->sens) {
        if (o.precision == 1) return fail(ctx, REMO_ERR_ARG, "sensitivities are computed in fp64: remo_opts_t.precision = 1 (mixed) is not supported by remo_solve_batch_sens");
        if (int64_t(b->n_mat) * b->sigma_comp > kSensMaxAcc) return fail(ctx, REMO_ERR_ARG, "too many materials for the sensitivity contraction");
    }
    if (b->secondary) {
        if (o.precision == 1) return fail(ctx, REMO_ERR_ARG, "the secondary formulation is fp64: remo_opts_t.precision = 1 (mixed) is not supported with remo_job_secondary_t.secondary");
        if (b->sens || b->field || b->warm) return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.secondary does not combine with functionals, groups, a warm object or field points");
        ctx->sec_ms = 0.0;
    }
    if (b->field && o.precision == 1)
        return fail(ctx, REMO_ERR_ARG, "field sections are formed from the fp64 solution: remo_opts_t.precision = 1 (mixed) is not supported by remo_solve_batch_field");
    b->has_system = false;
    b->amg64 = AmgT<double>{};
    b->amg32 = AmgT<float>{};
    b->run_id = ++ctx->run_id;
    const double t_start = now_ms();
    try {
        HIP_TRY(hipSetDevice(ctx->device));
        const Run r{ctx, b, o, st, ctx->stream, b->dim, (b->dim == 2) ? 10 : 20, (b->dim == 2) ? 9 : 6};
        hipStream_t s = r.s;

        // ---- host side: points, plan, arena -----------------------------------------------------------------------
        Points points = gather_points(b);
        const int npts = points.n();
        for (double c : points.P)
            if (!std::isfinite(c)) return fail(ctx, REMO_ERR_POINT, "non-finite point coordinate");
        plan_point_location(b, points);
        Field fld = field_plan(b);
        Secondary sec;
        if (int rc = plan_secondary(ctx, b, sec)) return rc;
        const int kmax_plan = std::min<int>(std::max(b->n_rhs, b->sens ? b->sens->n_fun : 0), REMO_MAX_RHS);
        const Plan plan = plan_batch(b, o, points, fld.bytes(b->dim), sec.bytes(b, kmax_plan));
        ctx->reserve(plan.arena_bytes);

        // ---- numbering, then every buffer of the solve (arena order), then the device work up to the one sync --------
        if (int rc = number_dofs(r, plan, t_start)) return rc;
        System sys = take_system(r, plan);
        PcgBuffers buf{};
        take_pcg_buffers(r, plan, sys, buf);
        const VertexSolverInput vin{r.dim, plan.kmax, o, b->sym.nvfree, sys.lite, plan.want_amg};
        VertexSolverBuilder vsb;
        vsb.take(ctx->ar, vin, buf.vs);   // degree, the chain's vectors, the bound's slot
        const DevicePoints dp = take_points(r, plan, points);
        take_secondary(r, plan, sec);
        field_take(r, fld);
        prepare_progress(r, buf);
        HIP_TRY(hipEventRecord(ctx->ev[0], s));
        upload_points(r, points, dp);
        upload_secondary(r, sec);
        HIP_TRY(hipEventRecord(ctx->ev[1], s));
        assemble_system(r, sys);
        HIP_TRY(hipEventRecord(ctx->ev[2], s));
        locate_points(r, points, dp);
        check_secondary_sources(r, sys, sec);
        field_locate_points(r, fld);
        HIP_TRY(hipEventRecord(ctx->ev[3], s));
        vsb.enqueue(ctx->ar, s, vin, sys.view(b->sym), sys.d_dinv, buf.vs);
        PatchBuild pb;
        patch_tables_enqueue(r, plan, sys, pb);
        int32_t h_err = 0;                  // ctx->d_err: 1 = mesh / material, 2 = point, 4 = secondary source
        HIP_TRY(hipMemcpyAsync(&h_err, ctx->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        patch_tables_one_round(r, plan, sys, pb);

        // ---- what came back: preconditioner images, mesh / point errors, operator -------------------------------------
        if (int rc = vsb.accept(ctx->ar, s, vin, sys.view(b->sym), sys.d_dinv, b->amg64, b->amg32, buf.vs, &st->coarse_used, ctx->err)) return rc;
        if (h_err & 1) return fail(ctx, REMO_ERR_MESH, "degenerate element or material index out of range");
        if (h_err & 2) return fail(ctx, REMO_ERR_POINT, "source or evaluation point outside the mesh");
        if (h_err & 4) return fail(ctx, REMO_ERR_POINT, "secondary formulation: a source lies in or on an element whose conductivity differs from sigma0 (the integrand is singular there)");
        bool patch_op = false;
        if (int rc = choose_operator(r, plan, sys, buf, pb, patch_op)) return rc;
        const Sens sens = b->sens ? sens_take(r, sys) : Sens{};
        const bool want_err = b->sens && b->sens->err;
        const ErrEst est = want_err ? err_take(r) : ErrEst{};
        const Pairs prs = b->pairs ? pairs_take(r) : Pairs{};
        // remo_solve_batch_sens_warm: the previous call's solutions, in the layout of `sens` (same block offsets in another allocation).
        // Until this run ends well the object counts as empty; a hit keeps its contents, a miss makes room for this run's.
        remo_warm *warm = b->sens ? b->warm : nullptr;
        Sens prev{};
        bool warm_hit = false;
        if (warm) {
            warm_hit = warm_matches(warm, b, o.condense != 0, sys.n);
            warm->filled = false;
            warm->used_last = warm_hit ? 1 : 0;
            if (!warm_hit) warm_reserve(warm, warm_doubles(sys.n, b->n_rhs, b->sens->n_fun));
            prev.keep = warm->d;
        }

        // ---- solve, chunk by chunk ----------------------------------------------------------------------------------
        // serialize_solves: batches of other contexts may number and assemble beside this PCG, but not run theirs
        std::unique_lock<std::mutex> solve_turn(g_solve_mutex, std::defer_lock);
        if (o.serialize_solves) solve_turn.lock();
        set_launch_shape(r, plan, sys, patch_op, buf);
        const bool mixed = (o.precision == 1);
        MixedBuffers mx;
        if (mixed) mx = mixed_buffers(r, plan, sys, buf, vsb, patch_op);   // fp32 images of the system for the inner solver
        std::vector<double> h_out(npts, std::nan(""));
        RunTotals tot;
        int chunk = 0;
        for (int c0 = 0; c0 < b->n_rhs; c0 += REMO_MAX_RHS, ++chunk) {
            const int k = std::min(b->n_rhs - c0, REMO_MAX_RHS);
            const int q0 = points.chunk_begin[chunk], nq = points.chunk_begin[chunk + 1] - q0;
            if (b->sens) b->d_x = buf.x = sens.block(sys.n, b->n_rhs, false, chunk);   // the solution is formed where it stays
            if (int rc = solve_chunk(r, plan, sys, dp, buf, mixed ? &mx : nullptr, k, q0, nq, h_out, tot,
                                     warm_hit ? prev.block(sys.n, b->n_rhs, false, chunk) : nullptr, sec.on ? &sec : nullptr, chunk)) return rc;
            if (b->field) field_eval_chunk(r, sys, dp, buf.x, fld, c0, k, q0, nq);   // while the chunk's solutions are there
            if (want_err) err_facets_chunk(r, sys, dp, buf.x, est, c0, k, q0, nq);
        }
        if (b->field) field_fetch(r, fld);
        for (int q = 0; q < npts; ++q)
            if (points.eval_slot[q] >= 0) b->u_out[points.eval_slot[q]] = h_out[q];
        if (const remo_sens_request *rq = b->sens) {   // adjoint columns: same operator, preconditioner and stopping rule; then the contraction
            for (int a0 = 0, ca = 0; a0 < rq->n_fun; a0 += REMO_MAX_RHS, ++ca, ++chunk) {
                const int k = std::min(rq->n_fun - a0, REMO_MAX_RHS);
                const int q0 = points.chunk_begin[chunk], nq = points.chunk_begin[chunk + 1] - q0;
                b->d_x = buf.x = sens.block(sys.n, b->n_rhs, true, ca);
                if (int rc = solve_chunk(r, plan, sys, dp, buf, nullptr, k, q0, nq, h_out, tot, warm_hit ? prev.block(sys.n, b->n_rhs, true, ca) : nullptr)) return rc;
                if (want_err) err_facets_chunk(r, sys, dp, buf.x, est, b->n_rhs + a0, k, q0, nq);
            }
            if (warm) {   // a warm chunk left its sum in the object already; a cold run's solutions are copied there whole
                if (!warm_hit) HIP_TRY(hipMemcpyAsync(warm->d, sens.keep, sizeof(double) * (warm_doubles(sys.n, b->n_rhs, rq->n_fun) - 64), hipMemcpyDeviceToDevice, s));
                warm_label(warm, b, o.condense != 0, sys.n);
            }
            std::vector<double> h_dJ;
            sens_contract(r, sys, dp, points, sens, h_dJ);
            for (int j = 0; j < rq->n_fun; ++j) rq->J_out[j] = 0.0;
            for (const auto &fr : points.fun_reads) {   // (fun_reads is ordered by functional within a chunk and fun_ptr ascends: a fixed order of additions)
                int j = 0;
                while (fr.second >= rq->fun_ptr[j + 1]) ++j;
                rq->J_out[j] += rq->fun_w[fr.second] * h_out[fr.first];
            }
            if (!h_dJ.empty()) std::memcpy(rq->dJ_out, h_dJ.data(), sizeof(double) * h_dJ.size());
            if (want_err) err_combine(r, est);
            if (b->pairs && b->pairs->n_pair > 0) pairs_contract(r, sys, dp, points, sens, prs);
        }
        fill_timing_stats(r, plan, sys, mixed, patch_op, tot);
        st->ms_total = now_ms() - t_start;
        if (tot.ret == REMO_NOT_CONVERGED) ctx->err = "PCG did not reach rtol within maxsteps";
        return tot.ret;
    } catch (const std::exception &ex) {
        std::fill(b->u_out.begin(), b->u_out.end(), std::nan(""));
        return fail(ctx, REMO_ERR_DEVICE, ex.what());
    }
}
