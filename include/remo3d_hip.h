/*
 * remo3d_hip.h — C ABI of libremo3d_hip.so: the MI355X (gfx950) replacement for ReMo3D's
 * per-measurement-point FEM hot path.
 *
 * Reference interface replaced (eMWu94/ReMo3D @ 2025-04-04):
 *   remo3d/ngsolve_functions.py:23-58      SolveBVP(mesh, sigma, tool_geometry, source_terms,
 *                                                   dirichlet_boundary, preconditioner, condense)
 *   remo3d/ngsolve_functions_gpu.py:15-54  the same entry, CUDA attempt (the plugin slot)
 *   remo3d/workers/worker.py:100-134       sigma wrapping, loop over the RHS of one batch,
 *                                          evaluation of gfu at the measuring electrodes
 * Because `mesh` and `gfu` are NGSolve objects in the reference, the native boundary sits one
 * step outside SolveBVP: it takes the arrays that define one batch (mesh + sigma + the point
 * sources of every right-hand side + the axis points where the potential is read) and returns
 * the potentials.  See INTEGRATION.md for the ctypes binding a ReMo3D maintainer would add.
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; the library never
 * keeps a host pointer past return.  Return codes: 0 ok, >0 warning (REMO_NOT_CONVERGED — the
 * reference is silent about that, ngsolve_functions.py:50), <0 error (outputs NaN-filled, which
 * reproduces the reference's NaN-per-batch convention, worker.py:135-138).  No C++ exception
 * crosses the ABI.  One calling thread per context; contexts are independent (own stream and device arena),
 * so one per GPU per process is the normal case and several may share a GPU (each with its own thread).
 */
#ifndef REMO3D_HIP_H
#define REMO3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define REMO_ABI_VERSION 7
#define REMO_MAX_RHS 8 /* right-hand sides solved as one block; longer batches are chunked */

#define REMO_OK 0
#define REMO_NOT_CONVERGED 1
#define REMO_ERR_ARG (-1)
#define REMO_ERR_DEVICE (-2)
#define REMO_ERR_MESH (-3)   /* inconsistent mesh (bad index, boundary facet not in mesh, ...) */
#define REMO_ERR_POINT (-4)  /* source / evaluation point outside the mesh */
#define REMO_ERR_NUMERIC (-5) /* breakdown (non-finite residual) */

/* One batch mesh = what worker.py:100 wraps with ngs.Mesh(): straight-sided simplices. */
typedef struct {
    int32_t dim;               /* 2 = axisymmetric (r, z) half disc; 3 = (x, y, z) half ball      */
    int64_t n_nodes;
    const double *coords;      /* [n_nodes * dim] row-major, metres, batch-centred frame          */
    int64_t n_elems;
    const int32_t *conn;       /* [n_elems * (dim+1)] 0-based vertex numbers, any orientation     */
    const int32_t *mat;        /* [n_elems] 0-based index into sigma (gmsh_functions.py:332-361)  */
    int64_t n_bfacets;
    const int32_t *bconn;      /* [n_bfacets * dim] boundary facets                               */
    const uint8_t *bdirichlet; /* [n_bfacets] 1 => u = 0 there (H1(..., dirichlet=...), :27)       */
} remo_mesh_t;

/* Solver options; zero-initialise then call remo_opts_default(). */
typedef struct {
    int32_t preconditioner; /* 0 = "local" (Jacobi, ngsolve_functions.py:46); 1 = "multigrid": two-level, Chebyshev
                               solve of the P1 (vertex) block + Jacobi on edge/face dofs                  */
    int32_t condense;       /* static condensation of the 2D cell bubble (ngsolve_functions.py:31) */
    int32_t maxsteps;       /* CG step limit, reference 1000 (ngsolve_functions.py:50)             */
    int32_t check_every;    /* host looks at the residual history every this many steps            */
    double rtol;            /* stop when sqrt(<Cr,r>) <= rtol * sqrt(<Cr0,r0>); NGSolve default 1e-8 */
    int32_t time_kernels;   /* k > 0: bracket every k-th SpMV launch of a solve with HIP events (bench roofline); 0 = off */
    int32_t coarse_degree;  /* "multigrid": Chebyshev degree on the vertex block (0 => default: 16 in 2D; in 3D 5 at 1e4 vertices,
                               growing like sqrt(vertices) up to 16) */
    int32_t coarse_ratio;   /* "multigrid": lmax / lmin of the Chebyshev interval (0 => default: 600 in 2D; in 3D 90 at 1e4 vertices, growing like
                               vertices^(2/3)) */
    int32_t precision;      /* 0 = fp64 throughout; 1 = mixed (BASELINE config 5): PCG in fp32 storage inside an fp64
                               residual-refinement loop, stopping test on the true fp64 residual           */
    int32_t inner_digits;   /* mixed: the fp32 residual is replaced by the true fp64 one every time <Cr,r> has gained this
                               many decimal digits (0 => 3; capped at 5, what an fp32 recurrence can hold)   */
    int32_t serialize_solves; /* 1: the solve phase of remo_batch_run (PCG + evaluation) takes a process-wide lock, so that with
                               several contexts driven by several host threads only ONE batch is in its PCG at any time while the
                               others number / assemble theirs beside it (software pipelining across batches); 0: no lock      */
    int32_t op;             /* how the CG applies A (CGSolver's a.mat, ngsolve_functions.py:50-51):
                               3 = patch operator (3D; a 2D batch runs on the CSR product whatever this says): matrix-free - the element
                                   list is cut into patches of 256 / k tetrahedra (twice that in fp64 solves with k >= 3), a workgroup stages the x rows of its patch in LDS, applies
                                   every K_e through the factorised reference tensors and writes each row once (rows shared by patches
                                   through a compact slab); same operator to rounding; results reproducible to rounding, not bit for bit
                                   (LDS atomics) - the one kernel of the path for which that holds;
                               2 = CSR SpMM on the assembled matrix (bit-reproducible);
                               0 = default: 3 in 3D (at the reference's resolution an application takes ~100 us against 370-450 us
                                   of the CSR product and moves 0.4 GB instead of 1.25 GB), 2 in 2D.
                               (1 was the round-2 element-wise operator with a slab of element results: removed with ABI 7, REMO_ERR_ARG.)
                               What is assembled: remo_opts_t.assemble */
    int32_t coarse;         /* "multigrid": the solver of the P1 (vertex) block.
                               1 = Chebyshev polynomial (coarse_degree, coarse_ratio);
                               2 = one V(1,1) cycle of a smoothed-aggregation multigrid hierarchy built per batch on the device
                                   (distance-2 independent-set aggregates, Galerkin products, dense coarsest solve);
                               0 = by dimension (default; a coarse_degree > 0 selects the polynomial): the cycle in 2D (graded axisymmetric meshes: 40 % fewer PCG steps than
                                   the polynomial of degree 28 at a quarter of its launches), the polynomial in 3D (there it is
                                   within 15 % of an exact vertex solve at degree 5-13 and the cycle gains nothing).
                               3 = the cycle if its hierarchy can be built, else the polynomial (coarse_degree / coarse_ratio): what `Model` asks
                                   for on the graded, sheared interface-conforming 3D meshes it builds, where the cycle takes 17 % less
                                   time than the best polynomial (187 against 198 steps at two thirds of the launches).
                               If the hierarchy cannot be built (a vertex of extreme valence) 0 and 3 fall back to the polynomial, 2 fails */
    int32_t assemble;       /* what a 3D batch that runs on the patch operator assembles (CGSolver's a.mat is never read there):
                               0 = by size (default): the whole matrix up to 200 k tetrahedra (inspection hooks, small cost), above that only
                                   the Jacobi diagonal and the P1 (vertex) block the preconditioner solves - pattern and values of a
                                   2 M-row matrix are 4.5 ms of an 80 ms batch and 1.2 GB;
                               1 = always the whole matrix; 2 = diagonal + P1 block whenever the patch operator runs.
                               Without the matrix remo_batch_get_system (rowptr / col / val) and products with more columns than the
                               batch has right-hand sides fail with REMO_ERR_ARG (remo_stats_t.assembled says which it was); op = 2 always assembles */
    int32_t quadrature;     /* 2D: how the reference tensors of `2 pi x sigma grad(u) grad(v)` (ngsolve_functions.py:34; a degree-5 integrand) are
                               integrated: 0 = exactly (default); 1 = by the 6-point rule that is exact to degree 4 - the alternative NGSolve
                               may be using (its rule order is not pinned by the reference).  3D integrands have degree 4: always exact */
} remo_opts_t;

typedef struct {
    int64_t n_dof;   /* dofs before Dirichlet elimination (condensed bubbles not counted)          */
    int64_t n_free;  /* rows of the linear system                                                 */
    int64_t nnz;     /* stored entries of the CSR matrix                                          */
    int64_t n_edges, n_faces;
    int32_t n_rhs;
    int32_t max_iterations;              /* over the RHS                                           */
    int32_t iterations[REMO_MAX_RHS];    /* of the last chunk                                      */
    double relres[REMO_MAX_RHS];         /* sqrt(<Cr,r>/<Cr0,r0>) of the last chunk                */
    double ms_symbolic;  /* dof numbering + CSR pattern                                            */
    double ms_h2d;       /* uploads                                                                */
    double ms_assemble;  /* geometry terms + CSR values (device, HIP events)                       */
    double ms_solve;     /* PCG, all RHS (device, HIP events)                                      */
    double ms_eval;      /* point location + RHS build + evaluation                                */
    double ms_total;     /* wall clock of the call                                                 */
    double spmv_ms;      /* sum of the event-timed SpMV launches (time_kernels > 0), minus the bracket
                            overhead below per launch                                             */
    int64_t spmv_launches;
    double spmv_bytes;   /* algorithmic bytes of ONE operator application: CSR product 12 nnz + 4 n + 16 k n;
                            patch operator 16 k n + 88 T (x read and y written once, 40 B of local indices + 48 B of
                            metric terms per element); fp32 storage (mixed): 8 nnz + 4 n + 8 k n / 8 k n + 88 T        */
    int64_t pcg_steps;   /* total PCG steps executed on the device (incl. post-convergence slack)  */
    double spmv_ms_raw;  /* the same sum before the correction                                     */
    double event_overhead_ms; /* elapsed time of an EMPTY hipEvent pair on the stream (min of 16),
                            i.e. what a bracket measures beyond the kernel it encloses             */
    int64_t refinement_cycles; /* mixed precision: fp32 inner solves that contributed a correction (all chunks) */
    int32_t op_used;     /* 0 = the CG applied A as a CSR SpMM, 3 = patch operator (remo_opts_t.op) */
    int32_t coarse_used; /* vertex-block solver of the run: 0 = none ("local"), 1 = Chebyshev polynomial, 2 = multigrid cycle */
    int32_t assembled;   /* 1 = the whole matrix, 2 = only the Jacobi diagonal and the P1 (vertex) block (remo_opts_t.assemble):
                            then remo_batch_get_system hands out dinv / freeid only and nnz reads 0                  */
    int32_t patch_rounds; /* patch operator: elements a lane of its kernel took, 1 or 2 (remo_debug_tune key 40); 0 with the CSR product.
                            (In the place of a reserved field: the layout is the one of ABI 7.) */
} remo_stats_t;

typedef struct remo_ctx remo_ctx_t;
typedef struct remo_batch remo_batch_t;

int remo_abi_version(void);
void remo_opts_default(remo_opts_t *opts);

/* One context per GPU (hipSetDevice(device_id), one stream, a grow-only device arena). */
remo_ctx_t *remo_ctx_create(int device_id);
void remo_ctx_destroy(remo_ctx_t *ctx);
/* Text of the last error on this context (or of the failed remo_ctx_create when ctx == NULL). */
const char *remo_last_error(remo_ctx_t *ctx);

/* The entries with an argument list, from here to remo_solve_job: each is remo_solve_job with axis positions z and the parts its name says. */
/*
 * Whole batch in one call: the inner hot loop of worker.py:104-131.
 * RHS k has point sources src_z[src_ptr[k] .. src_ptr[k+1]) on the borehole axis with strengths
 * src_I (zero strengths are skipped, ngsolve_functions.py:43) and is read at axis positions
 * eval_z[eval_ptr[k] .. eval_ptr[k+1]).  u_out[eval_ptr[n_rhs]] receives u_h at those points
 * (the raw FE potential; the 1/2 of the 3D half-space model and the geometric factor are applied
 * by the caller as in worker.py:124-131).
 */
int remo_solve_batch(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                     int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                     const int32_t *eval_ptr, const double *eval_z, double *u_out,
                     const remo_opts_t *opts, remo_stats_t *stats);

/*
 * The same for anisotropic materials (added within ABI 7: the change is additive - callers detect it by the
 * presence of the symbol, and REMO_ABI_VERSION stays 7).  sigma_tensor[n_mat * nc] holds, per material, the upper
 * triangle of a symmetric positive definite conductivity tensor, row-major, in the mesh's frame:
 *   dim 2 (r, z): nc = 3, [rr, rz, zz];   dim 3 (x, y, z): nc = 6, [xx, xy, xz, yy, yz, zz].
 * The element terms become |T| grad(l_a)^T S grad(l_b) (2D: weighted by 2 pi r as before); a tensor that is exactly
 * sigma * I gives terms bit-identical to remo_solve_batch with sigma.  A material whose entries are not finite or
 * whose leading principal minors are not all > 0 is rejected with REMO_ERR_ARG (outputs NaN).
 */
int remo_solve_batch_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                            int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                            const int32_t *eval_ptr, const double *eval_z, double *u_out,
                            const remo_opts_t *opts, remo_stats_t *stats);

/*
 * The same solves plus the derivatives of linear measurement functionals of the potentials with respect to the material
 * conductivities, by adjoint solves (added within ABI 7: additive, detected by the presence of the symbols).  Functional j reads
 * right-hand side fun_rhs[j] at the axis points fun_z[fun_ptr[j] .. fun_ptr[j+1]) with weights fun_w:
 *     J_j = sum_i fun_w[i] * u_rhs(fun_z[i])
 * - the reading of worker.py:113-131 (u_N - u_M, or u_M alone) before the geometric factor.  With A u = f, J = g^T u and
 * A lambda = g, dJ/dsigma_m = -lambda^T (dA/dsigma_m) u: one extra block of solves (the adjoint columns, chunks of REMO_MAX_RHS,
 * same operator, preconditioner and stopping rule as the forward columns) and one pass over the elements per functional.
 * J_out[n_fun]; dJ_out[n_fun * n_mat * nc], functional-major: nc = 1 and dJ_j/dsigma_m for the scalar entry; for the tensor entry
 * nc = 3 (2D) or 6 (3D) in the upper-triangle layout of sigma_tensor, the derivative with respect to the parameter that sets both
 * S_ab and S_ba (off-diagonal entries carry both halves).  In 2D with condense = 1 the derivative is that of the full system (the
 * cell bubbles of u and lambda are recovered).  The sums have a fixed order (no floating-point atomics): with op = 2 dJ_out is
 * reproducible bit for bit.  u_out is filled as by remo_solve_batch; stats cover the forward and the adjoint solves
 * (iterations / relres: the last chunk solved).  n_fun = 0 is allowed (the functional arrays may then be NULL).
 * Errors: as remo_solve_batch, all three outputs NaN-filled; a functional point outside the mesh gives REMO_ERR_POINT;
 * precision = 1 (mixed) gives REMO_ERR_ARG (the derivatives are formed in fp64), as does a fun_rhs outside [0, n_rhs).
 */
int remo_solve_batch_sens(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                          int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                          const int32_t *eval_ptr, const double *eval_z, double *u_out,
                          int32_t n_fun, const int32_t *fun_rhs /*[n_fun]: which right-hand side it reads*/,
                          const int32_t *fun_ptr /*[n_fun+1]*/, const double *fun_z, const double *fun_w,
                          double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat]*/,
                          const remo_opts_t *opts, remo_stats_t *stats);
int remo_solve_batch_sens_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                                 int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                                 const int32_t *eval_ptr, const double *eval_z, double *u_out,
                                 int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                                 double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat * nc]*/,
                                 const remo_opts_t *opts, remo_stats_t *stats);

/*
 * The same call plus the derivatives with respect to caller-defined GROUPS of elements - a pixel of a grid, one element, anything
 * (added within ABI 7: additive, detected by the presence of the symbols).  group[mesh->n_elems] labels every element, in the
 * caller's element order, with an id in [0, n_group), or -1 for "in no group".  With sigma_e = sigma_mat(e) + p_group(e),
 *     dJg_out[(j * n_group + g) * nc + c] = dJ_j/dp_g = -sum_{e in g} lambda_e^T (dK_e / d component c) u_e,
 * components as in dJ_out (nc = 1, or 3 / 6 for the tensor entry, off-diagonal entries carrying both halves).  A group may mix
 * materials; a group without elements gets 0; n_group is bounded by memory only (n_group = n_elems with group[e] = e is the
 * per-element map).  Every group's sum has a fixed order that depends only on the mesh and the grouping (no floating-point
 * atomics): with op = 2 dJg_out is reproducible bit for bit.  u_out, J_out and dJ_out are exactly what remo_solve_batch_sens
 * returns for the same inputs (the material pass runs as it does there).
 * Errors: n_group < 1, group == NULL or an id outside [-1, n_group) give REMO_ERR_ARG before any device work, all outputs
 * NaN-filled; everything else as remo_solve_batch_sens (precision = 1 gives REMO_ERR_ARG).
 */
int remo_solve_batch_sens_groups(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                                 int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                                 const int32_t *eval_ptr, const double *eval_z, double *u_out,
                                 int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                                 int32_t n_group, const int32_t *group /*[mesh->n_elems], caller's element order, -1 = in no group*/,
                                 double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat]*/, double *dJg_out /*[n_fun * n_group]*/,
                                 const remo_opts_t *opts, remo_stats_t *stats);
int remo_solve_batch_sens_groups_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                                        int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                                        const int32_t *eval_ptr, const double *eval_z, double *u_out,
                                        int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                                        int32_t n_group, const int32_t *group,
                                        double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat * nc]*/, double *dJg_out /*[n_fun * n_group * nc]*/,
                                        const remo_opts_t *opts, remo_stats_t *stats);

/*
 * Solutions that survive a call (added within ABI 7: additive, detected by the presence of the symbols).  A remo_warm_t owns one
 * device allocation on device_id (plain hipMalloc, grow-only) that after a successful remo_solve_batch_sens_warm holds the solutions
 * of all its forward and adjoint columns, n_free * (n_rhs + n_fun) doubles.  It is tied to the device, not to a context: any context
 * of that device may use it, one call at a time.  Meant for repeated calls on one mesh with slowly changing conductivities (an
 * inversion's iterations): the next call solves A d = f - A x_prev for a correction of the stored solutions instead of starting every
 * column from zero.
 *   warm == NULL                 exactly remo_solve_batch_sens.
 *   empty or mismatched object   (dim, n_nodes, n_elems, n_bfacets, condense, n_free, n_rhs or n_fun differs from what was stored:
 *                                a memory-safety check, nothing more) the solve runs cold - with op = 2 u_out, J_out and dJ_out
 *                                carry the bits of remo_solve_batch_sens - and the object is filled afterwards.
 *   matching object              per chunk of columns: q = A x_prev, f' = f - q, the unchanged PCG from zero on A d = f' down to the
 *                                absolute threshold the cold solve would have used (rtol^2 <C f, f> of the current system and
 *                                preconditioner, measured by one PCG step on f), x = x_prev + d.  A chunk whose f' is already below
 *                                it takes no further step.  Correctness never depends on the match: a stale guess only costs steps.
 *                                stats: relres is relative to <C f, f>; pcg_steps counts the measuring step of every chunk.
 * A call that returns < 0 leaves the object cleared; REMO_NOT_CONVERGED stores what it has.  precision = 1 gives REMO_ERR_ARG, an
 * object of another device than the context's too.  remo_warm_create returns NULL (text: remo_last_error(NULL)) without a device.
 * remo_warm_info: rows and columns stored (0 when empty), bytes allocated, and whether the last call that was handed the object
 * started from its solutions (used_last); any pointer may be NULL.
 */
typedef struct remo_warm remo_warm_t;
remo_warm_t *remo_warm_create(int device_id);
void remo_warm_destroy(remo_warm_t *w);
void remo_warm_clear(remo_warm_t *w); /* forget the stored solutions, keep the allocation */
int remo_warm_info(const remo_warm_t *w, int64_t *n_free, int32_t *n_cols, int64_t *bytes, int32_t *used_last);
int remo_solve_batch_sens_warm(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                               int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                               const int32_t *eval_ptr, const double *eval_z, double *u_out,
                               int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                               double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat]*/, remo_warm_t *warm,
                               const remo_opts_t *opts, remo_stats_t *stats);
int remo_solve_batch_sens_warm_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                                      int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                                      const int32_t *eval_ptr, const double *eval_z, double *u_out,
                                      int32_t n_fun, const int32_t *fun_rhs, const int32_t *fun_ptr, const double *fun_z, const double *fun_w,
                                      double *J_out /*[n_fun]*/, double *dJ_out /*[n_fun * n_mat * nc]*/, remo_warm_t *warm,
                                      const remo_opts_t *opts, remo_stats_t *stats);

/*
 * The same solves plus the solution AWAY from the borehole axis: the potential, its gradient and the current density at arbitrary
 * points of the mesh (added within ABI 7: additive, detected by the presence of the symbols).  pts[n_pts * dim] are points in the
 * mesh's frame, (r, z) in 2D and (x, y, z) in 3D; field_rhs[n_frhs] names the right-hand sides that are read there - any subset of
 * [0, n_rhs), in any order.  Outputs, each of which may be NULL, column-major over the entries of field_rhs:
 *     u_f[j * n_pts + q]                 u_h of right-hand side field_rhs[j] at point q (the raw FE potential, as u_out);
 *     grad_f[(j * n_pts + q) * dim + c]  grad u_h there, (d/dr, d/dz) or (d/dx, d/dy, d/dz): the gradient of the element the point
 *                                        was found in - grad u_h jumps across element faces;
 *     J_f[(j * n_pts + q) * dim + c]     J = -Sigma grad u_h with the conductivity (scalar or tensor) of that element's material;
 *     elem_f[q]                          the element the point was found in, numbered as in mesh->conn.
 * Among several elements that hold a point (shared faces, edges and vertices; in 3D the whole plane y = 0) the choice is
 * deterministic: two calls give the same elem_f.  A point in no element - a rectangular section may stick out of the domain - is no
 * error: elem_f = -1 and NaN in the three values.  The points are located once per batch through a cell grid over their bounding box
 * (no n_pts * n_elems pass), and every chunk of REMO_MAX_RHS right-hand sides is read right after its solve.  In 2D with
 * condense = 1 the cell bubbles are recovered as for u_out.  n_pts = 0 and n_frhs = 0 are allowed.
 * u_out and stats are what remo_solve_batch returns for the same inputs: bit for bit with op = 2, to rounding with op = 3.
 * Errors: as remo_solve_batch, all outputs NaN-filled and elem_f = -1; a field_rhs outside [0, n_rhs) gives REMO_ERR_ARG before any
 * device work, as does precision = 1 (the field is formed from the fp64 solution); a non-finite point gives REMO_ERR_POINT.
 */
int remo_solve_batch_field(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                           int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                           const int32_t *eval_ptr, const double *eval_z, double *u_out,
                           int32_t n_pts, const double *pts /*[n_pts * dim]*/, int32_t n_frhs, const int32_t *field_rhs /*[n_frhs]*/,
                           double *u_f /*[n_frhs * n_pts]*/, double *grad_f /*[n_frhs * n_pts * dim]*/, double *J_f /*[n_frhs * n_pts * dim]*/,
                           int32_t *elem_f /*[n_pts]*/, const remo_opts_t *opts, remo_stats_t *stats);
int remo_solve_batch_field_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                                  int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                                  const int32_t *eval_ptr, const double *eval_z, double *u_out,
                                  int32_t n_pts, const double *pts, int32_t n_frhs, const int32_t *field_rhs,
                                  double *u_f, double *grad_f, double *J_f, int32_t *elem_f,
                                  const remo_opts_t *opts, remo_stats_t *stats);

/*
 * One entry for all of the above, with sources and readings ANYWHERE in the mesh (added within ABI 7: additive, detected by the
 * presence of the symbols).  The caller describes the work in a struct instead of an argument list; every point is a full
 * coordinate in the mesh's frame, (r, z) in 2D and (x, y, z) in 3D, where the entries above take axis positions z.
 *   Zero-initialise the struct, set size = sizeof(remo_job_t), then sigma, the sources and the evaluation points: that is
 *   remo_solve_batch (tensor = 1: remo_solve_batch_tensor).  n_fun > 0 adds the functionals of remo_solve_batch_sens (their points
 *   fun_p), n_group > 0 the groups of remo_solve_batch_sens_groups, warm != NULL the object of remo_solve_batch_sens_warm; n_pts or
 *   n_frhs != 0 adds the field points of remo_solve_batch_field.  Each part follows the rules of the entry it comes from: argument
 *   checks, NaN-filled outputs (elem_f -1) on a negative return, stats, the warm object cleared on a negative return.
 *   Refused with REMO_ERR_ARG, as there is no entry above that does it: field points together with functionals; groups or a warm
 *   object without functionals; precision = 1 with functionals or field points.
 *   size: the struct may grow at its end.  A smaller size (an older caller) reads the missing members as zero; a larger one (a newer
 *   caller) is accepted if the bytes this library does not know are all zero, else REMO_ERR_ARG; a size that does not reach n_fun
 *   is REMO_ERR_ARG.
 * What a source is: the weak form's f += I * phi(p).  In 2D a source at r > 0 is a RING that carries the total current I (the form
 * has the weight 2 pi r already).  In 3D the half ball stands for the whole one by mirror symmetry in y = 0: a source in that plane
 * (the axis included) gives the solution of 2 I in the full space - the caller halves, as for axis sources - and a source at y > 0
 * stands for itself and its mirror image.
 * Points: a batch whose points all have lateral coordinates exactly 0.0 is located and read by the kernels of the axis entries -
 * with op = 2 its outputs carry the bits of the entry it stands for.  Otherwise all its points are located through the cell grid of
 * remo_solve_batch_field (same tolerances, lowest element number among several that hold a point).  A point in no element gives
 * REMO_ERR_POINT - in the half ball that includes y < 0 - and a non-finite coordinate gives REMO_ERR_POINT before any device work.
 *
 * secondary = 1: the SECONDARY-POTENTIAL formulation (added within ABI 7: four members BEHIND the job - remo_job_secondary_t below, a
 * job with size = sizeof(remo_job_secondary_t) - which a caller's smaller size leaves zero).  u = u_p + u_s with u_p the closed-form potential of the right-hand side's sources in a
 * homogeneous medium sigma0 inside a grounded sphere of radius sec_radius centred at the origin of the batch frame,
 *     u_p = I / (4 pi sigma0) G(x; a),   G(x; a) = 1 / |x - a| - (R / |a|) / |x - a*|,   a* = R^2 a / |a|^2
 * (|a| <= 1e-9 R: the image term is -1 / R; R = 0: no image term; 3D half ball: G(x; a) + G(x; a mirrored in y = 0), which gives a
 * source in the plane the 2 I of the convention above), and u_s the finite-element solution of
 *     a_Sigma(u_s, v) = - int (Sigma - sigma0 I) grad(u_p) . grad(v),   u_s = 0 on the Dirichlet boundary:
 * same operator, preconditioner and PCG, another load vector.  The integrand vanishes where Sigma = sigma0 I, so with sigma0 the
 * conductivity around the sources the elements never resolve a 1 / r singularity.  Per element with Sigma_e != sigma0 I
 *     f_e[i] = - sum_q w_q |T| (2 pi r_q in 2D) grad(phi_i)(x_q)^T (Sigma_e - sigma0 I) grad(u_p)(x_q)
 * by the collapsed (conical) Gauss-Legendre product rule with n = sec_quad points per direction on [0, 1] (0: the default, 7):
 *     2D  l_1 = u, l_2 = v (1 - u), weight 2 (1 - u) w_u w_v;   3D  l_1 = u, l_2 = v (1 - u), l_3 = w (1 - u)(1 - v), weight
 *     6 (1 - u)^2 (1 - v) w_u w_v w_w;   l_0 = 1 - the others, barycentrics of the element's vertices sorted by number.
 * The element vectors are added into f row by row in ascending element order (no floating-point atomics): with op = 2 two calls
 * give the same bits.  In 2D with condense = 1 every contributing element has a bubble load; it is folded into the nine outer
 * rows (f_j -= K_j9 f_9 / K_99) and used again when the bubble of an evaluation point's element is recovered.
 * u_out = u_s + u_p at every evaluation point.  A homogeneous model (Sigma = sigma0 I everywhere) has f = 0: u_s = 0, 0
 * iterations, REMO_OK.  sec_sigma0[n_rhs] is the background of every right-hand side; NULL, or an entry 0.0, stands for the
 * (scalar) conductivity of the element that holds the right-hand side's first source of non-zero strength.
 * Errors: an evaluation point on a source of its right-hand side, and a source in or on (k_locate's tolerance) an element with
 * Sigma_e != sigma0 I - a source on a conductivity contrast - give REMO_ERR_POINT.  Refused with REMO_ERR_ARG before any device
 * work: secondary together with functionals, groups, a warm object or field points; precision = 1; in 2D a source at r != 0.0 (a
 * ring); a sec_sigma0 entry that is negative or not finite; sec_quad outside [0, 16]; a negative sec_radius; and, where sigma0 is
 * left to the library, a source in an anisotropic material or sources of one right-hand side in materials of different
 * conductivity.  remo_batch_create_job reads the four members too (remo_batch_get_vectors then shows this f and u_s);
 * remo_batch_eval and remo_batch_field read u_h alone and refuse such a batch.
 */
typedef struct {
    uint32_t size;                 /* sizeof(remo_job_t) as the caller compiled it */
    int32_t tensor;                /* 0: sigma[n_mat]; 1: sigma[n_mat * nc] upper triangles (remo_solve_batch_tensor) */
    int32_t n_mat; const double *sigma;
    int32_t n_rhs; const int32_t *src_ptr; const double *src_p /*[src_ptr[n_rhs] * dim]*/; const double *src_I;
    const int32_t *eval_ptr; const double *eval_p /*[eval_ptr[n_rhs] * dim]*/; double *u_out;
    int32_t n_fun; const int32_t *fun_rhs, *fun_ptr; const double *fun_p /*[fun_ptr[n_fun] * dim]*/, *fun_w; double *J_out, *dJ_out;
    int32_t n_group; const int32_t *group; double *dJg_out;       /* n_group = 0: no groups */
    remo_warm_t *warm;                                            /* NULL: cold */
    int32_t n_pts; const double *pts; int32_t n_frhs; const int32_t *field_rhs; double *u_f, *grad_f, *J_f; int32_t *elem_f;
} remo_job_t;
/* The job grown at its end by the four members of the secondary-potential formulation (see above): the same bytes as a remo_job_t
 * with the members appended - job is 232 bytes, a multiple of every member's alignment, so nothing is padded - under a name of its
 * own, so that sizeof(remo_job_t) stays what callers compiled against it know.  Set job.size = sizeof(remo_job_secondary_t) and hand
 * &x.job to remo_solve_job / remo_batch_create_job. */
typedef struct {
    remo_job_t job;
    int32_t secondary;          /* 0: as before, bit for bit.  1: secondary-potential formulation */
    int32_t sec_quad;           /* points per direction of the element rule, 0 = default */
    double  sec_radius;         /* R of the grounded sphere of the primary field, 0 = none */
    const double *sec_sigma0;   /* [n_rhs] background conductivity per right-hand side; NULL or 0.0 = the (scalar) conductivity
                                   of the element that holds the right-hand side's first source */
} remo_job_secondary_t;
/*
 * err = 1: goal-oriented ERROR ESTIMATES of the functionals (added within ABI 7: five members behind remo_job_secondary_t, which
 * keeps its 256 bytes as remo_job_t keeps its 232; set job.size = sizeof(remo_job_error_t) and hand &x.sec.job to remo_solve_job).
 * The error a caller sees in a reading is the discretisation error of the mesh; J(u) - J(u_h) = a(u - u_h, lambda - lambda_h) is
 * bounded element by element by an indicator of u times one of the adjoint solution lambda the sensitivities solve for anyway.
 * For a solution column v, an element e (vertices sorted) and a facet F of e (a face in 3D, an edge in 2D) with unit normal n out of
 * e, q_e = n . Sigma_e grad v_h|_e:
 *     interior facet, shared with e':   [q] = q_e - n . Sigma_e' grad v_h|_e',  s_F = (n.Sigma_e n + n.Sigma_e' n) / 2,  c_F = 1/2;
 *     boundary facet, not Dirichlet:    [q] = q_e,  s_F = n.Sigma_e n,  c_F = 1   (y = 0 of the half ball, the axis in 2D);
 *     Dirichlet facet:                  0;
 *     eta_e(v)^2 = sum_F c_F h_F / (2 p s_F) int_F [q]^2 dS,  p = 3, h_F the longest edge of F, dS with 2 pi r in 2D,
 * integrated exactly (three Gauss-Legendre points on an edge, the symmetric six-point rule of degree 4 on a face); in 2D with
 * condense = 1 the cell bubbles of both elements are recovered first.  Functional j, which reads right-hand side fun_rhs[j]:
 *     E_je = eta_e(u_fun_rhs[j]) * eta_e(lambda_j),   err_out[j] = E_j = sum_e E_je   (in the units of J_j),
 *     errg_out[j * err_n_group + g] = sum over the elements e with err_group[e] = g of E_je   (an empty group: 0).
 * The constant is the conventional one and is not claimed to be sharp; the delta sources are not part of the residual - near an
 * electrode the estimate comes from the facet jumps alone.  The grouping is the estimate's own: group / dJg_out and err_group /
 * errg_out may differ in one call.  Every element sums its own facets and all sums have a fixed order (no floating-point atomics):
 * two calls give the same bits.  u_out, J_out, dJ_out and dJg_out are exactly what the same job returns with err = 0 (bit for bit
 * with op = 2).  Allowed with tensors, groups, a warm object and points off the axis.
 * Errors, REMO_ERR_ARG before any device work: err = 1 with n_fun = 0, with secondary = 1, with field points or with precision = 1;
 * an err other than 0 or 1; err_out == NULL; err_n_group < 0; err_n_group > 0 without err_group or errg_out; a group id outside
 * [-1, err_n_group).  On any negative return err_out and errg_out are NaN-filled like the other outputs.  remo_batch_create_job
 * refuses err = 1: a resident batch has no functionals.
 */
typedef struct {
    remo_job_secondary_t sec;
    int32_t err;                /* 0: as before, bit for bit.  1: error estimates of the functionals */
    int32_t err_n_group;        /* 0: no groups */
    const int32_t *err_group;   /* [mesh->n_elems], caller's element order, -1 = in no group */
    double *err_out;            /* [n_fun]               E_j  */
    double *errg_out;           /* [n_fun * err_n_group] Eg_j,g; may be NULL when err_n_group = 0 */
} remo_job_error_t;             /* 288 bytes */
/*
 * n_pair > 0: PAIR DERIVATIVES - the derivatives of all transfer impedances of an electrode array by reciprocity (added within ABI 7:
 * five members behind remo_job_error_t, which keeps its 288 bytes; set job.size = sizeof(remo_job_pairs_t) and hand &x.err.sec.job to
 * remo_solve_job).  A multi-electrode tool reads linear combinations of Z_ij, the potential at electrode i per unit current at
 * electrode j.  A is symmetric, so the adjoint of "read u at electrode i" is the forward solution of a source at electrode i:
 *     Z_ij = e_i^T A^{-1} f_j,    dZ_ij/dsigma_m = -u_i^T (dA/dsigma_m) u_j,
 * with u_i and u_j both right-hand sides of the batch - no adjoint solves.  For the right-hand sides a = pair_a[p], b = pair_b[p]
 *     dP_out[(p * n_mat + m) * nc + c] = -u_a^T (dA / d component c of material m) u_b,
 * components as in dJ_out (nc = 1, or 3 / 6 for tensor = 1, off-diagonal entries carrying both halves).  Any order, a == b and
 * repeats are allowed, and a pair may join columns of different chunks of REMO_MAX_RHS.  Z itself is what u_out gives when the
 * electrodes are listed as evaluation points.  In 2D with condense = 1 the cell bubbles of both columns are recovered, each with the
 * point loads of its own chunk.  One pass over the elements serves all pairs of one or two chunks (pairs.h): the element vector of
 * every column is gathered once and reduced to 30 (2D: 40) moments, and a pair costs an inner product of those.  Every sum has a fixed
 * order (no floating-point atomics): with op = 2 two calls give the same bits of dP_out.  n_fun = 0 is allowed with pairs; with
 * functionals, groups or err in the same job u_out, J_out, dJ_out, dJg_out and err_out are exactly what the job returns with
 * n_pair = 0 (bit for bit with op = 2).  n_pair = 0: as before, bit for bit.
 * Errors, REMO_ERR_ARG before any device work: a pair_a / pair_b outside [0, n_rhs); NULL arrays or a NULL dP_out with n_pair > 0;
 * n_pair < 0; pair_reserved != 0; pairs together with secondary = 1, with field points, with a warm object or with precision = 1.
 * On any negative return dP_out is NaN-filled like the other outputs.  remo_batch_create_job refuses n_pair > 0.
 */
typedef struct {
    remo_job_error_t err;
    int32_t n_pair;                   /* 0: as before, bit for bit */
    int32_t pair_reserved;            /* must be 0 */
    const int32_t *pair_a, *pair_b;   /* [n_pair] right-hand sides */
    double *dP_out;                   /* [n_pair * n_mat * nc], pair-major */
} remo_job_pairs_t;                   /* 320 bytes */
/*
 * pair_n_group > 0: PAIR DERIVATIVES PER GROUP OF ELEMENTS - the sensitivity maps of an electrode array (added within ABI 7: four
 * members behind remo_job_pairs_t, which keeps its 320 bytes; set job.size = sizeof(remo_job_pair_groups_t) and hand
 * &x.pairs.err.sec.job to remo_solve_job).  With u_a,e the element vector of right-hand side a = pair_a[p] on element e,
 *     dPg_out[(p * pair_n_group + g) * nc + c] = -sum over the elements e with pair_group[e] = g of u_a,e^T (dK_e / d component c) u_b,e,
 * components as in dP_out: with sigma_e = sigma_mat(e) + s_group(e) the derivative of the pair's transfer impedance with respect to
 * s_g.  A group may mix materials, an empty group gets +0, an element with pair_group[e] = -1 is in no group; pair_n_group is
 * bounded by memory only, and pair_group[e] = e gives the value of every element.  The grouping is the pairs' own, as err_group is
 * the estimate's own: group / dJg_out may differ from it in the same job.  The element pass of the pairs runs a second time in a
 * form that writes the value of every (pair, element); the elements are ordered by group once per job and every group's segment is
 * added as remo_solve_batch_sens_groups adds it, for all pairs of a slice in one launch.  Every sum has a fixed order that depends
 * only on the mesh, the grouping and the job (no floating-point atomics): with op = 2 two calls give the same bits of dPg_out.
 * u_out, J_out, dJ_out, dJg_out, err_out and dP_out are exactly what the same job returns with pair_n_group = 0 (bit for bit with
 * op = 2).  pair_n_group = 0: as before, bit for bit.
 * Errors, REMO_ERR_ARG before any device work: pair_n_group < 0; pair_group_reserved != 0; pair_n_group > 0 with n_pair = 0, without
 * pair_group or without dPg_out; a group id outside [-1, pair_n_group); and what pairs do not combine with.  On any negative return
 * dPg_out is NaN-filled like the other outputs.  remo_batch_create_job refuses pair_n_group > 0.
 */
typedef struct {
    remo_job_pairs_t pairs;
    int32_t pair_n_group;             /* 0: as before, bit for bit */
    int32_t pair_group_reserved;      /* must be 0 */
    const int32_t *pair_group;        /* [mesh->n_elems], caller's element order, -1 = in no group */
    double *dPg_out;                  /* [n_pair * pair_n_group * nc], pair-major */
} remo_job_pair_groups_t;             /* 344 bytes */
int remo_solve_job(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t *job, const remo_opts_t *opts, remo_stats_t *stats);

/*
 * Staged form of the same work, for callers that keep a batch resident (bench.py: inputs are in
 * HBM before the timed region).  create = validate + upload; run = numbering, pattern, assembly,
 * PCG, evaluation, all RHS; fetch = potentials to the host.
 */
int remo_batch_create(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma,
                      int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                      const int32_t *eval_ptr, const double *eval_z, remo_batch_t **out);
/* The same with the conductivity tensors of remo_solve_batch_tensor (same layout, same checks; added within ABI 7): the
 * resident form, so that the inspection hooks below see tensor batches too. */
int remo_batch_create_tensor(remo_ctx_t *ctx, const remo_mesh_t *mesh, int32_t n_mat, const double *sigma_tensor,
                             int32_t n_rhs, const int32_t *src_ptr, const double *src_z, const double *src_I,
                             const int32_t *eval_ptr, const double *eval_z, remo_batch_t **out);
/* The same from a job (reads tensor, sigma, the sources and the evaluation points only): the resident form of batches with points
 * off the axis.  remo_batch_eval stays an axis entry; remo_batch_field reads anywhere. */
int remo_batch_create_job(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t *job, remo_batch_t **out);
int remo_batch_run(remo_ctx_t *ctx, remo_batch_t *batch, const remo_opts_t *opts, remo_stats_t *stats);
int remo_batch_fetch(remo_ctx_t *ctx, remo_batch_t *batch, double *u_out);
void remo_batch_destroy(remo_ctx_t *ctx, remo_batch_t *batch);

/*
 * u_h of right-hand side `rhs` of the last remo_batch_run at further axis points - the
 * `gfu(mesh(0.0, z))` / `gfu(mesh(0.0, 0.0, z))` of worker.py:124-131 for callers that keep the
 * solution object around (remo3d_amd/ngsolve_functions_hip.py).  Valid until the next run on the
 * context, for batches of at most REMO_MAX_RHS right-hand sides.  Points outside the mesh give
 * NaN and REMO_ERR_POINT.
 */
int remo_batch_eval(remo_ctx_t *ctx, remo_batch_t *batch, int32_t rhs, int32_t n_points, const double *z, double *u_out);

/*
 * The same for arbitrary points of the mesh, with the outputs of remo_solve_batch_field for the one right-hand side `rhs`:
 * u[n_points], grad[n_points * dim], J[n_points * dim], elem[n_points] (any may be NULL).  Scalar and tensor batches alike; valid
 * as long as remo_batch_eval is.  Points outside the mesh give NaN / elem = -1 and are no error.
 */
int remo_batch_field(remo_ctx_t *ctx, remo_batch_t *batch, int32_t rhs, int32_t n_points, const double *pts,
                     double *u, double *grad, double *J, int32_t *elem);

/*
 * Inspection hooks used by the parity tests (tests/): the assembled system of the last
 * remo_batch_run on this batch.  Pass NULL to skip an array.  rowptr[n_free+1], col[nnz],
 * val[nnz], dinv[n_free] (Jacobi), freeid[n_dof] (free row of each dof or -1).
 */
int remo_batch_get_system(remo_ctx_t *ctx, remo_batch_t *batch, int32_t *rowptr, int32_t *col,
                          double *val, double *dinv, int32_t *freeid);
/* Solution and load vectors of the LAST chunk of right-hand sides of the last remo_batch_run (chunks hold at most
 * REMO_MAX_RHS columns): x[n_free * k], f[n_free * k], row-major with k = *k_out columns.  Either pointer may be NULL.
 * With remo_batch_spmv this lets a test measure the TRUE residual f - A x of what CGSolver's silent stopping rule
 * (ngsolve_functions.py:50-51) left behind. */
int remo_batch_get_vectors(remo_ctx_t *ctx, remo_batch_t *batch, double *x, double *f, int32_t *k_out);
/* Inspection hook (tests): z = one application of the multigrid cycle the last run built on the P1 block (remo_opts_t.coarse;
 * replaces the "multigrid" preconditioner object of ngsolve_functions.py:46 on that block) to k column-interleaved vectors
 * r[nv][k]; fp32 != 0: through the fp32 image of the hierarchy (what fp64 solves use by default).  nv_out receives the block size
 * (r and z may be NULL to ask for it).  Fails when the last run used the polynomial. */
int remo_batch_apply_coarse(remo_ctx_t *ctx, remo_batch_t *batch, int32_t k, const double *r, double *z, int32_t fp32, int64_t *nv_out);

/* y = A x on the device with the batch's matrix, k interleaved columns (x[n_free*k] row-major);
 * reps >= 1 launches are timed with HIP events, average ms returned in *ms_avg. */
int remo_batch_spmv(remo_ctx_t *ctx, remo_batch_t *batch, int32_t k, const double *x, double *y,
                    int32_t reps, double *ms_avg);

/*
 * Host-side pieces exposed for CPU-only tests (no GPU needed):
 *  - the pre-integrated reference tensors contracted with one element's metric terms, i.e. the
 *    element matrix the assembly kernel gathers from (nld x nld, nld = 10 or 20);
 *  - dof numbering + CSR pattern of a mesh.
 */
int remo_host_element_matrix(int32_t dim, const double *vertex_coords /*[(dim+1)*dim], sorted vertices*/,
                             double sigma, double *K_out);
/* The same with a conductivity tensor in the layout of remo_solve_batch_tensor (REMO_ERR_ARG if not finite and positive definite). */
int remo_host_element_matrix_tensor(int32_t dim, const double *vertex_coords, const double *sigma_tensor, double *K_out);
/* The element contraction of remo_solve_batch_sens on the host (the code the kernel runs): out[nc] = x_l^T (dK_e / d component) x_u
 * for element vectors x_l, x_u [nld]; tensor = 0: nc = 1 (d/dsigma), else nc = 3 / 6 (upper triangle, off-diagonal both halves). */
int remo_host_sens_element(int32_t dim, const double *vertex_coords, int32_t tensor, const double *x_l, const double *x_u, double *out);
/* The element arithmetic of remo_job_pairs_t on the host (the code the kernel runs): the moments of the k element vectors x[k * nld]
 * once, then out[p * nc + c] = x_a^T (dK_e / d component c) x_b for a = pa[p], b = pb[p] in [0, k) from the moments alone - the value
 * remo_host_sens_element forms from the two vectors, by another order of summation.  REMO_ERR_MESH for a degenerate element. */
int remo_host_pair_element(int32_t dim, const double *vertex_coords, int32_t tensor, int32_t k, const double *x, int32_t n_pair,
                           const int32_t *pa, const int32_t *pb, double *out);
/* The per-point arithmetic of remo_solve_batch_field on the host (the code the kernel runs): out[1 + 2 * dim] = u, grad u, J at
 * `point` [dim] of the element with sorted vertices vertex_coords and element vector x_e [nld].  sigma_tensor != NULL: the upper
 * triangle of the material's tensor (REMO_ERR_ARG if not finite and positive definite), else the scalar sigma. */
int remo_host_field_element(int32_t dim, const double *vertex_coords, const double *sigma_tensor, double sigma, const double *x_e,
                            const double *point, double *out);
/* The shape values of a point anywhere in an element on the host (the code k_point_shapes_at runs): phi_out[nld] at `point` [dim] of
 * the element with sorted vertices vertex_coords - what a source there adds to the load, times I, and what a reading there weighs
 * the element vector with.  REMO_ERR_MESH for a degenerate element. */
int remo_host_point_shapes(int32_t dim, const double *vertex_coords, const double *point, double *phi_out);
/* One element's load vector of the secondary formulation on the host (the code the kernel runs): f_out[nld] for a unit current at
 * src [dim] in the background sigma0 inside a grounded sphere of radius `radius` (0: none), n_quad points per direction (0: the
 * default); sigma_tensor != NULL: the upper triangle of the element's tensor, else the scalar sigma.  The raw element vector: no
 * bubble fold.  Sigma_e = sigma0 I gives exact zeros.  REMO_ERR_MESH for a degenerate element. */
int remo_host_secondary_element(int32_t dim, const double *vertex_coords, const double *sigma_tensor, double sigma,
                                double sigma0, double radius, const double *src /*[dim]*/, int32_t n_quad,
                                double *f_out /*[nld]*/);
/* The facet term of the error indicator of remo_job_error_t on the host (the code the kernel runs): *out = c_F h_F / (2 p s_F)
 * int_F [q]^2 dS of facet `facet` of element e - 3D: 0 .. 3, the faces 012 013 023 123 of its sorted vertices; 2D: 0 .. 2, the edges
 * 01 02 12 - from e's sorted vertex coordinates, element vector x_e [nld] and conductivity (sigma_tensor_e != NULL: the upper
 * triangle, else sigma_e).  vertex_coords_n != NULL: an interior facet, with the same three of the neighbour; NULL: a natural
 * boundary facet.  REMO_ERR_ARG for a tensor that is not finite and positive definite, REMO_ERR_MESH for a degenerate element. */
int remo_host_error_facet(int32_t dim, int32_t facet, const double *vertex_coords_e, const double *sigma_tensor_e, double sigma_e, const double *x_e,
                          const double *vertex_coords_n, const double *sigma_tensor_n, double sigma_n, const double *x_n, double *out);
/* max |sum_m B_a[m][i] B_b[m][j] - M_ab[i][j]|: how well the factorised reference tensors of the patch operator
 * (remo_opts_t.op = 3) reproduce the tensors the CSR assembly contracts (both exact polynomial integrals). */
double remo_host_factor_error(void);
int remo_host_symbolic(const remo_mesh_t *mesh, int32_t condense, int64_t *sizes /*[6]: n_dof,n_free,nnz,n_edges,n_faces,nld*/,
                       int32_t *rowptr /*[n_free+1] or NULL*/, int32_t *col /*[nnz] or NULL*/,
                       int32_t *freeid /*[n_dof] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* REMO3D_HIP_H */
