/*
 * remo3d_hip_debug.h — probes and tuning knobs of libremo3d_hip.so for tests/, tools/ and bench.py's `box` record.
 * NOT part of the drop-in boundary (include/remo3d_hip.h is: the surface SURVEY.md section 8b describes, replacing the seam
 * of remo3d/workers/worker.py:32-35, 110); nothing here is needed to run a batch, and the knobs are process-global.
 */
#ifndef REMO3D_HIP_DEBUG_H
#define REMO3D_HIP_DEBUG_H

#include "remo3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What this GPU streams (bench.py `box`): a read of `bytes` through a plain 16-byte-per-lane summing kernel and a device-to-device
 * copy of them, HIP events, best of six; GB/s (the copy counts read + write).  With bytes <= 192 MiB the read figure is that of four
 * back-to-back re-reads of the buffer, i.e. of the 256 MB Infinity Cache rather than of HBM. */
int remo_debug_stream(remo_ctx_t *ctx, int64_t bytes, double *read_gbs, double *copy_gbs);
/* Rate of a chain of DEPENDENT fp32 multiply-adds of one wave (1024 waves over the chip at once), in 1e9 per second: follows the
 * shader clock under load - the part of the box-to-box spread that the stream figures do not show. */
int remo_debug_clock(remo_ctx_t *ctx, double *gfma_per_wave);
/* Scattered 16-byte reads from a buffer of `bytes` (a power of two) by 4096 workgroups, useful GB/s: 2 MiB stays in every XCD's L2 (the
 * path of the SpMM's x gather); 256 MiB adds the address translation of pages scattered over the memory. */
int remo_debug_cache_gather(remo_ctx_t *ctx, int64_t bytes, double *gbs);
/* hipDeviceProp_t of the context's GPU: compute units, clock kHz, memory clock kHz, bus width, L2 bytes, memory MiB, LDS bytes per CU, revision. */
int remo_debug_device(remo_ctx_t *ctx, int64_t *out8);
/* XCD (hardware register XCC_ID) of workgroups 0 .. nblocks-1 of a probe launch: the SpMM's row schedule assumes b mod 8. */
int remo_debug_xcc(remo_ctx_t *ctx, int32_t *out, int32_t nblocks);


/* Where a workgroup of the patch operator (remo_opts_t.op = 3, k = 5, fp64) spends its time: clock ticks between the phase
 * boundaries of k_patch_apply averaged over the workgroups of one launch - out16[0..6] = row tables into LDS | staging of x | x into registers |
 * zeroing | tensor arithmetic + LDS accumulation | output | partial sums; [7] whole workgroup; [8] first start to last end of the
 * launch; [9] workgroups.  The last run on the batch must have used the patch operator. */
int remo_debug_patch_phases(remo_ctx_t *ctx, remo_batch_t *batch, int32_t fp32 /* the fp32 instantiation instead */, double *out16);

/* The same for the PERSISTENT form of the kernel (k_patch_apply_p): clock ticks per patch of wave 0, summed by the workgroups over their
 * patches and averaged - out16[0..8] = barrier B0 | issue of the next patch's LDS-DMA | x values into registers | barrier B1 | clearing + B2 |
 * tensor chains + LDS accumulation | wait for the DMA and older stores | barrier B3 | rows out; [10] patches, [11] workgroups, [12] ticks of the
 * busiest workgroup (sum of its phases), [13] microseconds per application without the stamps.  -DREMO_PROBES builds only. */
int remo_debug_patch_phases_p(remo_ctx_t *ctx, remo_batch_t *batch, int32_t fp32, double *out16);

/* Cost of a grid-wide barrier between the resident workgroups of one launch (nblocks <= 2048 workgroups of 256 threads; nbar
 * iterations of: agent-scope store, barrier, agent-scope load of another workgroup's store, barrier): out3[0] = microseconds per
 * barrier, [1] = 1 if a wait gave up, [2] = loads that did not see the store. */
int remo_debug_grid_barrier(remo_ctx_t *ctx, int32_t nblocks, int32_t nbar, double *out3);

/* The contraction launches of the last remo_solve_batch_sens on this context: out2[0] = their time in ms (HIP events around the
 * launches of all functionals and the reduction), [1] = their algorithmic bytes (per functional the x rows of the forward and the
 * adjoint column once, per element its dof numbers, vertices and material). */
int remo_debug_sens_timing(remo_ctx_t *ctx, double *out2);
/* The group path of the last remo_solve_batch_sens_groups on this context, ms by HIP events: out4[0] = the group order (upload of the
 * group array, keys, radix sort, offsets; once per batch); and, only from a run with remo_opts_t.time_kernels set (it then
 * synchronises after every functional), summed over the functionals: [1] = the material pass, [2] = the per-element pass,
 * [3] = the group sums.  0 where not measured. */
int remo_debug_sens_group_timing(remo_ctx_t *ctx, double *out4);
/* The field path of the last remo_solve_batch_field / remo_batch_field on this context, ms by HIP events: out2[0] = the location of
 * the points (cells, radix sort, offsets, both element passes; once per batch), out2[1] = the evaluation launches of all chunks. */
int remo_debug_field_timing(remo_ctx_t *ctx, double *out2);
/* How the last remo_batch_run on this context located the points of its right-hand sides: 0 = the kernels of the axis entries (every
 * lateral coordinate exactly 0), 1 = the cell grid of the field sections (a batch of remo_solve_job with a point off the axis). */
int remo_debug_point_location(remo_ctx_t *ctx);
/* Bytes per stored value of the PCG's search direction in the last remo_batch_run on this context: 4 or 8 (0 before the first run).
 * 4: a one-shot fp64 solve on the patch operator that carries only the evaluated values of x (remo_debug_tune key 41), or the mixed
 * mode (precision = 1), whose inner solver stores every vector in fp32.  8: every other fp64 solve - resident batches, the CSR
 * product and all of 2D, the sens, warm and field entries. */
int remo_debug_direction_bytes(remo_ctx_t *ctx);
/* ONE direction launch of an fp64 solve with the search direction in fp32 storage, on the caller's own data and in both forms: the
 * flat form (k_pcg_direction_flat<double, k, float>) and the row form (k_pcg_direction_row<double, k, float>), each from the same
 * inputs, `grid` workgroups of 256 threads.  r [n][k], p [n][k] (float), z [nv][k] (the vertex rows' preconditioned residual, stored
 * divided by the Jacobi factor; nv = 0: none), dinv [n]; part_even / part_odd [nb_rz][k]: the partial sums of <Cr, r> left by the
 * update launch of an even / odd step + 1 - the launch of `step` reads the set of (step + 1) & 1; scal48: the scalar block, 48 doubles:
 * <Cr0, r0> [8] | <p, A p> [8] | <Cr, r> of even steps [8] | of odd steps [8] | the done word (an int in the first of 8) | the floors [8].
 * Out: p after the launch and the scalar block after it (the new <Cr, r> forwarded in it), per form.  No solve is involved, so the two
 * forms are comparable bit for bit. */
int remo_debug_direction_forms(remo_ctx_t *ctx, int64_t n, int64_t nv, int32_t k, int32_t grid, int32_t step, double tol2, const double *r,
                               const float *p, const double *z, const double *dinv, const double *part_even, const double *part_odd,
                               int32_t nb_rz, const double *scal48, float *p_flat, float *p_row, double *scal_flat, double *scal_row);
/* ONE sparse product C = X Y of the multigrid hierarchy's setup (amg.hip: k_spgemm count pass, scan, clamp, fill pass) on the caller's
 * own matrices: X [nx rows] and Y [ny rows] as CSR on the host, the columns of X naming rows of Y, the columns inside a row of Y
 * distinct; slots = 128 or 512 (the kernel variant: a row of C may hold slots / 2 distinct columns); cap = the capacity of C's arrays.
 * Out: crp [nx + 1] (clamped to cap), cc and cv [cap + 2] - the arrays as the setup allocates them, every byte 0xFF where the launch
 * wrote nothing - and flags[0]: bit 1 = a row did not fit its tables (it is left empty), bit 2 = the product outgrew cap.
 * Row by row C holds the sorted distinct columns, and per column the sum, in the order of X's row and starting from + 0.0, of the
 * separately rounded products: reproducible bit for bit. */
int remo_debug_product(remo_ctx_t *ctx, int32_t slots, int64_t cap, int64_t nx, const int32_t *xrp, const int32_t *xc, const double *xv,
                       int64_t ny, const int32_t *yrp, const int32_t *yc, const double *yv, int32_t *crp, int32_t *cc, double *cv,
                       int32_t *flags);
/* ONE row operation of the multigrid cycle (amg.hip) on the caller's own CSR matrix [n rows, columns in 0 .. nx) and vectors [rows][k]
 * on the host, by the kernel the cycle launches, in device memory of its own that starts out as 0xFF bytes:
 *   op 0  y = M x, `lanes` (8, 16, 32 or 64) lanes per row - the restriction's form (the prolongation's is the same sum with 8);
 *         out = y [n][k]
 *   op 1  first half sweep: out = z = omega D^-1 r, out2 = t = r - omega A D^-1 r; x holds r; nx = n
 *   op 2  second half sweep of a coarser level: out = z + omega D^-1 (r - A z); x holds z; nx = n
 *   op 3  the finest level's second half sweep: out = (z + omega D^-1 (r - A z)) / D^-1 and out2 = the <r, z_new> partial sums of
 *         `nblocks` workgroups [nblocks][k], whose column sums are the products of the columns; x holds z; nx = n
 * dinv [n] = D^-1 (ops 1 - 3), r [n][k] (ops 2, 3).  reading: 0 = the sweep walks the CSR rows in 1024-thread workgroups, 1 = op 3
 * reads the fixed-width image of the matrix in 256-thread workgroups that keep four row groups in flight, as the cycle does where the
 * image exists (rows beyond the image's width come from its tail list); ops 1 - 3 take 8 lanes.
 * fp32 = 1: values, factors and the level's vectors are stored in float - out of ops 0 and 2 and out, out2 of op 1 are float arrays -
 * while r of op 1 and r, out of op 3 stay double, as in an fp64 solve that runs the cycle in fp32; fp32 = 0: everything double.
 * The partial sums are double.  out and out2 receive the raw bytes of the result arrays and of `guard` (<= 4096) further elements
 * behind each, which must still be 0xFF bytes.  Sums keep a fixed order: the same call twice gives the same bytes. */
int remo_debug_row_ops(remo_ctx_t *ctx, int32_t op, int32_t lanes, int32_t reading, int32_t fp32, int64_t n, int64_t nx, int32_t k, const int32_t *rowptr,
                       const int32_t *col, const double *val, const double *dinv, double omega, const double *x, const double *r, int32_t nblocks,
                       int32_t guard, void *out, void *out2);
/* Where a workgroup of the PCG's two vector launches spends its time before its first stored value (-DREMO_PROBES builds only):
 * on = 1 makes wave 0 of every workgroup of k_pcg_direction_flat and k_pcg_update_tile leave three clocks (on entry | scalars in
 * LDS | at the end) from now on; on = 0 stops that and reports the LAST launch of each kind that was not a no-op:
 * out8[0..3] = direction launch: mean ticks of the head, of the whole workgroup, mean of head / whole per workgroup, workgroups;
 * out8[4..7] = the same for the update launch.  Run a batch between the two calls.  ONE context of ONE device at a time: the stamp
 * buffer is process-wide and the kernels' pointer to it is set on the calling context's device; switch the probe off (on = 0) before
 * that context is destroyed. */
int remo_debug_vector_heads(remo_ctx_t *ctx, int32_t on, double *out8);
/* The load-vector launches (element vectors + row sums, all chunks) of the last remo_batch_run of a batch with remo_job_secondary_t.secondary
 * on this context, ms by HIP events; 0 when the last run was none. */
int remo_debug_secondary_timing(remo_ctx_t *ctx, double *ms);
/* The pair pass of the last job with remo_job_pairs_t.n_pair > 0 on this context: out2[0] = its time in ms (HIP events around the element
 * launches of all chunk pairs and the reduction), [1] = the number of element launches. */
int remo_debug_pairs_timing(remo_ctx_t *ctx, double *out2);
/* The group path of the last job with remo_job_pair_groups_t.pair_n_group > 0 on this context, ms by HIP events: out4[0] = the ordering
 * of the elements by group (upload, keys, sort, offsets), [1] = the per-element launches of all slices, [2] = their group sums - the
 * two are told apart only with remo_opts_t.time_kernels (one synchronisation per slice), else [1] holds both and [2] = 0 -,
 * [3] = the number of slices (one per-element launch and one batched group sum each).  Zeros when the last job had no pair groups. */
int remo_debug_pair_groups_timing(remo_ctx_t *ctx, double *out4);

/* Process-global knobs, two kinds.  Returns 0, or -1 for a key this build does not have.
 *
 * (a) ALWAYS THERE - keys that force one of the product's own paths, i.e. a choice the library makes by size or dimension, so that
 * a small test mesh reaches the code a large batch runs.  Every setting gives the same operator / preconditioner to rounding:
 *    3  row schedule of the CSR product (0 grid-stride, 1 XCD windows, 16 * nc XCD regions of nc chunks; -1 = by size);
 *    6  0 = one launch per Chebyshev step, 1 = paired steps on the squared vertex block in 2D (default), 2 = also in 3D;
 *    9  0 = first Chebyshev step as a launch of its own instead of inside the update launch (k_pcg_update_folded);
 *   13  0 = Chebyshev launches read the vertex block inside A, 1 = from a compact copy above 16 k vertices (default), 2 = always;
 *   15  0 = the Chebyshev chain of an fp64 solve stays in fp64 also above 32 k vertex rows (default there: fp32 storage), 2 = fp32 always;
 *   16  1 = never the multigrid cycle on the vertex block, 2 = always, any dimension (0: remo_opts_t.coarse decides);
 *   17  0 = the multigrid cycle of an fp64 solve stays in fp64 (default: fp32 storage);
 *   18  0 = elements taken in the caller's order (default 1: sorted by their two smallest vertices);
 *   22  0 = rows shared by patches summed by k_patch_reduce instead of the PCG's update launch;
 *   24  0 = Chebyshev launches walk the vertex block as CSR instead of its fixed-width image;
 *   25  0 = x += alpha p formed by the update launch instead of the direction launch of the step (bit-identical x);
 *   29  0 = the update launch fetches four slab slots for every row and weights the ones the row does not have by zero
 *          (k_pcg_update without MASKED; also keeps the tile form away);
 *   30  0 = the direction launch takes a k-wide row per lane (k_pcg_direction_row) instead of walking its vectors as flat arrays,
 *          16 bytes per lane (k_pcg_direction_flat);
 *   31  0 = the update launch takes a k-wide row per lane (k_pcg_update) instead of 64 rows per wave with a value per lane and
 *          pass (k_pcg_update_tile, fp64 storage);
 *   39  0 = one-shot fp64 solves (remo_solve_batch[_tensor]) carry the whole solution block instead of only the values the
 *       evaluation points read (default 1; bit-identical potentials on the CSR product).  Resident batches always keep the whole x.
 *   41  0 = those solves keep the search direction p in fp64 on the patch operator too (default 1: p is STORED in fp32 there and
 *       widened by its three readers - the direction launch, the operator's staging phase, the evaluated values of the update
 *       launch; r, q, the slab and every sum stay fp64; same potentials to the solve's tolerance, under 1 % more steps).  Keys
 *       39 = 0, 25 = 0 and 22 = 0 imply fp64.  remo_debug_direction_bytes says which form the last run took.
 *   42  0 = the pair derivatives of remo_job_pairs_t by one launch of k_sens_contract per pair, both columns forward, instead of
 *       the fused pass of k_pair_contract (default 1; the same values to rounding - what the fused pass is measured against).
 *   43  bytes of element values ev[pairs][elements][nc] one per-element launch of remo_job_pair_groups_t may write (0 = default,
 *       128 MB; always one pair at least): a (chunk, chunk) set of pairs with more takes several slices.  The order of the additions
 *       of a (pair, group) does not depend on the slice: the same bits at any setting.
 *   40  1 = the patch operator takes one element per lane: patches of 256 / k elements (k = right-hand sides of the batch);
 *       2 (default) = two elements per lane, one after the other, in fp64 solves with k >= 3: patches of 2 * (256 / k) elements
 *       (k_patch_apply ROUNDS = 2).  A batch whose largest such patch does not fit the tables or LDS gets the tables of 1.
 *       Read when a batch's tables are built (every run).
 *
 * (b) ONLY IN A LIBRARY BUILT WITH -DREMO_PROBES (`make -C remo3d_amd/csrc probes` -> libremo3d_hip_probes.so, loaded by the tools
 * through REMO_LIB=...): rejected experiments and ablations, some of which give WRONG RESULTS ON PURPOSE.  The product ignores them:
 *    0 SpMM variant, 1 lanes per row, 2 threads per workgroup, 4 grid size, 5 ablation mode of the pair kernel; 7 lanes per row of
 *    the paired Chebyshev kernel; 8: 0 = CSR pattern by the global sort; 21 ablation
 *    mode of the patch kernel (1 no LDS atomics, 2 no arithmetic, 3 no output); 26 register-lean order
 *    of the patch kernel (0 never, 1 always; product: fp32 storage only); 27: 0 = slab slots of a shared row fetched one by one;
 *    28: 0 = a row of <p, A p> per patch + a folding launch; 32 runs of the patch's list per wave (product: 4); 33: 0 = every
 *    workgroup walks the largest patch's row count; 34: 1 / 2 = the patch operator as persistent workgroups that prefetch the next patch by
 *    LDS-DMA / through registers (round 4: parity-green, 138 / 111.5 us against 112 at size L: DESIGN.md section 8), 35 their number per XCD
 *    (0 = as many as stay resident); 36 extra operator applications per PCG step (results discarded: what more applications would cost);
 *    44 lanes per row of R in the multigrid cycle's restrictions (8 / 16 / 32 / 64; product: by R's row lengths); 45: 0 = the cycle's
 *    last sweep walks CSR rows (no fixed-width image of level 0); 46: 1 = the cycle's last sweep on the image in 1024-thread workgroups.
 *    (Keys 19, 23, 37 and 38 - 512-thread workgroups, a row-major slab, unshared rows straight to y, staggered starts of the patch
 *    kernel - left with their code; DESIGN.md section 8 keeps the measurements.)
 *    remo_debug_patch_phases[_p] and remo_debug_grid_barrier also need that build. */
int remo_debug_tune(int32_t key, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* REMO3D_HIP_DEBUG_H */
