// tune.h — every process-wide tuning switch of remo_debug_tune with its key and default.  remo_debug.hip defines g_tune and is its
// only writer; the launchers and table builders read the fields where the comments say.  Not installed, not a public header.
#pragma once

namespace remo {

// "probe builds": the key exists in the library built with -DREMO_PROBES only (tools/); the field is there in both builds where
// product code reads it.  "Batches built afterwards": read when a batch's pattern or tables are built, not when a launch is made.
struct Tune {
    // the CSR product (kernels.hip spmm_dispatch, spmv_grid); 0 = heuristic default
    int spmm_variant = 0;    // key 0 (probe builds): 1 = lane per stored entry, 3 = edge row pairs (default)
    int spmm_lpr = 0;        // key 1 (probe builds): lanes per row
    int spmm_threads = 0;    // key 2 (probe builds): threads per workgroup
    int spmm_mapping = -1;   // key 3: row schedule of the pair kernel, -1 = by size (default); 0 is a setting of its own
    int spmm_grid = 0;       // key 4 (probe builds): workgroups
    int spmm_mode = 0;       // key 5 (probe builds): ablation mode of the pair kernel (K = 5, 16 lanes per row only)
    int square = 1;          // key 6: 0 = one launch per Chebyshev step, 1 = paired steps in 2D (default), 2 = paired steps always
    int sq_lanes = 0;        // key 7 (probe builds): lanes per row of the paired kernel (0 = by row length)
    int row_pattern = 1;     // key 8 (probe builds): 0 = always build the CSR pattern by the global sort instead of row by row (batches built afterwards)
    int fold_first = 1;      // key 9: 1 = FIRST Chebyshev step inside the update launch (default; k_pcg_update_folded), 0 = own launch
    int compact = 1;         // key 13: 1 = Chebyshev launches read a compact copy of the vertex block above 16 k vertex rows (default), 2 = at any size, 0 = the leading entries of A's rows in place
    int chain32 = 1;         // key 15: 1 = fp32 Chebyshev chain inside fp64 solves above 32 k vertex rows (default), 2 = at any size, 0 = chain in fp64
    int amg = 0;             // key 16: 0 = remo_opts_t.coarse decides, 1 = never the multigrid cycle, 2 = always (any dimension)
    int amg32 = 1;           // key 17: 1 = fp64 solves run the multigrid cycle in fp32 storage (default), 0 = in fp64
    int element_order = 1;   // key 18: 0 = keep the caller's element order (batches built afterwards)
    int defer_q = 1;         // key 22: 1 = the PCG's update launch sums the patch operator's shared rows itself (default), 0 = k_patch_reduce does
    int ell = 1;             // key 24: 1 = the Chebyshev launches of 3D read the fixed-width image of the vertex block (default), 0 = its CSR form
    int x_in_direction = 1;  // key 25: 1 = x += alpha p formed by the direction launch of the step (default), 0 = by the update launch
    int slab_ahead = 1;      // key 27 (probe builds): 0 = the update launch walks the slab slots of a shared row one by one (default 1: four in flight)
    int dot_bins = 1;        // key 28 (probe builds): 1 = the patches add their <p, A p> straight into the update launch's rows (default), 0 = a row per patch + k_patch_dot
    int slab_masked = 1;     // key 29: 1 = k_pcg_update<.., MASKED = true> (default), 0 = every row fetches four slab slots and weights the ones it does not have by zero (the form before)
    int flat_direction = 1;  // key 30: 1 = the direction launch walks its vectors as flat arrays, 16 bytes per lane (default; k_pcg_direction_flat), 0 = a k-wide row per lane (k_pcg_direction_row)
    int tile_update = 1;     // key 31: 1 = the update launch of fp64 storage takes 64 rows per wave, a value per lane and pass (default; k_pcg_update_tile), 0 = k_pcg_update
    int patch_spread = 4;    // key 32 (probe builds): runs of the patch's list the lanes of a wave take their elements from (batches built afterwards)
    int patch_trim = 1;      // key 33 (probe builds): 0 = every patch walks the largest patch's row count (batches built afterwards)
    int x_ev = 1;            // key 39: 1 = one-shot fp64 solves carry only the values of x the evaluation points read (default), 0 = the whole x
    int patch_rounds = 2;    // key 40: 2 = two elements per lane of the patch operator where the patch then fits its tables (default; patch_rounds), 1 = one; stored as 1 or 2 (batches built afterwards)
    int p32 = 1;             // key 41: 1 = those solves, on the patch operator, store the search direction in fp32 (default; PcgBuffersT::p32), 0 = in fp64
    int pairs_fused = 1;     // key 42: 1 = the pairs of remo_job_pairs_t in one fused element pass per chunk pair (default; k_pair_contract), 0 = one launch of k_sens_contract per pair
    int pair_ev_bytes = 0;   // key 43: bytes of element values one per-element launch of remo_job_pair_groups_t writes (0 = kPairEvBytes; always one pair at least)
#ifdef REMO_PROBES
    int patch_mode = 0;          // key 21 (probe builds): ablation mode of k_patch_apply (fp64, k = 5 only), 4 = phase stamps
    int patch_lean = -1;         // key 26 (probe builds): register-lean arithmetic phase of k_patch_apply: -1 = in fp32 storage only (default), 0 = never, 1 = always (patch.hip patch_dispatch)
    int patch_persist = 0;       // key 34 (probe builds): 1 / 2 = persistent forms (patch_persist.inc), 0 = k_patch_apply (default); stored as 0, 1 or 2
    int patch_wgs_per_xcd = 0;   // key 35 (probe builds): workgroups per XCD of the persistent forms (0 = as many as stay resident); tests make small meshes walk several patches per workgroup; stored >= 0
    int extra_apply = 0;         // key 36 (probe builds): extra operator applications (apply + shared-row sums, results discarded) per PCG step: what a step with more applications would cost
    int amg_r_lanes = 0;         // key 44 (probe builds): lanes per row of R in the cycle's restrictions, 8 / 16 / 32 / 64 (0 = by R's row lengths, AmgLevelT::r_lanes)
    int amg_image = 1;           // key 45 (probe builds): 0 = no fixed-width image of the cycle's level 0, its last sweep walks CSR rows in 1024-thread workgroups (batches built afterwards)
    int amg_post_wide = 0;       // key 46 (probe builds): 1 = the cycle's last sweep on the image in 1024-thread workgroups, a row group each (default 0: 256 threads, four row groups in flight)
#endif
};
extern Tune g_tune;

}  // namespace remo
