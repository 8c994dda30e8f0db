// patch.h — host side of the patch operator (patch.hip): the per-batch tables.
#pragma once
#include "kernels.h"
#include "symbolic_gpu.h"

namespace remo {

size_t patch_arena_bytes(int64_t nt, int64_t n_max, int kmax);
// Enqueues the table kernels on s (no synchronisation).  flag_and_max: three device ints the caller reads after its next
// synchronisation - [0] != 0: a patch holds more distinct rows than the tables do (use another operator), [1]: the largest
// row count of a patch (PatchOpT::lds_rows), [2]: slots of the boundary slab in use (the caller sets PatchTables::nslot_cap to it).
// rounds: elements a lane takes (PatchTables::rounds; 2 is honoured where patch_rounds allows it).
void build_patch_tables(Arena &ar, hipStream_t s, const DeviceSymbolic &sy, const double *C, int kmax, int rounds, PatchTables &out, int32_t *flag_and_max);
int patch_rounds(int kmax, int wanted);                   // 2 where wanted and 2 * (256 / kmax) elements fit the table builder (kmax >= 3), else 1
int patch_elements_per_group(int kmax, int rounds);       // E = rounds * (256 / kmax): one lane per (element, right-hand side) and round, at most 204
void set_patch_rounds(int v);                             // remo_debug_tune key 40 (product key): 2 = two rounds where they fit (default), 1 = one; batches built afterwards
int patch_rounds_wanted();

// Switches of patch.hip behind remo_debug_tune (remo_debug.hip); the keys exist in probe builds only (-DREMO_PROBES)
void set_patch_mode(int mode);                     // key 21: ablation mode of k_patch_apply (k = 5), 4 = phase stamps
void set_patch_stamps(long long *device_buffer);   // mode 4: [workgroups][8] phase time stamps
void set_patch_lean(int v);                        // key 26: register-lean arithmetic phase: -1 fp32 only (default), 0 never, 1 always
void set_patch_spread(int v);                      // key 32: runs of the patch's list the lanes of a wave take their elements from (batches built afterwards)
void set_patch_trim(int v);                        // key 33: 0 = every patch walks the largest patch's row count (batches built afterwards)
int set_patch_persist(int form);                   // key 34: 1 / 2 = persistent forms (patch_persist.inc), 0 = k_patch_apply; returns the setting it replaces
void set_patch_wgs_per_xcd(int n);                 // key 35: workgroups per XCD of the persistent forms

}  // namespace remo
