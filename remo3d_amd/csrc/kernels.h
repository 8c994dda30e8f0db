// kernels.h — launchers of the gfx950 kernels (kernels.hip; the PCG step's: pcg_kernels.hip; the vertex-block solver's: vertex_solver.h) and the dispatch on the column count
// they share (for_k).  All launches are asynchronous on the given stream; no launcher allocates or synchronises.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "elem_access.h"
#include "tune.h"
#include "vertex_solver.h"

namespace remo {

constexpr int kMaxPartialBlocks = 1024;   // grid cap of every kernel that leaves per-block partial sums
constexpr int kMaxPoints = 256;          // sources + evaluation points of one RHS chunk

template <int V> using int_c = std::integral_constant<int, V>;
// fn(int_c<K>) for the column counts the solver kernels are instantiated for: K = k for k in 1 .. 7, K = 8 for every other k (a
// launcher with a stricter contract checks k before it dispatches).  A generic lambda instantiates every kernel it names for all
// eight K: what exists for some T or some build only stays behind `if constexpr` inside it.
template <class F> void for_k(int k, F &&fn) {
    switch (k) {
        case 1: fn(int_c<1>{}); break;
        case 2: fn(int_c<2>{}); break;
        case 3: fn(int_c<3>{}); break;
        case 4: fn(int_c<4>{}); break;
        case 5: fn(int_c<5>{}); break;
        case 6: fn(int_c<6>{}); break;
        case 7: fn(int_c<7>{}); break;
        default: fn(int_c<8>{}); break;
    }
}
// fn(bool_constant<B>): a kernel's boolean template parameter from a run-time flag
template <class F> void for_bool(bool b, F &&fn) {
    if (b) fn(std::true_type{}); else fn(std::false_type{});
}
// the launches of the PCG step and of the vertex solver: `grid` workgroups of 256 threads, no dynamic LDS
template <class Kernel, class... Args> void launch256(Kernel kernel, int grid, hipStream_t s, Args... args) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, args...); }

// per-iteration record the PCG kernels write straight into mapped host memory
struct PcgProgress {
    double rz[8];        // <Cr,r> per column at the START of step `step`
    int32_t step;        // written last
    int32_t pad;
};

// T = storage type of matrix values and vectors: double (product path) or float (inner solver of the
// mixed-precision mode); scalars and partial sums are double in both
template <class T> struct PcgBuffersT {
    T *x, *r, *p, *q;       // [n*k]
    const T *dinv;          // [n]
    double *part_pq;        // [kMaxPartialBlocks*8] per-workgroup partial sums of <p, Ap>
    double *part_rz;        // [2][kMaxPartialBlocks*8] per-workgroup partial sums of <Cr, r> (even / odd step)
    double *rz0;            // [48] totals forwarded between launches: <Cr0,r0>[8] | <p,Ap>[8] | <Cr,r> of even / odd steps [8+8] | done flag [8] | floor of <Cr,r> [8]
    VertexSolverT<T> vs;    // the solver of the P1 (vertex) block of the two-level preconditioner (vertex_solver.h); vs.degree = 0 -> Jacobi
    // patch operator only: q = A p is left WITHOUT the sums of the rows shared by several patches - the update launch, which reads
    // q once anyway, forms them from the boundary slab itself (one launch and one pass over the slab less per step).  Set by the
    // host when the operator is the patch operator and the update launch does not gather q (no folded Chebyshev step).
    bool defer_q = false;
    // x += alpha p is formed by the DIRECTION launch of the step (it reads the old p anyway; alpha recomputed there from the same operands:
    // bit-identical x) instead of the update launch, which then reads neither p nor x: one pass over p less per step
    bool x_in_direction = false;
    // patch operator, with defer_q: the patches add their <p, A p> into kPqBins rows of part_pq themselves (atomic adds; two sets of
    // rows taken in turn by step parity, the update launch of a step clears the set of the next) - no launch that folds them
    bool pq_bins = false;
    // evaluated values only (one-shot fp64 solves, x = nullptr, x_in_direction): x_ev[j] carries x[x_ev_at[j]] (x_ev_at[j] = row * k +
    // column, or -1: nothing), formed by the update launch with the direction launch's arithmetic, so it holds the bits the full
    // x would.  The direction launch then neither reads nor writes x: two vectors of its ~five per step.  [x_ev_n]
    const int64_t *x_ev_at = nullptr;
    T *x_ev = nullptr;
    int x_ev_n = 0;
    // evaluated values only, on the patch operator with defer_q (T = double): the search direction is STORED in fp32 here and p is
    // nullptr.  p is written by the direction launch and read by it, by the operator's staging phase and by the x_ev slots of the
    // update launch - all three widen the stored value, none keeps an unrounded copy, so q = A p, x += alpha p and r -= alpha q use
    // one and the same p and the recurrences stay consistent; the stored direction loses conjugacy at the 6e-8 level only
    // (remo_debug_tune key 41).  [n*k]
    float *p32 = nullptr;
    PcgProgress *progress; // mapped host records [progress_len]: one per step, the last one is the "all columns frozen" record
    int progress_len;
    int nb_spmv, nb_vec;    // grid sizes actually used (partials valid for these many blocks)
};
using PcgBuffers = PcgBuffersT<double>;
constexpr int kPqBins = 256;       // rows of a set of <p, A p> bins (PcgBuffersT::pq_bins); set s starts at part_pq + s * kPqBins * 8
constexpr int kScalarSlots = 48;   // doubles behind PcgBuffersT::rz0
constexpr int kDoneSlot = 4 * 8;   // rz0[kDoneSlot] (as int): step + 1 of the update launch that froze every column (kutil.h solve_done)

// Patch operator (3D, remo_opts_t.op = 3; patch.hip): the element list cut into runs of E elements, one workgroup each
struct PatchTables {
    int64_t nt = 0, n = 0, npatch = 0;
    int E = 0;                         // elements per patch = rounds * (kPatchBlock / right-hand sides of the batch) (one lane per element and column, `rounds` elements per lane)
    int rows_cap = 0;                  // rows of prow / pout per patch
    // block, all_slab, stagger: CONSTANTS (build_patch_tables sets 256 / 1 / 0) that no code reads, kept where they are because the
    // struct is a by-value argument of every patch kernel: dropping them shifts every argument load (a follow-up)
    int block = 256;
    int trim = 1;                      // 1: a workgroup's staging / output phases stop at its own patch's row count
    int spread = 4;                    // the lanes of a wave take their elements from this many runs of the patch's list (k_patch_apply; <= 1: one run)
    const uint16_t *lidx = nullptr;    // [nt][20] local row of every element dof inside its patch, 0xFFFF = constrained
    const int32_t *pcount = nullptr;   // [npatch] distinct free rows of the patch
    const int32_t *prow = nullptr;     // [npatch][rows_cap] matrix row of local row m, ascending
    const int32_t *pout = nullptr;     // [npatch][rows_cap] slot of local row m in the slab: pboff[p] + m
    const int32_t *pboff = nullptr;    // [npatch + 1] first slab slot of every patch (its rows' slots are consecutive, in ascending row order)
    int all_slab = 1;                  // (layout only, see block)
    const int32_t *row4 = nullptr;     // [n][4] the first four slab slots of every row (-1 none, [3] = -2: five or more, the rest in bslot)
    const int32_t *bptr = nullptr;     // [n + 1] entries [bptr[r], bptr[r + 1]) of bslot belong to row r, one per patch that touches it
    const int32_t *bslot = nullptr;    // slab slot of each (row, patch) pair; the slab itself is patch-major (a patch's shared rows are one block)
    const double *C = nullptr;         // [nt][6] metric terms (launch_metric_terms)
    int64_t nslot_cap = 0;             // upper bound of bptr[n]: rows of the slab
    int stagger = 0;                   // (layout only, see block)
    int rounds = 1;                    // elements a lane of k_patch_apply takes, one after the other: E = rounds * (256 / right-hand sides) (in the struct's tail padding)
};
template <class T> struct PatchOpT {
    PatchTables t;
    T *Yb = nullptr;                   // [nslot_cap][k] boundary slab
    double *ppart = nullptr;           // [npatch][8] <x, y> of every patch's own rows
    int lds_rows = 0;                  // largest pcount: sizes the kernel's LDS
    bool dot_bins = false;             // PcgBuffersT::pq_bins of the solve that applies it
};
#ifndef REMO_PATCH_PASSES
#define REMO_PATCH_PASSES 12
#endif
constexpr int kPatchPasses = REMO_PATCH_PASSES;   // staging passes a lane's registers hold (k_patch_apply)
constexpr int kPatchBlock = 256;                  // threads per workgroup of k_patch_apply; the tables are laid out for it
// dynamic LDS of k_patch_apply: staged k-wide rows (later the fp64 accumulators; + the zero row and one of slack); a workgroup may
// ask for 64 KB less the kernel's static 128 k bytes.  (No row tables in LDS - the row numbers go straight into registers - so five
// workgroups of a 700-row batch share a CU's 160 KB; patches of two rounds have up to ~1000 rows at size L: 40 KB, three workgroups.)
inline size_t patch_lds_bytes(int lds_rows, int k) { return size_t(lds_rows + 2) * size_t(k) * 8; }
constexpr size_t kPatchLdsLimit = 63 * 1024;


template <class T> struct CsrViewT {
    int64_t n;
    int64_t nnz;
    const int32_t *rowptr;
    const int32_t *col;
    const T *val;          // [nnz + 1] allocated: the pair SpMM loads two values per stored entry, so the last entry of a single row reads one element past nnz
    // rows [pair_begin, pair_end) are the two dofs of each free edge, consecutive and with identical
    // column patterns; their VALUES are stored interleaved (launch_assemble).  0, 0 = no pairs, plain CSR
    int64_t pair_begin = 0, pair_end = 0;
    const PatchOpT<T> *patch = nullptr; // != nullptr: launch_spmm applies the patch operator (patch.hip)
    bool vertex_block_only = false;     // rowptr / col / val hold only the leading P1 block (rows and columns < the free vertex count): products need `patch`
};
using CsrView = CsrViewT<double>;

// WRITES em.C[nt][NTERM] (the view's pointer is const for its readers; the caller owns the buffer) from em.sigma[n_mat] scalars
// (em.eperm may be null); a bad material or a degenerate element raises bit 1 of *errflag
void launch_metric_terms(const ElemMesh &em, int32_t *errflag, hipStream_t s);
// anisotropic materials: em.sigma[n_mat][3 (2D: rr, rz, zz) or 6 (3D: xx, xy, xz, yy, yz, zz)] (fem_p3.h metric_terms_tensor)
void launch_metric_terms_tensor(const ElemMesh &em, int32_t *errflag, hipStream_t s);
// rows [pair_begin, pair_end) (the two dofs of every free edge) get their values interleaved: entry e of the first row
// at rowptr[row] + 2e, of the second at rowptr[row] + 2e + 1 (CsrViewT below); all other rows plain CSR
void launch_diag_rows(int dim, int64_t row0, int64_t nfree, const int32_t *adjptr, const uint32_t *adj, const double *C, const double *M, double *dinv, hipStream_t s);
void launch_assemble(int dim, bool condense, int64_t nfree, int64_t pair_begin, int64_t pair_end, const int32_t *rowptr, const int32_t *col,
                     const int32_t *adjptr, const uint32_t *adj, const int32_t *eldof, const double *C,
                     const double *M, double *val, double *dinv, hipStream_t s);

int spmv_grid(int64_t n, int lanes_per_row);
int vec_grid(int64_t n);
int choose_lanes_per_row(int64_t n, int64_t nnz);
// y = A x for k interleaved columns; if part != nullptr also leaves per-block partial sums of <x_c, y_c>
// scal != nullptr: the launch belongs to PCG step `step` and returns at once when an earlier step froze every column
template <class T> bool patch_applies(const CsrViewT<T> &A, int k);   // launch_spmm will take the patch operator for k columns
// defer = true (patch operator inside the PCG): rows shared by several patches are NOT summed into y (PcgBuffersT::defer_q)
template <class T> void launch_spmm(const CsrViewT<T> &A, int k, const T *x, T *y, double *part, const double *scal, int nblocks, hipStream_t s, int step = 0, bool defer = false);

template <class T> void launch_patch_spmm(const CsrViewT<T> &A, int k, const T *x, T *y, double *part, const double *scal, int nblocks, hipStream_t s, int step, bool defer);   // patch.hip
// the PCG's q = A p with p in fp32 storage (PcgBuffersT::p32): fp64 product, shared rows left in the slab, partials of <p, A p>; throws where the patch operator does not apply
void launch_patch_spmm_x32(const CsrViewT<double> &A, int k, const float *x, double *part, const double *scal, int nblocks, hipStream_t s, int step);   // patch.hip

template <class T> void launch_pcg_init(const CsrViewT<T> &A, int k, const T *f, const PcgBuffersT<T> &b, hipStream_t s);       // + C r0, p0
template <class T> void launch_pcg_update(const CsrViewT<T> &A, int k, int step, double tol2, const PcgBuffersT<T> &b, hipStream_t s);  // + C r (Chebyshev steps)
template <class T> void launch_pcg_direction(const CsrViewT<T> &A, int k, int step, double tol2, const PcgBuffersT<T> &b, hipStream_t s, bool add_x = true);
template <class T> void launch_pcg_final(int k, int step, const PcgBuffersT<T> &b, hipStream_t s);
// one direction launch (fp64 storage, direction in fp32) on the caller's own vectors and scalars, flat or row form (remo_debug_direction_forms)
void launch_direction_form(bool flat, int grid, int64_t n, int64_t nv, int k, int step, double tol2, int nb_rz, const double *part_rz_new,
                           double *scal, const double *r, float *p, const double *dinv, double *z, hipStream_t s);
void set_vector_stamps(long long *stamps);   // probe builds: where k_pcg_direction_flat / k_pcg_update_tile leave their clocks (remo_debug_vector_heads)

// probe of a grid-wide barrier (remo_debug_grid_barrier): nblocks must not exceed what the chip holds at once; counter / fail / mismatch zeroed by the caller
void launch_barrier_probe(int nblocks, int nbar, unsigned *counter, int *fail, float *buf, int *mismatch, hipStream_t s);

// mixed precision: conversions around the fp32 inner solve
void launch_to_float(int64_t n, const double *src, float *dst, hipStream_t s);
void launch_mixed_residual(int64_t n, const double *f, const double *q /* may be null */, float *r32, hipStream_t s);
void launch_mixed_accumulate(int64_t n, double *x, float *e, int zero_e, hipStream_t s);
// one PCG step's update with residual replacement (x32 += alpha p; x64 += x32; r32 = f - A64 x64; C r)
void launch_pcg_replace(const CsrViewT<float> &A, const CsrViewT<double> &A64, int k, int step, double tol2, const PcgBuffersT<float> &b,
                        const double *f64, double *x64, double *q64, hipStream_t s);

// point location on the borehole axis + shape values; found[] must be pre-set to INT_MAX
void launch_locate(int dim, int64_t nt, const double *coords, const int32_t *conn, int npts, const double *pz,
                   int32_t *found, hipStream_t s);
void launch_point_shapes(int dim, int npts, const double *pz, const int32_t *found, const double *coords,
                         const int32_t *conn, double *phi, int32_t *errflag, hipStream_t s);
// shape values at points anywhere in the mesh: pp[npts * dim] full coordinates, found[] from field_locate (field.h)
void launch_point_shapes_at(int dim, int npts, const double *pp, const int32_t *found, const double *coords,
                            const int32_t *conn, double *phi, int32_t *errflag, hipStream_t s);
// f[n*k] += I * phi at sources (with the condensed-bubble fold in 2D); bubble loads kept in fint[npts]
void launch_build_rhs(const ElemMesh &em, int npts, const int32_t *pt_rhs, const double *pt_I, const int32_t *found, const double *phi, int k, double *f,
                      double *fint, hipStream_t s);
// x_ev != nullptr: the values of x that point q reads are x_ev[q * N + i] (PcgBuffersT::x_ev, laid out by launch_eval_slots)
void launch_eval(const ElemMesh &em, int npts, const int32_t *pt_rhs, const double *pt_I, const int32_t *found, const double *phi, int k, const double *x,
                 const double *fint, double *out, hipStream_t s, const double *x_ev = nullptr,
                 const double *fbub = nullptr);   // fbub[element][k]: bubble loads of the secondary formulation (2D condensed), nullptr: none
// at[q * N + i] = row * k + pt_rhs[q] of local dof i of point q's element (N = 20 in 3D, 10 in 2D), -1 where k_eval reads no x
void launch_eval_slots(const ElemMesh &em, int npts, const int32_t *pt_rhs, const int32_t *found, int k, int64_t *at, hipStream_t s);

}  // namespace remo
