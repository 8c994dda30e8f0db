// vertex_solver.h — the solver of the P1 (vertex) block inside the two-level preconditioner (vertex_solver.hip):
// what a batch built for it, its launches and the host steps that build it.  Which image a launch reads is decided here alone.
#pragma once
#include "amg.h"
#include "tune.h"

namespace remo {
template <class T> struct CsrViewT;   // kernels.h
using CsrView = CsrViewT<double>;

// T = storage type of matrix values and vectors (kernels.h PcgBuffersT, which holds one of these as `vs`)
template <class T> struct VertexSolverT {
    // size, degree and interval: nv = free vertex dofs = size of the leading P1 block; degree = 0 -> Jacobi alone
    int64_t nv = 0;
    int degree = 0;
    double lmax = 0.0, lmin = 0.0;
    // the chain's vectors [nv * k]: running value (the finished one is stored divided by the Jacobi factor, so that the direction
    // launch treats it like r), residual, ping-pong directions
    T *z = nullptr, *res = nullptr, *d[2] = {nullptr, nullptr};
    // the block the chain reads, always there when the preconditioner is two-level: A's own arrays (the block's entries lead every
    // row: columns ascend), or the assembled arrays when only the P1 block was assembled, or the compact copy (inside the full matrix a
    // vertex row's ~15 leading entries sit in a row of ~110: three partly used cache lines).  compact: one of the latter two
    const int32_t *rowptr = nullptr, *col = nullptr;
    const T *val = nullptr;
    bool compact = false;
    // the squared block (launch_vblock_square): A_vv and B = A_vv D^-1 A_vv on B's pattern for the paired steps;
    // sq_rowptr = nullptr -> one launch per Chebyshev step on A_vv alone
    const int32_t *sq_rowptr = nullptr, *sq_col = nullptr;
    const T *sq_a = nullptr, *sq_b = nullptr;
    int sq_lanes = 16;      // lanes per row of the paired kernel (8 / 16 / 32 by the average row length of B)
    // the fixed-width image of the block (launch_vblock_ell): [nv][kEllWidth] columns and values, [nv][2] begin / end of a row's
    // further entries in (col, val) above; values in T and / or in float (the fp32 chain's); nullptr -> rows are walked as CSR
    const int32_t *ell_col = nullptr, *ell_tail = nullptr;
    const T *ell_val = nullptr;
    const float *ell_val32 = nullptr;
    // the fp32 chain inside an fp64 solve (vertex blocks above 32 k rows: the launches are HBM streams there, and a preconditioner
    // may be inexact): float copies of the compact block's values and of the vertex rows' Jacobi factors, chain vectors
    // [nv * k]; val32 = nullptr -> the chain runs in T
    const float *val32 = nullptr, *dinv32 = nullptr;
    float *z32 = nullptr, *res32 = nullptr, *d32[2] = {nullptr, nullptr};
    // the multigrid cycle instead of the polynomial (amg.h; 2D by default); nullptr -> Chebyshev
    const AmgT<T> *amg = nullptr;
    const AmgT<float> *amg32 = nullptr;   // fp64 solves: the cycle in fp32 storage (remo_debug_tune key 17), nullptr -> in T
};

// Which form the launches take - every test of the description, once.  Two Richardson factors of the polynomial per launch, on the squared block
template <class T> inline bool vertex_paired(const VertexSolverT<T> &v) { return v.sq_rowptr && (v.degree & 1) == 0; }
// the update launch takes the FIRST step along (and gathers q) when the polynomial has launches of its own left to commit the vertex
// residual (degree >= 3) and is not applied through the squared block.  Measured in the bench, fold on vs off on one box: -2.3 % solve
// time at 12.8 k vertices, -0.9 % at 27 k, +0.4 % at 83 k (there the step is real work, not launch latency): small vertex blocks only
template <class T> inline bool vertex_first_folds(const VertexSolverT<T> &v) { return g_tune.fold_first && !v.amg && v.degree >= 3 && v.nv > 0 && v.nv <= 32768 && !vertex_paired(v); }
// the chain in fp32 inside an fp64 solve: needs the compact block (its float copy), never together with the folded first step
template <class T> inline bool vertex_chain32(const VertexSolverT<T> &v, bool first_done) { return sizeof(T) == 8 && v.val32 && v.compact && !first_done; }
// the fixed-width image, in the storage type of the chain, if the host made one
template <class T> inline bool vertex_ell(const VertexSolverT<T> &v, bool chain32) { return v.ell_col && v.ell_tail && (chain32 ? v.ell_val32 != nullptr : v.ell_val != nullptr); }

// Two-level preconditioner ("multigrid" of the reference, ngsolve_functions.py:46: a lowest-order coarse space plus a smoother on the
// high-order dofs).  In the hierarchical basis the vertex functions ARE the P1 space and vertex dofs are numbered first, so the coarse
// problem is the leading nv x nv block of the assembled matrix, read in place (columns are sorted: the block's entries lead every
// row).  C = blockdiag( q_d(A_vv), D_hh^-1 ): a fixed Chebyshev polynomial of degree d in the Jacobi-scaled vertex block (spectrum
// bounds [lmax/ratio, lmax], lmax = Gershgorin bound, so q_d is positive definite on the whole spectrum and plain PCG stays valid)
// and Jacobi on edge/face dofs.  nv = 0 gives plain Jacobi ("local").
template <class T> struct ChebArgsT {
    int64_t nv;       // free vertex dofs (0: Jacobi)
    double inv_theta; // 1 / theta, theta = (lmax + lmin) / 2
    T *z, *res;       // [nv][K] polynomial value so far / residual of the vertex block system
    T *d0;            // [nv][K] first Chebyshev direction
};
template <class T> inline ChebArgsT<T> cheb_args(const VertexSolverT<T> &v) {
    if (v.degree <= 0) return {0, 0.0, v.z, v.res, v.d[0]};
    return {v.nv, 1.0 / (0.5 * (v.lmax + v.lmin)), v.z, v.res, v.d[0]};
}
struct ChebStep { double c1, c2, rho; };   // d' = c1 d + c2 D^-1 res of one step of the three-term recurrence, and the rho it hands to the next
// the first step (prev = nullptr: the chain's j = 0 and the step folded into the update launch) or the one after *prev
template <class T> inline ChebStep cheb_step(const VertexSolverT<T> &v, const ChebStep *prev = nullptr) {
    const double theta = 0.5 * (v.lmax + v.lmin), delta = 0.5 * (v.lmax - v.lmin);
    const double sig = theta / delta, rho = prev ? prev->rho : 1.0 / sig;
    const double rho_new = 1.0 / (2.0 * sig - rho);
    return {rho_new * rho, 2.0 * rho_new / delta, rho_new};
}

// workgroups of the launch that leaves the <r_v, z_v> partial sums (polynomial and cycle alike)
int cheb_grid(int64_t nv);
// C r for the vertex block: the cycle, or `degree` Chebyshev steps; the last launch leaves the <r_v, z_v> partials behind the nb_vec
// of the high-order part in part_slot.  r, dinv, rz0: the PCG's residual, Jacobi factors and scalars.  first_done: vertex_first_folds
template <class T> void launch_vertex_solve(const VertexSolverT<T> &v, int k, int step, T *r, const T *dinv, double *rz0, int nb_vec, double *part_slot,
                                            hipStream_t s, bool first_done = false);

void launch_vblock_bound(int64_t nv, const CsrView &A, const double *dinv, unsigned long long *out_bits, hipStream_t s);
// B = A_vv D^-1 A_vv (and A_vv itself) on the pattern of B, rows sorted; cnt / rowptr [nv + 1], col / a / b [capacity];
// *flag (device int, pre-zeroed) is raised when a row has more than kSquareSlots distinct columns or the capacity
// is too small: the caller then keeps the one-step path
constexpr int kSquareSlots = 512;
void launch_vblock_square(int64_t nv, const CsrView &A, const double *dinv, int32_t *sq_rowptr, int32_t *sq_col, double *sq_a, double *sq_b,
                          int64_t capacity, int32_t *flag, hipStream_t s);
// compact CSR copy of the leading nv x nv block of A (columns ascend, so the block's entries lead every row); *flag is raised
// when it does not fit `capacity` entries; vb_rowptr[nv] = entries
void launch_vblock_compact(int64_t nv, const CsrView &A, int32_t *vb_rowptr, int32_t *vb_col, double *vb_val, int64_t capacity, int32_t *flag,
                           hipStream_t s);
constexpr int kEllWidth = 24;   // entries per row of the fixed-width image: three per lane at eight lanes per row (3D P1 rows hold ~15)
// eval64 / eval32: either may be nullptr
void launch_vblock_ell(int64_t nv, const int32_t *rowptr, const int32_t *col, const double *val, int32_t *ecol, int32_t *tail, double *eval64,
                       float *eval32, hipStream_t s);

// The builder: the host steps of one batch, in the batch's order, on its arena (the ORDER of the takes fixes the
// addresses) and stream.  The read-backs of `enqueue` land in this struct: it must stay where it is until the batch has synchronised.
struct VertexSolverInput { int dim, kmax; const remo_opts_t &o; int64_t nvfree; bool lite, want_amg; };   // what it reads of the batch (lite: only the P1 block was assembled)
struct VertexSolverBuilder {
    bool two_level = false;                  // vertex-block solver + Jacobi (remo_opts_t.preconditioner), else Jacobi alone
    size_t nc = 0;                           // length of the chain's vectors
    double ratio_default = 0.0;              // lmax / lmin of this batch where the options name none
    unsigned long long *d_bound = nullptr, h_bound = 0;   // spectrum bound of the block: device slot, bits read back
    bool want_square = false, want_compact = false, amg32_ready = false;
    int32_t h_sq[2] = {1, 0}, h_vb[2] = {1, 0};           // squared / compact block: overflow flag, entries
    VertexSolverBuilder() = default; VertexSolverBuilder(const VertexSolverBuilder &) = delete;
    // upper bound of everything the steps below take (nv: all vertices; mixed: to_float will run), each term named by its step
    static size_t arena_bytes(int dim, int64_t nv, size_t kmax, bool want_amg, bool mixed);
    void take(Arena &ar, const VertexSolverInput &in, VertexSolverT<double> &vs);
    // before the batch's synchronisation: spectrum bound, squared block, compact copy (into vs), with their read-backs
    void enqueue(Arena &ar, hipStream_t s, const VertexSolverInput &in, const CsrView &A, const double *dinv, VertexSolverT<double> &vs);
    // after it: which images the solve uses and the ones built from those.  Returns REMO_OK, or an error code with its text in `why`
    int accept(Arena &ar, hipStream_t s, const VertexSolverInput &in, const CsrView &A, const double *dinv, AmgT<double> &amg64, AmgT<float> &amg32,
               VertexSolverT<double> &vs, int *coarse_used, std::string &why);
    // the mixed mode's fp32 inner solver: vectors taken, value arrays converted, the rest shared.  val32: the whole matrix' values
    VertexSolverT<float> to_float(Arena &ar, hipStream_t s, const VertexSolverT<double> &vs, const float *val32, const AmgT<float> &amg32) const;
};

}  // namespace remo
