// amg.h — smoothed-aggregation multigrid cycle on the P1 (vertex) block (amg.hip): the coarse solver of the two-level
// preconditioner where the Chebyshev polynomial needs a high degree (2D: graded axisymmetric meshes).  Replaces the
// "multigrid" choice of ngsolve_functions.py:46 on the vertex block; the edge / face dofs keep their Jacobi factors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "symbolic_gpu.h"

namespace remo {

constexpr int kAmgMaxLevels = 8;
constexpr int kAmgDenseMax = 64;   // the coarsest operator is inverted densely in LDS

// One level: operator A (CSR, columns ascending), its Jacobi factors, the prolongator P to the next level (n x n_next)
// and its transpose R, level vectors [n][k].  T = storage type of values and vectors.
template <class T> struct AmgLevelT {
    int64_t n = 0, nnz = 0, nnz_p = 0;   // rows and entries of A, entries of P (= of R)
    int r_lanes = 8;                     // lanes per row of R in the restriction (8 / 16 / 32 / 64, by R's row lengths: amg_build)
    const int32_t *rowptr = nullptr, *col = nullptr;
    const T *val = nullptr, *dinv = nullptr;
    const int32_t *p_rowptr = nullptr, *p_col = nullptr;
    const T *p_val = nullptr;
    const int32_t *r_rowptr = nullptr, *r_col = nullptr;
    const T *r_val = nullptr;
    double omega = 0.0;            // damped Jacobi smoother z += omega D^-1 (r - A z)
    // level 0 only (amg_level0_image): the fixed-width image of A for the last sweep of the cycle - [n][kEllWidth] columns and values,
    // [n][2] begin / end of a row's further entries in (col, val); nullptr -> that sweep walks the CSR rows like the others
    const int32_t *ell_col = nullptr, *ell_tail = nullptr;
    const T *ell_val = nullptr;
    T *r = nullptr, *z = nullptr, *z2 = nullptr, *t = nullptr;
};

template <class T> struct AmgT {
    int levels = 0;
    AmgLevelT<T> lev[kAmgMaxLevels];
    const T *inv = nullptr;        // dense inverse of the coarsest operator [nc][nc]
    int launches = 0;              // kernel launches of one cycle
    int kmax = 0;                  // columns the level vectors were allocated for
};

// Build the hierarchy (fp64) of the leading nv x nv block of A (rows' vertex entries lead: columns ascend).  Everything is
// enqueued on s; the function synchronises a few times per level to read sizes back.  Returns false (with the reason) when
// the hierarchy cannot be built (a row too long for the LDS tables, no coarsening, arena exhausted): the caller keeps the
// Chebyshev polynomial.
bool amg_setup(Arena &ar, hipStream_t s, int dim, int64_t nv, const int32_t *rowptr, const int32_t *col, const double *val, int kmax,
               AmgT<double> &out, std::string &why);
// fp32 image of a hierarchy (values converted, patterns shared, own vectors) for the inner solver of the mixed mode
void amg_to_float(Arena &ar, hipStream_t s, const AmgT<double> &in, int kmax, AmgT<float> &out);

// fixed-width image of level 0's operator (launch_vblock_ell, the kernel the polynomial's image comes from) for the last sweep of the
// cycle (k_amg_post_image): into h64 (values in fp64) when want64, into h32 (which shares the pattern; values in fp32) when h32 is given
void amg_level0_image(Arena &ar, hipStream_t s, AmgT<double> &h64, bool want64, AmgT<float> *h32);

// ONE row operation of the cycle on the caller's host arrays (remo_debug_row_ops), in device memory of its own that starts out as 0xFF
// bytes.  op 0: y = M x with `lanes` lanes per row (restriction form); 1: first half sweep (z, t); 2: second half sweep; 3: the finest
// level's second half sweep, which also leaves the <r, z> partials of `nblocks` workgroups.  ell: op 3 reads the fixed-width image.
// fp32: values, factors and level vectors in float (r and the finished z of ops 1 and 3 stay double).  out / out2: the raw bytes of
// the result arrays with `guard` elements behind them (remo3d_hip_debug.h).  Throws on arguments the kernels could not be trusted with.
void amg_debug_row_ops(hipStream_t s, int op, int lanes, bool ell, bool fp32, int64_t n, int64_t nx, int k, const int32_t *rowptr, const int32_t *col,
                       const double *val, const double *dinv, double omega, const double *x, const double *r, int nblocks, int guard, void *out, void *out2);

// ONE sparse product C = X Y of the setup on the caller's host arrays (remo_debug_product): count pass, scan, clamp to `cap` entries, fill
// pass with 128 or 512 hash slots per row, in device memory of its own that starts out as 0xFF bytes.  crp [nx + 1], cc / cv [cap + 2].
// Throws on arguments the kernels could not be trusted with.
void amg_debug_product(hipStream_t s, int slots, int64_t cap, int64_t nx, const int32_t *xrp, const int32_t *xc, const double *xv, int64_t ny,
                       const int32_t *yrp, const int32_t *yc, const double *yv, int32_t *crp, int32_t *cc, double *cv, int32_t *flags);

// z = V(1,1)-cycle(r) on the vertex rows; the last launch stores cz = z / dinv (the direction kernel treats it like r) and the
// <r, z> partial sums of `nblocks` workgroups [nblocks][k] in part.  scal / step: early exit of finished solves (kutil.h solve_done)
// T = storage type of the hierarchy, TR = type of r and cz: <float, double> is the cycle in fp32 inside an fp64 solve (a
// preconditioner may be applied inexactly; the recurrences of x and r never see it)
template <class T, class TR> void launch_amg_cycle(const AmgT<T> &H, int k, int step, const TR *r, TR *cz, double *part, int nblocks, const double *scal,
                                                   hipStream_t s);

}  // namespace remo
