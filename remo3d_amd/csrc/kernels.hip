// kernels.hip — hand-written gfx950 (CDNA4, wave64) kernels of the ReMo3D hot path around the PCG step:
//   metric terms -> CSR value gather-assembly -> the CSR product q = A p (edge-pair SpMM) -> conversions of the
//   mixed-precision mode -> axis point location / RHS build / evaluation.
// The vector kernels of the PCG step are pcg_kernels.hip, the solver of the preconditioner's P1 vertex block with the set-up of its
// images vertex_solver.hip, the patch operator patch.hip.
// All of it is HBM/L2-bound sparse work: no MFMA (a sparse row is not a dense contraction); the levers are
// coalesced CSR streams, DPP (not LDS) cross-lane reductions, XCD-aware row placement and LDS-staged reference
// tensors.  Reference lines each kernel replaces are cited at the kernel.  Element reads shared with the element passes of the
// other files (sens, pairs, errest, field, secondary) are elem_access.h's; the launchers that need the mesh take its ElemMesh view.
#include "kernels.h"

#include <limits.h>

#include "elem_access.h"
#include "fem_p3.h"
#include "wave_util.h"
#include "kutil.h"

namespace remo {

// Storage position of stored entry e of `row` (rows of an edge pair keep their values INTERLEAVED: the two rows have the
// same column pattern and the SpMM reads both values of an entry with one 16-byte load; every other row is plain CSR).
// rs = rowptr[row], len = row length.
__device__ __forceinline__ int64_t value_pos(int64_t row, int32_t rs, int32_t len, int32_t e, int64_t pair_begin, int64_t pair_end) {
    if (row < pair_begin || row >= pair_end) return int64_t(rs) + e;
    const bool second = ((row - pair_begin) & 1) != 0;
    return int64_t(second ? rs - len : rs) + 2 * int64_t(e) + (second ? 1 : 0);
}

// ------------------------------------------------------------------------------------------
// metric terms: one thread per element (ngsolve_functions.py:33-36: the coefficient part of the
// integrand; sigma per material as worker.py:101)

template <int DIM>
__global__ void __launch_bounds__(256) k_metric_terms(int64_t nt, const double *__restrict__ coords,
                                                      const int32_t *__restrict__ conn, const int32_t *__restrict__ mat,
                                                      const int32_t *__restrict__ eperm, const double *__restrict__ sigma, int nmat,
                                                      double *__restrict__ C, int32_t *errflag) {
    constexpr int NB = DIM + 1, NT = P3<DIM>::NTERM;
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double X[NB * DIM];
    load_vertices<DIM>(coords, conn, t, X);
    const int m = mat[caller_element(eperm, t)];   // the raw index: this is the kernel that reports a bad one (the others read elem_material)
    double c[NT];
    bool ok = (m >= 0 && m < nmat);
    if (ok) ok = metric_terms<DIM>(X, sigma[m], c);
    if (!ok) {
        atomicOr(errflag, 1);
#pragma unroll
        for (int i = 0; i < NT; ++i) c[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) C[t * NT + i] = c[i];
}

void launch_metric_terms(const ElemMesh &em, int32_t *errflag, hipStream_t s) {
    const int grid = int((em.nt + 255) / 256);
    double *C = const_cast<double *>(em.C);   // the one launch that writes what every other element pass reads through the view
    if (em.dim == 2)
        hipLaunchKernelGGL(k_metric_terms<2>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.n_mat, C, errflag);
    else
        hipLaunchKernelGGL(k_metric_terms<3>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.n_mat, C, errflag);
}

// the same for anisotropic materials: sigma_tensor[nmat][SigmaTensor<DIM>::N] (upper triangles, remo_solve_batch_tensor)
template <int DIM>
__global__ void __launch_bounds__(256) k_metric_terms_tensor(int64_t nt, const double *__restrict__ coords,
                                                             const int32_t *__restrict__ conn, const int32_t *__restrict__ mat,
                                                             const int32_t *__restrict__ eperm, const double *__restrict__ sigma_tensor,
                                                             int nmat, double *__restrict__ C, int32_t *errflag) {
    constexpr int NB = DIM + 1, NT = P3<DIM>::NTERM, NS = SigmaTensor<DIM>::N;
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double X[NB * DIM];
    load_vertices<DIM>(coords, conn, t, X);
    const int m = mat[caller_element(eperm, t)];
    double c[NT];
    bool ok = (m >= 0 && m < nmat);
    if (ok) {
        double S[NS];   // (read in place, not through load_sigma: with it the 3D kernel is allocated 72 registers for 76 and is another kernel)
#pragma unroll
        for (int i = 0; i < NS; ++i) S[i] = sigma_tensor[int64_t(m) * NS + i];
        ok = metric_terms_tensor<DIM>(X, S, c);
    }
    if (!ok) {
        atomicOr(errflag, 1);
#pragma unroll
        for (int i = 0; i < NT; ++i) c[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) C[t * NT + i] = c[i];
}

void launch_metric_terms_tensor(const ElemMesh &em, int32_t *errflag, hipStream_t s) {
    const int grid = int((em.nt + 255) / 256);
    double *C = const_cast<double *>(em.C);
    if (em.dim == 2)
        hipLaunchKernelGGL(k_metric_terms_tensor<2>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.n_mat, C, errflag);
    else
        hipLaunchKernelGGL(k_metric_terms_tensor<3>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.n_mat, C, errflag);
}

// ------------------------------------------------------------------------------------------
// CSR value assembly, gather formulation (a.Assemble(), ngsolve_functions.py:47).
// One wave owns one row; lane p owns stored entry p of the row and walks the row's incident
// elements in ascending order, adding K_e[li][lj] where the element's local dof lj is its
// column.  No atomics, every value written exactly once (coalesced), bit-reproducible.
// Reference tensors are staged in LDS (19.2 KB in 3D, 7.2 KB in 2D).

constexpr int kAsmRow = 448;   // stored entries of a row handled through LDS in k_assemble (longer rows: lane-per-entry walk)
template <int DIM, bool CONDENSE>
__global__ void __launch_bounds__(256) k_assemble(int64_t nfree, int64_t pair_begin, int64_t pair_end, const int32_t *__restrict__ rowptr,
                                                  const int32_t *__restrict__ col, const int32_t *__restrict__ adjptr,
                                                  const uint32_t *__restrict__ adj, const int32_t *__restrict__ eldof,
                                                  const double *__restrict__ C, const double *__restrict__ Mg,
                                                  double *__restrict__ val, double *__restrict__ dinv) {
    constexpr int N = P3<DIM>::NLD, NT = P3<DIM>::NTERM;
    constexpr int NK = CONDENSE ? 9 : N;  // local dofs that are unknowns
    __shared__ double M[NT * N * N];
    for (int i = threadIdx.x; i < NT * N * N; i += blockDim.x) M[i] = Mg[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // Rows of up to kAsmRow stored entries (all but pathological vertex rows): the row's columns and two accumulators
    // per stored entry live in LDS.  For every incident element, lane q < NK takes the element's local dof q: it finds
    // the position of that column in the row by binary search in LDS (the 20-compare search per stored entry AND element
    // of the first version was the cost of the kernel: 508 us per batch at 63 k tetrahedra, 5 % of the HBM roofline),
    // forms K_e[li][q] and adds it at that position.  The positions of one element are distinct and the elements are
    // walked in ascending order by the whole wave, so every stored entry still sums its contributions in the same
    // fixed order: bit-identical to the lane-per-entry walk, which remains for longer rows.
    __shared__ int32_t colL[4][kAsmRow];
    __shared__ double accL[4][kAsmRow];      // single rows: entry p at [p]; edge-row pairs: entry p of the two rows at [2p], [2p + 1]
    // workgroups are persistent over rows: the reference tensors are staged in LDS once per workgroup, not once per 4 rows
    for (int64_t row = int64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); row < nfree; row += int64_t(gridDim.x) * (blockDim.x >> 6)) {
    // the two dofs of an edge (rows r, r + 1 of the pair range) meet the same elements with local numbers li, li + 1 and
    // have the same columns: the wave of the first row computes both (one column search), the wave of the second rests
    const bool in_pairs = row >= pair_begin && row < pair_end;
    if (in_pairs && ((row - pair_begin) & 1)) continue;
    const int32_t rs = rowptr[row], re = rowptr[row + 1];
    const int32_t as = adjptr[row], ae = adjptr[row + 1];
    if (re - rs <= (in_pairs ? kAsmRow / 2 : kAsmRow)) {
        const int32_t len = re - rs;
        int32_t *cl = colL[wave];
        double *aa = accL[wave];
        const int sh = in_pairs ? 1 : 0;
        for (int32_t p = lane; p < len; p += 64) cl[p] = col[rs + p];
        for (int32_t p = lane; p < (len << sh); p += 64) aa[p] = 0.0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // NG incident elements per trip, one group of NK lanes each: the dependent chain of a trip (element's dofs -> position
        // in the row by binary search -> element matrix entries) is latency, so the groups run it side by side; only the adds
        // into the accumulators are taken group by group, in element order (two elements of a trip can hit the same entry).
        constexpr int NG = 64 / NK;
        const int grp = lane / NK, q = lane - grp * NK;
        for (int32_t a = as; a < ae; a += NG) {
            const bool have = grp < NG && a + grp < ae;
            int32_t pos = -1;
            double k = 0.0, k2 = 0.0;
            if (have) {
                const uint32_t code = adj[a + grp];
                const int64_t t = code >> 5;
                const int li = int(code & 31u);
                const int32_t j = eldof[t * N + q];
                if (j >= 0) {
                    int32_t lo = 0, hi = len;
                    while (lo < hi) {                  // columns ascend; j is one of them
                        const int32_t mid = (lo + hi) >> 1;
                        if (cl[mid] < j) lo = mid + 1; else hi = mid;
                    }
                    // (vertex-block-only assembly: the row holds vertex columns only, every other local dof of the element ends
                    // behind the row's last column or between two of them - a hit counts only if the column is really there;
                    // a row of exactly kAsmRow entries would otherwise add into the next wave's accumulators)
                    pos = (lo < len && cl[lo] == j) ? lo : -1;
                    const double *c = C + t * NT;
                    k = kentry<DIM>(c, M, li, q);
                    if (in_pairs) k2 = kentry<DIM>(c, M, li + 1, q);
                    if (CONDENSE) {  // Schur complement of the cell bubble (condense=True, ngsolve_functions.py:31)
                        const double kbj = kentry<DIM>(c, M, 9, q), kbb = kentry<DIM>(c, M, 9, 9);
                        k -= kentry<DIM>(c, M, li, 9) * kbj / kbb;
                        if (in_pairs) k2 -= kentry<DIM>(c, M, li + 1, 9) * kbj / kbb;
                    }
                }
            }
#pragma unroll
            for (int gg = 0; gg < NG; ++gg) {
                if (grp == gg && pos >= 0) {
                    aa[pos << sh] += k;
                    if (in_pairs) aa[2 * pos + 1] += k2;
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        for (int32_t p = lane; p < len; p += 64) {
            const int32_t j = cl[p];
            const double acc = aa[p << sh], acc2 = in_pairs ? aa[2 * p + 1] : 0.0;
            if (in_pairs) {   // interleaved values of the pair (value_pos)
                val[int64_t(rs) + 2 * p] = acc;
                val[int64_t(rs) + 2 * p + 1] = acc2;
                if (j == row) dinv[row] = 1.0 / acc;
                if (j == row + 1) dinv[row + 1] = 1.0 / acc2;
            } else {
                val[rs + p] = acc;
                if (j == row) dinv[row] = 1.0 / acc;  // Jacobi = Preconditioner(a, "local"), ngsolve_functions.py:46
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        continue;
    }
    for (int32_t base = rs; base < re; base += 64) {
        const int32_t p = base + lane;
        const int32_t j = (p < re) ? col[p] : -2;
        double acc = 0.0, acc2 = 0.0;
        for (int32_t a = as; a < ae; ++a) {
            const uint32_t code = adj[a];  // wave-uniform
            const int64_t t = code >> 5;
            const int li = int(code & 31u);
            const int32_t *ed = eldof + t * N;
            const double *c = C + t * NT;
            int lj = -1;
#pragma unroll
            for (int q = 0; q < NK; ++q)
                if (ed[q] == j) lj = q;
            if (lj >= 0) {
                double k = kentry<DIM>(c, M, li, lj);
                double k2 = in_pairs ? kentry<DIM>(c, M, li + 1, lj) : 0.0;
                if (CONDENSE) {  // Schur complement of the cell bubble (condense=True, ngsolve_functions.py:31)
                    const double kbj = kentry<DIM>(c, M, 9, lj), kbb = kentry<DIM>(c, M, 9, 9);
                    k -= kentry<DIM>(c, M, li, 9) * kbj / kbb;
                    if (in_pairs) k2 -= kentry<DIM>(c, M, li + 1, 9) * kbj / kbb;
                }
                acc += k;
                acc2 += k2;
            }
        }
        if (p < re) {
            if (in_pairs) {   // interleaved values of the pair (value_pos): entry e of rows r, r + 1 at rs + 2e, rs + 2e + 1
                val[int64_t(rs) + 2 * (p - rs)] = acc;
                val[int64_t(rs) + 2 * (p - rs) + 1] = acc2;
                if (j == row) dinv[row] = 1.0 / acc;
                if (j == row + 1) dinv[row + 1] = 1.0 / acc2;
            } else {
                val[p] = acc;
                if (j == row) dinv[row] = 1.0 / acc;  // Jacobi = Preconditioner(a, "local"), ngsolve_functions.py:46
            }
        }
    }
    }
}

// Jacobi factors of rows [row0, nfree) WITHOUT the assembled matrix (the patch operator's batches assemble only the P1 block):
// diagonal entry = sum over the row's incident elements of K_e[li][li].  One thread per row, same element order as the assembly.
template <int DIM>
__global__ void __launch_bounds__(256) k_diag_rows(int64_t row0, int64_t nfree, const int32_t *__restrict__ adjptr, const uint32_t *__restrict__ adj,
                                                   const double *__restrict__ C, const double *__restrict__ Mg, double *__restrict__ dinv) {
    constexpr int N = P3<DIM>::NLD, NT = P3<DIM>::NTERM;
    __shared__ double Md[NT * N];
    for (int i = threadIdx.x; i < NT * N; i += blockDim.x) Md[i] = Mg[((i / N) * N + (i % N)) * N + (i % N)];
    __syncthreads();
    const int64_t row = row0 + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= nfree) return;
    double s = 0.0;
    for (int32_t a = adjptr[row]; a < adjptr[row + 1]; ++a) {
        const uint32_t code = adj[a];
        const double *c = C + int64_t(code >> 5) * NT;
        const int li = int(code & 31u);
        double e = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) e += c[t] * Md[t * N + li];
        s += e;
    }
    dinv[row] = 1.0 / s;
}
void launch_diag_rows(int dim, int64_t row0, int64_t nfree, const int32_t *adjptr, const uint32_t *adj, const double *C, const double *M, double *dinv, hipStream_t s) {
    if (nfree <= row0) return;
    const int grid = int((nfree - row0 + 255) / 256);
    if (dim == 3) hipLaunchKernelGGL(k_diag_rows<3>, dim3(grid), dim3(256), 0, s, row0, nfree, adjptr, adj, C, M, dinv);
    else hipLaunchKernelGGL(k_diag_rows<2>, dim3(grid), dim3(256), 0, s, row0, nfree, adjptr, adj, C, M, dinv);
}

void launch_assemble(int dim, bool condense, int64_t nfree, int64_t pair_begin, int64_t pair_end, const int32_t *rowptr, const int32_t *col,
                     const int32_t *adjptr, const uint32_t *adj, const int32_t *eldof, const double *C,
                     const double *M, double *val, double *dinv, hipStream_t s) {
    int64_t g64 = (nfree + 3) / 4;
    if (g64 > 4096) g64 = 4096;
    const int grid = int(g64 < 1 ? 1 : g64);
    if (dim == 3)
        hipLaunchKernelGGL((k_assemble<3, false>), dim3(grid), dim3(256), 0, s, nfree, pair_begin, pair_end, rowptr, col, adjptr, adj, eldof, C, M, val, dinv);
    else if (condense)
        hipLaunchKernelGGL((k_assemble<2, true>), dim3(grid), dim3(256), 0, s, nfree, pair_begin, pair_end, rowptr, col, adjptr, adj, eldof, C, M, val, dinv);
    else
        hipLaunchKernelGGL((k_assemble<2, false>), dim3(grid), dim3(256), 0, s, nfree, pair_begin, pair_end, rowptr, col, adjptr, adj, eldof, C, M, val, dinv);
}

// ------------------------------------------------------------------------------------------
// CSR SpMM  y = A x  for K interleaved right-hand sides (x[n][K] row-major), the kernel the
// CG hot loop spends its time in (CGSolver, ngsolve_functions.py:50-51; cusparseSpMV in the
// reference's CUDA attempt, ngsolve_functions_gpu.py:41-47).
// LPR lanes cooperate on a row: values/columns are read as contiguous runs (rows are contiguous
// in CSR, so a wave streams one contiguous span), x rows are gathered K doubles at a time, the
// LPR partial sums are combined with wave shuffles.  Optionally leaves per-block partial sums of
// <x, y> (the CG's <p, Ap>) so the dot product costs no extra pass.

// Variant A ("lane per stored entry"): the fallback for matrices without edge-row pairs and the
// baseline of tools/probe_spmm.py.  T = double (the product path) or float (inner solver of the
// mixed-precision mode); dot-product partials are always accumulated in double.
template <class T, int K, int LPR, bool DOT>
__global__ void __launch_bounds__(512) k_spmm(int64_t n, int64_t pair_begin, int64_t pair_end, const int32_t *__restrict__ rowptr,
                                              const int32_t *__restrict__ col, const T *__restrict__ val,
                                              const T *__restrict__ x, T *__restrict__ y, double *__restrict__ part, const double *__restrict__ scal, int step) {
    if (scal && solve_done(scal, step)) return;
    const int rpb = blockDim.x / LPR;
    const int sub = threadIdx.x % LPR;
    const int grp = threadIdx.x / LPR;
    double dot[K];
#pragma unroll
    for (int c = 0; c < K; ++c) dot[c] = 0.0;
    for (int64_t row = int64_t(blockIdx.x) * rpb + grp; row < n; row += int64_t(gridDim.x) * rpb) {
        const int32_t rs = rowptr[row], re = rowptr[row + 1];
        T acc[K];
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = T(0);
        for (int32_t p = rs + sub; p < re; p += LPR) {
            const T v = val[value_pos(row, rs, re - rs, p - rs, pair_begin, pair_end)];
            const T *xr = x + int64_t(col[p]) * K;
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] += v * xr[c];
        }
#pragma unroll
        for (int c = 0; c < K; ++c) acc[c] = group_sum<LPR>(acc[c]);
        if (sub == 0) {
#pragma unroll
            for (int c = 0; c < K; ++c) y[row * K + c] = acc[c];
            if (DOT) {
                const T *xr = x + row * K;
#pragma unroll
                for (int c = 0; c < K; ++c) dot[c] += double(acc[c]) * double(xr[c]);
            }
        }
    }
    if (DOT) {
        __shared__ double smem[16 * K];
        block_sum<K>(dot, smem);
        if (threadIdx.x < K) part[blockIdx.x * K + threadIdx.x] = pick<K>(dot, threadIdx.x);
    }
}

// Variant C ("edge row pairs", the default): the two dofs of an edge are consecutive rows with the
// SAME column pattern, and edge rows hold ~3/4 of the stored entries.  A lane group takes both
// rows at once: one column index and ONE gather of the x row serve two stored entries.  Vertex and
// face rows are walked singly.
// The kernel is latency-bound, not bandwidth-bound (a stored entry costs two dependent memory
// round trips: column index, then the x row), so each lane issues the index/value loads of U
// passes of its row up front and then all U gathers, before any arithmetic: a row of <= U * LPR
// entries pays the two latencies once instead of once per pass.  Lanes past the row end read a
// safe address with a zero value (no branches between the loads).
template <class T, int K, int LPR, bool DOT, int MODE = 0>   // MODE != 0: ablations for tools/probe_ablate.py (wrong results on purpose)
__global__ void __launch_bounds__(512) k_spmm_pair(int64_t n, int64_t pair_begin, int64_t pair_end, int xcd_windows, const int32_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ col, const T *__restrict__ val,
                                                   const T *__restrict__ x, T *__restrict__ y, double *__restrict__ part, const double *__restrict__ scal, int step) {
    if (scal && solve_done(scal, step)) return;
    constexpr int U = 2;
    constexpr int MFP = treduce_out(2 * K, LPR), MFS = treduce_out(K, LPR);   // sums per lane after the reduction
    const int rpb = blockDim.x / LPR;
    const int sub = threadIdx.x % LPR;
    const int grp = threadIdx.x / LPR;
    const int64_t npair = (pair_end - pair_begin) >> 1;
    const int64_t ngroups = n - npair;
    // which of the 2K (pair) / K (single row) sums this lane ends up with: entry t of a pair is y[row*K + t]
    int idx_p[2 * K], idx_s[K], own_p[2 * K], own_s[K];
    towner_init<2 * K, LPR>(idx_p, own_p, sub);
    towner_init<K, LPR>(idx_s, own_s, sub);
    double dot_p[MFP], dot_s[MFS];
#pragma unroll
    for (int f = 0; f < MFP; ++f) dot_p[f] = 0.0;
#pragma unroll
    for (int f = 0; f < MFS; ++f) dot_s[f] = 0.0;
    // row of lane-group index g (edge rows are taken two at a time)
    auto row_of = [&](int64_t g, bool &pair) -> int64_t {
        pair = false;
        if (g < pair_begin) return g;
        if (g < pair_begin + npair) { pair = true; return pair_begin + 2 * (g - pair_begin); }
        return g + npair;
    };
    // Row schedule.  Workgroups b, b + 8, ... share an XCD (and its L2).
    //  xcd_windows 1: every sweep step of the chip is cut into 8 windows of neighbouring row groups, one per XCD
    //    (an XCD gathers from one window of x per step, but over the launch it walks through all of x, three
    //    times: vertex rows, edge rows, face rows);
    //  xcd_windows >= 16: REGIONS.  The dofs of each class are in Morton order of the mesh, so the same fraction
    //    of the vertex, edge and face rows covers the same part of space.  XCD j takes chunk j*nc .. j*nc + nc - 1
    //    (nc = xcd_windows / 16) of all three classes, one chunk after the other, vertex, edge and face rows
    //    of a chunk back to back: its L2 serves the three passes over a chunk's part of x from one fetch.
    const int per = int(gridDim.x >> 3), slot = int(blockIdx.x >> 3), xcd = int(blockIdx.x & 7);
    const int nchunk = xcd_windows >> 4;
    const int64_t nface = n - pair_end;
    // class sizes of one chunk, whole waves (4 lane groups of 16): waves stay uniform in the row class
    const int64_t tc = int64_t(8) * (nchunk > 0 ? nchunk : 1);
    const int64_t gran = 64 / LPR > 0 ? 64 / LPR : 1;
    const int64_t sv = ((pair_begin + tc - 1) / tc + gran - 1) / gran * gran;
    const int64_t se = ((npair + tc - 1) / tc + gran - 1) / gran * gran;
    const int64_t sf = ((nface + tc - 1) / tc + gran - 1) / gran * gran;
    const uint32_t S = uint32_t(sv + se + sf);
    int64_t g, gstep, glimit;
    if (nchunk > 0) {
        g = int64_t(slot) * rpb + grp; gstep = int64_t(per) * rpb; glimit = int64_t(nchunk) * S;
    } else {
        int vblock = int(blockIdx.x);
        if (xcd_windows) {
            const int inner = (xcd_windows == 2 && (per & 31) == 0) ? (slot & 31) * (per >> 5) + (slot >> 5) : slot;   // 2: also CU-adjacent (probe)
            vblock = xcd * per + inner;
        }
        g = int64_t(vblock) * rpb + grp; gstep = int64_t(gridDim.x) * rpb; glimit = ngroups;
    }
    // schedule position -> (row, pair); false: an empty slot of the last chunks
    auto locate = [&](int64_t pos, int64_t &row, bool &pair) -> bool {
        if (nchunk == 0) { row = row_of(pos, pair); return true; }
        const uint32_t c = uint32_t(pos) / S, o = uint32_t(pos) - c * S;
        const int64_t gc = int64_t(xcd) * nchunk + c;
        pair = false;
        if (o < uint32_t(sv)) { row = gc * sv + o; return row < pair_begin; }
        if (o < uint32_t(sv + se)) { const int64_t e = gc * se + (o - uint32_t(sv)); pair = true; row = pair_begin + 2 * e; return e < npair; }
        const int64_t f = gc * sf + (o - uint32_t(sv + se));
        row = pair_end + f;
        return f < nface;
    };
    bool pair_n = false, valid_n = false;
    int64_t row_n = 0;
    int32_t rs_n = 0, re_n = 0;
    if (g < glimit) {
        valid_n = locate(g, row_n, pair_n);
        if (valid_n) { rs_n = rowptr[row_n]; re_n = rowptr[row_n + 1]; }
    }
    for (; g < glimit; g += gstep) {
        const int64_t row = row_n;
        const bool pair = pair_n, valid = valid_n;
        const int32_t rs = rs_n, re = re_n;
        // the row pointers of the NEXT row are requested now: one of the three dependent round trips
        // of a row (pointers -> indices -> x) leaves the critical path
        if (g + gstep < glimit) {
            valid_n = locate(g + gstep, row_n, pair_n);
            if (valid_n) { rs_n = rowptr[row_n]; re_n = rowptr[row_n + 1]; }
        }
        if (!valid) continue;
        T acc[2 * K];                             // [0, K): row, [K, 2K): row + 1
#pragma unroll
        for (int c = 0; c < 2 * K; ++c) acc[c] = T(0);
        for (int32_t p0 = rs + sub; p0 < re; p0 += U * LPR) {
            int32_t j[U];
            T v0[U], v1[U], xv[U][K];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t p = p0 + u * LPR;
                j[u] = -1; v0[u] = T(0); v1[u] = T(0);
                if (p < re) {                        // lanes past the row end issue nothing (exec-masked loads)
                    j[u] = col[p];
                    // one 16-byte (fp32: 8-byte) load either way: the interleaved values of the two rows of a pair, or a
                    // single row's value plus its unused right neighbour (val is allocated with one element of slack, CsrViewT)
                    typedef T pair_t __attribute__((ext_vector_type(2), aligned(sizeof(T))));
                    const pair_t vv = *reinterpret_cast<const pair_t *>(val + rs + (pair ? 2 * (p - rs) : (p - rs)));
                    v0[u] = vv.x; v1[u] = vv.y;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < K; ++c) xv[u][c] = T(0);
                if (j[u] >= 0) {
                    if (MODE == 1) {          // no gather at all
#pragma unroll
                        for (int c = 0; c < K; ++c) xv[u][c] = T(j[u]);
                    } else {
                        const T *xr = x + int64_t(MODE == 2 ? (j[u] & 255) : j[u]) * K;   // 2: L1-resident gather
#pragma unroll
                        for (int c = 0; c < K; ++c) xv[u][c] = xr[c];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < K; ++c) {
                    acc[c] += v0[u] * xv[u][c];
                    acc[K + c] += v1[u] * xv[u][c];
                }
        }
        if (MODE == 3) {   // no reduction, (practically) no store
            T t = T(0);
#pragma unroll
            for (int c = 0; c < 2 * K; ++c) t += acc[c];
            if (t == T(1.2345e30)) y[row * K] = t;
            continue;
        }
        // wave-uniform choice (row classes are contiguous, so all but a handful of waves are uniform)
        if (__builtin_amdgcn_ballot_w64(pair) != 0) {
            TReduce<2 * K, LPR>::run(acc, sub);
#pragma unroll
            for (int f = 0; f < MFP; ++f)
                if (own_p[f] && (pair || idx_p[f] < K)) {
                    const int64_t at = row * K + idx_p[f];
                    y[at] = acc[f];
                    if (DOT) dot_p[f] += double(acc[f]) * double(x[at]);
                }
        } else {
            TReduce<K, LPR>::run(acc, sub);
#pragma unroll
            for (int f = 0; f < MFS; ++f)
                if (own_s[f]) {
                    const int64_t at = row * K + idx_s[f];
                    y[at] = acc[f];
                    if (DOT) dot_s[f] += double(acc[f]) * double(x[at]);
                }
        }
    }
    if (DOT) {
        __shared__ double smem[16 * K];
        double dot[K];   // back to one slot per column for the block sum
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double d = 0.0;
#pragma unroll
            for (int f = 0; f < MFP; ++f) d += (idx_p[f] % K == c) ? dot_p[f] : 0.0;
#pragma unroll
            for (int f = 0; f < MFS; ++f) d += (idx_s[f] == c) ? dot_s[f] : 0.0;
            dot[c] = d;
        }
        block_sum<K>(dot, smem);
        if (threadIdx.x < K) part[blockIdx.x * K + threadIdx.x] = pick<K>(dot, threadIdx.x);
    }
}

int choose_lanes_per_row(int64_t n, int64_t nnz) {
    if (g_tune.spmm_lpr) return g_tune.spmm_lpr;
    const double avg = double(nnz) / double(n > 0 ? n : 1);
    if (avg > 40) return 16;
    if (avg > 20) return 8;
    return 4;
}
static int spmm_threads() { return g_tune.spmm_threads ? g_tune.spmm_threads : 256; }

int spmv_grid(int64_t n, int lpr) {
    if (g_tune.spmm_grid) return g_tune.spmm_grid;
    const int64_t rpb = spmm_threads() / lpr;
    int64_t g = (n + rpb - 1) / rpb;
    g = (g + 7) / 8 * 8;  // whole residue classes mod 8 (one per XCD)
    // whole multiples of the 256 CUs finish together; measured at k = 5, 329 k rows, interleaved pair values:
    // 1024 -> 55.4 us, 896 -> 61.0, 768 -> 57.5, 640 -> 69.3 (before the interleaving 768 was ahead: 59.3 vs 59.7)
    constexpr int kSpmmBlocks = 1024;
    static_assert(kSpmmBlocks <= kMaxPartialBlocks, "partials buffer");
    if (g > kSpmmBlocks) g = kSpmmBlocks;
    if (g < 8) g = 8;
    return int(g);
}

template <class T, int K> static void spmm_dispatch(const CsrViewT<T> &A, const T *x, T *y, double *part, const double *scal, int step, int nb, hipStream_t s) {
    int lpr = choose_lanes_per_row(A.n, A.nnz);
    const int threads = spmm_threads();
    int variant = g_tune.spmm_variant ? g_tune.spmm_variant : 3;
    if (variant == 3 && !(A.pair_end > A.pair_begin)) variant = 1;
    // default row schedule of the pair kernel: XCD windows (measured 69 -> 60 us at 334k rows, k = 5); once the matrix no
    // longer stays in the 256 MB of MALL between launches (3D, more than ~20 M stored entries), XCD regions (4 chunks
    // each in these measurements): inside the solver loop (bench.py --tune 3=1 against 3=64 on one box) 152.7 -> 149.8 us at 716k rows,
    // 490.8 -> 480.2 us at 2.17 M rows, but 58.6 -> 60.0 us at 289k rows (the stand-alone probe, tools/probe_regions.py,
    // shows 2 ... 16 chunks within 1 % of each other)
    // chunks per XCD: about 0.4 MB of x per chunk, 4 ... 64 (bench at 5.4 M rows: 4 chunks 1257 us, 16: 1227, 64: 1216)
    int64_t nc = (A.n * int64_t(K) * int64_t(sizeof(T)) / 8 + 210000) / 420000;
    nc = nc < 4 ? 4 : (nc > 64 ? 64 : nc);
    const int mapping = (g_tune.spmm_mapping >= 0) ? g_tune.spmm_mapping : ((lpr == 16 && A.nnz > 20000000) ? int(16 * nc) : 1);
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(nb), dim3(threads), 0, s, A.n, A.pair_begin, A.pair_end, A.rowptr, A.col, A.val, x, y, part, scal, step); };
    auto launch_pair = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(nb), dim3(threads), 0, s, A.n, A.pair_begin, A.pair_end, mapping, A.rowptr, A.col, A.val, x, y, part, scal, step); };
    if constexpr (K == 5 && sizeof(T) == 8) {   // ablation modes of tools/probe_ablate.py
        const int mode = g_tune.spmm_mode;
        if (variant == 3 && lpr == 16 && mode >= 1 && mode <= 3 && !part) {
            if (mode == 1) launch_pair(k_spmm_pair<T, 5, 16, false, 1>);
            if (mode == 2) launch_pair(k_spmm_pair<T, 5, 16, false, 2>);
            if (mode == 3) launch_pair(k_spmm_pair<T, 5, 16, false, 3>);
            return;
        }
    }
    // the lanes per row the kernels are instantiated for; `part`: the launch leaves partial sums of <x, y> (DOT)
    auto for_lanes = [&](auto fn) {
        if (lpr >= 32) fn(int_c<32>{});
        else if (lpr == 16) fn(int_c<16>{});
        else if (lpr == 8) fn(int_c<8>{});
        else fn(int_c<4>{});
    };
    for_lanes([&](auto lc) {
        constexpr int L = decltype(lc)::value;
        if (variant == 3) { if (part) launch_pair(k_spmm_pair<T, K, L, true>); else launch_pair(k_spmm_pair<T, K, L, false>); }
        else { if (part) launch(k_spmm<T, K, L, true>); else launch(k_spmm<T, K, L, false>); }
    });
}

template <class T> bool patch_applies(const CsrViewT<T> &A, int k) {
    return A.patch && k * (A.patch->t.E / A.patch->t.rounds) <= kPatchBlock && patch_lds_bytes(A.patch->lds_rows, k) <= kPatchLdsLimit;
}
template bool patch_applies<double>(const CsrViewT<double> &, int);
template bool patch_applies<float>(const CsrViewT<float> &, int);

template <class T> void launch_spmm(const CsrViewT<T> &A, int k, const T *x, T *y, double *part, const double *scal, int nb, hipStream_t s, int step, bool defer) {
    // patch operator (patch.hip): its tables are laid out for the batch's own column count - a product with more columns than
    // that (inspection hooks only) goes through the stored matrix
    if (patch_applies(A, k)) {
        launch_patch_spmm(A, k, x, y, part, scal, nb, s, step, defer);
        return;
    }
    for_k(k, [&](auto kc) { constexpr int K = decltype(kc)::value; spmm_dispatch<T, K>(A, x, y, part, scal, step, nb, s); });
}
template void launch_spmm<double>(const CsrViewT<double> &, int, const double *, double *, double *, const double *, int, hipStream_t, int, bool);
template void launch_spmm<float>(const CsrViewT<float> &, int, const float *, float *, double *, const double *, int, hipStream_t, int, bool);

// ---- grid barrier (probe and, if it pays, the Chebyshev chain as one launch) ---------------------------------------------------
// Every workgroup of a launch whose workgroups are all resident (grid <= what the chip holds at once: the caller's duty) arrives
// at a counter that only grows - arrival e of nblocks workgroups waits for e * nblocks - and leaves when all have.  Data that
// crosses the barrier is written and read with agent-scope accesses (the eight L2s of the chip are not coherent with each other
// for plain ones).  A wait gives up after kBarrierSpins polls and raises *fail: every wave reaches the end of the kernel.
constexpr long long kBarrierSpins = 1ll << 22;
__device__ __forceinline__ bool grid_barrier(unsigned *counter, unsigned nblocks, unsigned &epoch, int *fail) {
    __shared__ int ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        ++epoch;
        const unsigned target = epoch * nblocks;
        __atomic_thread_fence(__ATOMIC_RELEASE);   // (agent scope is HIP's default for the builtin)
        (void)__hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        long long spins = 0;
        int good = 1;
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            if (++spins > kBarrierSpins || __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { good = 0; break; }
            __builtin_amdgcn_s_sleep(2);
        }
        if (!good) __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        ok = good;
    }
    __syncthreads();
    return ok != 0;
}

__global__ void __launch_bounds__(256) k_barrier_probe(unsigned nblocks, int nbar, unsigned *counter, int *fail, float *buf, int *mismatch) {
    unsigned epoch = 0;
    const unsigned other = (blockIdx.x + 37u) % nblocks;
    int bad = 0;
    for (int it = 0; it < nbar; ++it) {
        __hip_atomic_store(buf + size_t(blockIdx.x) * 256 + threadIdx.x, float(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!grid_barrier(counter, nblocks, epoch, fail)) return;
        const float v = __hip_atomic_load(buf + size_t(other) * 256 + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bad += (v != float(it + 1)) ? 1 : 0;
        if (!grid_barrier(counter, nblocks, epoch, fail)) return;     // nobody overwrites what a neighbour still reads
    }
    if (bad) atomicAdd(mismatch, bad);
}

void launch_barrier_probe(int nblocks, int nbar, unsigned *counter, int *fail, float *buf, int *mismatch, hipStream_t s) {
    hipLaunchKernelGGL(k_barrier_probe, dim3(nblocks), dim3(256), 0, s, unsigned(nblocks), nbar, counter, fail, buf, mismatch);
}

// ------------------------------------------------------------------------------------------
// mixed precision (BASELINE config 5): fp32 inner PCG, fp64 residual refinement.  The outer loop is
//   r = f - A x (fp64 SpMM)  ->  r32 = (float) r  ->  inner PCG on A32 e = r32  ->  x += e

__global__ void __launch_bounds__(256) k_to_float(int64_t n, const double *__restrict__ src, float *__restrict__ dst) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) dst[i] = float(src[i]);
}
// r32 = float(f - q)   (q = nullptr: x = 0, r = f)
__global__ void __launch_bounds__(256) k_mixed_residual(int64_t n, const double *__restrict__ f, const double *__restrict__ q, float *__restrict__ r32) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        r32[i] = float(q ? f[i] - q[i] : f[i]);
}
// x += e (and e = 0 when the inner solve carries on)
__global__ void __launch_bounds__(256) k_mixed_accumulate(int64_t n, double *__restrict__ x, float *__restrict__ e, int zero) {
    for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
        x[i] += double(e[i]);
        if (zero) e[i] = 0.f;
    }
}
int stream_grid(int64_t n) {   // (also warm.hip's streams)
    int64_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    return int(g < 1 ? 1 : g);
}
void launch_to_float(int64_t n, const double *src, float *dst, hipStream_t s) {
    hipLaunchKernelGGL(k_to_float, dim3(stream_grid(n)), dim3(256), 0, s, n, src, dst);
}
void launch_mixed_residual(int64_t n, const double *f, const double *q, float *r32, hipStream_t s) {
    hipLaunchKernelGGL(k_mixed_residual, dim3(stream_grid(n)), dim3(256), 0, s, n, f, q, r32);
}
void launch_mixed_accumulate(int64_t n, double *x, float *e, int zero, hipStream_t s) {
    hipLaunchKernelGGL(k_mixed_accumulate, dim3(stream_grid(n)), dim3(256), 0, s, n, x, e, zero);
}

// ------------------------------------------------------------------------------------------
// axis points: mesh(0, z) / mesh(0, 0, z) point location, AddPointSource and gfu(point)
// (ngsolve_functions.py:10-21, worker.py:124-131).  All points lie on the borehole axis.

template <int DIM>
__global__ void __launch_bounds__(256) k_locate(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                int npts, const double *__restrict__ pz, int32_t *found) {
    constexpr int NB = DIM + 1;
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double X[NB * DIM];
    double lo[DIM], hi[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) { lo[k] = 1e300; hi[k] = -1e300; }
#pragma unroll
    for (int a = 0; a < NB; ++a) {
        const int64_t v = conn[t * NB + a];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            const double c = coords[v * DIM + k];
            X[a * DIM + k] = c;
            lo[k] = fmin(lo[k], c);
            hi[k] = fmax(hi[k], c);
        }
    }
    // the axis is x = 0 (2D) / x = y = 0 (3D): reject elements that do not touch it
    bool touch = true;
#pragma unroll
    for (int k = 0; k < DIM - 1; ++k) {
        const double ext = 1e-9 * (1.0 + hi[k] - lo[k]);
        if (lo[k] > ext || hi[k] < -ext) touch = false;
    }
    if (!touch) return;
    const double extz = 1e-9 * (1.0 + hi[DIM - 1] - lo[DIM - 1]);
    for (int q = 0; q < npts; ++q) {
        const double z = pz[q];
        if (z < lo[DIM - 1] - extz || z > hi[DIM - 1] + extz) continue;
        double P[DIM], l[NB];
#pragma unroll
        for (int k = 0; k < DIM; ++k) P[k] = 0.0;
        P[DIM - 1] = z;
        if (!barycentrics<DIM>(X, P, l)) continue;
        bool in = true;
#pragma unroll
        for (int a = 0; a < NB; ++a)
            if (l[a] < -1e-10) in = false;
        if (in) atomicMin(&found[q], int32_t(t));  // lowest element number: deterministic choice
    }
}

void launch_locate(int dim, int64_t nt, const double *coords, const int32_t *conn, int npts, const double *pz, int32_t *found,
                   hipStream_t s) {
    const int grid = int((nt + 255) / 256);
    if (dim == 2)
        hipLaunchKernelGGL(k_locate<2>, dim3(grid), dim3(256), 0, s, nt, coords, conn, npts, pz, found);
    else
        hipLaunchKernelGGL(k_locate<3>, dim3(grid), dim3(256), 0, s, nt, coords, conn, npts, pz, found);
}

template <int DIM>
__global__ void k_point_shapes(int npts, const double *__restrict__ pz, const int32_t *__restrict__ found,
                               const double *__restrict__ coords, const int32_t *__restrict__ conn, double *__restrict__ phi,
                               int32_t *errflag) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npts) return;
    const int32_t t = found[q];
    if (t == INT_MAX) {
        atomicOr(errflag, 2);
        for (int i = 0; i < N; ++i) phi[q * N + i] = 0.0;
        return;
    }
    double X[NB * DIM], P[DIM], l[NB], ph[N];
    load_vertices<DIM>(coords, conn, t, X);
    for (int k = 0; k < DIM; ++k) P[k] = 0.0;
    P[DIM - 1] = pz[q];
    barycentrics<DIM>(X, P, l);
    shape<DIM>(l, ph);
    for (int i = 0; i < N; ++i) phi[q * N + i] = ph[i];
}

void launch_point_shapes(int dim, int npts, const double *pz, const int32_t *found, const double *coords, const int32_t *conn,
                         double *phi, int32_t *errflag, hipStream_t s) {
    const int grid = (npts + 63) / 64;
    if (dim == 2)
        hipLaunchKernelGGL(k_point_shapes<2>, dim3(grid), dim3(64), 0, s, npts, pz, found, coords, conn, phi, errflag);
    else
        hipLaunchKernelGGL(k_point_shapes<3>, dim3(grid), dim3(64), 0, s, npts, pz, found, coords, conn, phi, errflag);
}

// The same for points anywhere in the mesh (remo_solve_job): P[q] holds DIM coordinates, found[q] the element field_locate gave it.
template <int DIM>
__global__ void __launch_bounds__(64) k_point_shapes_at(int npts, const double *__restrict__ pp, const int32_t *__restrict__ found,
                                                        const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                        double *__restrict__ phi, int32_t *errflag) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npts) return;
    const int32_t t = found[q];
    double ph[N];
#pragma unroll
    for (int i = 0; i < N; ++i) ph[i] = 0.0;
    if (t == INT_MAX) {
        atomicOr(errflag, 2);
    } else {
        double X[NB * DIM], P[DIM];
        load_vertices<DIM>(coords, conn, t, X);
#pragma unroll
        for (int k = 0; k < DIM; ++k) P[k] = pp[int64_t(q) * DIM + k];
        point_shapes<DIM>(X, P, ph);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) phi[int64_t(q) * N + i] = ph[i];
}

void launch_point_shapes_at(int dim, int npts, const double *pp, const int32_t *found, const double *coords, const int32_t *conn,
                            double *phi, int32_t *errflag, hipStream_t s) {
    const int grid = (npts + 63) / 64;
    if (dim == 2)
        hipLaunchKernelGGL(k_point_shapes_at<2>, dim3(grid), dim3(64), 0, s, npts, pp, found, coords, conn, phi, errflag);
    else
        hipLaunchKernelGGL(k_point_shapes_at<3>, dim3(grid), dim3(64), 0, s, npts, pp, found, coords, conn, phi, errflag);
}

// One thread per source: f[dof][rhs] += I phi (a handful of points: atomics are irrelevant here).
template <int DIM, bool CONDENSE>
__global__ void k_build_rhs(int npts, const int32_t *__restrict__ pt_rhs, const double *__restrict__ pt_I,
                            const int32_t *__restrict__ found, const double *__restrict__ phi, const int32_t *__restrict__ eldof,
                            const double *__restrict__ C, const double *__restrict__ M, int k, double *f, double *fint) {
    constexpr int N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = CONDENSE ? 9 : N;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npts) return;
    fint[q] = 0.0;
    const double I = pt_I[q];
    const int32_t t = found[q];
    if (I == 0.0 || t == INT_MAX) return;  // zero strengths are skipped (ngsolve_functions.py:43)
    const int c = pt_rhs[q];
    const int32_t *ed = eldof + int64_t(t) * N;
    for (int i = 0; i < NK; ++i) {
        const int32_t row = ed[i];
        if (row >= 0) atomicAdd(&f[int64_t(row) * k + c], I * phi[q * N + i]);
    }
    if (CONDENSE) {  // fold the bubble load: f_b -= K_bi K_ii^-1 f_i (recover_bubble, elem_access.h, takes it back out of fint)
        const double fi = I * phi[q * N + 9];
        fint[q] = fi;
        if (fi != 0.0) {
            const double *ce = C + int64_t(t) * NT;
            const double kbb = kentry<DIM>(ce, M, 9, 9);
            for (int j = 0; j < 9; ++j) {
                const int32_t row = ed[j];
                if (row >= 0) atomicAdd(&f[int64_t(row) * k + c], -kentry<DIM>(ce, M, 9, j) * fi / kbb);
            }
        }
    }
}

void launch_build_rhs(const ElemMesh &em, int npts, const int32_t *pt_rhs, const double *pt_I, const int32_t *found, const double *phi, int k, double *f,
                      double *fint, hipStream_t s) {
    const int grid = (npts + 63) / 64;
    for_elem_kind(em.dim, em.condense, [&](auto d, auto co) {
        hipLaunchKernelGGL((k_build_rhs<decltype(d)::value, decltype(co)::value>), dim3(grid), dim3(64), 0, s, npts, pt_rhs, pt_I, found, phi, em.eldof, em.C, em.M, k,
                           f, fint);
    });
}

// One thread per point: u_h(point) = sum phi_i x[dof_i] (+ recovered bubble when condensed:
// u_i = K_ii^-1 (f_i - K_ib u_b), ngsolve_functions.py:53-56).  Points with I != 0 are sources:
// they get NaN-free zeros in `out` slots they do not own (out is indexed by point).  (The bubble here is weighted by phi, reads x_ev
// and adds fbub: the plain recovery of a whole column is recover_bubble, elem_access.h.)
template <int DIM, bool CONDENSE>
__global__ void k_eval(int npts, const int32_t *__restrict__ pt_rhs, const double *__restrict__ pt_I,
                       const int32_t *__restrict__ found, const double *__restrict__ phi, const int32_t *__restrict__ eldof,
                       const double *__restrict__ C, const double *__restrict__ M, int k, const double *__restrict__ x,
                       const double *__restrict__ fint, double *__restrict__ out, const double *__restrict__ x_ev,
                       const double *__restrict__ fbub) {
    constexpr int N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = CONDENSE ? 9 : N;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npts) return;
    const int32_t t = found[q];
    if (t == INT_MAX) { out[q] = nan(""); return; }
    const int c = pt_rhs[q];
    const int32_t *ed = eldof + int64_t(t) * N;
    auto xval = [&](int i, int32_t row) { return x_ev ? x_ev[q * N + i] : x[int64_t(row) * k + c]; };
    double s = 0.0;
    for (int i = 0; i < NK; ++i) {
        const int32_t row = ed[i];
        if (row >= 0) s += phi[q * N + i] * xval(i, row);
    }
    if (CONDENSE) {
        const double pb = phi[q * N + 9];
        if (pb != 0.0) {
            const double *ce = C + int64_t(t) * NT;
            double acc = 0.0;
            for (int w = 0; w < npts; ++w)
                if (pt_I[w] != 0.0 && found[w] == t && pt_rhs[w] == c) acc += fint[w];
            if (fbub) acc += fbub[int64_t(t) * k + c];   // secondary formulation: the element's distributed bubble load (secondary.hip)
            for (int j = 0; j < 9; ++j) {
                const int32_t row = ed[j];
                if (row >= 0) acc -= kentry<DIM>(ce, M, 9, j) * xval(j, row);
            }
            s += pb * acc / kentry<DIM>(ce, M, 9, 9);
        }
    }
    out[q] = s;
}

void launch_eval(const ElemMesh &em, int npts, const int32_t *pt_rhs, const double *pt_I, const int32_t *found, const double *phi, int k, const double *x,
                 const double *fint, double *out, hipStream_t s, const double *x_ev, const double *fbub) {
    const int grid = (npts + 63) / 64;
    for_elem_kind(em.dim, em.condense, [&](auto d, auto co) {
        hipLaunchKernelGGL((k_eval<decltype(d)::value, decltype(co)::value>), dim3(grid), dim3(64), 0, s, npts, pt_rhs, pt_I, found, phi, em.eldof, em.C, em.M, k, x,
                           fint, out, x_ev, fbub);
    });
}

// The entries of x that k_eval reads, one slot per (point, local dof): the slot of a row that several points read is repeated, and
// every copy is formed by the same operations on the same operands (pcg_kernels.hip pcg_update_head), so each holds the bits of the full x
template <int DIM>
__global__ void k_eval_slots(int npts, int nk, const int32_t *__restrict__ pt_rhs, const int32_t *__restrict__ found,
                             const int32_t *__restrict__ eldof, int k, int64_t *__restrict__ at) {
    constexpr int N = P3<DIM>::NLD;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npts * N) return;
    const int q = j / N, i = j - q * N;
    const int32_t t = found[q];
    int64_t a = -1;
    if (t != INT_MAX && i < nk) {
        const int32_t row = eldof[int64_t(t) * N + i];
        if (row >= 0) a = int64_t(row) * k + pt_rhs[q];
    }
    at[j] = a;
}

void launch_eval_slots(const ElemMesh &em, int npts, const int32_t *pt_rhs, const int32_t *found, int k, int64_t *at, hipStream_t s) {
    const int N = (em.dim == 3) ? 20 : 10, nk = (em.dim == 2 && em.condense) ? 9 : N;
    const int grid = (npts * N + 255) / 256;
    if (grid == 0) return;
    if (em.dim == 3)
        hipLaunchKernelGGL(k_eval_slots<3>, dim3(grid), dim3(256), 0, s, npts, nk, pt_rhs, found, em.eldof, k, at);
    else
        hipLaunchKernelGGL(k_eval_slots<2>, dim3(grid), dim3(256), 0, s, npts, nk, pt_rhs, found, em.eldof, k, at);
}

}  // namespace remo
