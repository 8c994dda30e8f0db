// elem_access.h — what every element-pass kernel reads of its element, defined once: the vertices through conn, the material through
// eperm, one column of the element vector of x[n][k] and (2D condensed) its cell bubble; and, for the host side, the mesh as one view
// (ElemMesh), the chunk's point loads (PointLoads) and the dispatch on (dim, condense, tensor).  The kernels keep their own parameter
// lists: a launcher unpacks the view.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fem_p3.h"

namespace remo {

// ---- device: reads of one element ---------------------------------------------------------------------------------------------------
// sorted vertex coordinates X[(DIM + 1) * DIM] of device element t
template <int DIM>
__device__ __forceinline__ void load_vertices(const double *__restrict__ coords, const int32_t *__restrict__ conn, int64_t t, double *X) {
    constexpr int NB = DIM + 1;
#pragma unroll
    for (int a = 0; a < NB; ++a) {
        const int64_t v = conn[t * NB + a];
#pragma unroll
        for (int k = 0; k < DIM; ++k) X[a * DIM + k] = coords[v * DIM + k];
    }
}

// device element t in the caller's element order: materials and groups stay in that order (symbolic_gpu.hip); eperm may be null
__device__ __forceinline__ int64_t caller_element(const int32_t *__restrict__ eperm, int64_t t) { return eperm ? int64_t(eperm[t]) : t; }

// material of device element t, -1 when out of range (k_metric_terms flags that: the batch fails before anything else is read)
__device__ __forceinline__ int32_t elem_material(const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm, int64_t t, int nmat) {
    int32_t m = mat[caller_element(eperm, t)];
    if (m < 0 || m >= nmat) m = -1;
    return m;
}

// conductivity of material m: one scalar, or (TENSOR) the upper triangle of sigma_tensor[nmat][3 | 6]
template <int DIM, bool TENSOR>
__device__ __forceinline__ void load_sigma(const double *__restrict__ sigma, int32_t m, double *S) {
    constexpr int NS = TENSOR ? SigmaTensor<DIM>::N : 1;
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = sigma[int64_t(m) * NS + i];
}

// element vector of column c of x[n][k]: constrained rows read 0; NK rows are gathered (2D condensed: recover_bubble gives the tenth)
template <int N, int NK>
__device__ __forceinline__ void gather_column(const int32_t *__restrict__ ed, const double *__restrict__ x, int k, int c, double (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int32_t row = (i < NK) ? ed[i] : -1;
        v[i] = (row >= 0) ? x[int64_t(row) * k + c] : 0.0;
    }
}

// condensed cell bubble of column c: x_9 = (f_9 - sum_j K_9j x_j) / K_99, f_9 the bubble loads of the column's points q0 .. q0 + nq - 1
// that lie in element t.  (k_eval, k_build_rhs and k_sec_elements hold the weighted forms of the same recovery.)
__device__ __forceinline__ void recover_bubble(int32_t t, const double *ce, const double *M, int c, int q0, int nq, const int32_t *__restrict__ pt_rhs,
                                               const double *__restrict__ pt_I, const int32_t *__restrict__ found, const double *__restrict__ fint,
                                               double (&v)[10]) {
    double acc = 0.0;
    for (int w = q0; w < q0 + nq; ++w)
        if (pt_I[w] != 0.0 && found[w] == t && pt_rhs[w] == c) acc += fint[w];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc -= kentry<2>(ce, M, 9, j) * v[j];
    v[9] = acc / kentry<2>(ce, M, 9, 9);
}

// ---- host: the views the launchers take ---------------------------------------------------------------------------------------------
// The mesh of a batch as the element kernels see it.  Owns nothing; a member a launcher does not read may stay null.
struct ElemMesh {
    int dim = 0;
    bool condense = false;
    int64_t nt = 0;
    const double *coords = nullptr;                                   // [nv][dim]
    const int32_t *conn = nullptr, *mat = nullptr, *eperm = nullptr;   // [nt][dim + 1] sorted vertices; materials in the caller's order; device -> caller element, or null
    const double *sigma = nullptr;                                    // [n_mat][sigma_comp]
    int sigma_comp = 1, n_mat = 0;
    const int32_t *eldof = nullptr;                                   // [nt][NLD] free row of every local dof, -1 constrained
    const double *C = nullptr, *M = nullptr;                          // metric terms [nt][NTERM], reference tensors
    const int32_t *adjptr = nullptr;                                  // adjacency lists of the rows (DeviceSymbolic::adj)
    const uint32_t *adj = nullptr;
    bool tensor() const { return sigma_comp > 1; }
};

// The axis points of a chunk of right-hand sides (2D condensed: the bubble loads of sources inside an element, as k_eval reads them)
struct PointLoads {
    const int32_t *pt_rhs = nullptr;
    const double *pt_I = nullptr;
    const int32_t *found = nullptr;
    const double *fint = nullptr;
    int nq = 0;
};

// fn(integral_constant<int, DIM>, bool_constant<CONDENSE>) for the kinds of element the kernels are instantiated for: (3, false),
// (2, true), (2, false); the second form adds bool_constant<TENSOR>
template <class F> void for_elem_kind(int dim, bool condense, F &&fn) {
    if (dim == 3) fn(std::integral_constant<int, 3>{}, std::false_type{});
    else if (condense) fn(std::integral_constant<int, 2>{}, std::true_type{});
    else fn(std::integral_constant<int, 2>{}, std::false_type{});
}
template <class F> void for_elem_kind(int dim, bool condense, bool tensor, F &&fn) {
    for_elem_kind(dim, condense, [&](auto d, auto co) {
        if (tensor) fn(d, co, std::true_type{}); else fn(d, co, std::false_type{});
    });
}

}  // namespace remo
