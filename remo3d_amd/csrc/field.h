// field.h — the solution away from the borehole axis (remo_solve_batch_field, remo_batch_field): u_h, grad u_h and the current
// density J = -Sigma grad u_h at arbitrary points of the mesh.  The per-point arithmetic shared by host and gfx950 code, and the
// launchers of field.hip (location of the points, evaluation).
//
// With the hierarchical basis of fem_p3.h, phi_i a polynomial in the barycentrics l_0 .. l_DIM of the element's SORTED vertices:
//     u = sum_i x_i phi_i(l),   D_a = sum_i x_i dphi_i/dl_a (all DIM + 1 barycentrics taken as independent),
//     grad u = sum_a D_a grad(l_a) = sum_{a >= 1} (D_a - D_0) grad(l_a)      (grad(l_0) = -sum_{a >= 1} grad(l_a)),
// grad(l_a) from bary_gradients.  2D is the (r, z) half plane: grad u = (du/dr, du/dz) and the tensor [rr, rz, zz].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/remo3d_hip.h"
#include "elem_access.h"
#include "fem_p3.h"

namespace remo {

// values per point: u, grad u [DIM], J [DIM]
template <int DIM> struct FieldOut { static constexpr int N = 1 + 2 * DIM; };

// u, grad u and J at barycentrics l of an element.  g: bary_gradients of the sorted vertices; xe: the element's NLD values
// (constrained dofs 0); S: the material's conductivity, one scalar or the upper triangle of remo_solve_batch_tensor.
template <int DIM, bool TENSOR>
REMO_HD void field_element(const double g[DIM][DIM], const double *l, const double *xe, const double *S, double *out) {
    constexpr int NB = DIM + 1;
    double u = 0.0, D[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) D[a] = 0.0;
    int k = 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        u += xe[k] * l[i];
        D[i] += xe[k];
        ++k;
    }
#pragma unroll
    for (int e = 0; e < P3<DIM>::NEDGE; ++e) {
        const int a = edge_a(DIM, e), b = edge_b(DIM, e);
        const double la = l[a], lb = l[b];
        u += xe[k] * (la * lb);
        D[a] += xe[k] * lb;
        D[b] += xe[k] * la;
        ++k;
        u += xe[k] * (la * lb * (lb - la));
        D[a] += xe[k] * (lb * (lb - 2.0 * la));
        D[b] += xe[k] * (la * (2.0 * lb - la));
        ++k;
    }
    if constexpr (DIM == 2) {
        u += xe[k] * (l[0] * l[1] * l[2]);
        D[0] += xe[k] * (l[1] * l[2]);
        D[1] += xe[k] * (l[0] * l[2]);
        D[2] += xe[k] * (l[0] * l[1]);
    } else {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            int a, b, c;
            face_abc(f, a, b, c);
            u += xe[k] * (l[a] * l[b] * l[c]);
            D[a] += xe[k] * (l[b] * l[c]);
            D[b] += xe[k] * (l[a] * l[c]);
            D[c] += xe[k] * (l[a] * l[b]);
            ++k;
        }
    }
    double gu[DIM];
#pragma unroll
    for (int p = 0; p < DIM; ++p) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) s += (D[a + 1] - D[0]) * g[a][p];
        gu[p] = s;
    }
    out[0] = u;
#pragma unroll
    for (int p = 0; p < DIM; ++p) out[1 + p] = gu[p];
    if constexpr (!TENSOR) {
#pragma unroll
        for (int p = 0; p < DIM; ++p) out[1 + DIM + p] = -(S[0] * gu[p]);
    } else if constexpr (DIM == 2) {
        out[3] = -(S[0] * gu[0] + S[1] * gu[1]);
        out[4] = -(S[1] * gu[0] + S[2] * gu[1]);
    } else {
        out[4] = -(S[0] * gu[0] + S[1] * gu[1] + S[2] * gu[2]);
        out[5] = -(S[1] * gu[0] + S[3] * gu[1] + S[4] * gu[2]);
        out[6] = -(S[2] * gu[0] + S[4] * gu[1] + S[5] * gu[2]);
    }
}

// barycentrics of P from the gradients of bary_gradients (the arithmetic of fem_p3.h barycentrics)
template <int DIM> REMO_HD void bary_from_gradients(const double *X, const double g[DIM][DIM], const double *P, double *l) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) v += g[a][k] * (P[k] - X[k]);
        l[a + 1] = v;
        s += v;
    }
    l[0] = 1.0 - s;
}

// The same at a point P of the element with sorted vertex coordinates X.  Returns false for a degenerate element.
template <int DIM, bool TENSOR>
REMO_HD bool field_point(const double *X, const double *P, const double *xe, const double *S, double *out) {
    double g[DIM][DIM], l[DIM + 1];
    const double vol = bary_gradients<DIM>(X, g);
    if (!(vol > 0.0)) return false;
    bary_from_gradients<DIM>(X, g, P, l);
    field_element<DIM, TENSOR>(g, l, xe, S, out);
    return true;
}

// ---- location of arbitrary points (field.hip) -------------------------------------------------------------------------------------
// A uniform grid of cells over the points' bounding box (no cells along a direction without extent); cell number with the first
// coordinate fastest, so the points of a run of cells along it are one range of the list sorted by cell.
struct FieldGrid {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0}, inv[3] = {0.0, 0.0, 0.0};   // inv: cells per metre (0: one cell)
    int32_t nc[3] = {1, 1, 1};
    int32_t ncell = 1;
};
FieldGrid field_grid(int dim, int64_t n_pts, const double *pts);   // host; pts finite

struct FieldLocate {                  // device buffers of one location (field_locate_take)
    uint32_t *keys_in = nullptr, *keys = nullptr;    // [n_pts] cell of every point, unsorted and sorted
    int32_t *ids = nullptr, *perm = nullptr;         // [n_pts] 0 .. n_pts - 1 and the points sorted by cell (stable)
    int32_t *off = nullptr;                          // [ncell + 1] first sorted position of every cell
    int32_t *big = nullptr, *nbig = nullptr;         // [nt], [1] elements that overlap many cells: a wave each
    void *tmp = nullptr;                             // the radix sort's temporary storage
    size_t tmp_bytes = 0;
};
size_t field_sort_bytes(int64_t n_pts, int32_t ncell);   // no device work
// bytes of all buffers of FieldLocate (each rounded up to 256) for n_pts points and nt elements
size_t field_locate_bytes(int64_t n_pts, int64_t nt, int32_t ncell, size_t sort_bytes);
// carve the buffers out of one allocation of field_locate_bytes
FieldLocate field_locate_carve(char *base, int64_t n_pts, int64_t nt, int32_t ncell, size_t sort_bytes);
// found[q] = lowest number of an element of conn (device order) that contains pts[q], INT_MAX where none does.  n_pts >= 1.
void field_locate(int dim, int64_t nt, const double *coords, const int32_t *conn, int64_t n_pts, const double *pts, const FieldGrid &grid,
                  const FieldLocate &buf, int32_t *found, hipStream_t s);
// elem[q] = the caller's number of element found[q] (through eperm), -1 where found[q] == INT_MAX
void launch_field_elem(int64_t n_pts, const int32_t *found, const int32_t *eperm, int32_t *elem, hipStream_t s);

// ---- evaluation -------------------------------------------------------------------------------------------------------------------
// Which columns of the solution block x[n][k] are evaluated and which of the outputs' column slots each goes to.
struct FieldCols {
    int n = 0;
    int col[REMO_MAX_RHS] = {}, slot[REMO_MAX_RHS] = {};
};
// u[slot][n_pts], grad[slot][n_pts][dim], J[slot][n_pts][dim] of the columns of `cols` (any of the three may be nullptr); NaN
// where found[q] == INT_MAX.  em.sigma: [n_mat] scalars, or (tensor) [n_mat][3 | 6] upper triangles; src: the axis points of the
// block's right-hand sides (elem_access.h).
void launch_field_eval(const ElemMesh &em, int64_t n_pts, const double *pts, const int32_t *found, int k, const double *x, const FieldCols &cols,
                       const PointLoads &src, double *u, double *grad, double *J, hipStream_t s);

}  // namespace remo
