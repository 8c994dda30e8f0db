// field.hip — gfx950 kernels of the field sections (remo_solve_batch_field, remo_batch_field): location of arbitrary points of the
// mesh and evaluation of u_h, grad u_h and J = -Sigma grad u_h there (field.h).
//
// Location.  The points are binned on a uniform grid of cells over their bounding box and sorted by cell (rocPRIM's stable radix
// sort, as sens_group_order does with the groups); the cell number has the first coordinate fastest, so the points of a run of cells
// along it are ONE range of the sorted list.  The elements are the other side: k_field_locate_lane gives every element a lane, which
// clips the element's box to the grid and tests the points of the cell rows it overlaps - a few cells for the bulk of a graded mesh.
// An element that overlaps more than kFieldLaneCells cells (the large outer elements cover the whole section) is appended to a list
// instead, and k_field_locate_wave gives each of those a wave whose lanes stride over the same ranges.  Points, not elements, are
// sorted because the points are the smaller side (a 256 x 256 section against 350 k tetrahedra) and the element side then needs no
// list per cell: an element names its cells by its box alone.  Among several elements that hold a point (shared faces, edges,
// vertices; in 3D the plane y = 0) the lowest device element number wins through atomicMin, as in k_locate: the result does not
// depend on the order in which elements reach the list or the points.  Tolerances are k_locate's.
//
// Evaluation.  k_field_eval: a workgroup takes 256 / kp points and kp >= (wanted columns of the block) lanes per point, the column
// fastest: the kp lanes of a point read the kp neighbouring values of a row of x[n][k] in one instruction - one 8 k byte piece of a
// row per request instead of one 8-byte value per lane and row.  Every lane holds one column's element vector in registers
// (compile-time indices only) and calls field_point, the code remo_host_field_element runs.  The results go through LDS so that
// the stores run along the points: plain vector stores, consecutive lanes on consecutive addresses.  Its reads of the element are
// elem_access.h's; field_elem_setup keeps a vertex loop of its own, which folds the element's box in.
#include <limits.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <stdexcept>

#include "elem_access.h"
#include "field.h"

namespace remo {

namespace {

constexpr int kFieldLaneCells = 16;       // an element that overlaps more cells gets a wave
constexpr int kFieldMaxCellsDir = 2048;   // cells along one direction
constexpr int64_t kFieldMaxCells = int64_t(1) << 22;

// cell of coordinate v along one direction: monotone in v, so a point inside an element's box lies in a cell of the box's range
REMO_HD int32_t field_cell1(double v, double lo, double inv, int32_t nc) {
    const double c = floor((v - lo) * inv);
    if (!(c >= 0.0)) return 0;
    if (c > double(nc - 1)) return nc - 1;
    return int32_t(c);
}

template <int DIM>
__global__ void __launch_bounds__(256) k_field_cells(int64_t n_pts, const double *__restrict__ pts, FieldGrid G, uint32_t *__restrict__ keys,
                                                     int32_t *__restrict__ ids, int32_t *__restrict__ found) {
    const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_pts) return;
    int64_t key = 0;
#pragma unroll
    for (int k = DIM - 1; k >= 0; --k) key = key * G.nc[k] + field_cell1(pts[i * DIM + k], G.lo[k], G.inv[k], G.nc[k]);
    keys[i] = uint32_t(key);
    ids[i] = int32_t(i);
    found[i] = INT_MAX;   // what the atomicMin of the element passes starts from
}

// off[c] = first sorted position whose cell is >= c, c = 0 .. ncell
__global__ void __launch_bounds__(256) k_field_offsets(int64_t n_pts, int32_t ncell, const uint32_t *__restrict__ keys, int32_t *__restrict__ off) {
    const int64_t c = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (c > ncell) return;
    int64_t lo = 0, hi = n_pts;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < uint32_t(c)) lo = mid + 1; else hi = mid;
    }
    off[c] = int32_t(lo);
}

// vertices, barycentric gradients, the box with k_locate's slack and the cells it overlaps; false: degenerate, or away from every point
template <int DIM>
__device__ __forceinline__ bool field_elem_setup(int64_t t, const double *__restrict__ coords, const int32_t *__restrict__ conn, const FieldGrid &G,
                                                 double *X, double g[DIM][DIM], double *lo, double *hi, int32_t *c0, int32_t *c1) {
    constexpr int NB = DIM + 1;
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
    bool near = true;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const double ext = 1e-9 * (1.0 + hi[k] - lo[k]);
        lo[k] -= ext;
        hi[k] += ext;
        if (lo[k] > G.hi[k] || hi[k] < G.lo[k]) near = false;
        c0[k] = field_cell1(lo[k], G.lo[k], G.inv[k], G.nc[k]);
        c1[k] = field_cell1(hi[k], G.lo[k], G.inv[k], G.nc[k]);
    }
    if (!near) return false;
    return bary_gradients<DIM>(X, g) > 0.0;
}

// the points of the element's cells, lane `lane` of `stride` taking every stride-th of a row's range
template <int DIM>
__device__ __forceinline__ void field_elem_walk(int32_t t, const double *X, const double g[DIM][DIM], const double *lo, const double *hi, const int32_t *c0,
                                                const int32_t *c1, const FieldGrid &G, const int32_t *__restrict__ off, const int32_t *__restrict__ perm,
                                                const double *__restrict__ pts, int32_t *found, int lane, int stride) {
    constexpr int NB = DIM + 1;
    const int32_t z0 = (DIM == 3) ? c0[DIM - 1] : 0, z1 = (DIM == 3) ? c1[DIM - 1] : 0;
    for (int32_t cz = z0; cz <= z1; ++cz)
        for (int32_t cy = c0[1]; cy <= c1[1]; ++cy) {
            const int64_t base = ((DIM == 3) ? int64_t(cz) * G.nc[1] + cy : int64_t(cy)) * G.nc[0];
            const int32_t jb = off[base + c0[0]], je = off[base + c1[0] + 1];
            for (int32_t j = jb + lane; j < je; j += stride) {
                const int64_t i = perm[j];
                double P[DIM], l[NB];
                bool in = true;
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    P[k] = pts[i * DIM + k];
                    in = in && P[k] >= lo[k] && P[k] <= hi[k];
                }
                if (!in) continue;
                bary_from_gradients<DIM>(X, g, P, l);
#pragma unroll
                for (int a = 0; a < NB; ++a) in = in && l[a] >= -1e-10;
                if (in) atomicMin(&found[i], t);   // lowest element number: deterministic choice
            }
        }
}

template <int DIM>
__global__ void __launch_bounds__(256) k_field_locate_lane(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn, FieldGrid G,
                                                           const int32_t *__restrict__ off, const int32_t *__restrict__ perm,
                                                           const double *__restrict__ pts, int32_t *found, int32_t *big, int32_t *nbig) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= nt) return;
    double X[(DIM + 1) * DIM], g[DIM][DIM], lo[DIM], hi[DIM];
    int32_t c0[DIM], c1[DIM];
    if (!field_elem_setup<DIM>(t, coords, conn, G, X, g, lo, hi, c0, c1)) return;
    int64_t cells = 1;
#pragma unroll
    for (int k = 0; k < DIM; ++k) cells *= int64_t(c1[k] - c0[k] + 1);
    if (cells > kFieldLaneCells) {
        big[atomicAdd(nbig, 1)] = int32_t(t);   // at most one entry per element: the list holds nt
        return;
    }
    field_elem_walk<DIM>(int32_t(t), X, g, lo, hi, c0, c1, G, off, perm, pts, found, 0, 1);
}

template <int DIM>
__global__ void __launch_bounds__(256) k_field_locate_wave(const double *__restrict__ coords, const int32_t *__restrict__ conn, FieldGrid G,
                                                           const int32_t *__restrict__ off, const int32_t *__restrict__ perm,
                                                           const double *__restrict__ pts, int32_t *found, const int32_t *__restrict__ big,
                                                           const int32_t *__restrict__ nbig) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6), nwaves = int64_t(gridDim.x) * 4;
    const int32_t n = *nbig;
    for (int64_t w = wave; w < n; w += nwaves) {
        const int32_t t = big[w];
        double X[(DIM + 1) * DIM], g[DIM][DIM], lo[DIM], hi[DIM];
        int32_t c0[DIM], c1[DIM];
        if (!field_elem_setup<DIM>(t, coords, conn, G, X, g, lo, hi, c0, c1)) continue;
        field_elem_walk<DIM>(t, X, g, lo, hi, c0, c1, G, off, perm, pts, found, lane, 64);
    }
}

__global__ void __launch_bounds__(256) k_field_elem(int64_t n_pts, const int32_t *__restrict__ found, const int32_t *__restrict__ eperm,
                                                    int32_t *__restrict__ elem) {
    const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (q >= n_pts) return;
    const int32_t t = found[q];
    elem[q] = (t == INT_MAX) ? -1 : (eperm ? eperm[t] : t);
}

unsigned key_bits(int32_t ncell) {   // the keys run from 0 to ncell - 1
    unsigned bits = 1;
    while (bits < 32 && (uint32_t(ncell) >> bits) != 0) ++bits;
    return bits;
}

// entry j of a small array of the kernel's arguments, by compile-time indices
__device__ __forceinline__ int pick(const int (&a)[REMO_MAX_RHS], int j) {
    int v = -1;
#pragma unroll
    for (int i = 0; i < REMO_MAX_RHS; ++i) v = (i == j) ? a[i] : v;
    return v;
}

}  // namespace

// kp = 1 << kp_log2 lanes per point (>= cols.n), 256 >> kp_log2 points per workgroup
template <int DIM, bool CONDENSE, bool TENSOR>
__global__ void __launch_bounds__(256) k_field_eval(int64_t n_pts, const double *__restrict__ pts, const int32_t *__restrict__ found,
                                                    const double *__restrict__ coords, const int32_t *__restrict__ conn, const int32_t *__restrict__ mat,
                                                    const int32_t *__restrict__ eperm, const double *__restrict__ sigma, int n_mat,
                                                    const int32_t *__restrict__ eldof, const double *__restrict__ C, const double *__restrict__ M, int k,
                                                    const double *__restrict__ x, FieldCols cols, PointLoads src, int kp_log2, double *__restrict__ u,
                                                    double *__restrict__ grad, double *__restrict__ J) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = (DIM == 2 && CONDENSE) ? 9 : N, NO = FieldOut<DIM>::N;
    constexpr int NS = TENSOR ? SigmaTensor<DIM>::N : 1;
    __shared__ double s_out[NO * 256];   // u [c][point], then grad and J [c][point][DIM]
    const int tid = threadIdx.x, ppb = 256 >> kp_log2;
    const int c = tid & ((1 << kp_log2) - 1), pl = tid >> kp_log2;
    const int64_t p0 = int64_t(blockIdx.x) * ppb, p = p0 + pl;
    const int col = (c < cols.n) ? pick(cols.col, c) : -1;
    double out[NO];
#pragma unroll
    for (int i = 0; i < NO; ++i) out[i] = nan("");
    const int32_t t = (p < n_pts && col >= 0) ? found[p] : INT_MAX;
    if (t != INT_MAX) {
        const int32_t m = elem_material(mat, eperm, t, n_mat);
        if (m >= 0) {   // (otherwise k_metric_terms has flagged it: the batch fails)
            double X[NB * DIM], P[DIM], S[NS], xe[N];
            load_vertices<DIM>(coords, conn, t, X);
#pragma unroll
            for (int d = 0; d < DIM; ++d) P[d] = pts[p * DIM + d];
            load_sigma<DIM, TENSOR>(sigma, m, S);
            gather_column<N, NK>(eldof + int64_t(t) * N, x, k, col, xe);
            if constexpr (DIM == 2 && CONDENSE) recover_bubble(t, C + int64_t(t) * NT, M, col, 0, src.nq, src.pt_rhs, src.pt_I, src.found, src.fint, xe);
            double res[NO];
            if (field_point<DIM, TENSOR>(X, P, xe, S, res)) {
#pragma unroll
                for (int i = 0; i < NO; ++i) out[i] = res[i];
            }
        }
    }
    const int at = c * ppb + pl;
    s_out[at] = out[0];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
        s_out[256 + at * DIM + d] = out[1 + d];
        s_out[256 + 256 * DIM + at * DIM + d] = out[1 + DIM + d];
    }
    __syncthreads();
    // stores along the points: column cc of the workgroup's ppb points is one run of ppb (* DIM) doubles in every output
    const int64_t left = n_pts - p0;   // > 0
    if (u) {
        const int cc = tid / ppb, q = tid - cc * ppb;
        const int slot = (cc < cols.n) ? pick(cols.slot, cc) : -1;
        if (slot >= 0 && q < left) u[int64_t(slot) * n_pts + p0 + q] = s_out[tid];
    }
    for (int idx = tid; idx < 256 * DIM; idx += 256) {
        const int cc = idx / (ppb * DIM), rem = idx - cc * (ppb * DIM);
        const int slot = (cc < cols.n) ? pick(cols.slot, cc) : -1;
        if (slot < 0 || rem >= left * DIM) continue;
        const int64_t o = (int64_t(slot) * n_pts + p0) * DIM + rem;
        if (grad) grad[o] = s_out[256 + idx];
        if (J) J[o] = s_out[256 + 256 * DIM + idx];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
FieldGrid field_grid(int dim, int64_t n_pts, const double *pts) {
    FieldGrid G;
    if (n_pts <= 0) return G;
    double ext[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < dim; ++k) { G.lo[k] = G.hi[k] = pts[k]; }
    for (int64_t i = 1; i < n_pts; ++i)
        for (int k = 0; k < dim; ++k) {
            G.lo[k] = std::fmin(G.lo[k], pts[i * dim + k]);
            G.hi[k] = std::fmax(G.hi[k], pts[i * dim + k]);
        }
    int nd = 0;
    double vol = 1.0;
    for (int k = 0; k < dim; ++k) {
        ext[k] = G.hi[k] - G.lo[k];
        if (ext[k] > 0.0 && std::isfinite(ext[k])) { ++nd; vol *= ext[k]; } else ext[k] = 0.0;
    }
    if (nd == 0) return G;   // one point, or all points identical: one cell
    // about two points per cell, cells as near to cubes as the bounds allow
    const double target = double(std::min<int64_t>(std::max<int64_t>(n_pts / 2, 1), kFieldMaxCells));
    const double h = std::pow(vol / target, 1.0 / nd);
    for (int k = 0; k < dim; ++k) {
        if (ext[k] == 0.0) continue;
        const double want = std::ceil(ext[k] / h);
        G.nc[k] = int32_t(std::fmin(std::fmax(want, 1.0), double(kFieldMaxCellsDir)));
    }
    auto total = [&]() { return int64_t(G.nc[0]) * G.nc[1] * G.nc[2]; };
    while (total() > kFieldMaxCells) {
        int big = 0;
        for (int k = 1; k < dim; ++k)
            if (G.nc[k] > G.nc[big]) big = k;
        G.nc[big] = (G.nc[big] + 1) / 2;
    }
    for (int k = 0; k < dim; ++k) G.inv[k] = (ext[k] > 0.0) ? double(G.nc[k]) / ext[k] : 0.0;
    G.ncell = int32_t(total());
    return G;
}

size_t field_sort_bytes(int64_t n_pts, int32_t ncell) {
    size_t tb = 0;
    uint32_t *k = nullptr;
    int32_t *v = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, tb, k, k, v, v, size_t(n_pts > 0 ? n_pts : 1), 0u, key_bits(ncell), hipStream_t(nullptr)) != hipSuccess)
        throw std::runtime_error("rocprim::radix_sort_pairs: size query failed");
    return tb;
}

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

size_t field_locate_bytes(int64_t n_pts, int64_t nt, int32_t ncell, size_t sort_bytes) {
    const size_t np = size_t(n_pts > 0 ? n_pts : 1);
    return 4 * up256(np * 4) + up256((size_t(ncell) + 1) * 4) + up256(size_t(nt) * 4) + 256 + up256(sort_bytes + 256);
}

FieldLocate field_locate_carve(char *base, int64_t n_pts, int64_t nt, int32_t ncell, size_t sort_bytes) {
    const size_t np = size_t(n_pts > 0 ? n_pts : 1);
    FieldLocate b;
    size_t at = 0;
    auto take = [&](size_t bytes) { char *p = base + at; at += up256(bytes); return p; };
    b.keys_in = reinterpret_cast<uint32_t *>(take(np * 4)); b.keys = reinterpret_cast<uint32_t *>(take(np * 4));
    b.ids = reinterpret_cast<int32_t *>(take(np * 4)); b.perm = reinterpret_cast<int32_t *>(take(np * 4));
    b.off = reinterpret_cast<int32_t *>(take((size_t(ncell) + 1) * 4));
    b.big = reinterpret_cast<int32_t *>(take(size_t(nt) * 4));
    b.nbig = reinterpret_cast<int32_t *>(take(4));
    b.tmp = take(sort_bytes + 256);
    b.tmp_bytes = sort_bytes;
    return b;
}

void field_locate(int dim, int64_t nt, const double *coords, const int32_t *conn, int64_t n_pts, const double *pts, const FieldGrid &G,
                  const FieldLocate &b, int32_t *found, hipStream_t s) {
    if (n_pts <= 0 || nt <= 0) return;
    const unsigned gp = unsigned((n_pts + 255) / 256), gt = unsigned((nt + 255) / 256);
    const unsigned gw = unsigned(std::min<int64_t>((nt + 3) / 4, 2048));
    if (dim == 2) hipLaunchKernelGGL(k_field_cells<2>, dim3(gp), dim3(256), 0, s, n_pts, pts, G, b.keys_in, b.ids, found);
    else hipLaunchKernelGGL(k_field_cells<3>, dim3(gp), dim3(256), 0, s, n_pts, pts, G, b.keys_in, b.ids, found);
    size_t tb = b.tmp_bytes;
    if (rocprim::radix_sort_pairs(b.tmp, tb, b.keys_in, b.keys, b.ids, b.perm, size_t(n_pts), 0u, key_bits(G.ncell), s) != hipSuccess)
        throw std::runtime_error("rocprim::radix_sort_pairs failed");
    hipLaunchKernelGGL(k_field_offsets, dim3(unsigned((int64_t(G.ncell) + 1 + 255) / 256)), dim3(256), 0, s, n_pts, G.ncell, b.keys, b.off);
    if (hipMemsetAsync(b.nbig, 0, sizeof(int32_t), s) != hipSuccess) throw std::runtime_error("hipMemsetAsync failed");
    if (dim == 2) {
        hipLaunchKernelGGL(k_field_locate_lane<2>, dim3(gt), dim3(256), 0, s, nt, coords, conn, G, b.off, b.perm, pts, found, b.big, b.nbig);
        hipLaunchKernelGGL(k_field_locate_wave<2>, dim3(gw), dim3(256), 0, s, coords, conn, G, b.off, b.perm, pts, found, b.big, b.nbig);
    } else {
        hipLaunchKernelGGL(k_field_locate_lane<3>, dim3(gt), dim3(256), 0, s, nt, coords, conn, G, b.off, b.perm, pts, found, b.big, b.nbig);
        hipLaunchKernelGGL(k_field_locate_wave<3>, dim3(gw), dim3(256), 0, s, coords, conn, G, b.off, b.perm, pts, found, b.big, b.nbig);
    }
}

void launch_field_elem(int64_t n_pts, const int32_t *found, const int32_t *eperm, int32_t *elem, hipStream_t s) {
    if (n_pts <= 0) return;
    hipLaunchKernelGGL(k_field_elem, dim3(unsigned((n_pts + 255) / 256)), dim3(256), 0, s, n_pts, found, eperm, elem);
}

void launch_field_eval(const ElemMesh &em, int64_t n_pts, const double *pts, const int32_t *found, int k, const double *x, const FieldCols &cols,
                       const PointLoads &src, double *u, double *grad, double *J, hipStream_t s) {
    if (n_pts <= 0 || cols.n <= 0) return;
    int kp_log2 = 0;
    while ((1 << kp_log2) < cols.n) ++kp_log2;
    const int ppb = 256 >> kp_log2;
    const unsigned grid = unsigned((n_pts + ppb - 1) / ppb);
    for_elem_kind(em.dim, em.condense, em.tensor(), [&](auto d, auto co, auto te) {
        hipLaunchKernelGGL((k_field_eval<decltype(d)::value, decltype(co)::value, decltype(te)::value>), dim3(grid), dim3(256), 0, s, n_pts, pts, found, em.coords,
                           em.conn, em.mat, em.eperm, em.sigma, em.n_mat, em.eldof, em.C, em.M, k, x, cols, src, kp_log2, u, grad, J);
    });
}

}  // namespace remo
