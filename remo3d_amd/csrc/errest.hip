// errest.hip — gfx950 kernels of the goal-oriented error estimates (remo_job_error_t.err; the formula is in errest.h).
//
// k_error_facets runs right after a chunk's solve, forward and adjoint chunks alike, and writes eta_e^2 of every element for all
// k <= 8 columns of the chunk in one launch.  As in k_field_eval a workgroup takes 256 / kp elements and kp >= k lanes per element,
// the column fastest: the kp lanes of an element read the kp neighbouring values of a row of x[n][k] in one request, so a gathered
// row serves all columns.  The kernel is gather-bound: per lane the rows of the element and of up to DIM + 1 neighbours.  A lane
// holds one column's element vector of e and of one neighbour at a time in registers; the facets are unrolled (compile-time
// indices only), the quadrature points are a loop over the rule in LDS.  The neighbour across a facet is read from the adjacency
// list of the facet's dof row - the lists the numbering keeps for all rows, also when only the P1 block has a pattern.  Every
// element sums its own facets, so a shared facet is computed from both sides: no floating-point atomics, and the result depends on
// the mesh only.  The values leave through LDS so that the stores run along the elements.
//
// k_error_combine: E_je = sqrt(eta_e^2(u) eta_e^2(lambda)) per functional, with the sign k_sens_reduce / k_sens_group_sum take off
// again, and the workgroups' sums in a fixed order.
// err_load puts together elem_access.h's reads of an element (vertices, conductivity, a column's element vector, the condensed bubble).
#include "elem_access.h"
#include "errest.h"
#include "sens.h"
#include "wave_util.h"

namespace remo {

namespace {

// 3 Gauss-Legendre points on [0, 1]; the symmetric 6-point rule of degree 4 on the triangle (Dunavant)
const double kRule2[ErrRule<2>::NTAB] = {
    0.88729833462074168852, 0.11270166537925831148, 5.0 / 18.0,
    0.5, 0.5, 8.0 / 18.0,
    0.11270166537925831148, 0.88729833462074168852, 5.0 / 18.0};
const double kRule3[ErrRule<3>::NTAB] = {
    0.10810301816807022736, 0.44594849091596488632, 0.44594849091596488632, 0.22338158967801146570,
    0.44594849091596488632, 0.10810301816807022736, 0.44594849091596488632, 0.22338158967801146570,
    0.44594849091596488632, 0.44594849091596488632, 0.10810301816807022736, 0.22338158967801146570,
    0.81684757298045851308, 0.09157621350977074346, 0.09157621350977074346, 0.10995174365532186764,
    0.09157621350977074346, 0.81684757298045851308, 0.09157621350977074346, 0.10995174365532186764,
    0.09157621350977074346, 0.09157621350977074346, 0.81684757298045851308, 0.10995174365532186764};

// vertices, conductivity and column `col` of the element vector of device element t; false: the material is out of range
template <int DIM, bool CONDENSE, bool TENSOR>
__device__ __forceinline__ bool err_load(int32_t t, const double *__restrict__ coords, const int32_t *__restrict__ conn, const int32_t *__restrict__ mat,
                                         const int32_t *__restrict__ eperm, const double *__restrict__ sigma, int n_mat, const int32_t *__restrict__ eldof,
                                         const double *__restrict__ C, const double *__restrict__ M, int k, const double *__restrict__ x, int col,
                                         const PointLoads &src, double *X, double *S, double (&xe)[P3<DIM>::NLD]) {
    constexpr int N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NK = (DIM == 2 && CONDENSE) ? 9 : N;
    const int32_t m = elem_material(mat, eperm, t, n_mat);
    if (m < 0) return false;
    load_vertices<DIM>(coords, conn, t, X);
    load_sigma<DIM, TENSOR>(sigma, m, S);
    gather_column<N, NK>(eldof + int64_t(t) * N, x, k, col, xe);
    if constexpr (DIM == 2 && CONDENSE) recover_bubble(t, C + int64_t(t) * NT, M, col, 0, src.nq, src.pt_rhs, src.pt_I, src.found, src.fint, xe);
    return true;
}

}  // namespace

// kp = 1 << kp_log2 lanes per element (>= k), 256 >> kp_log2 elements per workgroup
template <int DIM, bool CONDENSE, bool TENSOR>
__global__ void __launch_bounds__(256) k_error_facets(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                      const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm, const double *__restrict__ sigma,
                                                      int n_mat, const int32_t *__restrict__ eldof, const int32_t *__restrict__ adjptr,
                                                      const uint32_t *__restrict__ adj, const double *__restrict__ C, const double *__restrict__ M,
                                                      const double *__restrict__ rule, int k, const double *__restrict__ x, PointLoads src, int kp_log2,
                                                      double *__restrict__ eta2) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD, NS = TENSOR ? SigmaTensor<DIM>::N : 1, NTAB = ErrRule<DIM>::NTAB;
    constexpr int FD0 = (DIM == 3) ? 16 : 3, FDS = (DIM == 3) ? 1 : 2;   // local dof of facet f: FD0 + FDS * f
    __shared__ double s_rule[NTAB];
    __shared__ double s_out[256];
    const int tid = threadIdx.x, ppb = 256 >> kp_log2;
    if (tid < NTAB) s_rule[tid] = rule[tid];
    __syncthreads();
    const int c = tid & ((1 << kp_log2) - 1), pl = tid >> kp_log2;
    const int64_t t0 = int64_t(blockIdx.x) * ppb, t = t0 + pl;
    double eta = 0.0;
    if (t < nt && c < k) {
        double Xe[NB * DIM], Se[NS], xe[N];
        if (err_load<DIM, CONDENSE, TENSOR>(int32_t(t), coords, conn, mat, eperm, sigma, n_mat, eldof, C, M, k, x, c, src, Xe, Se, xe)) {
            double ge[DIM][DIM];
            const double vol = bary_gradients<DIM>(Xe, ge);
            if (vol > 0.0) {
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    const int32_t row = eldof[t * N + FD0 + FDS * f];
                    if (row < 0) continue;   // Dirichlet facet
                    const int32_t a0 = adjptr[row], cnt = adjptr[row + 1] - a0;
                    int64_t tn = -1;         // the other element of the facet's list, if there is one
                    if (cnt >= 2) {
                        const int64_t e0 = int64_t(adj[a0] >> 5), e1 = int64_t(adj[a0 + 1] >> 5);
                        tn = (e0 == t) ? e1 : e0;
                        if (tn < 0 || tn >= nt || tn == t) tn = -1;
                    }
                    double Xn[NB * DIM], Sn[NS], xn[N];
                    bool interior = false;
                    if (tn >= 0) {
                        if (!err_load<DIM, CONDENSE, TENSOR>(int32_t(tn), coords, conn, mat, eperm, sigma, n_mat, eldof, C, M, k, x, c, src, Xn, Sn, xn)) continue;
                        interior = true;
                    }
                    eta += error_facet<DIM, TENSOR>(s_rule, f, Xe, ge, vol, xe, Se, interior, Xn, xn, Sn);
                }
            }
        }
    }
    s_out[c * ppb + pl] = eta;
    __syncthreads();
    // stores along the elements: column cc of the workgroup's ppb elements is one run of ppb doubles
    const int cc = tid / ppb, q = tid - cc * ppb;
    if (cc < k && t0 + q < nt) eta2[int64_t(cc) * nt + t0 + q] = s_out[tid];
}

// tiles of 256 elements, grid-stride; a lane adds its elements in ascending order, then the fixed butterfly and the four waves in order
__global__ void __launch_bounds__(256) k_error_combine(int64_t nt, const double *__restrict__ eu, const double *__restrict__ el, double *__restrict__ ev,
                                                       double *__restrict__ part) {
    __shared__ double s_w[4];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t t = int64_t(blockIdx.x) * 256 + tid; t < nt; t += int64_t(gridDim.x) * 256) {
        const double v = 0.0 - sqrt(eu[t] * el[t]);
        if (ev) ev[t] = v;
        acc += v;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

const double *err_rule(int dim) { return dim == 2 ? kRule2 : kRule3; }

void launch_error_facets(const ElemMesh &em, const double *rule, int k, const double *x, const PointLoads &src, double *eta2, hipStream_t s) {
    if (em.nt <= 0 || k <= 0) return;
    int kp_log2 = 0;
    while ((1 << kp_log2) < k) ++kp_log2;
    const int ppb = 256 >> kp_log2;
    const unsigned grid = unsigned((em.nt + ppb - 1) / ppb);
    for_elem_kind(em.dim, em.condense, em.tensor(), [&](auto d, auto co, auto te) {
        hipLaunchKernelGGL((k_error_facets<decltype(d)::value, decltype(co)::value, decltype(te)::value>), dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn,
                           em.mat, em.eperm, em.sigma, em.n_mat, em.eldof, em.adjptr, em.adj, em.C, em.M, rule, k, x, src, kp_log2, eta2);
    });
}

void launch_error_combine(int64_t nt, const double *eu, const double *el, double *ev, double *part, hipStream_t s) {
    hipLaunchKernelGGL(k_error_combine, dim3(sens_grid(nt)), dim3(256), 0, s, nt, eu, el, ev, part);
}

}  // namespace remo
