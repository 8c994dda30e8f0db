// secondary.hip — load vector of the secondary-potential formulation (secondary.h) on gfx950, and the primary field at the
// evaluation points.  fp64 vector code.
//
// k_sec_elements: one wave per element.  The lanes share the element's quadrature points; every lane keeps the NLD partial sums of
// one column at a time in registers (all arrays are indexed by unrolled loops: nothing in scratch), a transposing wave reduction
// (wave_util.h) leaves each sum on one lane, which stores it.  k_sec_gather then adds, per row, the entries of the row's elements in
// ascending element order.  Both orders are fixed: two runs give the same bits.  Vertices and material come through elem_access.h; the
// conductivity is read with the run-time stride ncomp here (a scalar table is widened to a tensor), not through load_sigma.
// At the end of the file, the host side: what a job entry checks and resolves before any device work.
#include <limits.h>

#include <algorithm>
#include <cmath>

#include "elem_access.h"
#include "secondary.h"
#include "wave_util.h"
#include "remo_internal.h"

namespace remo {

// ---- the element rule ---------------------------------------------------------------------------------------------------------------
namespace {

// Gauss-Legendre nodes and weights on [0, 1] (Newton on P_n from the Chebyshev guess)
void gauss01(int n, std::vector<double> &x, std::vector<double> &w) {
    x.assign(size_t(n), 0.0); w.assign(size_t(n), 0.0);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n; ++i) {
        double z = std::cos(pi * (i + 0.75) / (n + 0.5)), dp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p0 = 1.0, p1 = z;
            for (int m = 2; m <= n; ++m) {
                const double p2 = ((2.0 * m - 1.0) * z * p1 - (m - 1.0) * p0) / m;
                p0 = p1; p1 = p2;
            }
            dp = n * (z * p1 - p0) / (z * z - 1.0);
            const double dz = p1 / dp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        {   // derivative at the converged node
            double p0 = 1.0, p1 = z;
            for (int m = 2; m <= n; ++m) {
                const double p2 = ((2.0 * m - 1.0) * z * p1 - (m - 1.0) * p0) / m;
                p0 = p1; p1 = p2;
            }
            dp = n * (z * p1 - p0) / (z * z - 1.0);
        }
        x[size_t(n - 1 - i)] = 0.5 * (z + 1.0);                       // ascending
        w[size_t(n - 1 - i)] = 1.0 / ((1.0 - z * z) * dp * dp);       // (2 / ((1 - z^2) P_n'^2)) / 2
    }
}

}  // namespace

std::vector<double> sec_rule(int dim, int n) {
    std::vector<double> x, w, rule;
    gauss01(n, x, w);
    for (int iu = 0; iu < n; ++iu)
        for (int iv = 0; iv < n; ++iv) {
            const double u = x[size_t(iu)], v = x[size_t(iv)];
            if (dim == 2) {
                const double l1 = u, l2 = v * (1.0 - u);
                rule.insert(rule.end(), {1.0 - l1 - l2, l1, l2, 2.0 * (1.0 - u) * w[size_t(iu)] * w[size_t(iv)]});
                continue;
            }
            for (int iw = 0; iw < n; ++iw) {
                const double t = x[size_t(iw)];
                const double l1 = u, l2 = v * (1.0 - u), l3 = t * (1.0 - u) * (1.0 - v);
                rule.insert(rule.end(), {1.0 - l1 - l2 - l3, l1, l2, l3,
                                         6.0 * (1.0 - u) * (1.0 - u) * (1.0 - v) * w[size_t(iu)] * w[size_t(iv)] * w[size_t(iw)]});
            }
        }
    return rule;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------
namespace {

// one thread per element: does it hold a source (k_locate's box slack and barycentric tolerance) while its conductivity differs
// from the sigma0 of that source's right-hand side?
template <int DIM>
__global__ void __launch_bounds__(256) k_sec_check(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                   const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm,
                                                   const double *__restrict__ sigma, int ncomp, int nmat, int ns,
                                                   const double *__restrict__ src, int32_t *errflag) {
    constexpr int NB = DIM + 1, NS = SigmaTensor<DIM>::N;
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    double X[NB * DIM], lo[DIM], hi[DIM];
    load_vertices<DIM>(coords, conn, t, X);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        lo[k] = X[k]; hi[k] = X[k];
#pragma unroll
        for (int a = 1; a < NB; ++a) { lo[k] = fmin(lo[k], X[a * DIM + k]); hi[k] = fmax(hi[k], X[a * DIM + k]); }
    }
    const int m = elem_material(mat, eperm, t, nmat);
    if (m < 0) return;   // (k_metric_terms reports it)
    double S[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = (i < ncomp) ? sigma[int64_t(m) * ncomp + i] : 0.0;
    for (int q = 0; q < ns; ++q) {
        const double *a = src + int64_t(q) * kSecSrc;
        bool in = true;
        double P[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            P[k] = a[k];
            const double ext = 1e-9 * (1.0 + hi[k] - lo[k]);
            if (P[k] < lo[k] - ext || P[k] > hi[k] + ext) in = false;
        }
        if (!in) continue;
        double l[NB], D[NS];
        if (!barycentrics<DIM>(X, P, l)) continue;
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (l[b] < -1e-10) in = false;
        if (in && sec_contrast<DIM>(S, ncomp > 1, a[4], D)) atomicOr(errflag, 4);
    }
}

template <int DIM, bool CONDENSE>
__global__ void __launch_bounds__(64) k_sec_elements(int64_t nt, const double *__restrict__ coords, const int32_t *__restrict__ conn,
                                                     const int32_t *__restrict__ mat, const int32_t *__restrict__ eperm,
                                                     const double *__restrict__ sigma, int ncomp, int nmat, const double *__restrict__ C,
                                                     const double *__restrict__ M, const double *__restrict__ rule, int nq,
                                                     const double *__restrict__ src, const int32_t *__restrict__ ptr, int k, double R,
                                                     double *__restrict__ fe, double *__restrict__ fbub) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD, NT = P3<DIM>::NTERM, NS = SigmaTensor<DIM>::N, NK = CONDENSE ? 9 : N;
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    if (t >= nt) return;
    double X[NB * DIM], g[DIM][DIM], S[NS];
    load_vertices<DIM>(coords, conn, t, X);
    const double vol = bary_gradients<DIM>(X, g);
    const int m = elem_material(mat, eperm, t, nmat);
    const bool ok = vol > 0.0 && m >= 0;   // (a degenerate element or a bad material is k_metric_terms' error)
#pragma unroll
    for (int i = 0; i < NS; ++i) S[i] = (ok && i < ncomp) ? sigma[int64_t(m) * ncomp + i] : 0.0;
    double fold[9];   // 2D condensed: K_j9 / K_99, what the bubble load takes from the outer rows (the unweighted recovery: recover_bubble, elem_access.h)
    if (CONDENSE) {
        const double *ce = C + t * NT;
        const double kbb = kentry<DIM>(ce, M, 9, 9);
#pragma unroll
        for (int j = 0; j < 9; ++j) fold[j] = ok ? kentry<DIM>(ce, M, 9, j) / kbb : 0.0;
    }
    int idx[N], own[N];
    towner_init<N, 64>(idx, own, lane);
    for (int c = 0; c < k; ++c) {
        const int s0 = ptr[c], ns = ptr[c + 1] - s0;
        double D[NS], acc[N];
#pragma unroll
        for (int i = 0; i < N; ++i) acc[i] = 0.0;
        const bool contributes = ok && ns > 0 && sec_contrast<DIM>(S, ncomp > 1, src[int64_t(s0) * kSecSrc + 4], D);   // wave-uniform
        if (contributes) {
            for (int p = lane; p < nq; p += 64) {
                double lw[NB + 1];
#pragma unroll
                for (int i = 0; i <= NB; ++i) lw[i] = rule[int64_t(p) * (NB + 1) + i];
                sec_point<DIM>(X, g, vol, D, lw, src + int64_t(s0) * kSecSrc, ns, R, acc);
            }
            if (CONDENSE) {   // f_j -= K_j9 f_9 / K_99, lane by lane (the fold is linear)
#pragma unroll
                for (int j = 0; j < 9; ++j) acc[j] -= fold[j] * acc[9];
            }
            TReduce<N, 64>::run(acc, lane);
        }
        // after the reduction lane `lane` holds the sum of entry idx[0] in acc[0] (one sum per lane: N <= 64)
        if (own[0]) {
            if (idx[0] < NK) fe[(t * N + idx[0]) * k + c] = acc[0];
            else if (CONDENSE) fbub[t * k + c] = acc[0];
        }
    }
}

template <int N>
__global__ void __launch_bounds__(256) k_sec_gather(int64_t n, int k, const int32_t *__restrict__ adjptr, const uint32_t *__restrict__ adj,
                                                    const double *__restrict__ fe, double *__restrict__ f) {
    const int64_t at = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (at >= n * k) return;
    const int64_t row = at / k;
    const int c = int(at - row * k);
    double s = 0.0;
    for (int32_t a = adjptr[row]; a < adjptr[row + 1]; ++a) {
        const uint32_t code = adj[a];
        s += fe[(int64_t(code >> 5) * N + int64_t(code & 31u)) * k + c];
    }
    f[at] = s;
}

template <int DIM>
__global__ void __launch_bounds__(64) k_sec_add_primary(int npts, const int32_t *__restrict__ pt_rhs, const double *__restrict__ pt_I,
                                                        const double *__restrict__ pp, int on_axis, const double *__restrict__ src,
                                                        const int32_t *__restrict__ ptr, double R, double *__restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npts || pt_I[q] != 0.0) return;   // sources read nothing
    double x[DIM], du[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) { x[k] = on_axis ? 0.0 : pp[int64_t(q) * DIM + k]; du[k] = 0.0; }
    if (on_axis) x[DIM - 1] = pp[q];
    const int c = pt_rhs[q];
    double up = 0.0;
    for (int s = ptr[c]; s < ptr[c + 1]; ++s) {
        double u = 0.0;
        sec_primary<DIM>(x, src + int64_t(s) * kSecSrc, R, u, du);
        up += src[int64_t(s) * kSecSrc + 3] * u;
    }
    out[q] += up;
}

}  // namespace

void launch_sec_check(const ElemMesh &em, int ns, const double *src, int32_t *errflag, hipStream_t s) {
    if (ns <= 0) return;
    const int grid = int((em.nt + 255) / 256);
    if (em.dim == 2)
        hipLaunchKernelGGL(k_sec_check<2>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.sigma_comp, em.n_mat, ns, src, errflag);
    else
        hipLaunchKernelGGL(k_sec_check<3>, dim3(grid), dim3(256), 0, s, em.nt, em.coords, em.conn, em.mat, em.eperm, em.sigma, em.sigma_comp, em.n_mat, ns, src, errflag);
}

void launch_sec_elements(const ElemMesh &em, const double *rule, int nq, const double *src, const int32_t *ptr, int k, double R, double *fe, double *fbub,
                         hipStream_t s) {
    for_elem_kind(em.dim, em.condense, [&](auto d, auto co) {
        hipLaunchKernelGGL((k_sec_elements<decltype(d)::value, decltype(co)::value>), dim3(unsigned(em.nt)), dim3(64), 0, s, em.nt, em.coords, em.conn, em.mat,
                           em.eperm, em.sigma, em.sigma_comp, em.n_mat, em.C, em.M, rule, nq, src, ptr, k, R, fe, fbub);
    });
}

void launch_sec_gather(int dim, int64_t n, int k, const int32_t *adjptr, const uint32_t *adj, const double *fe, double *f, hipStream_t s) {
    const int64_t grid = (n * k + 255) / 256;
    if (grid <= 0) return;
    if (dim == 3)
        hipLaunchKernelGGL(k_sec_gather<20>, dim3(unsigned(grid)), dim3(256), 0, s, n, k, adjptr, adj, fe, f);
    else
        hipLaunchKernelGGL(k_sec_gather<10>, dim3(unsigned(grid)), dim3(256), 0, s, n, k, adjptr, adj, fe, f);
}

void launch_sec_add_primary(int dim, int npts, const int32_t *pt_rhs, const double *pt_I, const double *pp, bool on_axis, const double *src,
                            const int32_t *ptr, double R, double *out, hipStream_t s) {
    if (npts <= 0) return;
    const int grid = (npts + 63) / 64;
    if (dim == 2)
        hipLaunchKernelGGL(k_sec_add_primary<2>, dim3(grid), dim3(64), 0, s, npts, pt_rhs, pt_I, pp, on_axis ? 1 : 0, src, ptr, R, out);
    else
        hipLaunchKernelGGL(k_sec_add_primary<3>, dim3(grid), dim3(64), 0, s, npts, pt_rhs, pt_I, pp, on_axis ? 1 : 0, src, ptr, R, out);
}

// ---- host: what the job entries check and resolve for remo_job_secondary_t.secondary, before any device work ------------------------------
// sigma0[n_rhs]: the job's values, or - where it gives none - the scalar conductivity of the element that holds the right-hand
// side's first source (lowest element number among several; all sources of the right-hand side must see that conductivity).
int resolve_secondary(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_secondary_t &x, const remo_opts_t *opts,
                      std::vector<double> &sigma0) {
    if (j.n_fun != 0 || j.n_group != 0 || j.warm || j.n_pts != 0 || j.n_frhs != 0)
        return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.secondary does not combine with functionals, groups, a warm object or field points");
    if (opts && opts->precision == 1)
        return fail(ctx, REMO_ERR_ARG, "the secondary formulation is fp64: remo_opts_t.precision = 1 (mixed) is not supported with remo_job_secondary_t.secondary");
    if (x.sec_quad < 0 || x.sec_quad > kSecQuadMax) return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.sec_quad must be in [0, 16]");
    if (!(x.sec_radius >= 0.0) || !std::isfinite(x.sec_radius)) return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.sec_radius must be finite and not negative");
    if (int rc = check_batch_args(ctx, mesh, j, true)) return rc;
    const int dim = mesh->dim, nb = dim + 1, ncomp = j.tensor ? ((dim == 2) ? 3 : 6) : 1;
    const int ns = j.src_ptr[j.n_rhs];
    if (dim == 2)
        for (int q = 0; q < ns; ++q)
            if (j.src_p[size_t(q) * 2] != 0.0) return fail(ctx, REMO_ERR_ARG, "secondary formulation in 2D: sources on the axis only (r == 0.0), no ring sources");
    sigma0.assign(size_t(j.n_rhs), 0.0);
    std::vector<int> pending;   // sources (I != 0) of the right-hand sides without a sigma0
    for (int r = 0; r < j.n_rhs; ++r) {
        const double s0 = x.sec_sigma0 ? x.sec_sigma0[r] : 0.0;
        if (s0 != 0.0) {
            if (!(s0 > 0.0) || !std::isfinite(s0)) return fail(ctx, REMO_ERR_ARG, "remo_job_secondary_t.sec_sigma0 must be positive and finite (0.0: the conductivity at the source)");
            sigma0[size_t(r)] = s0;
            continue;
        }
        for (int q = j.src_ptr[r]; q < j.src_ptr[r + 1]; ++q)
            if (j.src_I[q] != 0.0) pending.push_back(q);
    }
    if (pending.empty()) {
        for (double &v : sigma0) if (v == 0.0) v = 1.0;   // a right-hand side without sources: u_p = 0 whatever sigma0
        return REMO_OK;
    }
    std::vector<int64_t> elem(pending.size(), -1);
    for (int64_t t = 0; t < mesh->n_elems; ++t) {   // the tolerances of k_locate
        double X[12], lo[3], hi[3];
        bool good = true;
        for (int a = 0; a < nb && good; ++a) {
            const int64_t v = mesh->conn[t * nb + a];
            if (v < 0 || v >= mesh->n_nodes) { good = false; break; }
            for (int k = 0; k < dim; ++k) {
                const double c = mesh->coords[v * dim + k];
                X[a * dim + k] = c;
                lo[k] = a ? std::min(lo[k], c) : c; hi[k] = a ? std::max(hi[k], c) : c;
            }
        }
        if (!good) continue;   // (the numbering reports the bad index)
        for (size_t i = 0; i < pending.size(); ++i) {
            if (elem[i] >= 0) continue;
            const double *P = j.src_p + size_t(pending[i]) * dim;
            bool in = true;
            for (int k = 0; k < dim; ++k) {
                const double ext = 1e-9 * (1.0 + hi[k] - lo[k]);
                if (P[k] < lo[k] - ext || P[k] > hi[k] + ext) in = false;
            }
            if (!in) continue;
            double l[4];
            if (!(dim == 2 ? barycentrics<2>(X, P, l) : barycentrics<3>(X, P, l))) continue;
            for (int a = 0; a < nb; ++a)
                if (l[a] < -1e-10) in = false;
            if (in) elem[i] = t;
        }
    }
    for (size_t i = 0; i < pending.size(); ++i) {
        if (elem[i] < 0) return fail(ctx, REMO_ERR_POINT, "source outside the mesh");
        const int m = mesh->mat[elem[i]];
        if (m < 0 || m >= j.n_mat) return fail(ctx, REMO_ERR_MESH, "material index out of range");
        const double *S = j.sigma + size_t(m) * ncomp;
        if (j.tensor) {
            bool iso = S[0] == S[dim == 2 ? 2 : 3] && S[0] == S[ncomp - 1];
            for (int c = 0; c < ncomp; ++c)
                if (c != 0 && c != (dim == 2 ? 2 : 3) && c != ncomp - 1 && S[c] != 0.0) iso = false;
            if (!iso) return fail(ctx, REMO_ERR_ARG, "secondary formulation: the material at a source is anisotropic - give remo_job_secondary_t.sec_sigma0");
        }
        int r = 0;
        while (pending[i] >= j.src_ptr[r + 1]) ++r;
        if (sigma0[size_t(r)] == 0.0) sigma0[size_t(r)] = S[0];
        else if (sigma0[size_t(r)] != S[0])
            return fail(ctx, REMO_ERR_ARG, "secondary formulation: the sources of one right-hand side lie in materials of different conductivity - give remo_job_secondary_t.sec_sigma0");
    }
    for (double &v : sigma0) if (v == 0.0) v = 1.0;
    return REMO_OK;
}

void attach_secondary(remo_batch *b, const remo_job_secondary_t &x, std::vector<double> &sigma0) {
    b->secondary = true;
    b->sec_quad = x.sec_quad;
    b->sec_radius = x.sec_radius;
    b->sec_sigma0.swap(sigma0);
}

}  // namespace remo
