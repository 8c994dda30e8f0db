// secondary.h — secondary-potential formulation (remo_job_secondary_t.secondary; secondary.hip): the closed-form primary field of a point
// source and one quadrature point's share of an element's load vector, shared by host and gfx950 code.
//
// u = u_p + u_s.  u_p is the potential of the sources in a homogeneous medium sigma0 inside a grounded sphere of radius R centred
// at the origin of the batch frame (Kelvin image), u_s the finite-element solution of
//     a_Sigma(u_s, v) = - int (Sigma - sigma0 I) grad(u_p) . grad(v),    u_s = 0 on the Dirichlet boundary.
// The integrand vanishes where Sigma = sigma0 I - with sigma0 the conductivity at the source that is the neighbourhood of the
// source, so the elements never see the 1/r singularity.
//   G(x; a) = 1 / |x - a| - (R / |a|) / |x - a*|,  a* = R^2 a / |a|^2   (|a| <= 1e-9 R: the image term is -1 / R; R = 0: none)
//   u_p = I / (4 pi sigma0) G(x; a);  3D half ball: G(x; a) + G(x; a mirrored in y = 0), so that a source in the plane gives the
//   2 I of remo_solve_job's convention.  2D: sources on the axis only, the same formula in (r, z).
// Element rule: the collapsed (conical) Gauss-Legendre product rule, n points per direction on [0, 1]:
//   2D  l_1 = u, l_2 = v (1 - u),                        weight 2 (1 - u) w_u w_v
//   3D  l_1 = u, l_2 = v (1 - u), l_3 = w (1 - u)(1 - v), weight 6 (1 - u)^2 (1 - v) w_u w_v w_w
//   l_0 = 1 - the others, barycentrics of the SORTED vertices; point index (iu * n + iv) [* n + iw]; weights are fractions of |T|.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/remo3d_hip.h"
#include "elem_access.h"
#include "fem_p3.h"

namespace remo {

constexpr int kSecQuadDefault = 7;   // points per direction when remo_job_secondary_t.sec_quad = 0
constexpr int kSecQuadMax = 16;
constexpr int kSecSrc = 5;           // doubles of one source record (SecSources::src): x, y, z (2D: r, z, unused), I / (4 pi sigma0), sigma0

// G(x; a) and its gradient, ADDED to G / dG
template <int DIM> REMO_HD void sec_green(const double *x, const double *a, double R, double &G, double *dG) {
    double d[DIM], r2 = 0.0, a2 = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) { d[k] = x[k] - a[k]; r2 += d[k] * d[k]; a2 += a[k] * a[k]; }
    const double inv = 1.0 / sqrt(r2), inv3 = inv / r2;
    G += inv;
#pragma unroll
    for (int k = 0; k < DIM; ++k) dG[k] -= d[k] * inv3;
    if (!(R > 0.0)) return;
    const double an = sqrt(a2);
    if (an <= 1e-9 * R) { G -= 1.0 / R; return; }
    const double s = R * R / a2, q = R / an;
    double e2 = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) { d[k] = x[k] - s * a[k]; e2 += d[k] * d[k]; }
    const double jnv = 1.0 / sqrt(e2), jnv3 = jnv / e2;
    G -= q * jnv;
#pragma unroll
    for (int k = 0; k < DIM; ++k) dG[k] += q * d[k] * jnv3;
}

// u_p / (I / (4 pi sigma0)) of one source at a and its gradient, ADDED to u / du (3D: the source and its mirror image in y = 0)
template <int DIM> REMO_HD void sec_primary(const double *x, const double *a, double R, double &u, double *du) {
    sec_green<DIM>(x, a, R, u, du);
    if (DIM == 3) {
        const double m[3] = {a[0], -a[1], a[DIM - 1]};
        sec_green<DIM>(x, m, R, u, du);
    }
}

// D = Sigma_e - sigma0 I in the SigmaTensor layout; false when it vanishes (the element adds nothing to the load)
template <int DIM> REMO_HD bool sec_contrast(const double *S, bool tensor, double sigma0, double *D) {
    constexpr int NS = SigmaTensor<DIM>::N;
    if (tensor) {
#pragma unroll
        for (int i = 0; i < NS; ++i) D[i] = S[i];
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) D[i] = 0.0;
        D[0] = S[0]; D[DIM == 2 ? 2 : 3] = S[0]; D[NS - 1] = S[0];
    }
    D[0] -= sigma0; D[DIM == 2 ? 2 : 3] -= sigma0;
    if (DIM == 3) D[NS - 1] -= sigma0;
    bool any = false;
#pragma unroll
    for (int i = 0; i < NS; ++i) any = any || (D[i] != 0.0);
    return any;
}

// One quadrature point's share of f_e: acc[i] -= w |T| (2 pi r) grad(phi_i)^T D grad(u_p), u_p summed over the ns sources src
// (records of kSecSrc doubles).  X: sorted vertices, g: bary_gradients, lw: l[DIM+1] and the weight.
template <int DIM> REMO_HD void sec_point(const double *X, const double (*g)[DIM], double vol, const double *D, const double *lw,
                                          const double *src, int ns, double R, double *acc) {
    constexpr int NB = DIM + 1, N = P3<DIM>::NLD;
    double x[DIM], du[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < NB; ++a) s += lw[a] * X[a * DIM + k];
        x[k] = s; du[k] = 0.0;
    }
    for (int s = 0; s < ns; ++s) {
        double u = 0.0, dg[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) dg[k] = 0.0;
        sec_primary<DIM>(x, src + s * kSecSrc, R, u, dg);
        const double amp = src[s * kSecSrc + 3];
#pragma unroll
        for (int k = 0; k < DIM; ++k) du[k] += amp * dg[k];
    }
    double wt = -lw[NB] * vol;
    if (DIM == 2) wt *= 6.283185307179586476925286766559 * x[0];
    double v[DIM];
    if (DIM == 2) {
        v[0] = wt * (D[0] * du[0] + D[1] * du[1]);
        v[1] = wt * (D[1] * du[0] + D[2] * du[1]);
    } else {
        v[0] = wt * (D[0] * du[0] + D[1] * du[1] + D[2] * du[DIM - 1]);
        v[1] = wt * (D[1] * du[0] + D[3] * du[1] + D[4] * du[DIM - 1]);
        v[DIM - 1] = wt * (D[2] * du[0] + D[4] * du[1] + D[5] * du[DIM - 1]);
    }
    double t[NB], gp[N];
    t[0] = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) s += g[a][k] * v[k];
        t[a + 1] = s;
        t[0] -= s;
    }
    grad_shape<DIM>(lw, t, gp);
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += gp[i];
}

// ---- host: the element rule, the source records of a batch, the launchers (secondary.hip) -----------------------------------------
// rule[nq][DIM + 2]: barycentrics l_0 .. l_DIM and the weight; nq = n^DIM
std::vector<double> sec_rule(int dim, int n);

// the sources of every chunk of right-hand sides, column by column: ptr[chunk * (REMO_MAX_RHS + 1) + c] .. [.. + c + 1] are the
// records of column c of the chunk (zero strengths left out)
struct SecSources {
    std::vector<double> src;     // [ns][kSecSrc]
    std::vector<int32_t> ptr;    // [chunks][REMO_MAX_RHS + 1]
    int n() const { return int(src.size() / kSecSrc); }
};

// a contributing element (Sigma_e != sigma0 I) that holds a source within k_locate's tolerance raises bit 4 of *errflag
void launch_sec_check(const ElemMesh &em, int ns, const double *src, int32_t *errflag, hipStream_t s);
// element vectors fe[nt][NLD][k] of one chunk (zeros where Sigma_e = sigma0 I; 2D condensed: the bubble load folded into the nine
// outer entries as k_build_rhs folds a point source's, and kept in fbub[nt][k]), one wave per element
void launch_sec_elements(const ElemMesh &em, const double *rule, int nq, const double *src, const int32_t *ptr, int k, double R, double *fe, double *fbub,
                         hipStream_t s);
// f[row][c] = the sum of the row's element entries in ascending element order (DeviceSymbolic::adj): no atomics, a fixed order
void launch_sec_gather(int dim, int64_t n, int k, const int32_t *adjptr, const uint32_t *adj, const double *fe, double *f, hipStream_t s);
// out[q] += u_p(point q) for the points that are no sources; pp: z per point (on_axis) or dim coordinates
void launch_sec_add_primary(int dim, int npts, const int32_t *pt_rhs, const double *pt_I, const double *pp, bool on_axis, const double *src,
                            const int32_t *ptr, double R, double *out, hipStream_t s);

// ---- host: the job entries (remo_api.hip), before any device work ------------------------------------------------------------------
// Checks the members of x and the batch's own arguments (check_batch_args, points as full coordinates) and resolves sigma0[n_rhs]:
// the job's values, or the scalar conductivity of the element that holds the right-hand side's first source.  opts may be NULL.
int resolve_secondary(remo_ctx_t *ctx, const remo_mesh_t *mesh, const remo_job_t &j, const remo_job_secondary_t &x, const remo_opts_t *opts,
                      std::vector<double> &sigma0);
// marks the batch for the formulation and hands it sigma0 (swapped out of the argument)
void attach_secondary(remo_batch_t *b, const remo_job_secondary_t &x, std::vector<double> &sigma0);

}  // namespace remo
