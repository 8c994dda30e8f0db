// remo_host.cpp — the CPU hooks of include/remo3d_hip.h (remo_host_*): element matrices from the exact reference tensors, the
// host numbering, and the material-tensor check they share with batch creation.  No device code, no device calls.
#include <cmath>
#include <cstring>
#include <string>

#include "remo_internal.h"
#include "fem_p3.h"
#include "symbolic.h"
#include "sens.h"
#include "pairs.h"
#include "field.h"
#include "secondary.h"
#include "errest.h"

namespace remo {

// Symmetric positive definite (leading principal minors > 0) and finite: the upper triangle of one material's tensor.
bool tensor_ok(int dim, const double *S) {
    const int n = (dim == 2) ? 3 : 6;
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(S[i])) return false;
    if (dim == 2) return S[0] > 0.0 && S[0] * S[2] - S[1] * S[1] > 0.0;
    const double m2 = S[0] * S[3] - S[1] * S[1];
    const double m3 = S[0] * (S[3] * S[5] - S[4] * S[4]) - S[1] * (S[1] * S[5] - S[4] * S[2]) + S[2] * (S[1] * S[4] - S[3] * S[2]);
    return S[0] > 0.0 && m2 > 0.0 && m3 > 0.0 && std::isfinite(m3);
}

}  // namespace remo

using namespace remo;

// remo_host_secondary_element: the quadrature loop of k_sec_elements, point after point
template <int DIM>
static int secondary_element(const double *X, const double *sigma_tensor, double sigma, double sigma0, double radius, const double *src, int n, double *f) {
    constexpr int N = P3<DIM>::NLD, NS = SigmaTensor<DIM>::N;
    double g[DIM][DIM], D[NS], acc[N];
    const double vol = bary_gradients<DIM>(X, g);
    if (!(vol > 0.0)) return REMO_ERR_MESH;
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    if (sec_contrast<DIM>(sigma_tensor ? sigma_tensor : &sigma, sigma_tensor != nullptr, sigma0, D)) {
        const double rec[kSecSrc] = {src[0], src[1], DIM == 3 ? src[DIM - 1] : 0.0, 1.0 / (12.566370614359172953850573533118 * sigma0), sigma0};
        const std::vector<double> rule = sec_rule(DIM, n);
        for (size_t p = 0; p < rule.size(); p += DIM + 2) sec_point<DIM>(X, g, vol, D, &rule[p], rec, 1, radius, acc);
    }
    for (int i = 0; i < N; ++i) f[i] = acc[i];
    return REMO_OK;
}

// remo_host_error_facet: error_facet as k_error_facets calls it
template <int DIM, bool TENSOR>
static int error_facet_host(int f, const double *Xe, const double *Se, const double *xe, const double *Xn, const double *Sn, const double *xn, double *out) {
    double ge[DIM][DIM];
    const double vol = bary_gradients<DIM>(Xe, ge);
    if (!(vol > 0.0)) return REMO_ERR_MESH;
    if (Xn) {
        double gn[DIM][DIM];
        if (!(bary_gradients<DIM>(Xn, gn) > 0.0)) return REMO_ERR_MESH;
    }
    *out = error_facet<DIM, TENSOR>(err_rule(DIM), f, Xe, ge, vol, xe, Se, Xn != nullptr, Xn, xn, Sn);
    return REMO_OK;
}

// remo_host_pair_element: pair_moments of every column once, then pair_value per pair, as k_pair_contract stages them
template <int DIM>
static int pair_element_host(const double *X, const double *tab, bool tensor, int k, const double *x, int n_pair, const int32_t *pa, const int32_t *pb, double *out) {
    constexpr int N = P3<DIM>::NLD, NM = PairMom<DIM>::N, NS = SigmaTensor<DIM>::N;
    double g[DIM][DIM];
    const double vol = bary_gradients<DIM>(X, g);
    if (!(vol > 0.0)) return REMO_ERR_MESH;
    std::vector<double> mom(size_t(k) * NM);
    for (int c = 0; c < k; ++c) pair_moments<DIM>(X, g, tab, x + size_t(c) * N, &mom[size_t(c) * NM]);
    for (int p = 0; p < n_pair; ++p) {
        const double *ma = &mom[size_t(pa[p]) * NM], *mb = &mom[size_t(pb[p]) * NM];
        if (tensor) pair_value<DIM, true>(vol, g, ma, mb, out + size_t(p) * NS);
        else pair_value<DIM, false>(vol, g, ma, mb, out + p);
    }
    return REMO_OK;
}

extern "C" {

int remo_host_element_matrix(int32_t dim, const double *X, double sigma, double *K_out) {
    if ((dim != 2 && dim != 3) || !X || !K_out) return REMO_ERR_ARG;
    const double *M = ref_tables(dim);
    if (dim == 2) {
        double C[9];
        if (!metric_terms<2>(X, sigma, C)) return REMO_ERR_MESH;
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j < 10; ++j) K_out[i * 10 + j] = kentry<2>(C, M, i, j);
    } else {
        double C[6];
        if (!metric_terms<3>(X, sigma, C)) return REMO_ERR_MESH;
        for (int i = 0; i < 20; ++i)
            for (int j = 0; j < 20; ++j) K_out[i * 20 + j] = kentry<3>(C, M, i, j);
    }
    return REMO_OK;
}

int remo_host_element_matrix_tensor(int32_t dim, const double *X, const double *sigma_tensor, double *K_out) {
    if ((dim != 2 && dim != 3) || !X || !sigma_tensor || !K_out) return REMO_ERR_ARG;
    if (!tensor_ok(dim, sigma_tensor)) return REMO_ERR_ARG;
    const double *M = ref_tables(dim);
    if (dim == 2) {
        double C[9];
        if (!metric_terms_tensor<2>(X, sigma_tensor, C)) return REMO_ERR_MESH;
        for (int i = 0; i < 10; ++i)
            for (int j = 0; j < 10; ++j) K_out[i * 10 + j] = kentry<2>(C, M, i, j);
    } else {
        double C[6];
        if (!metric_terms_tensor<3>(X, sigma_tensor, C)) return REMO_ERR_MESH;
        for (int i = 0; i < 20; ++i)
            for (int j = 0; j < 20; ++j) K_out[i * 20 + j] = kentry<3>(C, M, i, j);
    }
    return REMO_OK;
}

int remo_host_sens_element(int32_t dim, const double *X, int32_t tensor, const double *xl, const double *xu, double *out) {
    if ((dim != 2 && dim != 3) || !X || !xl || !xu || !out) return REMO_ERR_ARG;
    bool ok;
    if (dim == 2) ok = tensor ? sens_element<2, true>(X, ref_tables(2), xl, xu, out) : sens_element<2, false>(X, ref_tables(2), xl, xu, out);
    else ok = tensor ? sens_element<3, true>(X, ref_factors3(), xl, xu, out) : sens_element<3, false>(X, ref_factors3(), xl, xu, out);
    return ok ? REMO_OK : REMO_ERR_MESH;
}

int remo_host_pair_element(int32_t dim, const double *X, int32_t tensor, int32_t k, const double *x, int32_t n_pair, const int32_t *pa, const int32_t *pb,
                           double *out) {
    if ((dim != 2 && dim != 3) || !X || !x || k < 1 || n_pair < 0 || (n_pair > 0 && (!pa || !pb || !out))) return REMO_ERR_ARG;
    for (int p = 0; p < n_pair; ++p)
        if (pa[p] < 0 || pa[p] >= k || pb[p] < 0 || pb[p] >= k) return REMO_ERR_ARG;
    return (dim == 2) ? pair_element_host<2>(X, ref_tables(2), tensor != 0, k, x, n_pair, pa, pb, out)
                      : pair_element_host<3>(X, ref_factors3(), tensor != 0, k, x, n_pair, pa, pb, out);
}

int remo_host_field_element(int32_t dim, const double *X, const double *sigma_tensor, double sigma, const double *x_e, const double *point, double *out) {
    if ((dim != 2 && dim != 3) || !X || !x_e || !point || !out) return REMO_ERR_ARG;
    if (sigma_tensor && !tensor_ok(dim, sigma_tensor)) return REMO_ERR_ARG;
    bool ok;
    if (dim == 2) ok = sigma_tensor ? field_point<2, true>(X, point, x_e, sigma_tensor, out) : field_point<2, false>(X, point, x_e, &sigma, out);
    else ok = sigma_tensor ? field_point<3, true>(X, point, x_e, sigma_tensor, out) : field_point<3, false>(X, point, x_e, &sigma, out);
    return ok ? REMO_OK : REMO_ERR_MESH;
}

int remo_host_point_shapes(int32_t dim, const double *X, const double *point, double *phi_out) {
    if ((dim != 2 && dim != 3) || !X || !point || !phi_out) return REMO_ERR_ARG;
    const bool ok = (dim == 2) ? point_shapes<2>(X, point, phi_out) : point_shapes<3>(X, point, phi_out);
    return ok ? REMO_OK : REMO_ERR_MESH;
}

int remo_host_secondary_element(int32_t dim, const double *X, const double *sigma_tensor, double sigma, double sigma0, double radius,
                                const double *src, int32_t n_quad, double *f_out) {
    if ((dim != 2 && dim != 3) || !X || !src || !f_out || n_quad < 0 || n_quad > kSecQuadMax) return REMO_ERR_ARG;
    if (!(sigma0 > 0.0) || !std::isfinite(sigma0) || !(radius >= 0.0)) return REMO_ERR_ARG;
    if (sigma_tensor && !tensor_ok(dim, sigma_tensor)) return REMO_ERR_ARG;
    const int n = n_quad > 0 ? n_quad : kSecQuadDefault;
    return dim == 2 ? secondary_element<2>(X, sigma_tensor, sigma, sigma0, radius, src, n, f_out)
                    : secondary_element<3>(X, sigma_tensor, sigma, sigma0, radius, src, n, f_out);
}

int remo_host_error_facet(int32_t dim, int32_t facet, const double *Xe, const double *sigma_tensor_e, double sigma_e, const double *x_e, const double *Xn,
                          const double *sigma_tensor_n, double sigma_n, const double *x_n, double *out) {
    if ((dim != 2 && dim != 3) || facet < 0 || facet > dim || !Xe || !x_e || !out || (Xn && !x_n)) return REMO_ERR_ARG;
    if (Xn && (sigma_tensor_e != nullptr) != (sigma_tensor_n != nullptr)) return REMO_ERR_ARG;
    if (sigma_tensor_e && (!tensor_ok(dim, sigma_tensor_e) || (Xn && !tensor_ok(dim, sigma_tensor_n)))) return REMO_ERR_ARG;
    const bool tensor = sigma_tensor_e != nullptr;
    const double *Se = tensor ? sigma_tensor_e : &sigma_e, *Sn = tensor ? sigma_tensor_n : &sigma_n;
    if (dim == 2) return tensor ? error_facet_host<2, true>(facet, Xe, Se, x_e, Xn, Sn, x_n, out) : error_facet_host<2, false>(facet, Xe, Se, x_e, Xn, Sn, x_n, out);
    return tensor ? error_facet_host<3, true>(facet, Xe, Se, x_e, Xn, Sn, x_n, out) : error_facet_host<3, false>(facet, Xe, Se, x_e, Xn, Sn, x_n, out);
}

double remo_host_factor_error(void) { return ref_factors3_error(); }

int remo_host_symbolic(const remo_mesh_t *mesh, int32_t condense, int64_t *sizes, int32_t *rowptr, int32_t *col, int32_t *freeid) {
    if (!mesh || !sizes) return REMO_ERR_ARG;
    Symbolic sy;
    std::string err;
    const int rc = build_symbolic(*mesh, condense != 0, true, sy, err);
    if (rc != REMO_OK) { g_create_error = err; return rc; }
    sizes[0] = sy.ndof; sizes[1] = sy.nfree; sizes[2] = sy.nnz; sizes[3] = sy.ne; sizes[4] = sy.nf; sizes[5] = sy.nld;
    if (rowptr) std::memcpy(rowptr, sy.rowptr.data(), sizeof(int32_t) * (sy.nfree + 1));
    if (col) std::memcpy(col, sy.col.data(), sizeof(int32_t) * sy.nnz);
    if (freeid) std::memcpy(freeid, sy.freeid.data(), sizeof(int32_t) * sy.ndof);
    return REMO_OK;
}

}  // extern "C"
