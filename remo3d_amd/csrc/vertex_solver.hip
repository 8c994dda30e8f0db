// vertex_solver.hip — vertex_solver.h for gfx950: the Chebyshev kernels and their launcher, the set-up kernels of the block's images
// and the builder.  The multigrid cycle is amg.hip; the first Chebyshev step folded into the update launch is pcg_kernels.hip's.
#include "vertex_solver.h"

#include <limits.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "remo_internal.h"
#include "kutil.h"

namespace remo {

// One Chebyshev step on the vertex block, 8 lanes per row:
//   z += d;  res -= A_vv d;  d' = c1 d + c2 D^-1 res
// FIRST: z = 0, res = r, d = D^-1 r / theta are formed on the fly from the PCG residual (no set-up pass).  LAST = 1 (degree 1 only):
// z = d, nothing else.  LAST = 2: the polynomial's last term needs no product of its own (z_final = z + d + d'), so the launch that
// forms d' also finishes z and leaves the <r, z> partial sums for the PCG scalars: a polynomial of `degree` terms costs degree - 1 launches.
// TC = storage type of the chain (block values, Jacobi factors, directions, residual, running z): T, or float inside an fp64
// solve (large vertex blocks: the launches are HBM streams there, and a preconditioner may be applied inexactly - the
// recurrences of x and r never see it).  r (read) and the finished z (written for the direction kernel) stay in T.
// ELL: the first kEllWidth entries of a row come from the fixed-width image (ecol, eval; k_vblock_ell) and `rowptr` holds the
// begin / end PAIRS of the entries beyond them in (col, val).
template <class T, class TC, int K, bool FIRST, int LAST, bool ELL = false>
__global__ void __launch_bounds__(256) k_cheb_step(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const TC *__restrict__ val, const TC *__restrict__ dinv,
                                                   const TC *__restrict__ d_old, TC *__restrict__ d_new,
                                                   TC *__restrict__ zc, TC *__restrict__ res, T *__restrict__ z, double c1_, double c2_, double inv_theta_,
                                                   T *__restrict__ r, double *__restrict__ part, const double *__restrict__ scal, int commit, int step,
                                                   const int32_t *__restrict__ ecol = nullptr, const TC *__restrict__ eval = nullptr) {
    const TC c1 = TC(c1_), c2 = TC(c2_), inv_theta = TC(inv_theta_);
    constexpr int LPR = 8, RPB = 256 / LPR;
    constexpr bool SAME = sizeof(T) == sizeof(TC);
    static_assert(K <= LPR, "one column per lane after the transposing reduction");
    if (solve_done(scal, step)) return;
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    // the kernel is a chain of dependent round trips on a tiny block (launch-latency class): after the
    // transposing reduction lane `sub` owns column mycol of its row, so the vectors of the update are
    // requested per lane BEFORE the row is walked and need no round trip of their own
    int idx[K], own[K];
    towner_init<K, LPR>(idx, own, sub);
    const int mycol = idx[0];
    const bool mine = own[0] != 0;
    double dot = 0.0;
    for (int64_t row = int64_t(blockIdx.x) * RPB + grp; row < nv; row += int64_t(gridDim.x) * RPB) {
        constexpr int NE = ELL ? kEllWidth / LPR : 1;
        int32_t ej[NE];
        TC ev[NE];
        int32_t rs, re;
        if constexpr (ELL) {
            const int64_t eb = row * kEllWidth + sub;
#pragma unroll
            for (int u = 0; u < NE; ++u) { ej[u] = ecol[eb + u * LPR]; ev[u] = eval[eb + u * LPR]; }
            rs = rowptr[2 * row]; re = rowptr[2 * row + 1];
        } else {
            rs = rowptr[row]; re = rowptr[row + 1];
        }
        const int64_t at = row * K + mycol;
        TC di = TC(0), dold_in = TC(0), z_in = TC(0), res_in = TC(0);
        T rr = T(0);
        if (mine) {
            di = dinv[row];
            if (SAME && commit) {   // the update launch ran the FIRST step and left the new vertex residual in d_new (free until this
                rr = T(d_new[at]);  // launch writes it): r could not take it while the neighbours' rows were still gathering r
                r[at] = rr;
            } else {
                rr = r[at];
            }
            if (!FIRST) { dold_in = d_old[at]; z_in = zc[at]; res_in = res[at]; }
        }
        TC t[K];
#pragma unroll
        for (int c = 0; c < K; ++c) t[c] = TC(0);
        if constexpr (ELL) {
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int32_t j = ej[u];
                const TC v = FIRST ? ev[u] * dinv[j] * inv_theta : ev[u];
                if (FIRST) {
                    const T *dj = r + int64_t(j) * K;
#pragma unroll
                    for (int c = 0; c < K; ++c) t[c] += v * TC(dj[c]);
                } else {
                    const TC *dj = d_old + int64_t(j) * K;
#pragma unroll
                    for (int c = 0; c < K; ++c) t[c] += v * dj[c];
                }
            }
        }
        for (int32_t p = rs + sub; p < re; p += LPR) {
            const int32_t j = col[p];
            if (j >= nv) break;  // columns ascend: the vertex block leads the row
            const TC v = FIRST ? val[p] * dinv[j] * inv_theta : val[p];
            if (FIRST) {
                const T *dj = r + int64_t(j) * K;
#pragma unroll
                for (int c = 0; c < K; ++c) t[c] += v * TC(dj[c]);
            } else {
                const TC *dj = d_old + int64_t(j) * K;
#pragma unroll
                for (int c = 0; c < K; ++c) t[c] += v * dj[c];
            }
        }
        TReduce<K, LPR>::run(t, sub);
        if (mine) {
            const TC dold = FIRST ? di * TC(rr) * inv_theta : dold_in;
            TC zi = FIRST ? dold : z_in + dold;
            const TC ri = (FIRST ? TC(rr) : res_in) - t[0];
            const TC dn = c1 * dold + c2 * di * ri;
            if (LAST == 2) zi += dn;
            if (LAST) z[at] = T(zi / di);   // LAST: stored pre-divided by dinv so the direction kernel treats it like r
            else {
                zc[at] = zi;
                res[at] = ri;
                d_new[at] = dn;
            }
            if (LAST) dot += double(rr) * double(zi);
        }
    }
    if (LAST) {
        __shared__ double smem[16 * K];
        double dcol[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dcol[c] = (mine && c == mycol) ? dot : 0.0;
        block_sum<K>(dcol, smem);
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (threadIdx.x == c) part[blockIdx.x * K + c] = dcol[c];
    }
}

// Two Chebyshev (Richardson) factors per launch, 16 lanes per row of B's pattern.  State: z and w = D^-1 res.
//   t1 = A w, t2 = B w;   z += (a + b) w - a b D^-1 t1;   w' = w - (a + b) D^-1 t1 + a b D^-1 t2
// FIRST: z = 0, w = D^-1 r formed on the fly; LAST: z is stored divided by dinv (the direction kernel treats it like r) and the <r, z> partial sums are left.
template <class T, int K, int LPR, bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) k_cheb_pair(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                   const T *__restrict__ va, const T *__restrict__ vb, const T *__restrict__ dinv,
                                                   const T *__restrict__ w_old, T *__restrict__ w_new, T *__restrict__ z, double ab_sum_, double ab_prod_,
                                                   const T *__restrict__ r, double *__restrict__ part, const double *__restrict__ scal, int step) {
    constexpr int RPB = 256 / LPR, U = 2;
    static_assert(K <= LPR, "one column per lane after the transposing reduction");
    if (solve_done(scal, step)) return;
    const T ab_sum = T(ab_sum_), ab_prod = T(ab_prod_);
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    int idx[K], own[K];
    towner_init<K, LPR>(idx, own, sub);
    const int mycol = idx[0];
    const bool mine = own[0] != 0;
    double dot = 0.0;
    for (int64_t row = int64_t(blockIdx.x) * RPB + grp; row < nv; row += int64_t(gridDim.x) * RPB) {
        const int32_t rs = rowptr[row], re = rowptr[row + 1];
        const int64_t at = row * K + mycol;
        T di = T(0), wi = T(0), zi = T(0), rr = T(0);
        if (mine) {
            di = dinv[row];
            if (FIRST || LAST) rr = r[at];
            wi = FIRST ? di * rr : w_old[at];
            if (!FIRST) zi = z[at];
        }
        T t1[K], t2[K];
#pragma unroll
        for (int c = 0; c < K; ++c) { t1[c] = T(0); t2[c] = T(0); }
        for (int32_t p0 = rs + sub; p0 < re; p0 += U * LPR) {   // U passes of loads in flight, as in the SpMM
            int32_t j[U];
            T a[U], b[U], w[U][K];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int32_t p = p0 + u * LPR;
                j[u] = -1; a[u] = T(0); b[u] = T(0);
                if (p < re) { j[u] = col[p]; a[u] = va[p]; b[u] = vb[p]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int c = 0; c < K; ++c) w[u][c] = T(0);
                if (j[u] >= 0) {
                    const T *wj = (FIRST ? r : w_old) + int64_t(j[u]) * K;
                    const T dj = FIRST ? dinv[j[u]] : T(1);
#pragma unroll
                    for (int c = 0; c < K; ++c) w[u][c] = FIRST ? dj * wj[c] : wj[c];
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < K; ++c) { t1[c] += a[u] * w[u][c]; t2[c] += b[u] * w[u][c]; }
        }
        TReduce<K, LPR>::run(t1, sub);
        TReduce<K, LPR>::run(t2, sub);
        if (mine) {
            const T zn = zi + ab_sum * wi - ab_prod * di * t1[0];
            z[at] = LAST ? zn / di : zn;
            if (!LAST) w_new[at] = wi - ab_sum * di * t1[0] + ab_prod * di * t2[0];
            if (LAST) dot += double(rr) * double(zn);
        }
    }
    if (LAST) {
        __shared__ double smem[16 * K];
        double dcol[K];
#pragma unroll
        for (int c = 0; c < K; ++c) dcol[c] = (mine && c == mycol) ? dot : 0.0;
        block_sum<K>(dcol, smem);
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (threadIdx.x == c) part[blockIdx.x * K + c] = dcol[c];
    }
}

int cheb_grid(int64_t nv) { return nv <= 0 ? 0 : int(std::min<int64_t>((nv + 31) / 32, kMaxPartialBlocks / 2)); }

template <class T> void launch_vertex_solve(const VertexSolverT<T> &v, int k, int step, T *r, const T *dinv, double *rz0, int nb_vec, double *part_slot,
                                            hipStream_t s, bool first_done) {
    if (v.degree <= 0 || v.nv <= 0) return;
    double *part = part_slot + int64_t(nb_vec) * k;
    if (v.amg) {   // multigrid cycle instead of the polynomial (amg.hip)
        if constexpr (sizeof(T) == 8)
            if (v.amg32) return launch_amg_cycle<float, double>(*v.amg32, k, step, (const double *)r, v.z, part, cheb_grid(v.nv), (const double *)rz0, s);
        return launch_amg_cycle<T, T>(*v.amg, k, step, (const T *)r, v.z, part, cheb_grid(v.nv), (const double *)rz0, s);
    }
    const double theta = 0.5 * (v.lmax + v.lmin), delta = 0.5 * (v.lmax - v.lmin);
    if (vertex_paired(v)) {   // two Richardson factors of the Chebyshev polynomial per launch
        const int m = v.degree, np = m / 2;
        // 3D rows of B hold ~65 entries (32 lanes per row), 2D rows ~19 (8 lanes)
        const int g_last = cheb_grid(v.nv);
        for (int j = 0; j < np; ++j) {
            // roots of the shifted Chebyshev polynomial, paired from the two ends of the interval inwards
            const double r1 = theta - delta * cos(M_PI * (2.0 * (j + 1) - 1.0) / (2.0 * m));
            const double r2 = theta - delta * cos(M_PI * (2.0 * (m - j) - 1.0) / (2.0 * m));
            const double a = 1.0 / r1, bb = 1.0 / r2;
            const bool first = (j == 0), last = (j + 1 == np);
            // only the LAST launch leaves partial sums, so only it is tied to the cheb_grid slots
            auto grid_for = [&](int lpr) { int64_t gg = (v.nv + 256 / lpr - 1) / (256 / lpr); if (last && gg > g_last) gg = g_last; if (gg > 4096) gg = 4096; return int(gg); };
            auto for_lanes = [&](auto fn) {
                if (v.sq_lanes >= 32) fn(int_c<32>{});
                else if (v.sq_lanes >= 16) fn(int_c<16>{});
                else fn(int_c<8>{});
            };
            for_k(k, [&](auto kc) { for_lanes([&](auto lc) { for_bool(first, [&](auto fc) { for_bool(last, [&](auto ec) {
                constexpr int K = decltype(kc)::value, LPR = decltype(lc)::value;
                launch256(k_cheb_pair<T, K, LPR, decltype(fc)::value, decltype(ec)::value>, grid_for(LPR), s, v.nv, v.sq_rowptr, v.sq_col, v.sq_a,
                          v.sq_b, dinv, (const T *)v.d[j & 1], v.d[(j + 1) & 1], v.z, a + bb, a * bb, r, part, rz0, step);
            }); }); }); });
        }
        return;
    }
    const double inv_theta = 1.0 / theta;
    const int g = cheb_grid(v.nv);
    const int launches = v.degree > 1 ? v.degree - 1 : 1;   // the last term rides on the launch before it
    const bool chain32 = vertex_chain32(v, first_done), ell = vertex_ell(v, chain32);
    ChebStep cs{};
    for (int j = 0; j < launches; ++j) {
        cs = cheb_step(v, j == 0 ? nullptr : &cs);
        const bool first = (j == 0), last = (j + 1 == launches);
        if (first && first_done) continue;        // k_pcg_update_folded did it (with the coefficients of the same cheb_step)
        const int commit = (first_done && j == 1) ? 1 : 0;
        // only the launch that leaves partial sums is tied to the cheb_grid slots; the others take one row group per
        // workgroup slot (at 83 k vertices 512 workgroups walk five row groups each, a chain of five dependent round trips:
        // 17.9 us per launch under rocprofv3, profiles/r01_f_kernel_stats_sizeL_10depths_before_grid_fix.csv; after: 14.2 us, …_after_grid_fix.csv)
        const int64_t g_rows = (v.nv + 31) / 32;
        const int gl = last ? g : int(g_rows < 8192 ? g_rows : 8192);
        // k_cheb_step<.., FIRST, LAST, ELL> as the launches of a chain take it: (FIRST, LAST) = (1, 1) the only step of degree 1, (1, 2) the
        // only launch of a higher degree, (1, 0), (0, 2) and (0, 0) - there is no (0, 1)
        auto go = [&](auto fc, auto lc) {
            for_k(k, [&](auto kc) { for_bool(ell, [&](auto ec) {
                constexpr int K = decltype(kc)::value, LAST = decltype(lc)::value;
                constexpr bool FIRST = decltype(fc)::value, ELL = decltype(ec)::value;
                if (chain32)
                    launch256(k_cheb_step<T, float, K, FIRST, LAST, ELL>, gl, s, v.nv, ELL ? v.ell_tail : v.rowptr, v.col, v.val32, v.dinv32,
                              (const float *)v.d32[j & 1], v.d32[(j + 1) & 1], v.z32, v.res32, v.z, cs.c1, cs.c2, inv_theta, r, part, rz0, 0, step,
                              v.ell_col, v.ell_val32);
                else
                    launch256(k_cheb_step<T, T, K, FIRST, LAST, ELL>, gl, s, v.nv, ELL ? v.ell_tail : v.rowptr, v.col, v.val, dinv, (const T *)v.d[j & 1], v.d[(j + 1) & 1],
                              v.z, v.res, v.z, cs.c1, cs.c2, inv_theta, r, part, rz0, commit, step, v.ell_col, v.ell_val);
            }); });
        };
        if (first && last) { if (v.degree == 1) go(std::true_type{}, int_c<1>{}); else go(std::true_type{}, int_c<2>{}); }
        else if (first) go(std::true_type{}, int_c<0>{});
        else if (last) go(std::false_type{}, int_c<2>{});
        else go(std::false_type{}, int_c<0>{});
    }
}
template void launch_vertex_solve<double>(const VertexSolverT<double> &, int, int, double *, const double *, double *, int, double *, hipStream_t, bool);
template void launch_vertex_solve<float>(const VertexSolverT<float> &, int, int, float *, const float *, double *, int, double *, hipStream_t, bool);

// Gershgorin bound of the Jacobi-scaled vertex block: max_i dinv_i * sum_j |a_ij|, j < nv
__global__ void __launch_bounds__(256) k_vblock_bound(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                      const double *__restrict__ val, const double *__restrict__ dinv,
                                                      unsigned long long *out_bits) {
    double m = 0.0;
    for (int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; row < nv; row += int64_t(gridDim.x) * blockDim.x) {
        double s = 0.0;
        for (int32_t p = rowptr[row]; p < rowptr[row + 1]; ++p) {
            if (col[p] >= nv) break;
            s += fabs(val[p]);
        }
        m = fmax(m, s * dinv[row]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out_bits, (unsigned long long)__double_as_longlong(m));  // positive doubles order like their bits
}

void launch_vblock_bound(int64_t nv, const CsrView &A, const double *dinv, unsigned long long *out_bits, hipStream_t s) {
    const int64_t g = std::clamp<int64_t>((nv + 255) / 256, 1, 512);
    hipLaunchKernelGGL(k_vblock_bound, dim3(int(g)), dim3(256), 0, s, nv, A.rowptr, A.col, A.val, dinv, out_bits);
}

// Squared vertex block.  A Chebyshev step is a launch of ~5 us on a block of ~1e4 rows: pure launch latency, and there are 6 (3D) /
// 8 (2D) of them per PCG step.  Two consecutive Richardson factors of the same polynomial,
//   res'' = (I - b M)(I - a M) res = res - (a + b) M res + a b M^2 res,   M = A_vv D^-1,
// need M^2, i.e. B = A_vv D^-1 A_vv, once per matrix (a 2-hop pattern, ~65 entries per row in 3D): then ONE launch applies two
// factors, and the chain is half as long.  The polynomial is the same (product over the Chebyshev roots instead of the three-term
// recurrence), so the PCG iteration is unchanged up to rounding.  One wave per row: distinct 2-hop columns through an LDS hash set,
// sorted (bitonic, so that the result does not depend on the insertion order), values by sorted-row lookups in a fixed order: bit-reproducible.

template <int PASS>   // 0: count the distinct columns of every row; 1: fill (row offsets known)
__global__ void __launch_bounds__(256) k_vblock_square(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const double *__restrict__ val, const double *__restrict__ dinv,
                                                       int32_t *__restrict__ cnt, const int32_t *__restrict__ sq_rowptr,
                                                       int32_t *__restrict__ sq_col, double *__restrict__ sq_a, double *__restrict__ sq_b,
                                                       int64_t capacity, int32_t *flag) {
    __shared__ int32_t keys[4][kSquareSlots];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = int64_t(blockIdx.x) * 4 + wave;
    const bool active = row < nv;
    int32_t *K = keys[wave];
    for (int sl = lane; sl < kSquareSlots; sl += 64) K[sl] = INT_MAX;
    __syncthreads();
    int32_t rs = 0, re = 0;
    bool overflow = false;
    if (active) {
        rs = rowptr[row]; re = rowptr[row + 1];
        for (int32_t p = rs; p < re; ++p) {
            const int32_t k = col[p];
            if (k >= nv) break;                       // wave-uniform: the vertex block leads the row
            const int32_t ke = rowptr[k + 1];
            for (int32_t q = rowptr[k] + lane; q < ke; q += 64) {
                const int32_t j = col[q];
                if (j >= nv) break;
                uint32_t h = (uint32_t(j) * 2654435761u) >> 23;
                bool placed = false;
                for (int probe = 0; probe < kSquareSlots; ++probe) {
                    const int32_t old = atomicCAS(&K[h], INT_MAX, j);
                    if (old == INT_MAX || old == j) { placed = true; break; }
                    h = (h + 1) & (kSquareSlots - 1);
                }
                overflow |= !placed;
            }
        }
    }
    __syncthreads();
    int c = 0;
    for (int sl = lane; sl < kSquareSlots; sl += 64) c += K[sl] != INT_MAX;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (__builtin_amdgcn_ballot_w64(overflow) != 0 || c > kSquareSlots - 64) {   // keep the table sparse enough to probe quickly
        if (lane == 0) atomicOr(flag, 1);
        c = 0;
    }
    if (PASS == 0) {
        if (active && lane == 0) cnt[row] = c;
        return;
    }
    // bitonic sort of the table (empty slots = INT_MAX end up last); every wave sorts its own table, the
    // barriers keep the four waves of the block in step
    for (int size = 2; size <= kSquareSlots; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = lane; t < kSquareSlots / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const int32_t a = K[lo], b = K[hi];
                if ((a > b) == up) { K[lo] = b; K[hi] = a; }
            }
        }
    __syncthreads();
    if (!active || c == 0) return;
    const int64_t off = sq_rowptr[row];
    if (off + c > capacity) {
        if (lane == 0) atomicOr(flag, 2);
        return;
    }
    for (int t = lane; t < c; t += 64) {
        const int32_t j = K[t];
        double a = 0.0, b = 0.0;
        for (int32_t p = rs; p < re; ++p) {           // fixed order over the row's vertex entries
            const int32_t k = col[p];
            if (k >= nv) break;
            if (k == j) a = val[p];
            const int32_t ks = rowptr[k], ke = rowptr[k + 1];
            const int32_t q = lower_bound_i32(col, ks, ke, j);
            if (q < ke && col[q] == j) b += val[p] * dinv[k] * val[q];
        }
        sq_col[off + t] = j;
        sq_a[off + t] = a;
        sq_b[off + t] = b;
    }
}

// exclusive scan of cnt[0 .. n) into out[0 .. n]; one workgroup (n is the vertex count)
__global__ void __launch_bounds__(1024) k_scan_counts(int64_t n, const int32_t *__restrict__ cnt, int32_t *__restrict__ out) {
    __shared__ int64_t part[1024];
    const int64_t chunk = (n + 1023) / 1024;
    const int64_t b = int64_t(threadIdx.x) * chunk, e = (b + chunk < n) ? b + chunk : n;
    int64_t sum = 0;
    for (int64_t i = b; i < e; ++i) sum += cnt[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < 1024; ++t) { const int64_t v = part[t]; part[t] = run; run += v; }
        out[n] = int32_t(run < INT_MAX ? run : INT_MAX);
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = b; i < e; ++i) { out[i] = int32_t(run < INT_MAX ? run : INT_MAX); run += cnt[i]; }
}

void launch_vblock_square(int64_t nv, const CsrView &A, const double *dinv, int32_t *sq_rowptr, int32_t *sq_col, double *sq_a, double *sq_b,
                          int64_t capacity, int32_t *flag, hipStream_t s) {
    if (nv <= 0) return;
    const int g = int((nv + 3) / 4);
    int32_t *cnt = sq_col;   // the counts live in the (not yet used) column array: capacity >= nv is required by the caller
    hipLaunchKernelGGL((k_vblock_square<0>), dim3(g), dim3(256), 0, s, nv, A.rowptr, A.col, A.val, dinv, cnt, (const int32_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr, (double *)nullptr, capacity, flag);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, nv, cnt, sq_rowptr);
    hipLaunchKernelGGL((k_vblock_square<1>), dim3(g), dim3(256), 0, s, nv, A.rowptr, A.col, A.val, dinv, (int32_t *)nullptr, sq_rowptr, sq_col, sq_a, sq_b,
                       capacity, flag);
}

// compact copy of the vertex block: PASS 0 counts the leading entries (column < nv) of every vertex row, PASS 1 copies them
template <int PASS>
__global__ void __launch_bounds__(256) k_vblock_compact(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const double *__restrict__ val, int32_t *__restrict__ cnt,
                                                        const int32_t *__restrict__ vb_rowptr, int32_t *__restrict__ vb_col,
                                                        double *__restrict__ vb_val, int64_t capacity, int32_t *flag) {
    const int64_t row = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (row >= nv) return;
    const int32_t rs = rowptr[row], re = rowptr[row + 1];
    if (PASS == 0) {
        cnt[row] = lower_bound_i32(col, rs, re, int32_t(nv)) - rs;
    } else {
        const int32_t at = vb_rowptr[row], len = vb_rowptr[row + 1] - at;
        if (int64_t(at) + len > capacity) { if (len > 0) atomicOr(flag, 1); return; }
        for (int32_t e = 0; e < len; ++e) { vb_col[at + e] = col[rs + e]; vb_val[at + e] = val[rs + e]; }   // vertex rows are plain CSR
    }
}

void launch_vblock_compact(int64_t nv, const CsrView &A, int32_t *vb_rowptr, int32_t *vb_col, double *vb_val, int64_t capacity, int32_t *flag,
                           hipStream_t s) {
    if (nv <= 0) return;
    const int g = int((nv + 255) / 256);
    int32_t *cnt = vb_col;   // the counts live in the (not yet used) column array: capacity >= nv is required by the caller
    hipLaunchKernelGGL((k_vblock_compact<0>), dim3(g), dim3(256), 0, s, nv, A.rowptr, A.col, A.val, cnt, (const int32_t *)nullptr, (int32_t *)nullptr,
                       (double *)nullptr, capacity, flag);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, nv, cnt, vb_rowptr);
    hipLaunchKernelGGL((k_vblock_compact<1>), dim3(g), dim3(256), 0, s, nv, A.rowptr, A.col, A.val, (int32_t *)nullptr, vb_rowptr, vb_col, vb_val,
                       capacity, flag);
}

// Fixed-width image of the vertex block for the Chebyshev launches.  A launch on the CSR form is a chain of dependent round
// trips per row - row bounds, then columns and values (once per eight entries), then the gathered vector rows - on a block that
// lives in the caches: latency, not bytes.  Here the first kEllWidth entries of row i sit at [i][0 .. kEllWidth) (padded with
// (i, 0)), so a lane asks for all its columns and values at once, then for all the vector rows: two trips.  tail[i] = the
// begin / end of the row's remaining entries in the arrays the image was made from (equal: none - the usual case).
__global__ void __launch_bounds__(256) k_vblock_ell(int64_t nv, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                    const double *__restrict__ val, int32_t *__restrict__ ecol, int32_t *__restrict__ tail,
                                                    double *__restrict__ eval64, float *__restrict__ eval32) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= nv * kEllWidth) return;
    const int64_t row = i / kEllWidth;
    const int e = int(i - row * kEllWidth);
    const int32_t rs = rowptr[row], re = rowptr[row + 1];
    int32_t c = int32_t(row);
    double v = 0.0;
    if (rs + e < re) {
        const int32_t j = col[rs + e];
        if (j < nv) { c = j; v = val[rs + e]; }     // columns ascend: the vertex block leads a row of the whole matrix
    }
    ecol[i] = c;
    if (eval64) eval64[i] = v;
    if (eval32) eval32[i] = float(v);
    if (e == 0) {
        const int32_t end = lower_bound_i32(col, rs, re, int32_t(nv));
        const bool more = end - rs > kEllWidth;
        tail[2 * row] = more ? rs + kEllWidth : 0;
        tail[2 * row + 1] = more ? end : 0;
    }
}

void launch_vblock_ell(int64_t nv, const int32_t *rowptr, const int32_t *col, const double *val, int32_t *ecol, int32_t *tail, double *eval64,
                       float *eval32, hipStream_t s) {
    if (nv <= 0) return;
    hipLaunchKernelGGL(k_vblock_ell, dim3(int((nv * kEllWidth + 255) / 256)), dim3(256), 0, s, nv, rowptr, col, val, ecol, tail, eval64, eval32);
}

// ---- the builder.  Degree of the Chebyshev polynomial on the vertex block and the ratio lmax / lmin of its interval, from GPU scans
// (tools/scan_coarse2d.py, scan_coarse3d.py).
static std::pair<int, double> cheb_defaults(int dim, int64_t nvfree) {
    // 3D: the best degree / interval grow with the vertex count (kappa of the P1 block ~ nv^(2/3), degree ~ sqrt(kappa)): (5, 90) at
    // 12.6 k vertices, (8-10, 150-200) at 24 k, (12-16, 300-600) at 80 k; fine scan after the first / last step lost their launches
    // (tools/scan_coarse3d_fine.py): (5, 70-90) at 12.8 k, (8, 120-160) at 27 k (7: +3 %, 9: +4.5 %).  2D (launch-bound steps, paired Chebyshev launches): (16, 600).
    const double nv_rel = double(nvfree > 0 ? nvfree : 1) / 12600.0;
    // 2D, round 2 (tools/run_2d_batches.py at the 80 k vertices of config 2 with the 0.35 default mesh scale): (16, 600) 173 ms per four
    // batches, (24, 1200) 162, (32, 2400) 155, 752 / 561 / 446 steps - the product of degree and steps grows slowly, a launch pair costs
    // 14 us; (16, 600) was the optimum at 25 k vertices: degree ~ sqrt(vertices), ratio ~ vertices, even degrees (paired launches).
    // The paired (root-product) form must stay in fp64: in fp32 storage it needs MORE steps at degree 16 and breaks down above.
    const double nv2 = double(nvfree > 0 ? nvfree : 1) / 25000.0;
    const int deg2 = 2 * int(std::min(16.0, std::max(8.0, std::floor(8.0 * std::sqrt(nv2) + 0.5))));
    // round 3, size L with the patch operator (83 k vertices, tools/scan_coarse3d_fine.py L, profiles/r03_scan_coarse_L.log): steps per
    // four batches 675 / 637 / 638 / 630 / 601 at degrees 11 / 12 / 13 / 14 / 16 - an odd degree above 7 buys nothing over the even one
    // below it (M: 8 best, 7 and 9 worse) - solve 300 / 289 / 295 / 297 / 294 ms: even degrees from 8 up
    int deg3 = int(std::min(16.0, std::max(5.0, std::floor(5.0 * std::sqrt(nv_rel) + 0.9))));
    if (deg3 > 8) deg3 &= ~1;
    if (dim == 3) return {deg3, std::min(1200.0, std::max(60.0, 90.0 * std::pow(nv_rel, 2.0 / 3.0)))};
    return {deg2, std::min(2400.0, std::max(600.0, 600.0 * nv2 * 1.25))};
}

#ifdef REMO_PROBES
static bool amg_wants_image() { return g_tune.amg_image != 0; }   // key 45
#else
static constexpr bool amg_wants_image() { return true; }
#endif

constexpr int64_t kCompactPerRow = 48;   // capacity of the compact copy per vertex (3D P1 rows hold ~15 entries; a copy that does not fit is not used)

size_t VertexSolverBuilder::arena_bytes(int dim, int64_t nv, size_t kmax, bool want_amg, bool mixed) {
    size_t need = size_t(nv + 64) * 8 * 4 * kmax;                    // take: z, res, d[0], d[1]
    need += size_t(nv + 64) * 200 * 20 + size_t(nv + 64) * 8;        // enqueue: squared block (paired steps): sq_col, sq_a, sq_b; sq_rowptr
    need += size_t(nv + 64) * kCompactPerRow * 16 + size_t(nv + 64) * 8;   // enqueue: compact block (+ its fp32 values): col, val, val32 / to_float's; rowptr
    need += size_t(nv + 64) * kEllWidth * 12 + size_t(nv + 64) * 8;  // accept: its fixed-width image: ell_col, ell_val (or ell_val32); ell_tail
    need += size_t(nv + 64) * (4 * 4 * kmax + 8);                    // accept: fp32 chain of the fp64 solve: z32, res32, d32[0], d32[1]; dinv32
    if (want_amg) need += size_t(nv + 64) * (dim == 2 ? 1536 : 3072) * 2 + (1 << 20);   // accept: multigrid hierarchy of the block + its scratch (amg_setup, amg_to_float)
    if (want_amg && dim == 3) need += size_t(nv + 64) * kEllWidth * 16 + size_t(nv + 64) * 8;   // accept: image of its level 0 (amg_level0_image): columns, fp64 and fp32 values; tail
    if (mixed) need += size_t(nv + 64) * 200 * 8 + size_t(nv + 64) * 4 * 4 * kmax + (1 << 16);   // to_float: fp32 sq_a, sq_b; z, res, d[0], d[1]
    return need;
}

void VertexSolverBuilder::take(Arena &ar, const VertexSolverInput &in, VertexSolverT<double> &vs) {
    two_level = (in.o.preconditioner != 0) && in.nvfree > 0;
    vs.nv = two_level ? in.nvfree : 0;
    const auto [degree, ratio] = cheb_defaults(in.dim, in.nvfree);
    ratio_default = ratio;
    vs.degree = two_level ? (in.o.coarse_degree > 0 ? in.o.coarse_degree : degree) : 0;
    nc = size_t(vs.nv) * in.kmax + 2;
    vs.z = ar.lo<double>(nc); vs.res = ar.lo<double>(nc);
    vs.d[0] = ar.lo<double>(nc); vs.d[1] = ar.lo<double>(nc);
    d_bound = ar.lo<unsigned long long>(2);
}

void VertexSolverBuilder::enqueue(Arena &ar, hipStream_t s, const VertexSolverInput &in, const CsrView &A, const double *dinv, VertexSolverT<double> &vs) {
    // paired steps pay off where B stays small: 2D (~19 entries per row: 81 vs 93 us per PCG step); in 3D B has ~65
    // entries per row and three launches on it cost more than six on A_vv (153 vs 149 us) - forced by tune value 2
    want_square = two_level && !in.want_amg && (vs.degree % 2 == 0) && ((g_tune.square == 1 && in.dim == 2) || g_tune.square == 2);
    // compact copy of the vertex block for the Chebyshev launches (remo_debug_tune key 13: 0 = read A in place)
    // measured in the bench (--tune 13=0 against 13=1, one box): 538.9 -> 516.1 ms solve per step at 83 k vertices; at 12.8 k the
    // launches are latency, not bytes (714 -> 710 ms) and building the copy costs what it saves: larger blocks only (2 forces it)
    want_compact = !in.lite && two_level && !want_square && (g_tune.compact == 2 || (g_tune.compact == 1 && vs.nv > 16384));
    const int64_t nvc = vs.nv;
    auto read_back = [&](const int32_t *d_flag, const int32_t *rowptr, int32_t (&h)[2]) {
        HIP_TRY(hipMemcpyAsync(&h[0], d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(&h[1], rowptr + nvc, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    };
    if (two_level) {  // spectrum bound of the Jacobi-scaled vertex block for the Chebyshev interval
        HIP_TRY(hipMemsetAsync(d_bound, 0, sizeof(unsigned long long), s));
        launch_vblock_bound(nvc, A, dinv, d_bound, s);
        HIP_TRY(hipMemcpyAsync(&h_bound, d_bound, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    if (want_square) {   // B = A_vv D^-1 A_vv for the paired Chebyshev steps (k_cheb_pair); accept drops it if it overflowed
        const int64_t cap = nvc * 200;
        int32_t *rowptr = ar.lo<int32_t>(size_t(nvc) + 2), *col = ar.lo<int32_t>(size_t(cap));
        double *a = ar.lo<double>(size_t(cap)), *b = ar.lo<double>(size_t(cap));
        int32_t *d_flag = ar.lo<int32_t>(1);
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
        launch_vblock_square(nvc, A, dinv, rowptr, col, a, b, cap, d_flag, s);
        read_back(d_flag, rowptr, h_sq);
        vs.sq_rowptr = rowptr; vs.sq_col = col; vs.sq_a = a; vs.sq_b = b;
    }
    if (want_compact) {   // accept puts A's own arrays back if the copy did not fit
        const int64_t cap = (nvc + 64) * kCompactPerRow;
        int32_t *rowptr = ar.lo<int32_t>(size_t(nvc) + 2), *col = ar.lo<int32_t>(size_t(cap));
        double *val = ar.lo<double>(size_t(cap));
        int32_t *d_flag = ar.lo<int32_t>(1);
        HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), s));
        launch_vblock_compact(nvc, A, rowptr, col, val, cap, d_flag, s);
        read_back(d_flag, rowptr, h_vb);
        vs.rowptr = rowptr; vs.col = col; vs.val = val;
    }
}

int VertexSolverBuilder::accept(Arena &ar, hipStream_t s, const VertexSolverInput &in, const CsrView &A, const double *dinv, AmgT<double> &amg64,
                                AmgT<float> &amg32, VertexSolverT<double> &vs, int *coarse_used, std::string &why) {
    // the block the chain reads: the copy if it fits, else A's own arrays - in place or (only the P1 block was assembled) as the compact block they ARE
    const bool copied = want_compact && h_vb[0] == 0 && h_vb[1] > 0;
    if (two_level && !copied) { vs.rowptr = A.rowptr; vs.col = A.col; vs.val = A.val; }
    if (in.lite && two_level) { h_vb[0] = 0; h_vb[1] = int32_t(A.nnz); }
    vs.compact = copied || (in.lite && two_level);
    // fp32 chain inside the fp64 solve (remo_debug_tune key 15: 0 = off): more than 32 k vertex rows (no folded first step) and the compact block
    if (g_tune.chain32 && in.o.precision == 0 && vs.compact && (vs.nv > 32768 || g_tune.chain32 == 2)) {   // 2: forced (tests)
        float *v32c = ar.lo<float>(size_t(h_vb[1]) + 4), *d32c = ar.lo<float>(size_t(vs.nv) + 4);
        launch_to_float(h_vb[1], vs.val, v32c, s);
        launch_to_float(vs.nv, dinv, d32c, s);
        vs.val32 = v32c; vs.dinv32 = d32c;
        vs.z32 = ar.lo<float>(nc); vs.res32 = ar.lo<float>(nc);
        vs.d32[0] = ar.lo<float>(nc); vs.d32[1] = ar.lo<float>(nc);
    }
    // fixed-width image of the block for the polynomial's launches (k_vblock_ell; remo_debug_tune key 24: 0 = off)
    if (g_tune.ell && two_level && !in.want_amg && !want_square && in.dim == 3) {
        const size_t cells = size_t(vs.nv) * kEllWidth + 8;
        int32_t *ell_col = ar.lo<int32_t>(cells), *ell_tail = ar.lo<int32_t>(size_t(vs.nv) * 2 + 8);
        double *e64 = (in.o.precision == 0 && !vs.val32) ? ar.lo<double>(cells) : nullptr;
        float *e32 = (in.o.precision != 0 || vs.val32) ? ar.lo<float>(cells) : nullptr;
        launch_vblock_ell(vs.nv, vs.rowptr, vs.col, vs.val, ell_col, ell_tail, e64, e32, s);
        vs.ell_col = ell_col; vs.ell_tail = ell_tail; vs.ell_val = e64; vs.ell_val32 = e32;
    }
    if (two_level && in.want_amg) {   // multigrid cycle on the vertex block instead of the polynomial (amg.hip)
        std::string reason;
        if (amg_setup(ar, s, in.dim, vs.nv, A.rowptr, A.col, A.val, in.kmax, amg64, reason)) vs.amg = &amg64;
        else if (in.o.coarse == 2 || g_tune.amg == 2) { why = "multigrid hierarchy of the vertex block: " + reason; return REMO_ERR_NUMERIC; }
    }
    if (vs.amg && (in.o.precision == 1 || g_tune.amg32)) {   // fp32 image of the hierarchy: the mixed mode's inner solver, or the cycle of an fp64 solve
        amg_to_float(ar, s, amg64, in.kmax, amg32);
        amg32_ready = true;
        if (in.o.precision == 0) vs.amg32 = &amg32;
    }
    // fixed-width image of the hierarchy's level 0 for the cycle's last sweep (3D, like the polynomial's image): in the storage
    // type the cycle will run in - an fp64 solve whose cycle runs in fp32 needs no fp64 image, and the mixed mode cycles only the fp32
    // hierarchy (run_pcg_mixed takes the fp64 side for products and residuals alone); a hierarchy without an image walks its CSR rows
    if (vs.amg && in.dim == 3 && amg_wants_image()) amg_level0_image(ar, s, amg64, in.o.precision == 0 && !vs.amg32, amg32_ready ? &amg32 : nullptr);
    *coarse_used = !two_level ? 0 : (vs.amg ? 2 : 1);
    if (two_level) {
        double lmax;
        std::memcpy(&lmax, &h_bound, sizeof lmax);
        if (!(lmax > 0.0) || !std::isfinite(lmax)) { why = "vertex block has no positive spectrum bound"; return REMO_ERR_NUMERIC; }
        vs.lmax = lmax;
        vs.lmin = lmax / (in.o.coarse_ratio > 0 ? double(in.o.coarse_ratio) : ratio_default);
    }
    if (want_square && h_sq[0] != 0) vs.sq_rowptr = nullptr;   // a vertex of very high valence: the one-step launches stay
    if (vs.sq_rowptr) {
        const double avg = double(h_sq[1]) / double(vs.nv > 0 ? vs.nv : 1);
        vs.sq_lanes = g_tune.sq_lanes ? g_tune.sq_lanes : (avg > 40.0 ? 32 : (avg > 24.0 ? 16 : 8));   // 2D rows of B hold ~19 entries: 8 lanes (two passes in flight) 145 vs 150 ms with 16
    }
    return REMO_OK;
}

// (The answer of vertex_first_folds cannot differ between the two descriptions: it reads amg, degree, nv and sq_rowptr, and amg is
// set here exactly when it is there - a mixed run always has the hierarchy's fp32 image.)
VertexSolverT<float> VertexSolverBuilder::to_float(Arena &ar, hipStream_t s, const VertexSolverT<double> &vs, const float *val32, const AmgT<float> &amg32) const {
    VertexSolverT<float> f;
    f.nv = vs.nv; f.degree = vs.degree; f.lmax = vs.lmax; f.lmin = vs.lmin;
    f.z = ar.lo<float>(nc); f.res = ar.lo<float>(nc);
    f.d[0] = ar.lo<float>(nc); f.d[1] = ar.lo<float>(nc);
    if (vs.amg && amg32_ready) f.amg = &amg32;
    f.rowptr = vs.rowptr; f.col = vs.col; f.val = val32; f.compact = vs.compact;   // in place: the fp32 values of the whole matrix
    if (vs.compact) {
        float *vb32 = ar.lo<float>(size_t(h_vb[1]) + 1);
        launch_to_float(h_vb[1], vs.val, vb32, s);
        f.val = vb32;
    }
    f.ell_col = vs.ell_col; f.ell_tail = vs.ell_tail; f.ell_val = vs.ell_val32;
    if (vs.sq_rowptr) {
        float *a32 = ar.lo<float>(size_t(h_sq[1]) + 1), *b32 = ar.lo<float>(size_t(h_sq[1]) + 1);
        launch_to_float(h_sq[1], vs.sq_a, a32, s);
        launch_to_float(h_sq[1], vs.sq_b, b32, s);
        f.sq_rowptr = vs.sq_rowptr; f.sq_col = vs.sq_col; f.sq_a = a32; f.sq_b = b32; f.sq_lanes = vs.sq_lanes;
    }
    return f;
}

}  // namespace remo
