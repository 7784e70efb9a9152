// K20 -- second-order Moller-Plesset on the device: amplitudes, correlation energy and the unrelaxed one-particle density from the
// (ia|jb) blocks that dmk_ao2mo_s4 writes (rows (i, a), columns (j, b), unpacked).  Replaces PySCF's MP2 / the reference's UIMP2
// behind SCF.MP2 (solver/scf.py:1245-1264, solver/mp.py:33-95).
//
// mp2_amp_kernel    ONE fused elementwise pass per block: denominators (e_i + e_j) - (e_a + e_b), (anti)symmetrisation, the
//                   amplitudes in (i, j, a, b) order and the energy partial sum of every workgroup (grid-stride in a fixed grid, tree
//                   reduction in LDS; the partials are summed by one workgroup in a fixed order).
// densities         products over the amplitudes on dmk_dgemm_batched.  Each has M, N of a few hundred and K = o v^2 or o^2 v, which
//                   one launch would put on a handful of workgroups: K is cut along an OCCUPIED index into the batch (o slabs of
//                   K = v^2 or o v, at constant strides of the (i, j, a, b) array) and mp2_density_kernel sums the slabs in a fixed
//                   order while it symmetrises and adds the reference occupation.  No atomics anywhere.
#include "devres.h"
#include <algorithm>

namespace {

constexpr int NT = 256;
constexpr int AMP_GRID = 2048;

enum { AMP_RHF = 0, AMP_SAME = 1, AMP_OPP = 2 };

// V: (o1 v1) x (o2 v2).  t[i][j][a][b]; second output: AMP_RHF 2 t_ij^ab - t_ij^ba in the same order, AMP_OPP t transposed to [j][i][b][a]
template <int MODE>
__global__ __launch_bounds__(NT) void mp2_amp_kernel(int o1, int o2, int v1, int v2, const double *__restrict__ V,
                                                     const double *__restrict__ eo1, const double *__restrict__ ev1,
                                                     const double *__restrict__ eo2, const double *__restrict__ ev2,
                                                     double *__restrict__ t, double *__restrict__ t_other, double *__restrict__ partial) {
    __shared__ double red[NT];
    const long long vv = (long long)v1 * v2, ld = (long long)o2 * v2, total = (long long)o1 * o2 * vv;
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        const long long ij = e / vv, ab = e % vv;
        const int i = (int)(ij / o2), j = (int)(ij % o2), a = (int)(ab / v2), b = (int)(ab % v2);
        const double d = (eo1[i] + eo2[j]) - (ev1[a] + ev2[b]);
        const double w = V[((long long)i * v1 + a) * ld + (long long)j * v2 + b];
        if (MODE == AMP_OPP) {
            const double x = w / d;
            t[e] = x;
            t_other[(((long long)j * o1 + i) * v2 + b) * v1 + a] = x;
            s = fma(x, w, s);
        } else {
            const double wx = V[((long long)i * v1 + b) * ld + (long long)j * v2 + a];      // (ib|ja)
            if (MODE == AMP_RHF) {
                const double x = w / d, y = wx / d, tt = 2.0 * x - y;
                t[e] = x;
                t_other[e] = tt;
                s = fma(tt, w, s);
            } else {
                const double g = w - wx, x = g / d;
                t[e] = x;
                s = fma(0.25 * x, g, s);
            }
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// *out = sum of `count` partials, one workgroup, fixed order
__global__ __launch_bounds__(NT) void mp2_sum_kernel(int count, const double *__restrict__ partial, double *__restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int t = threadIdx.x; t < count; t += NT) s += partial[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// out[m][n] = diag delta_mn + c1 (S1[m][n] + sym1 S1[n][m]) + c2 S2[m][n],  S = sum_b P[b] in the order of b (a null P gives nothing)
__global__ void mp2_density_kernel(int d, double diag, double c1, int sym1, const double *__restrict__ P1, int nb1, double c2,
                                   const double *__restrict__ P2, int nb2, double *__restrict__ out) {
    const long long dd = (long long)d * d;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < dd; e += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(e / d), n = (int)(e % d);
        const long long et = (long long)n * d + m;
        double s1 = 0.0, s1t = 0.0, s2 = 0.0;
        for (int b = 0; b < nb1 && P1; ++b) { s1 += P1[b * dd + e]; s1t += P1[b * dd + et]; }
        for (int b = 0; b < nb2 && P2; ++b) s2 += P2[b * dd + e];
        out[e] = (m == n ? diag : 0.0) + c1 * (s1 + (sym1 ? s1t : 0.0)) + c2 * s2;
    }
}

// amplitudes t (o1, o2, v1, v2), t' likewise.  The three density products, each as o slabs of K with partials P[slab][d][d]:
//   OO1  P[j][i][i'] = sum_ab  t[i][j][a][b] t'[i'][j][a][b]            (o2 slabs, d = o1)
//   OO2  P[i][j][j'] = sum_ab  t[i][j][a][b] t'[i][j'][a][b]            (o1 slabs, d = o2)
//   VV2  P[i][b][b'] = sum_ja  t[i][j][a][b] t'[i][j][a][b']            (o1 slabs, d = v2)
enum { OO1, OO2, VV2 };
int density_product(dmk_ctx *ctx, int which, int o1, int o2, int v1, int v2, const double *t, const double *tp, double *P) {
    const long long vv = (long long)v1 * v2;
    if (which == OO1) return dmk_dgemm_batched(ctx, 0, 1, o1, o1, (int)vv, o2, 1.0, t, o2 * vv, vv, tp, o2 * vv, vv, 0.0, P, o1, (long long)o1 * o1);
    if (which == OO2) return dmk_dgemm_batched(ctx, 0, 1, o2, o2, (int)vv, o1, 1.0, t, vv, o2 * vv, tp, vv, o2 * vv, 0.0, P, o2, (long long)o2 * o2);
    return dmk_dgemm_batched(ctx, 1, 0, v2, v2, o2 * v1, o1, 1.0, t, v2, o2 * vv, tp, v2, o2 * vv, 0.0, P, v2, (long long)v2 * v2);
}

int density_out(dmk_ctx *ctx, int d, double diag, double c1, int sym1, const double *P1, int nb1, double c2, const double *P2, int nb2,
                double *out) {
    if (d <= 0) return DMK_OK;
    hipLaunchKernelGGL(mp2_density_kernel, dim3(std::max(1, dmk_grid1d((long long)d * d, 4096))), dim3(256), 0, ctx->stream, d, diag, c1, sym1, P1, nb1, c2, P2,
                       nb2, out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

template <int MODE>
int amp_launch(dmk_ctx *ctx, int o1, int o2, int v1, int v2, const double *V, const double *eo1, const double *ev1, const double *eo2,
               const double *ev2, double *t, double *t_other, double *partial) {
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(mp2_amp_kernel<MODE>, dim3(AMP_GRID), dim3(NT), 0, ctx->stream, o1, o2, v1, v2, V, eo1, ev1, eo2, ev2, t, t_other,
                       partial);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

}  // namespace

extern "C" {

int dmk_mp2_rhf(dmk_ctx *ctx, int nocc, int nvir, const double *ovov, const double *e_occ, const double *e_vir, double *e_corr_dev,
                double *doo, double *dvv, double *t2) {
    if (!ctx) return DMK_ERR_INVALID;
    if (nocc < 1 || nvir < 1 || !ovov || !e_occ || !e_vir || !e_corr_dev || !doo || !dvv)
        return dmk_fail(ctx, DMK_ERR_INVALID, "mp2_rhf: bad arguments (nocc, nvir >= 1; integrals, energies and outputs)");
    if ((long long)nocc * nvir * nvir > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "mp2_rhf: nocc nvir^2 beyond 2^31");
    const int o = nocc, v = nvir;
    const long long nt = (long long)o * o * v * v;
    double *t = nullptr, *tt = nullptr, *part = nullptr, *Poo = nullptr, *Pvv = nullptr;
    auto carve = [&](void *base) {
        Carver c(base);
        t = t2 ? t2 : c.take(nt);
        tt = c.take(nt); part = c.take(AMP_GRID); Poo = c.take((long long)o * o * o); Pvv = c.take((long long)o * v * v);
        return (size_t)(c.p - static_cast<char *>(base));
    };
    DevMem ws;
    const size_t bytes = carve(nullptr);
    if (ws.alloc(ctx, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "mp2_rhf: no device memory for a workspace of %zu bytes", bytes);
    }
    StreamDrain drain{ctx->stream};
    carve(ws.get<void>());
    int rc = amp_launch<AMP_RHF>(ctx, o, o, v, v, ovov, e_occ, e_vir, e_occ, e_vir, t, tt, part);
    if (rc) return rc;
    hipLaunchKernelGGL(mp2_sum_kernel, dim3(1), dim3(NT), 0, ctx->stream, AMP_GRID, part, e_corr_dev);
    DMK_CHECK_LAUNCH(ctx);
    // X_ij = sum_kab t_ik^ab t~_jk^ab ; Y_ab = sum_ijc t_ij^ac t~_ij^bc = sum_ijc t[i][j][c][a] t~[i][j][c][b] (t_ij^ab = t_ji^ba)
    if ((rc = density_product(ctx, OO1, o, o, v, v, t, tt, Poo))) return rc;
    if ((rc = density_product(ctx, VV2, o, o, v, v, t, tt, Pvv))) return rc;
    if ((rc = density_out(ctx, o, 2.0, -1.0, 1, Poo, o, 0.0, nullptr, 0, doo))) return rc;
    return density_out(ctx, v, 0.0, 1.0, 1, Pvv, o, 0.0, nullptr, 0, dvv);
}

int dmk_mp2_uhf(dmk_ctx *ctx, int nocc_a, int nvir_a, int nocc_b, int nvir_b, const double *ovov, const double *OVOV, const double *ovOV,
                const double *e_occ_a, const double *e_vir_a, const double *e_occ_b, const double *e_vir_b, double *e_corr_dev,
                double *doo_a, double *dvv_a, double *doo_b, double *dvv_b, double *t2aa, double *t2ab, double *t2bb) {
    if (!ctx) return DMK_ERR_INVALID;
    const int oa = nocc_a, va = nvir_a, ob = nocc_b, vb = nvir_b;
    if (oa < 1 || va < 1 || ob < 1 || vb < 1 || !ovov || !OVOV || !ovOV || !e_occ_a || !e_vir_a || !e_occ_b || !e_vir_b || !e_corr_dev ||
        !doo_a || !dvv_a || !doo_b || !dvv_b)
        return dmk_fail(ctx, DMK_ERR_INVALID, "mp2_uhf: bad arguments (nocc, nvir >= 1 per spin; integrals, energies and outputs)");
    const int om = std::max(oa, ob), vm = std::max(va, vb);
    if ((long long)om * vm * vm > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "mp2_uhf: nocc nvir^2 beyond 2^31");
    const long long naa = (long long)oa * oa * va * va, nbb = (long long)ob * ob * vb * vb, nab = (long long)oa * ob * va * vb;
    double *taa = nullptr, *tbb = nullptr, *tab = nullptr, *tba = nullptr, *part = nullptr;
    double *Poo_aa = nullptr, *Pvv_aa = nullptr, *Poo_bb = nullptr, *Pvv_bb = nullptr, *Poo_ab = nullptr, *Pvv_ab = nullptr,
           *Poo_ba = nullptr, *Pvv_ba = nullptr;
    auto carve = [&](void *base) {
        Carver c(base);
        taa = t2aa ? t2aa : c.take(naa);
        tbb = t2bb ? t2bb : c.take(nbb);
        tab = t2ab ? t2ab : c.take(nab);
        tba = c.take(nab);                      // t_ab as [J][i][B][a]
        part = c.take(3 * AMP_GRID);
        Poo_aa = c.take((long long)oa * oa * oa); Pvv_aa = c.take((long long)oa * va * va);
        Poo_bb = c.take((long long)ob * ob * ob); Pvv_bb = c.take((long long)ob * vb * vb);
        Poo_ab = c.take((long long)ob * oa * oa); Pvv_ab = c.take((long long)ob * va * va);      // alpha blocks from t_ab
        Poo_ba = c.take((long long)oa * ob * ob); Pvv_ba = c.take((long long)oa * vb * vb);      // beta blocks from t_ab
        return (size_t)(c.p - static_cast<char *>(base));
    };
    DevMem ws;
    const size_t bytes = carve(nullptr);
    if (ws.alloc(ctx, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "mp2_uhf: no device memory for a workspace of %zu bytes", bytes);
    }
    StreamDrain drain{ctx->stream};
    carve(ws.get<void>());
    int rc;
    if ((rc = amp_launch<AMP_SAME>(ctx, oa, oa, va, va, ovov, e_occ_a, e_vir_a, e_occ_a, e_vir_a, taa, nullptr, part))) return rc;
    if ((rc = amp_launch<AMP_SAME>(ctx, ob, ob, vb, vb, OVOV, e_occ_b, e_vir_b, e_occ_b, e_vir_b, tbb, nullptr, part + AMP_GRID))) return rc;
    if ((rc = amp_launch<AMP_OPP>(ctx, oa, ob, va, vb, ovOV, e_occ_a, e_vir_a, e_occ_b, e_vir_b, tab, tba, part + 2 * AMP_GRID))) return rc;
    hipLaunchKernelGGL(mp2_sum_kernel, dim3(1), dim3(NT), 0, ctx->stream, 3 * AMP_GRID, part, e_corr_dev);      // aa, then bb, then ab
    DMK_CHECK_LAUNCH(ctx);
    // same spin: sum_kab t_ik^ab t_jk^ab and sum_ijc t_ij^ca t_ij^cb (= sum_ijc t_ij^ac t_ij^bc: t_ij^ab = t_ji^ba exactly)
    if ((rc = density_product(ctx, OO1, oa, oa, va, va, taa, taa, Poo_aa))) return rc;
    if ((rc = density_product(ctx, VV2, oa, oa, va, va, taa, taa, Pvv_aa))) return rc;
    if ((rc = density_product(ctx, OO1, ob, ob, vb, vb, tbb, tbb, Poo_bb))) return rc;
    if ((rc = density_product(ctx, VV2, ob, ob, vb, vb, tbb, tbb, Pvv_bb))) return rc;
    // opposite spin: the alpha blocks contract J, a | B of t[i][J][a][B] -- OO1 of t, VV2 of its transpose; the beta blocks i, a
    if ((rc = density_product(ctx, OO1, oa, ob, va, vb, tab, tab, Poo_ab))) return rc;
    if ((rc = density_product(ctx, VV2, ob, oa, vb, va, tba, tba, Pvv_ab))) return rc;
    if ((rc = density_product(ctx, OO2, oa, ob, va, vb, tab, tab, Poo_ba))) return rc;
    if ((rc = density_product(ctx, VV2, oa, ob, va, vb, tab, tab, Pvv_ba))) return rc;
    if ((rc = density_out(ctx, oa, 1.0, -0.5, 0, Poo_aa, oa, -1.0, Poo_ab, ob, doo_a))) return rc;
    if ((rc = density_out(ctx, va, 0.0, 0.5, 0, Pvv_aa, oa, 1.0, Pvv_ab, ob, dvv_a))) return rc;
    if ((rc = density_out(ctx, ob, 1.0, -0.5, 0, Poo_bb, ob, -1.0, Poo_ba, oa, doo_b))) return rc;
    return density_out(ctx, vb, 0.0, 0.5, 0, Pvv_bb, ob, 1.0, Pvv_ba, oa, dvv_b);
}

}  // extern "C"
