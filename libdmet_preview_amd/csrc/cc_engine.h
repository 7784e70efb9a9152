// What csrc/ccsd.hip (K21) and csrc/uccsd.hip (K24) share: ONE copy of the particle-particle ladder kernel, the permute kernels, the
// element-wise helpers, the contraction engine over index letters, what a handle is made of (Parts: the layout of an amplitude vector;
// Ring: a vector with its DIIS ring; Core: what dmk_rccsd and dmk_uccsd derive from, with the moves their entry points share) and the
// DIIS iteration over them.  Everything is in an unnamed namespace: each of the two files compiles its own instance.
#pragma once
#include "devres.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <string>

namespace {

constexpr int NT = 256, BM = 64, BN = 64, BK = 16, LDT = 81;
constexpr int DOT_GRID = 1024, DIIS_MAX = 12;

long long pair_of(long long k) { return k * (k + 1) / 2; }

// out[r][a][B] (+)= sum_{c,D} tau[r][c][D] W[pair(a,c)][pair(B,D)]: rows of W over va, columns over vb (the same-spin ladder: va = vb)
struct Ladder {
    long long m; int va, vb;
    const double *W; long long ld;
    const double *tau; double alpha, beta; double *out;
};

__global__ __launch_bounds__(NT) void cc_ladder_kernel(Ladder g) {
    __shared__ double As[2][BK][LDT], Bs[2][BK][LDT];
    const int va = g.va, vb = g.vb;
    const long long vv = (long long)va * vb;
    const int tilesN = (vb + BN - 1) / BN;
    const long long tilesM = (g.m + BM - 1) / BM;
    long long bid = blockIdx.x;
    const int tn = (int)(bid % tilesN); bid /= tilesN;
    const long long tm = bid % tilesM;
    const int a = (int)(bid / tilesM);
    const long long m0 = tm * BM;
    const int n0 = tn * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int c64 = tid & 63, k4 = tid >> 6;          // lanes along b: k = k4 + 4 j
    const int kg = tid & 15, mg = tid >> 4;           // lanes along k: row / column mg + 16 j
    const int nd = (vb + BK - 1) / BK;                // chunks of d per c
    const int nk = va * nd;

    double ra[4], rb[4];
    auto along_b = [&](int d0) { return d0 >= n0 + BN / 2; };
    auto load = [&](int t) {
        const int c = t / nd, d0 = (t - c * nd) * BK;
        const int hi = a > c ? a : c, lo = a > c ? c : a;
        const double *row = g.W + ((long long)hi * (hi + 1) / 2 + lo) * g.ld;
        const double *ta = g.tau + (long long)c * vb + d0 + kg;
        const bool ab = along_b(d0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long m = m0 + mg + 16 * j;
            ra[j] = (m < g.m && d0 + kg < vb) ? ta[m * vv] : 0.0;
            const int d = ab ? d0 + k4 + 4 * j : d0 + kg;
            const int b = ab ? n0 + c64 : n0 + mg + 16 * j;
            const int h = b > d ? b : d, l = b > d ? d : b;
            rb[j] = (b < vb && d < vb) ? row[(long long)h * (h + 1) / 2 + l] : 0.0;
        }
    };
    auto stage = [&](int buf, int t) {
        const int c = t / nd, d0 = (t - c * nd) * BK;
        const bool ab = along_b(d0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[buf][kg][mg + 16 * j] = ra[j];
            if (ab) Bs[buf][k4 + 4 * j][c64] = rb[j];
            else Bs[buf][kg][mg + 16 * j] = rb[j];
        }
    };

    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    load(0);
    stage(0, 0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) load(t + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            double fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = As[buf][4 * kk + q][wm + 16 * i + x];
                fb[i] = Bs[buf][4 * kk + q][wn + 16 * i + x];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nk) stage(buf ^ 1, t + 1);      // the other stage was last read before the previous barrier
        __syncthreads();
    }
    // D layout: row = (lane >> 4) + 4 r, column = lane & 15
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm + 16 * i + q + 4 * r;
                const int b = n0 + wn + 16 * j + x;
                if (m >= g.m || b >= vb) continue;
                double *p = g.out + m * vv + (long long)a * vb + b;
                const double s = g.alpha * acc[i][j][r];
                *p = g.beta != 0.0 ? s + g.beta * *p : s;
            }
}

int ladder_launch(dmk_ctx *ctx, const Ladder &g) {
    const long long tilesM = (g.m + BM - 1) / BM, tilesN = (g.vb + BN - 1) / BN;
    const long long blocks = tilesM * tilesN * g.va;
    if (blocks > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "cc_ladder_s4: a launch of %lld workgroups", blocks);
    FamScope fs(ctx, DMK_FAM_DGEMM);
    fs.mfma_flops(2.0 * BM * BN * BK * (double)g.va * ((g.vb + BK - 1) / BK) * (double)blocks);
    hipLaunchKernelGGL(cc_ladder_kernel, dim3((unsigned)blocks), dim3(NT), 0, ctx->stream, g);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// ---- permute-and-combine -------------------------------------------------------------------------------------------------------
// Source axes 0..3 (row-major, axis 3 fastest) of extents d[], each with the stride os[] it has in the destination.
struct PermLin { long long d[4], os[4]; };

__global__ __launch_bounds__(NT) void cc_perm_lin_kernel(long long total, PermLin p, double alpha, const double *__restrict__ in, double beta,
                                                         double *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        long long r = e;
        const long long i3 = r % p.d[3]; r /= p.d[3];
        const long long i2 = r % p.d[2]; r /= p.d[2];
        const long long i1 = r % p.d[1], i0 = r / p.d[1];
        double *q = out + i0 * p.os[0] + i1 * p.os[1] + i2 * p.os[2] + i3 * p.os[3];
        const double s = alpha * in[e];
        *q = beta != 0.0 ? s + beta * *q : s;
    }
}

// plane (x: fastest axis of the source, y: fastest axis of the destination), the other two axes r, s are the batch
struct PermTile { long long dx, dy, dr, ds, isy, isr, iss, osx, osr, oss; };

__global__ __launch_bounds__(NT) void cc_perm_tile_kernel(PermTile p, double alpha, const double *__restrict__ in, double beta,
                                                          double *__restrict__ out) {
    __shared__ double tile[32][33];
    const long long tcx = (p.dx + 31) / 32, tcy = (p.dy + 31) / 32;
    long long bid = blockIdx.x;
    const long long x0 = (bid % tcx) * 32; bid /= tcx;
    const long long y0 = (bid % tcy) * 32; bid /= tcy;
    const long long s = bid % p.ds, r = bid / p.ds;
    in += r * p.isr + s * p.iss;
    out += r * p.osr + s * p.oss;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long y = y0 + ty + 8 * k, xx = x0 + tx;
        if (y < p.dy && xx < p.dx) tile[ty + 8 * k][tx] = in[y * p.isy + xx];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long xx = x0 + ty + 8 * k, y = y0 + tx;
        if (y < p.dy && xx < p.dx) {
            double *q = out + xx * p.osx + y;
            const double w = alpha * tile[tx][ty + 8 * k];
            *q = beta != 0.0 ? w + beta * *q : w;
        }
    }
}

// ---- elementwise ---------------------------------------------------------------------------------------------------------------
// out[i][j][a][b] = c2 t2[i][j][a][b] + c1 ti[i][a] tj[j][b]; i < oi, j < oj, a < va, b < vb
__global__ __launch_bounds__(NT) void cc_tau_kernel(int oi, int oj, int va, int vb, double c2, double c1, const double *__restrict__ ti,
                                                    const double *__restrict__ tj, const double *__restrict__ t2, double *__restrict__ out) {
    const long long vv = (long long)va * vb, total = (long long)oi * oj * vv;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        const long long ij = e / vv, ab = e % vv;
        const int i = (int)(ij / oj), j = (int)(ij % oj), a = (int)(ab / vb), b = (int)(ab % vb);
        out[e] = c2 * t2[e] + c1 * ti[(long long)i * va + a] * tj[(long long)j * vb + b];
    }
}

// out = in / D: D_ia = ei_i - ea_a (two == 0, in (oi, va)) or D_ijab = ei_i + ej_j - ea_a - eb_b (in (oi, oj, va, vb))
struct Denoms { int oi, oj, va, vb; const double *ei, *ej, *ea, *eb; };
__global__ __launch_bounds__(NT) void cc_div_kernel(Denoms D, int two, const double *__restrict__ in, double *__restrict__ out) {
    const long long vv = two ? (long long)D.va * D.vb : D.va, total = (two ? (long long)D.oi * D.oj : D.oi) * vv;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        const long long ij = e / vv, ab = e % vv;
        double d;
        if (two) d = (D.ei[ij / D.oj] + D.ej[ij % D.oj]) - (D.ea[ab / D.vb] + D.eb[ab % D.vb]);
        else d = D.ei[ij] - D.ea[ab];
        out[e] = in[e] / d;
    }
}

// the Fock matrix (n x n) cut into f_oo and f_vv without their diagonals, f_ov, and the diagonals
__global__ __launch_bounds__(NT) void cc_fock_split_kernel(int o, int v, const double *__restrict__ f, double *__restrict__ foo,
                                                           double *__restrict__ fvv, double *__restrict__ fov, double *__restrict__ eo,
                                                           double *__restrict__ ev) {
    const int n = o + v;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < (long long)n * n; e += (long long)gridDim.x * NT) {
        const int p = (int)(e / n), q = (int)(e % n);
        const double x = f[e];
        if (p < o && q < o) { foo[(long long)p * o + q] = p == q ? 0.0 : x; if (p == q) eo[p] = x; }
        else if (p >= o && q >= o) { fvv[(long long)(p - o) * v + q - o] = p == q ? 0.0 : x; if (p == q) ev[p - o] = x; }
        else if (p < o) fov[(long long)p * v + q - o] = x;
    }
}

// partial[block] = sum x y over a fixed grid; then *out = (acc ? *out : 0) + scale sum partial, one workgroup, fixed order
__global__ __launch_bounds__(NT) void cc_dot_kernel(long long n, const double *__restrict__ x, const double *__restrict__ y,
                                                    double *__restrict__ partial) {
    __shared__ double red[NT];
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) s = fma(x[e], y[e], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(NT) void cc_sum_kernel(int count, const double *__restrict__ partial, double scale, int acc, double *__restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int t = threadIdx.x; t < count; t += NT) s += partial[t];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (acc ? *out : 0.0) + scale * red[0];
}

// out = sum_q c[q] x_q, x_q = base + q stride
struct LinComb { int m; double c[DIIS_MAX]; };
__global__ __launch_bounds__(NT) void cc_lincomb_kernel(long long n, LinComb L, const double *__restrict__ base, long long stride,
                                                        double *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        double s = 0.0;
        for (int q = 0; q < L.m; ++q) s = fma(L.c[q], base[q * stride + e], s);
        out[e] = s;
    }
}

int grid_of(long long n) { return std::max(1, dmk_grid1d(n, 4096)); }

// ---- the contraction engine ------------------------------------------------------------------------------------------------------
// Index letters: i j k l occupied, a b c d virtual; lower case: the first (alpha) pair of extents o, v; upper case I J K L / A B C D:
// the second (beta) pair O, V.  Tensors are row-major in the order of their letters.
struct Engine {
    dmk_ctx *ctx = nullptr;
    int o = 0, v = 0, O = 0, V = 0;
    double *PA = nullptr, *PB = nullptr, *PC = nullptr;      // scratch of `big` doubles each

    void extents(int oa, int va, int ob, int vb) { o = oa; v = va; O = ob; V = vb; }
    long long dim(char c) const { return c >= 'a' ? (c >= 'i' ? o : v) : (c >= 'I' ? O : V); }
    long long count(const std::string &s) const { long long n = 1; for (char c : s) n *= dim(c); return n; }

    // out (order so) = alpha in (order si) + beta out
    int perm(double alpha, const double *in, const char *si, double beta, double *out, const char *so) const {
        const int nd = (int)std::strlen(si), off = 4 - nd;
        if (nd < 1 || nd > 4 || (int)std::strlen(so) != nd) return dmk_fail(ctx, DMK_ERR_INVALID, "cc: permute '%s' -> '%s'", si, so);
        long long d[4] = {1, 1, 1, 1}, is[4] = {0, 0, 0, 0}, os[4] = {0, 0, 0, 0}, ost[4];
        for (int k = 0; k < nd; ++k) d[off + k] = dim(si[k]);
        is[3] = 1;
        for (int k = 2; k >= 0; --k) is[k] = is[k + 1] * d[k + 1];
        long long run = 1;
        for (int q = nd - 1; q >= 0; --q) { ost[q] = run; run *= dim(so[q]); }
        for (int k = 0; k < nd; ++k) {
            const char *w = std::strchr(so, si[k]);
            if (!w) return dmk_fail(ctx, DMK_ERR_INVALID, "cc: permute '%s' -> '%s'", si, so);
            os[off + k] = ost[w - so];
        }
        const long long total = d[0] * d[1] * d[2] * d[3];
        FamScope fs(ctx, DMK_FAM_MISC);
        if (os[3] == 1) {
            PermLin p;
            for (int k = 0; k < 4; ++k) { p.d[k] = d[k]; p.os[k] = os[k]; }
            hipLaunchKernelGGL(cc_perm_lin_kernel, dim3(grid_of(total)), dim3(NT), 0, ctx->stream, total, p, alpha, in, beta, out);
        } else {
            int y = -1, rs[2], nrs = 0;
            for (int k = 0; k < 3; ++k) { if (os[k] == 1 && d[k] > 1 && y < 0) y = k; }
            if (y < 0) for (int k = 0; k < 3; ++k) if (os[k] == 1 && y < 0) y = k;
            if (y < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "cc: permute '%s' -> '%s' has no unit stride", si, so);
            for (int k = 0; k < 3; ++k) if (k != y) rs[nrs++] = k;
            PermTile p{d[3], d[y], d[rs[0]], d[rs[1]], is[y], is[rs[0]], is[rs[1]], os[3], os[rs[0]], os[rs[1]]};
            const long long blocks = ((p.dx + 31) / 32) * ((p.dy + 31) / 32) * p.dr * p.ds;
            if (blocks > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "cc: a permute of %lld tiles", blocks);
            hipLaunchKernelGGL(cc_perm_tile_kernel, dim3((unsigned)blocks), dim3(NT), 0, ctx->stream, p, alpha, in, beta, out);
        }
        DMK_CHECK_LAUNCH(ctx);
        return DMK_OK;
    }

    // out = alpha in + beta out over n contiguous doubles
    int axpby(long long n, double alpha, const double *in, double beta, double *out) const {
        FamScope fs(ctx, DMK_FAM_MISC);
        const PermLin p{{1, 1, 1, n}, {0, 0, 0, 1}};
        hipLaunchKernelGGL(cc_perm_lin_kernel, dim3(grid_of(n)), dim3(NT), 0, ctx->stream, n, p, alpha, in, beta, out);
        DMK_CHECK_LAUNCH(ctx);
        return DMK_OK;
    }

    // C = alpha op(A) op(B) + beta C with M cut so that no launch exceeds the grid's second dimension
    int gemm(int opA, int opB, long long M, long long N, long long K, double alpha, const double *A, const double *B, double beta,
             double *C) const {
        if (N > 0x7fffffffLL || K > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "cc: a product of %lld x %lld x %lld", M, N, K);
        const long long lda = opA ? M : K, ldb = opB ? K : N, chunk = 32LL * 65535;
        for (long long m0 = 0; m0 < M; m0 += chunk) {
            const int mc = (int)std::min(chunk, M - m0);
            const int rc = dmk_dgemm_batched(ctx, opA, opB, mc, (int)N, (int)K, 1, alpha, A + (opA ? m0 : m0 * lda), lda, 0, B, ldb, 0, beta,
                                             C + m0 * N, N, 0);
            if (rc) return rc;
        }
        return DMK_OK;
    }

    // C[sc] = alpha sum_(letters shared by sa and sb) A[sa] B[sb] + beta C[sc]
    int contract(double alpha, const double *A, const char *sa, const double *B, const char *sb, double beta, double *C,
                 const char *sc) const {
        std::string FA, K, FB;
        for (const char *p = sa; *p; ++p) (std::strchr(sb, *p) ? K : FA) += *p;
        for (const char *p = sb; *p; ++p) if (!std::strchr(sa, *p)) FB += *p;
        int opA = 0, opB = 0, rc;
        if (FA + K == sa) opA = 0;
        else if (K + FA == sa) opA = 1;
        else { if ((rc = perm(1.0, A, sa, 0.0, PA, (FA + K).c_str()))) return rc; A = PA; }
        if (K + FB == sb) opB = 0;
        else if (FB + K == sb) opB = 1;
        else { if ((rc = perm(1.0, B, sb, 0.0, PB, (K + FB).c_str()))) return rc; B = PB; }
        const long long M = count(FA), N = count(FB), Kd = count(K);
        const std::string prod = FA + FB;
        if (prod == sc) return gemm(opA, opB, M, N, Kd, alpha, A, B, beta, C);
        if ((rc = gemm(opA, opB, M, N, Kd, alpha, A, B, 0.0, PC))) return rc;
        return perm(1.0, PC, prod.c_str(), beta, C, sc);
    }
};

long long pad32(long long k) { return (k + 31) / 32 * 32; }
// the largest tensor a contraction handles: two indices of one spin (oo, ov or vv) times two of the same or of the other spin, every
// product but vv x vv, which only the ladder kernel reads.  With (O, V) = (o, v): max(o^4, o^3 v, o^2 v^2, o v^3)
long long big_pair(long long o, long long v, long long O, long long V) {
    const long long p[3] = {o * o, o * v, v * v}, q[3] = {O * O, O * V, V * V};
    long long big = 0;
    for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y)
            if (x + y < 4) big = std::max(big, p[x] * q[y]);
    return big;
}
long long big_of(long long o, long long v, long long O, long long V) {
    return std::max(std::max(big_pair(o, v, o, v), big_pair(O, V, O, V)), big_pair(o, v, O, V));
}

// *out = (acc ? *out : 0) + scale sum x y; part: 2048 doubles of the caller
int cc_dot(dmk_ctx *ctx, double *part, long long n, const double *x, const double *y, double scale, int acc, double *out) {
    FamScope fs(ctx, DMK_FAM_MISC);
    const int grid = (int)std::min<long long>(DOT_GRID, (n + NT - 1) / NT);
    hipLaunchKernelGGL(cc_dot_kernel, dim3(grid), dim3(NT), 0, ctx->stream, n, x, y, part);
    hipLaunchKernelGGL(cc_sum_kernel, dim3(1), dim3(NT), 0, ctx->stream, grid, part, scale, acc, out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// ---- what the handles of ccsd.hip and uccsd.hip are made of ---------------------------------------------------------------------------
// The layout of an amplitude vector: np parts of cnt[] doubles at off[], every offset a multiple of 32 doubles, nx doubles in all.  The
// padding behind a part is zero in every vector; the last part is padded as well only where pad_last says so.
constexpr int PARTS_MAX = 5;
struct Parts {
    int np = 0;
    long long off[PARTS_MAX] = {0}, cnt[PARTS_MAX] = {0}, nx = 0;
    Parts() = default;
    Parts(std::initializer_list<long long> counts, bool pad_last) {
        for (long long c : counts) { off[np] = pad32(nx); cnt[np] = c; nx = off[np++] + c; }
        if (pad_last) nx = pad32(nx);
    }
};

// A vector under iteration: the current one, the one an update writes, and the DIIS ring of `diis` vectors and `diis` steps
struct Ring {
    double *x = nullptr, *xnew = nullptr, *ring_x = nullptr, *ring_e = nullptr;
    long long nx = 0;
    void carve(Carver &c, long long n, int diis) {
        nx = n;
        x = c.take(nx); xnew = c.take(nx);
        ring_x = reinterpret_cast<double *>(c.p);
        for (int q = 0; q < diis; ++q) c.take(nx);
        ring_e = reinterpret_cast<double *>(c.p);
        for (int q = 0; q < diis; ++q) c.take(nx);
    }
    long long ring_stride() const { return (long long)(dmk_align256((size_t)nx * 8) / 8); }
};

// What dmk_rccsd and dmk_uccsd derive from: the layout P of the vector, the T ring, the two allocations (mem: what the handle's
// carve() lays out; ws: the three scratch thirds of the engine), the reduction scratch and the records (rec[15]: E(MP2) of init).
struct Core {
    dmk_ctx *ctx = nullptr;
    int diis = 0;
    Parts P;
    DevMem mem, ws;
    Engine E;
    Ring T;
    double *part = nullptr, *rec = nullptr;
    bool have_amps = false;

    Core(dmk_ctx *c, int o, int v, int O, int V, int diis_dim) : ctx(c), diis(diis_dim) { E.ctx = c; E.extents(o, v, O, V); }
    // doubles of a tensor named by o v (alpha) and O V (beta) extents, "oOvV"
    long long ext(const char *t) const {
        long long n = 1;
        for (; *t; ++t) n *= *t == 'o' ? E.o : *t == 'O' ? E.O : *t == 'v' ? E.v : E.V;
        return n;
    }
    struct Slot { double **p; const char *t; };
    template <size_t N> void take(Carver &c, const Slot (&tab)[N]) { for (const Slot &e : tab) *e.p = c.take(ext(e.t)); }
    int64_t ws_bytes() const { return 3 * (int64_t)dmk_align256((size_t)big_of(E.o, E.v, E.O, E.V) * 8); }

    // `body`, then the stream is waited for
    template <class Body> int synced(Body body) {
        const int rc = body();
        if (rc) return rc;
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return DMK_OK;
    }
    // np device arrays into the parts of the vector `dst`, waited for; *have: there are amplitudes now
    int set(const double *const *src, double *dst, bool *have) {
        for (int p = 0; p < P.np; ++p) DMK_HIP(ctx, hipMemcpyAsync(dst + P.off[p], src[p], (size_t)P.cnt[p] * 8, hipMemcpyDeviceToDevice, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *have = true;
        return DMK_OK;
    }
    // np device arrays src[] of the parts' sizes out to dst[], not waited for
    int parts_out(const double *const *src, double *const *dst) {
        for (int p = 0; p < P.np; ++p) DMK_HIP(ctx, hipMemcpyAsync(dst[p], src[p], (size_t)P.cnt[p] * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return DMK_OK;
    }
    // part p of the vector `vec` (p == np: E(MP2)) out, waited for
    int get(const double *vec, int p, double *out) {
        const double *src = p < P.np ? vec + P.off[p] : rec + 15;
        DMK_HIP(ctx, hipMemcpyAsync(out, src, (size_t)(p < P.np ? P.cnt[p] : 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return DMK_OK;
    }
    // one application of `update(from, to)` to the vector of ring r, waited for
    template <class Update> int step(Ring &r, Update update) {
        const int rc = update(r.x, r.xnew);
        if (rc) return rc;
        std::swap(r.x, r.xnew);
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return DMK_OK;
    }
};

int cc_dot(Core *h, long long n, const double *x, const double *y, double scale, int acc, double *out) {
    return cc_dot(h->ctx, h->part, n, x, y, scale, acc, out);
}

// The common course of dmk_rccsd_create and dmk_uccsd_create over a fresh handle h (extents, layout and integrals set): both
// allocations, the carve, the scratch thirds, zeros, then `fill` (the Fock split and the arrays made from the integrals).  On failure
// the handle is deleted, after the stream has been waited for once work may be queued on it.
template <class H, class Fill> int cc_create(H *h, const char *who, Fill fill, H **out) {
    dmk_ctx *ctx = h->ctx;
    const int64_t bytes[2] = {(int64_t)h->carve(nullptr), h->ws_bytes()};
    if (h->mem.alloc(ctx, (size_t)bytes[0]) != hipSuccess || h->ws.alloc(ctx, (size_t)bytes[1]) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return dmk_fail(ctx, DMK_ERR_NOMEM, "%s: no device memory for %lld + %lld bytes", who, (long long)bytes[0], (long long)bytes[1]);
    }
    h->carve(h->mem.template get<void>());
    const size_t third = (size_t)bytes[1] / 3;
    h->E.PA = h->ws.template get<double>();
    h->E.PB = reinterpret_cast<double *>(h->ws.template get<char>() + third);
    h->E.PC = reinterpret_cast<double *>(h->ws.template get<char>() + 2 * third);
    auto fail = [&](int code) { (void)hipStreamSynchronize(ctx->stream); delete h; return code; };
    if (hipMemsetAsync(h->mem.template get<void>(), 0, (size_t)bytes[0], ctx->stream) != hipSuccess)
        return fail(dmk_fail(ctx, DMK_ERR_HIP, "%s: memset failed", who));
    const int rc = fill();
    if (rc) return fail(rc);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(dmk_fail(ctx, DMK_ERR_HIP, "%s: the stream failed", who));
    *out = h;
    return DMK_OK;
}

template <class H> int cc_free(H *h) {
    if (!h) return DMK_OK;
    (void)hipStreamSynchronize(h->ctx->stream);      // work that reads the handle's memory may still be queued
    delete h;
    return DMK_OK;
}

// The iteration of dmk_rccsd_run, dmk_rccsd_lambda_run and dmk_uccsd_run over a handle: `update(from, to)` on the vector of `ring`,
// DIIS over the ring with the steps new - old as error vectors, ONE record read back per iteration.
// energy(vec, e_dev): the T iteration (the energy of every new vector, |dE| < tol_e part of the test); energy == false: the test
// is |dx|_2 < tol_x alone.  step[]: where the step of each part is kept when there is no ring.
struct Iterate {
    Ring *ring;
    double *step[PARTS_MAX];
    bool energy;
    const char *who;
};

template <class Update, class Energy>
int cc_iterate(Core *h, const Iterate &s, int max_iter, double tol_e, double tol_x, Update update, Energy energy, double *result) {
    dmk_ctx *ctx = h->ctx;
    Ring &r = *s.ring;
    const Parts &P = h->P;
    int rc;
    const int dim = h->diis;
    const long long nx = P.nx, rs = r.ring_stride();
    double B[DIIS_MAX][DIIS_MAX] = {{0.0}}, rec[16], e_old, e = 0.0, dE = 0.0, dt = 0.0;
    if (s.energy) {
        if ((rc = energy(r.x, h->rec))) return rc;
        DMK_HIP(ctx, hipMemcpyAsync(rec, h->rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        e = rec[0];
    }
    int it = 0, converged = 0, stored = 0;
    while (it < max_iter) {
        ++it;
        const int slot = dim ? (stored % dim) : 0;
        double *dst = dim ? r.ring_x + slot * rs : r.xnew;
        double *ering = dim ? r.ring_e + slot * rs : nullptr;
        if ((rc = update(r.x, dst))) return rc;
        if (s.energy && (rc = energy(dst, h->rec))) return rc;
        // the step new - old: a ring slot, or step[], free between updates
        for (int p = 0; p < P.np; ++p) {
            double *ep = dim ? ering + P.off[p] : s.step[p];
            if ((rc = h->E.axpby(P.cnt[p], 1.0, dst + P.off[p], 0.0, ep))) return rc;
            if ((rc = h->E.axpby(P.cnt[p], -1.0, r.x + P.off[p], 1.0, ep))) return rc;
        }
        const int m = dim ? std::min(stored + 1, dim) : 1;
        if (dim) {
            for (int q = 0; q < m; ++q)
                if ((rc = cc_dot(h, nx, ering, r.ring_e + q * rs, 1.0, 0, h->rec + 1 + q))) return rc;
        } else {
            for (int p = 0; p < P.np; ++p)
                if ((rc = cc_dot(h, P.cnt[p], s.step[p], s.step[p], 1.0, p > 0, h->rec + 1))) return rc;
        }
        DMK_HIP(ctx, hipMemcpyAsync(rec, h->rec, (size_t)(1 + m) * 8, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        e_old = e;
        e = s.energy ? rec[0] : 0.0;
        dE = e - e_old;
        dt = std::sqrt(rec[1 + (dim ? slot : 0)]);
        if (!std::isfinite(e) || !std::isfinite(dt)) return dmk_fail(ctx, DMK_ERR_NOCONV, "%s: non-finite energy or amplitudes in iteration %d", s.who, it);
        if (std::fabs(dE) < tol_e && dt < tol_x) converged = 1;
        if (!dim || converged) {
            if (dim) DMK_HIP(ctx, hipMemcpyAsync(r.x, dst, (size_t)nx * 8, hipMemcpyDeviceToDevice, ctx->stream));
            else std::swap(r.x, r.xnew);
            if (converged) break;
            continue;
        }
        for (int q = 0; q < m; ++q) B[slot][q] = B[q][slot] = rec[1 + q];
        ++stored;
        double Bm[DIIS_MAX * DIIS_MAX];
        LinComb L{};
        L.m = m;
        for (int p = 0; p < m; ++p)
            for (int q = 0; q < m; ++q) Bm[p * m + q] = B[p][q];
        if (dmk_diis_coeffs(m, Bm, L.c) != DMK_OK) {          // no usable extrapolation: the newest vector
            for (int q = 0; q < m; ++q) L.c[q] = q == slot ? 1.0 : 0.0;
        }
        {
            FamScope fs(ctx, DMK_FAM_MISC);
            hipLaunchKernelGGL(cc_lincomb_kernel, dim3(grid_of(nx)), dim3(NT), 0, ctx->stream, nx, L, r.ring_x, rs, r.x);
            DMK_CHECK_LAUNCH(ctx);
        }
    }
    if (s.energy && dim && !converged && it > 0) {
        // left unconverged with a ring: *x is the extrapolated vector, not the update whose energy `e` is.  The energy reported
        // is the one of the amplitudes dmk_rccsd_get returns (dE stays the difference the convergence test saw)
        if ((rc = energy(r.x, h->rec))) return rc;
        DMK_HIP(ctx, hipMemcpyAsync(rec, h->rec, 8, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        e = rec[0];
    }
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    result[0] = e; result[1] = converged; result[2] = it; result[3] = dt; result[4] = dE;
    return DMK_OK;
}

}  // namespace
