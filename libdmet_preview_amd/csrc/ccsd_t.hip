// K22 -- the perturbative triples (T) of restricted CCSD on the device, over a dmk_rccsd handle (csrc/ccsd.hip, K21): PySCF's closed-shell
// ccsd_t with Fock-DIAGONAL denominators and the f_ov term kept.  Replaces self.cisolver.ccsd_t(eris=eris) behind the reference's
// CCSD.run (solver/cc.py:1073-1076).  The equations are stated in DESIGN.md K22; in short, for every UNIQUE triple a >= b >= c
//     w_ijk^abc = sum_f (ia|bf) t_kj^cf - sum_m (ia|jm) t_mk^bc,      W = the six simultaneous permutations of (i,a), (j,b), (k,c) of w,
//     Y^abc     = sum_ijk r3(W)_ijk (W_ijk + 1/2 P6[(ia|jb) t_kc + t_ij^ab f_kc]) / D_ijk,     E_(T) = sum mult(abc) Y^abc.
//
// cct_w_kernel    THE HOT KERNEL: one of the six w of every triple of a batch, added into that triple's W (o^3 doubles of the scoped
//                 workspace) through the output strides of the permutation.  For a fixed triple and a fixed middle index j both terms of
//                 w are one o x o product over rows i and columns k with ONE K loop of length v + o (the sign of the hole term folded
//                 into the A operand), on v_mfma_f64_16x16x4_f64.  Tile geometry of K19 / K21: four waves in 2 x 2, K tile 16, k-major
//                 LDS tiles, two stages, one barrier per K tile; the workgroup tile is 64 x 64 (2 x 2 accumulators a wave) where
//                 o > 32 and 32 x 32 (one a wave) below.  The particle part reads (ia|bf) and t_kj^cf along f where they lie, the
//                 hole part (ia|jm) along m and a permuted copy t2T[b][c][m][k] along k.  Six launches per batch, stream-ordered: every
//                 element of W is written once per launch, so the order of the six additions is fixed.
// cct_y_kernel    one workgroup per triple: r3(W), V, the division and the sum over i j k in a fixed order, times the multiplicity,
//                 into the triple's own slot of an array of v (v + 1) (v + 2) / 6 doubles.
// cct_part/sum    the fixed-order sum of that array: a fixed grid of partial sums, then one workgroup.
// No atomics; the partial of a triple does not depend on which batch it ran in, so E_(T) is bit-identical between calls and
// independent of the workspace budget.
#include "devres.h"
#include "ccsd_view.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int NT = 256, BK = 16, SUM_GRID = 1024;

long long ntriples(long long v) { return v * (v + 1) * (v + 2) / 6; }

// the g-th triple a >= b >= c in the order g = a (a + 1) (a + 2) / 6 + b (b + 1) / 2 + c
__device__ inline void triple_of(long long g, int &a, int &b, int &c) {
    long long x = (long long)cbrt(6.0 * (double)g);
    while (x > 0 && x * (x + 1) * (x + 2) / 6 > g) --x;
    while ((x + 1) * (x + 2) * (x + 3) / 6 <= g) ++x;
    const long long r = g - x * (x + 1) * (x + 2) / 6;
    long long y = (long long)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
    while (y > 0 && y * (y + 1) / 2 > r) --y;
    while ((y + 1) * (y + 2) / 2 <= r) ++y;
    a = (int)x; b = (int)y; c = (int)(r - y * (y + 1) / 2);
}

__device__ inline int pick(int p, int x0, int x1, int x2) { return p == 0 ? x0 : p == 1 ? x1 : x2; }

// p0 p1 p2: which of the triple's (a, b, c) -- and with it which of W's axes (i, j, k) -- the first, second and third pair of this w is
struct TW {
    int o, v, p0, p1, p2, beta;
    long long g0;
    const double *ovvv, *ovoo, *t2, *t2T;
    double *W;
};

template <int WT>
__global__ __launch_bounds__(NT) void cct_w_kernel(TW g) {
    constexpr int TS = 32 * WT, LDT = TS + 17, NJ = 2 * WT, KP = NT / TS;
    __shared__ double As[2][BK][LDT], Bs[2][BK][LDT];
    const int o = g.o, v = g.v;
    const int tiles = (o + TS - 1) / TS;
    long long bid = blockIdx.x;
    const int k0 = (int)(bid % tiles) * TS; bid /= tiles;
    const int i0 = (int)(bid % tiles) * TS; bid /= tiles;
    const int j = (int)(bid % o);
    const long long t = bid / o;
    int x0, x1, x2;
    triple_of(g.g0 + t, x0, x1, x2);
    const int a = pick(g.p0, x0, x1, x2), b = pick(g.p1, x0, x1, x2), c = pick(g.p2, x0, x1, x2);
    const long long oo = (long long)o * o, vv = (long long)v * v;
    const long long si = g.p0 == 0 ? oo : g.p0 == 1 ? o : 1;
    const long long sj = g.p1 == 0 ? oo : g.p1 == 1 ? o : 1;
    const long long sk = g.p2 == 0 ? oo : g.p2 == 1 ? o : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xl = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 16 * WT, wn = (wave & 1) * 16 * WT;
    const int kg = tid & 15, mg = tid >> 4;           // lanes along the summed index: row / column mg + 16 jj
    const int cB = tid % TS, kB = tid / TS;           // lanes along k (the hole part of B): summed index kB + KP jj
    const int nkv = (v + BK - 1) / BK, nk = nkv + (o + BK - 1) / BK;
    const double *Ap = g.ovvv + ((long long)a * v + b) * v;         // + i v^3 + f
    const double *Ah = g.ovoo + ((long long)a * o + j) * o;         // + i v o^2 + m
    const double *Bp = g.t2 + ((long long)j * v + c) * v;           // + k o v^2 + f
    const double *Bh = g.t2T + ((long long)b * v + c) * oo;         // + m o + k
    const long long sAp = vv * v, sAh = (long long)v * oo, sBp = (long long)o * vv;

    double ra[NJ], rb[NJ];
    auto load = [&](int tt) {
        if (tt < nkv) {
            const int f = tt * BK + kg;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int i = i0 + mg + 16 * jj, k = k0 + mg + 16 * jj;
                ra[jj] = (i < o && f < v) ? Ap[i * sAp + f] : 0.0;
                rb[jj] = (k < o && f < v) ? Bp[k * sBp + f] : 0.0;
            }
        } else {
            const int m0 = (tt - nkv) * BK, m = m0 + kg;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int i = i0 + mg + 16 * jj, mm = m0 + kB + KP * jj, k = k0 + cB;
                ra[jj] = (i < o && m < o) ? -Ah[i * sAh + m] : 0.0;
                rb[jj] = (k < o && mm < o) ? Bh[(long long)mm * o + k] : 0.0;
            }
        }
    };
    auto stage = [&](int buf, int tt) {
        const bool hole = tt >= nkv;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            As[buf][kg][mg + 16 * jj] = ra[jj];
            if (hole) Bs[buf][kB + KP * jj][cB] = rb[jj];
            else Bs[buf][kg][mg + 16 * jj] = rb[jj];
        }
    };

    d4_t acc[WT][WT];
#pragma unroll
    for (int r = 0; r < WT; ++r)
#pragma unroll
        for (int s = 0; s < WT; ++s) acc[r][s] = d4_t{0.0, 0.0, 0.0, 0.0};
    load(0);
    stage(0, 0);
    __syncthreads();
#pragma unroll 1
    for (int tt = 0; tt < nk; ++tt) {
        const int buf = tt & 1;
        if (tt + 1 < nk) load(tt + 1);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            double fa[WT], fb[WT];
#pragma unroll
            for (int r = 0; r < WT; ++r) {
                fa[r] = As[buf][4 * kk + q][wm + 16 * r + xl];
                fb[r] = Bs[buf][4 * kk + q][wn + 16 * r + xl];
            }
#pragma unroll
            for (int r = 0; r < WT; ++r)
#pragma unroll
                for (int s = 0; s < WT; ++s) acc[r][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[r], fb[s], acc[r][s], 0, 0, 0);
        }
        if (tt + 1 < nk) stage(buf ^ 1, tt + 1);      // the other stage was last read before the previous barrier
        __syncthreads();
    }
    // D layout: row = (lane >> 4) + 4 r, column = lane & 15
    double *Wt = g.W + t * oo * o + (long long)j * sj;
#pragma unroll
    for (int r = 0; r < WT; ++r)
#pragma unroll
        for (int s = 0; s < WT; ++s)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = i0 + wm + 16 * r + q + 4 * e, k = k0 + wn + 16 * s + xl;
                if (i >= o || k >= o) continue;
                double *p = Wt + i * si + k * sk;
                *p = g.beta ? *p + acc[r][s][e] : acc[r][s][e];
            }
}

struct TY {
    int o, v;
    long long g0;
    const double *W, *ovov, *t1, *t2, *fov, *eo, *ev;
    double *part;
};

// (pa|qb) t_rc + t_pq^ab f_rc
__device__ inline double cct_x(const TY &g, int p, int a, int q, int b, int r, int c) {
    const long long o = g.o, v = g.v;
    return g.ovov[((p * v + a) * o + q) * v + b] * g.t1[r * v + c] + g.t2[((p * o + q) * v + a) * v + b] * g.fov[r * v + c];
}

__global__ __launch_bounds__(NT) void cct_y_kernel(TY g) {
    __shared__ double red[NT];
    const int o = g.o;
    const long long oo = (long long)o * o, n = oo * o;
    const long long t = blockIdx.x;
    int a, b, c;
    triple_of(g.g0 + t, a, b, c);
    const double *W = g.W + t * n;
    const double eabc = g.ev[a] + g.ev[b] + g.ev[c];
    double s = 0.0;
    for (long long e = threadIdx.x; e < n; e += NT) {
        const int i = (int)(e / oo), j = (int)(e / o % o), k = (int)(e % o);
        const double w = W[e];
        const double r3 = 4.0 * w + W[(j * (long long)o + k) * o + i] + W[(k * (long long)o + i) * o + j]
                          - 2.0 * (W[(k * (long long)o + j) * o + i] + W[(i * (long long)o + k) * o + j] + W[(j * (long long)o + i) * o + k]);
        const double x = cct_x(g, i, a, j, b, k, c) + cct_x(g, i, a, k, c, j, b) + cct_x(g, j, b, i, a, k, c)
                         + cct_x(g, j, b, k, c, i, a) + cct_x(g, k, c, i, a, j, b) + cct_x(g, k, c, j, b, i, a);
        const double d = (g.eo[i] + g.eo[j] + g.eo[k]) - eabc;
        s += r3 * (w + 0.5 * x) / d;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mult = (a == b && b == c) ? 1.0 / 3.0 : (a == b || b == c) ? 1.0 : 2.0;
        g.part[g.g0 + t] = mult * red[0];
    }
}

// out[block] = sum of in over the block's grid-stride share (a fixed grid); with one workgroup: the sum
__global__ __launch_bounds__(NT) void cct_sum_kernel(long long n, const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) s += in[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// bytes[0]: the permuted t2, one double per unique triple, the partial sums and the result; bytes[1]: one triple's W
void t_plan(long long o, long long v, int64_t *bytes) {
    bytes[0] = (int64_t)(dmk_align256((size_t)(o * o * v * v) * 8) + dmk_align256((size_t)ntriples(v) * 8) + dmk_align256((size_t)SUM_GRID * 8) + 256);
    bytes[1] = (int64_t)dmk_align256((size_t)(o * o * o) * 8);
}

long long w_blocks_per_triple(int o) {
    const long long tiles = o > 32 ? (o + 63) / 64 : 1;
    return tiles * tiles * o;
}

}  // namespace

extern "C" {

int dmk_rccsd_t_plan(int nocc, int nvir, int64_t *bytes_host) {
    if (!bytes_host || nocc < 1 || nvir < 1 || nocc > 512 || nvir > 512) return DMK_ERR_INVALID;
    t_plan(nocc, nvir, bytes_host);
    return DMK_OK;
}

int dmk_rccsd_t(dmk_rccsd *h, int64_t max_bytes, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    RccsdView V;
    dmk_rccsd_view(h, &V);
    dmk_ctx *ctx = V.ctx;
    if (!result_host) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_t: NULL result");
    if (!V.have_amps) return dmk_fail(ctx, DMK_ERR_STATE, "rccsd_t: no amplitudes yet (run, init or set first)");
    const int o = V.o, v = V.v;
    int64_t plan[2];
    t_plan(o, v, plan);
    long long budget = max_bytes;
    if (budget <= 0) {          // "what is free": three quarters of it, the rest stays for the caller
        size_t fr = 0, tot = 0;
        DMK_HIP(ctx, hipMemGetInfo(&fr, &tot));
        budget = (long long)(fr / 4 * 3);
    }
    if (plan[0] + plan[1] > budget)
        return dmk_fail(ctx, DMK_ERR_NOMEM, "rccsd_t: nocc = %d, nvir = %d needs %lld bytes + %lld per triple in flight, the budget is %lld bytes",
                        o, v, (long long)plan[0], (long long)plan[1], budget);
    const long long ntr = ntriples(v), per = w_blocks_per_triple(o);
    const long long T = std::min(std::min(ntr, (budget - plan[0]) / plan[1]), 0x7fffffffLL / per);
    DevMem ws;
    if (ws.alloc(ctx, (size_t)(plan[0] + T * plan[1])) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "rccsd_t: no device memory for %lld bytes", (long long)(plan[0] + T * plan[1]));
    }
    StreamDrain drain{ctx->stream};          // the scoped workspace must not go while launches that use it are queued
    char *p = ws.get<char>();
    double *t2T = reinterpret_cast<double *>(p);        p += dmk_align256((size_t)o * o * v * v * 8);
    double *part = reinterpret_cast<double *>(p);       p += dmk_align256((size_t)ntr * 8);
    double *bsum = reinterpret_cast<double *>(p);       p += dmk_align256((size_t)SUM_GRID * 8);
    double *res = reinterpret_cast<double *>(p);        p += 256;
    double *W = reinterpret_cast<double *>(p);
    int rc;
    if ((rc = dmk_cc_perm(ctx, o, v, 1.0, V.t2, "ijab", 0.0, t2T, "abij"))) return rc;
    static const int P6[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const long long ts = o > 32 ? 64 : 32, tiles = (o + ts - 1) / ts, kt = (v + BK - 1) / BK + (o + BK - 1) / BK;
    long long batches = 0;
    for (long long g0 = 0; g0 < ntr; g0 += T, ++batches) {
        const long long nt = std::min(T, ntr - g0);
        {
            FamScope fs(ctx, DMK_FAM_DGEMM);
            fs.mfma_flops(6.0 * 2.0 * (double)(ts * ts * BK) * (double)kt * (double)(tiles * tiles * o) * (double)nt);
            for (int q = 0; q < 6; ++q) {
                const TW g{o, v, P6[q][0], P6[q][1], P6[q][2], q > 0, g0, V.ovvv, V.ovoo, V.t2, t2T, W};
                if (o > 32) hipLaunchKernelGGL(cct_w_kernel<2>, dim3((unsigned)(nt * per)), dim3(NT), 0, ctx->stream, g);
                else hipLaunchKernelGGL(cct_w_kernel<1>, dim3((unsigned)(nt * per)), dim3(NT), 0, ctx->stream, g);
            }
            DMK_CHECK_LAUNCH(ctx);
        }
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(cct_y_kernel, dim3((unsigned)nt), dim3(NT), 0, ctx->stream, TY{o, v, g0, W, V.ovov, V.t1, V.t2, V.fov, V.eo, V.ev, part});
        DMK_CHECK_LAUNCH(ctx);
    }
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        const int grid = (int)std::min<long long>(SUM_GRID, (ntr + NT - 1) / NT);
        hipLaunchKernelGGL(cct_sum_kernel, dim3(grid), dim3(NT), 0, ctx->stream, ntr, part, bsum);
        hipLaunchKernelGGL(cct_sum_kernel, dim3(1), dim3(NT), 0, ctx->stream, (long long)grid, bsum, res);
        DMK_CHECK_LAUNCH(ctx);
    }
    double e = 0.0;
    DMK_HIP(ctx, hipMemcpyAsync(&e, res, 8, hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    result_host[0] = e;
    result_host[1] = (double)batches;
    return DMK_OK;
}

}  // extern "C"
