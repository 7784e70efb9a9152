// Density-fitted k-point J/K build (include/libdmetk.h, dmk_dfjk_*).
//
//   rho[s][L]     = sum_k sum_pq B^(k,k)[L,p,q] dm[s,k][q,p]
//   vj[s,k][r,t]  = (1/nk) sum_L rho[s][L] B^(k,k)[L,r,t]
//   vk[s,ki][p,t] = (1/nk) sum_kj sum_L sum_qr B^(ki,kj)[L,p,q] dm[s,kj][q,r] conj(B^(ki,kj)[L,t,r])
//
// Exchange, per pushed block: W[L,p,(s,r)] = sum_q B[L,p,q] dm[s,kj][q,r] (first product, one GEMM with M = naux nao), then
// vk[s,ki] += sum_(L,r) W[L,p,(s,r)] conj(B[L,t,r]) (second product: an nao x nao result over K = naux nao, split over the
// auxiliary index into chunks whose partial tiles go to a workspace and are summed chunk by chunk in a fixed order).  Both
// products are the same kernel, C = A B^T or A B^H with both operands stored [row][k]: dm is transposed once at begin.
// Complex products are 3M on v_mfma_f64_16x16x4_f64, as in the half transform (zhot_common.h).
// All offsets are 64-bit; a block of 4 GiB or more is refused at begin.  No atomics anywhere: two runs give the same bits.
#include "common.h"
#include "devres.h"
#include <new>

namespace {

constexpr int TM = 64, TN = 64, KT = 16, LDP = KT + 1;      // workgroup tile, K tile (complex), padded LDS row
constexpr double FLOP_PER_WG_STEP = 4.0 * (KT / 4) * 12.0 * 2048.0;   // 4 waves x 4 k steps x (2 x 2 tiles x 3 MFMAs) x 2048 flop

struct ZntArgs {
    const double2 *A; long long lda, M;      // A: M rows of K, row stride lda (elements)
    const double2 *B; long long ldb, N;      // B: N rows of K
    int K;
    int nbatch; long long sA, sB;            // batches (the auxiliary index in the second product) summed into one result
    int nchunk;                              // gridDim.y: chunk c sums batches [c nbatch / nchunk, (c + 1) nbatch / nchunk)
    double2 *C; long long ldc, sC;           // result of chunk c at C + c sC
    int tiles_n;
};

// C[chunk][m][n] = sum_batch sum_k A[batch][m][k] * (CONJB ? conj(B[batch][n][k]) : B[batch][n][k]); K zero-padded to the K tile.
template <bool CONJB>
__global__ __launch_bounds__(256, 2) void dfjk_znt_kernel(ZntArgs a) {
    __shared__ double sm[2][3][TM * LDP];                // [operand][re | im | re + im][row][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long tile = blockIdx.x;
    const long long row0 = (tile / a.tiles_n) * TM, col0 = (tile % a.tiles_n) * (long long)TN;
    const int chunk = blockIdx.y;
    const int b0 = (int)((long long)chunk * a.nbatch / a.nchunk), b1 = (int)((long long)(chunk + 1) * a.nbatch / a.nchunk);
    const int ktiles = (a.K + KT - 1) / KT;
    const int nsteps = (b1 - b0) * ktiles;

    // staging: thread -> rows (tid >> 4) + 16 i, column tid & 15 of the K tile; out-of-range elements are loaded from a clamped
    // (valid) address and zeroed afterwards, so that no load sits behind a branch
    const int sr = tid >> 4, sk = tid & 15;
    double2 ra[4], rb[4];
    auto gload = [&](int step) {
        const int b = b0 + step / ktiles, k = (step % ktiles) * KT + sk;
        const bool kin = k < a.K;
        const int kc = kin ? k : a.K - 1;
        const double2 *Ab = a.A + (long long)b * a.sA + kc, *Bb = a.B + (long long)b * a.sB + kc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = row0 + sr + 16 * i, c = col0 + sr + 16 * i;
            const bool rin = r < a.M, cin = c < a.N;
            double2 va = Ab[(rin ? r : a.M - 1) * a.lda], vb = Bb[(cin ? c : a.N - 1) * a.ldb];
            if (!(rin && kin)) va = make_double2(0.0, 0.0);
            if (!(cin && kin)) vb = make_double2(0.0, 0.0);
            ra[i] = va; rb[i] = vb;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = (sr + 16 * i) * LDP + sk;
            const double bi = CONJB ? -rb[i].y : rb[i].y;
            sm[0][0][o] = ra[i].x; sm[0][1][o] = ra[i].y; sm[0][2][o] = ra[i].x + ra[i].y;
            sm[1][0][o] = rb[i].x; sm[1][1][o] = bi;      sm[1][2][o] = rb[i].x + bi;
        }
    };

    const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
    d4_t p[2][2], q[2][2], t[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) { p[mi][ni] = d4_t{0, 0, 0, 0}; q[mi][ni] = d4_t{0, 0, 0, 0}; t[mi][ni] = d4_t{0, 0, 0, 0}; }

    if (nsteps > 0) gload(0);
    for (int step = 0; step < nsteps; ++step) {
        lstore();
        __syncthreads();
        if (step + 1 < nsteps) gload(step + 1);
#pragma unroll
        for (int kk = 0; kk < KT / 4; ++kk) {
            double ar[2], ai[2], as[2], br[2], bi[2], bs[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int oa = (wm * 32 + m * 16 + fr) * LDP + kk * 4 + fq, ob = (wn * 32 + m * 16 + fr) * LDP + kk * 4 + fq;
                ar[m] = sm[0][0][oa]; ai[m] = sm[0][1][oa]; as[m] = sm[0][2][oa];
                br[m] = sm[1][0][ob]; bi[m] = sm[1][1][ob]; bs[m] = sm[1][2][ob];
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni) {
                    p[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[mi], br[ni], p[mi][ni], 0, 0, 0);
                    q[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(ai[mi], bi[ni], q[mi][ni], 0, 0, 0);
                    t[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[mi], bs[ni], t[mi][ni], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    double2 *C = a.C + (long long)chunk * a.sC;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long row = row0 + wm * 32 + mi * 16 + fq + 4 * r, col = col0 + wn * 32 + ni * 16 + fr;
                if (row < a.M && col < a.N)
                    C[row * a.ldc + col] = make_double2(p[mi][ni][r] - q[mi][ni][r], (t[mi][ni][r] - p[mi][ni][r]) - q[mi][ni][r]);
            }
}

// out[e] += sum_c part[c][e], c ascending: the fixed order of the split-K reduction (n doubles per chunk)
__global__ __launch_bounds__(256) void dfjk_reduce_kernel(long long n, int nchunk, const double *part, double *out) {
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n; e += 256LL * gridDim.x) {
        double s = out[e];
        for (int c = 0; c < nchunk; ++c) s += part[(long long)c * n + e];
        out[e] = s;
    }
}

// dmT[k][s][r][q] = dm[s][k][q][r]
__global__ __launch_bounds__(256) void dfjk_dmT_kernel(int nk, int spin, int nao, const double2 *dm, double2 *dmT) {
    const long long n2 = (long long)nao * nao, total = n2 * nk * spin;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += 256LL * gridDim.x) {
        const long long mat = e / n2, o = e % n2;
        const int k = (int)(mat / spin), s = (int)(mat % spin), r = (int)(o / nao), q = (int)(o % nao);
        dmT[e] = dm[((long long)s * nk + k) * n2 + (long long)q * nao + r];
    }
}

// Coulomb pass 1: rho_k[s][L] = sum_pq B[L][p][q] dm[s,k][q][p] = sum_e B[L][e] dmT[k][s][e]; one workgroup per (L, s), the
// partial sums of its threads combined by a fixed LDS tree
__global__ __launch_bounds__(256) void dfjk_rho_kernel(int nao, int naux, const double2 *B, const double2 *dmT_k, double2 *rho_k) {
    __shared__ double2 red[256];
    const long long n2 = (long long)nao * nao;
    const int L = blockIdx.x, s = blockIdx.y;
    const double2 *b = B + (long long)L * n2, *d = dmT_k + (long long)s * n2;
    double re = 0.0, im = 0.0;
    for (long long e = threadIdx.x; e < n2; e += 256) {
        const double2 x = b[e], y = d[e];
        re += x.x * y.x - x.y * y.y;
        im += x.x * y.y + x.y * y.x;
    }
    red[threadIdx.x] = make_double2(re, im);
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { red[threadIdx.x].x += red[threadIdx.x + w].x; red[threadIdx.x].y += red[threadIdx.x + w].y; }
        __syncthreads();
    }
    if (threadIdx.x == 0) rho_k[(long long)s * naux + L] = red[0];
}

// rho[s][L] = sum_k (weight) rho_k[k][s][L], k ascending; with time reversal the partner of a weight-2 point adds the conjugate
__global__ __launch_bounds__(256) void dfjk_rho_sum_kernel(int nk, int n, const int *weights, const double2 *rho_k, double2 *rho) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double re = 0.0, im = 0.0;
    for (int k = 0; k < nk; ++k) {
        const int w = weights ? weights[k] : 1;
        if (w == 0) continue;
        const double2 x = rho_k[(long long)k * n + e];
        if (w == 2) re += 2.0 * x.x;
        else { re += x.x; im += x.y; }
    }
    rho[e] = make_double2(re, im);
}

// Coulomb pass 2: vj[s][e] = scale sum_L rho[s][L] B[L][e]
template <int SPIN>
__global__ __launch_bounds__(64) void dfjk_vj_kernel(int nao, int naux, const double2 *B, const double2 *rho, double scale,
                                                     double2 *vj, long long spin_stride) {
    const long long n2 = (long long)nao * nao, e = blockIdx.x * 64LL + threadIdx.x;
    if (e >= n2) return;
    double re[SPIN], im[SPIN];
#pragma unroll
    for (int s = 0; s < SPIN; ++s) re[s] = im[s] = 0.0;
#pragma unroll 4
    for (int L = 0; L < naux; ++L) {
        const double2 x = B[(long long)L * n2 + e];
#pragma unroll
        for (int s = 0; s < SPIN; ++s) {
            const double2 r = rho[(long long)s * naux + L];
            re[s] += r.x * x.x - r.y * x.y;
            im[s] += r.x * x.y + r.y * x.x;
        }
    }
#pragma unroll
    for (int s = 0; s < SPIN; ++s) vj[s * spin_stride + e] = make_double2(re[s] * scale, im[s] * scale);
}

// x[s][k] *= scale for the k with mask[k] != 0
__global__ __launch_bounds__(256) void dfjk_scale_kernel(int nk, long long n2, const int *mask, double scale, double2 *x) {
    const int mat = blockIdx.y, k = mat % nk;
    if (!mask[k]) return;
    double2 *m = x + (long long)mat * n2;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n2; e += 256LL * gridDim.x) { m[e].x *= scale; m[e].y *= scale; }
}

// x[s][k] += y[s][k] for the k with mask[k] != 0
__global__ __launch_bounds__(256) void dfjk_add_kernel(int nk, long long n2, const int *mask, const double2 *y, double2 *x) {
    const int mat = blockIdx.y, k = mat % nk;
    if (!mask[k]) return;
    const long long o = (long long)mat * n2;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n2; e += 256LL * gridDim.x) { x[o + e].x += y[o + e].x; x[o + e].y += y[o + e].y; }
}

// time-reversal fill: weight 0 -> conj of the partner's matrix; weight 1 (its own partner) -> imaginary part dropped
__global__ __launch_bounds__(256) void dfjk_trfill_kernel(int nk, long long n2, const int *weights, const int *minus_k, const int *mask,
                                                          double2 *x) {
    const int mat = blockIdx.y, k = mat % nk, w = weights[k];
    if (w == 2) return;
    const int src = minus_k[k];
    if (!mask[src]) return;
    double2 *m = x + (long long)mat * n2;
    const double2 *f = x + (long long)(mat - k + src) * n2;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < n2; e += 256LL * gridDim.x) {
        if (w == 0) m[e] = make_double2(f[e].x, -f[e].y);
        else m[e].y = 0.0;
    }
}

}  // namespace

struct dmk_dfjk {
    dmk_ctx *ctx = nullptr;
    int nk = 0, nao = 0, naux = 0, spin = 0, flags = 0;
    bool with_j = false, with_k = false, tr = false, finished = false, pushed = false;
    const double2 *dm = nullptr; double2 *vj = nullptr, *vk = nullptr;
    long long n2 = 0;
    size_t block_bytes = 0;
    DevMem dmT, W, part, rho_k, rho, ew;          // c128 workspaces
    DevMem tab_dev;                               // int [weights | minus_k | row mask | all ones] x nk
    std::vector<int> weights, minus_k, kcount, j1, j2;
    bool rho_ready = false;
    int nchunk = 1;
    double madelung = 0.0; const double2 *ovlp = nullptr; bool ewald = false;
    DevMem ring; int ring_slots = 0;
    HostFeed feed;                                // dmk_dfjk_push_block_host
    double flops[2] = {0.0, 0.0};
};

// the streams are drained, then the handle goes with everything it owns
static void dfjk_release(dmk_dfjk *h) {
    (void)hipStreamSynchronize(h->ctx->stream);
    h->feed.sync();
    delete h;
}

static bool dfjk_required(const dmk_dfjk *h, int k) { return !h->tr || h->weights[k] > 0; }

static int dfjk_launch_znt(dmk_dfjk *h, bool conjb, const ZntArgs &a, int product) {
    dmk_ctx *ctx = h->ctx;
    const long long tiles = ((a.M + TM - 1) / TM) * a.tiles_n;
    if (tiles <= 0 || tiles > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: %lld tiles in one launch", tiles);
    FamScope fs(ctx, DMK_FAM_JK);
    if (conjb) hipLaunchKernelGGL(dfjk_znt_kernel<true>, dim3((unsigned)tiles, a.nchunk), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(dfjk_znt_kernel<false>, dim3((unsigned)tiles, a.nchunk), dim3(256), 0, ctx->stream, a);
    DMK_CHECK_LAUNCH(ctx);
    const double f = (double)tiles * a.nbatch * ((a.K + KT - 1) / KT) * FLOP_PER_WG_STEP;
    fs.mfma_flops(f);
    h->flops[product] += f;
    return DMK_OK;
}

static int dfjk_exchange(dmk_dfjk *h, int ki, int kj, const double2 *B) {
    dmk_ctx *ctx = h->ctx;
    const int n = h->nao, sn = h->spin * n;
    ZntArgs a1{};
    a1.A = B; a1.lda = n; a1.M = (long long)h->naux * n;
    a1.B = h->dmT.get<double2>() + (long long)kj * h->spin * h->n2; a1.ldb = n; a1.N = sn;
    a1.K = n; a1.nbatch = 1; a1.sA = a1.sB = 0; a1.nchunk = 1;
    a1.C = h->W.get<double2>(); a1.ldc = sn; a1.sC = 0; a1.tiles_n = (sn + TN - 1) / TN;
    int rc = dfjk_launch_znt(h, false, a1, 0);
    if (rc) return rc;
    if (h->flags & DMK_DFJK_FIRST_ONLY) return DMK_OK;       // measurement: the first product alone
    for (int s = 0; s < h->spin; ++s) {
        ZntArgs a2{};
        a2.A = h->W.get<double2>() + (long long)s * n; a2.lda = sn; a2.M = n;
        a2.B = B; a2.ldb = n; a2.N = n;
        a2.K = n; a2.nbatch = h->naux; a2.sA = (long long)n * sn; a2.sB = h->n2; a2.nchunk = h->nchunk;
        a2.C = h->part.get<double2>(); a2.ldc = n; a2.sC = h->n2; a2.tiles_n = (n + TN - 1) / TN;
        rc = dfjk_launch_znt(h, true, a2, 1);
        if (rc) return rc;
        FamScope fs(ctx, DMK_FAM_JK);
        const long long nd = 2 * h->n2;
        hipLaunchKernelGGL(dfjk_reduce_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, ctx->stream, nd, h->nchunk,
                           h->part.get<const double>(), (double *)(h->vk + ((long long)s * h->nk + ki) * h->n2));
        DMK_CHECK_LAUNCH(ctx);
    }
    return DMK_OK;
}

static int dfjk_upload_tables(dmk_dfjk *h) {
    std::vector<int> t(4 * (size_t)h->nk);
    for (int k = 0; k < h->nk; ++k) {
        t[k] = h->weights[k]; t[h->nk + k] = h->minus_k[k];
        t[2 * h->nk + k] = (h->kcount[k] == h->nk) ? 1 : 0; t[3 * h->nk + k] = 1;
    }
    DMK_HIP(h->ctx, hipMemcpyAsync(h->tab_dev.get<void>(), t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice, h->ctx->stream));
    DMK_HIP(h->ctx, hipStreamSynchronize(h->ctx->stream));       // `t` is pageable and goes out of scope
    return DMK_OK;
}

extern "C" {

int dmk_dfjk_begin(dmk_ctx *ctx, int nk, int nao, int naux, int spin, int flags, const void *dm, void *vj_out, void *vk_out,
                   dmk_dfjk **out) {
    if (!ctx || !out) return DMK_ERR_INVALID;
    *out = nullptr;
    if (nk < 1 || nao < 1 || naux < 1 || spin < 1 || spin > 2) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: bad shape nk %d nao %d naux %d spin %d", nk, nao, naux, spin);
    const bool wj = flags & DMK_DFJK_WITH_J, wk = flags & DMK_DFJK_WITH_K;
    if (!wj && !wk) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: neither J nor K asked for");
    if (!dm || (wj && !vj_out) || (wk && !vk_out)) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: null array");
    if (((uintptr_t)dm | (uintptr_t)vj_out | (uintptr_t)vk_out) & 15) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: arrays must be 16-byte aligned");
    const double bytes = 16.0 * naux * (double)nao * nao;
    if (bytes >= 4294967296.0) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: an AO block of %.0f bytes (>= 4 GiB) is not supported", bytes);
    dmk_dfjk *h = new (std::nothrow) dmk_dfjk;
    if (!h) return DMK_ERR_NOMEM;
    h->ctx = ctx; h->nk = nk; h->nao = nao; h->naux = naux; h->spin = spin; h->flags = flags;
    h->with_j = wj; h->with_k = wk;
    h->dm = (const double2 *)dm; h->vj = (double2 *)vj_out; h->vk = (double2 *)vk_out;
    h->n2 = (long long)nao * nao;
    h->block_bytes = (size_t)naux * h->n2 * 16;
    h->weights.assign(nk, 1); h->minus_k.assign(nk, 0); h->kcount.assign(nk, 0); h->j1.assign(nk, 0); h->j2.assign(nk, 0);
    for (int k = 0; k < nk; ++k) h->minus_k[k] = k;
    const long long tiles = (long long)((nao + TM - 1) / TM) * ((nao + TN - 1) / TN);
    long long nc = (1024 + tiles - 1) / tiles;
    if (nc > naux / 2) nc = naux / 2;
    if (nc < 1) nc = 1;
    h->nchunk = (int)nc;
    const size_t mats = (size_t)spin * nk * h->n2 * 16;
    hipError_t e = h->dmT.alloc(ctx, mats);
    if (e == hipSuccess) e = h->tab_dev.alloc(ctx, 4 * (size_t)nk * sizeof(int));
    if (e == hipSuccess && wk) e = h->W.alloc(ctx, h->block_bytes * spin);
    if (e == hipSuccess && wk) e = h->part.alloc(ctx, (size_t)h->nchunk * h->n2 * 16);
    if (e == hipSuccess && wj) e = h->rho_k.alloc(ctx, (size_t)nk * spin * naux * 16);
    if (e == hipSuccess && wj) e = h->rho.alloc(ctx, (size_t)spin * naux * 16);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        dfjk_release(h);
        return dmk_fail(ctx, DMK_ERR_NOMEM, "dfjk: workspace allocation failed: %s", hipGetErrorString(e));
    }
    {
        FamScope fs(ctx, DMK_FAM_JK);
        hipLaunchKernelGGL(dfjk_dmT_kernel, dim3(1024), dim3(256), 0, ctx->stream, nk, spin, nao, h->dm, h->dmT.get<double2>());
    }
    hipError_t le = hipGetLastError();
    if (le == hipSuccess && wk) le = hipMemsetAsync(h->vk, 0, mats, ctx->stream);
    if (le == hipSuccess && wj) le = hipMemsetAsync(h->vj, 0, mats, ctx->stream);
    if (le == hipSuccess && wj) le = hipMemsetAsync(h->rho_k.get<void>(), 0, (size_t)nk * spin * naux * 16, ctx->stream);
    if (le != hipSuccess) {
        dfjk_release(h);
        return dmk_fail(ctx, DMK_ERR_HIP, "dfjk: begin failed: %s", hipGetErrorString(le));
    }
    *out = h;
    return DMK_OK;
}

int dmk_dfjk_set_t_reversal(dmk_dfjk *h, const int32_t *minus_k_host, const int32_t *weights_host) {
    if (!h) return DMK_ERR_INVALID;
    if (h->pushed || h->finished) return dmk_fail(h->ctx, DMK_ERR_STATE, "dfjk: time reversal must be set before the first block");
    if (!minus_k_host || !weights_host) return dmk_fail(h->ctx, DMK_ERR_INVALID, "dfjk: null table");
    for (int k = 0; k < h->nk; ++k) {
        const int m = minus_k_host[k], w = weights_host[k];
        bool ok = m >= 0 && m < h->nk && w >= 0 && w <= 2;
        if (ok) ok = minus_k_host[m] == k && ((w == 1) == (m == k)) && (m == k || w + weights_host[m] == 2);
        if (!ok) return dmk_fail(h->ctx, DMK_ERR_INVALID, "dfjk: inconsistent time-reversal tables at k = %d", k);
    }
    h->minus_k.assign(minus_k_host, minus_k_host + h->nk);
    h->weights.assign(weights_host, weights_host + h->nk);
    h->tr = true;
    return DMK_OK;
}

int dmk_dfjk_set_ewald(dmk_dfjk *h, double madelung, const void *ovlp) {
    if (!h) return DMK_ERR_INVALID;
    if (h->finished) return dmk_fail(h->ctx, DMK_ERR_STATE, "dfjk: already finished");
    if (!h->with_k) return dmk_fail(h->ctx, DMK_ERR_STATE, "dfjk: the Ewald term belongs to K, which this handle does not build");
    if (!ovlp || ((uintptr_t)ovlp & 15)) return dmk_fail(h->ctx, DMK_ERR_INVALID, "dfjk: ovlp null or misaligned");
    if (!h->ew) {
        hipError_t e = h->ew.alloc(h->ctx, 2 * (size_t)h->spin * h->nk * h->n2 * 16);
        if (e != hipSuccess) { (void)hipGetLastError(); return dmk_fail(h->ctx, DMK_ERR_NOMEM, "dfjk: Ewald workspace: %s", hipGetErrorString(e)); }
    }
    h->madelung = madelung; h->ovlp = (const double2 *)ovlp; h->ewald = true;
    return DMK_OK;
}

int dmk_dfjk_push_block(dmk_dfjk *h, int ki, int kj, int what, const void *Lpq) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (h->finished) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: push after finish");
    if (ki < 0 || ki >= h->nk || kj < 0 || kj >= h->nk) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: k index (%d, %d) outside [0, %d)", ki, kj, h->nk);
    if (!Lpq || ((uintptr_t)Lpq & 15)) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: block null or misaligned");
    if (what != DMK_DFJK_EXCHANGE && what != DMK_DFJK_COULOMB1 && what != DMK_DFJK_COULOMB2)
        return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: unknown contribution %d", what);
    const double2 *B = (const double2 *)Lpq;
    if (what == DMK_DFJK_EXCHANGE) {
        if (!h->with_k) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: exchange block pushed to a handle without K");
        if (!dfjk_required(h, ki)) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: row ki = %d is filled by time reversal", ki);
        if (h->kcount[ki] >= h->nk) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: row ki = %d already has its %d blocks", ki, h->nk);
        h->pushed = true;
        const int rc = dfjk_exchange(h, ki, kj, B);
        if (rc) return rc;
        h->kcount[ki] += 1;
        return DMK_OK;
    }
    if (!h->with_j) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: Coulomb block pushed to a handle without J");
    if (ki != kj) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: the Coulomb passes take diagonal blocks, got (%d, %d)", ki, kj);
    if (!dfjk_required(h, ki)) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: k = %d is filled by time reversal", ki);
    if (what == DMK_DFJK_COULOMB1) {
        if (h->rho_ready) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: Coulomb pass 1 after pass 2 has begun");
        if (h->j1[ki]) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: Coulomb pass 1 of k = %d pushed twice", ki);
        h->pushed = true;
        FamScope fs(ctx, DMK_FAM_JK);
        hipLaunchKernelGGL(dfjk_rho_kernel, dim3(h->naux, h->spin), dim3(256), 0, ctx->stream, h->nao, h->naux, B,
                           h->dmT.get<const double2>() + (long long)ki * h->spin * h->n2, h->rho_k.get<double2>() + (long long)ki * h->spin * h->naux);
        DMK_CHECK_LAUNCH(ctx);
        h->j1[ki] = 1;
        return DMK_OK;
    }
    for (int k = 0; k < h->nk; ++k)
        if (dfjk_required(h, k) && !h->j1[k]) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: Coulomb pass 2 before pass 1 of k = %d", k);
    if (h->j2[ki]) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: Coulomb pass 2 of k = %d pushed twice", ki);
    if (!h->rho_ready) {
        const int rc = dfjk_upload_tables(h);
        if (rc) return rc;
        FamScope fs(ctx, DMK_FAM_JK);
        const int n = h->spin * h->naux;
        hipLaunchKernelGGL(dfjk_rho_sum_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, h->nk, n,
                           h->tr ? h->tab_dev.get<const int>() : (const int *)nullptr, h->rho_k.get<const double2>(), h->rho.get<double2>());
        DMK_CHECK_LAUNCH(ctx);
        h->rho_ready = true;
    }
    {
        FamScope fs(ctx, DMK_FAM_JK);
        const unsigned nb = (unsigned)((h->n2 + 63) / 64);
        double2 *vj = h->vj + (long long)ki * h->n2;
        if (h->spin == 1) hipLaunchKernelGGL(dfjk_vj_kernel<1>, dim3(nb), dim3(64), 0, ctx->stream, h->nao, h->naux, B, h->rho.get<const double2>(), 1.0 / h->nk, vj, (long long)h->nk * h->n2);
        else hipLaunchKernelGGL(dfjk_vj_kernel<2>, dim3(nb), dim3(64), 0, ctx->stream, h->nao, h->naux, B, h->rho.get<const double2>(), 1.0 / h->nk, vj, (long long)h->nk * h->n2);
        DMK_CHECK_LAUNCH(ctx);
    }
    h->j2[ki] = 1;
    return DMK_OK;
}

int dmk_dfjk_block_ring(dmk_dfjk *h, void **ring_out, int *nslots_out) {
    if (!h || !ring_out || !nslots_out) return DMK_ERR_INVALID;
    if (h->finished) return dmk_fail(h->ctx, DMK_ERR_STATE, "dfjk: already finished");
    if (!h->ring) {
        for (int n = 4; n >= 1 && !h->ring; n >>= 1) {
            if (h->ring.alloc(h->ctx, h->block_bytes * n) == hipSuccess) h->ring_slots = n;
            else (void)hipGetLastError();
        }
        if (!h->ring) return dmk_fail(h->ctx, DMK_ERR_NOMEM, "dfjk: no memory for a block ring");
    }
    *ring_out = h->ring.get<void>(); *nslots_out = h->ring_slots;
    return DMK_OK;
}

int dmk_dfjk_push_block_host(dmk_dfjk *h, int ki, int kj, int what, const void *Lpq_host, int slot) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (h->finished) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: push after finish");
    if (slot < 0 || slot > 1 || !Lpq_host) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: bad host slot / buffer");
    if (ki < 0 || ki >= h->nk || kj < 0 || kj >= h->nk) return dmk_fail(ctx, DMK_ERR_INVALID, "dfjk: k index (%d, %d) outside [0, %d)", ki, kj, h->nk);
    if (int rc = h->feed.open(ctx)) return rc;
    void *staged = nullptr;
    if (int rc = h->feed.stage(slot, Lpq_host, h->block_bytes, &staged)) return rc;
    if (int rc = dmk_dfjk_push_block(h, ki, kj, what, staged)) return rc;
    return h->feed.done(slot);
}

int dmk_dfjk_host_slot_wait(dmk_dfjk *h, int slot) {
    if (!h || slot < 0 || slot > 1) return DMK_ERR_INVALID;
    return h->feed.wait_copied(slot);
}

int dmk_dfjk_finish(dmk_dfjk *h) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (h->finished) return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: finish called twice");
    // everything is checked before anything is launched
    if (h->with_j)
        for (int k = 0; k < h->nk; ++k)
            if (dfjk_required(h, k) && !(h->j1[k] && h->j2[k]))
                return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: finish before both Coulomb passes of k = %d", k);
    if (h->with_k)
        for (int k = 0; k < h->nk; ++k)
            if (h->kcount[k] != 0 && h->kcount[k] != h->nk)
                return dmk_fail(ctx, DMK_ERR_STATE, "dfjk: row ki = %d has %d of %d exchange blocks", k, h->kcount[k], h->nk);
    int rc = dfjk_upload_tables(h);
    if (rc) return rc;
    const int *w_dev = h->tab_dev.get<int>(), *mk_dev = w_dev + h->nk, *mask_dev = w_dev + 2 * h->nk, *ones_dev = w_dev + 3 * h->nk;
    const dim3 grid((unsigned)((h->n2 + 255) / 256 > 64 ? 64 : (h->n2 + 255) / 256), h->spin * h->nk);
    if (h->with_k) {
        {
            FamScope fs(ctx, DMK_FAM_JK);
            hipLaunchKernelGGL(dfjk_scale_kernel, grid, dim3(256), 0, ctx->stream, h->nk, h->n2, mask_dev, 1.0 / h->nk, h->vk);
            DMK_CHECK_LAUNCH(ctx);
        }
        if (h->ewald) {
            // vk[s,k] += madelung S[k] dm[s,k] S[k]
            double2 *T1 = h->ew.get<double2>(), *T2 = T1 + (long long)h->spin * h->nk * h->n2;
            for (int s = 0; s < h->spin; ++s) {
                const long long o = (long long)s * h->nk * h->n2;
                rc = dmk_zgemm_batched(ctx, 0, 0, h->nao, h->nao, h->nao, h->nk, 1.0, h->ovlp, h->n2, h->dm + o, h->n2, T1 + o, h->n2);
                if (rc) return rc;
                rc = dmk_zgemm_batched(ctx, 0, 0, h->nao, h->nao, h->nao, h->nk, h->madelung, T1 + o, h->n2, h->ovlp, h->n2, T2 + o, h->n2);
                if (rc) return rc;
            }
            FamScope fs(ctx, DMK_FAM_JK);
            hipLaunchKernelGGL(dfjk_add_kernel, grid, dim3(256), 0, ctx->stream, h->nk, h->n2, mask_dev, (const double2 *)T2, h->vk);
            DMK_CHECK_LAUNCH(ctx);
        }
        if (h->tr) {
            FamScope fs(ctx, DMK_FAM_JK);
            hipLaunchKernelGGL(dfjk_trfill_kernel, grid, dim3(256), 0, ctx->stream, h->nk, h->n2, w_dev, mk_dev, mask_dev, h->vk);
            DMK_CHECK_LAUNCH(ctx);
        }
    }
    if (h->with_j && h->tr) {
        FamScope fs(ctx, DMK_FAM_JK);
        hipLaunchKernelGGL(dfjk_trfill_kernel, grid, dim3(256), 0, ctx->stream, h->nk, h->n2, w_dev, mk_dev, ones_dev, h->vj);
        DMK_CHECK_LAUNCH(ctx);
    }
    h->finished = true;
    return DMK_OK;
}

int dmk_dfjk_flops(const dmk_dfjk *h, double flops_host[2]) {
    if (!h || !flops_host) return DMK_ERR_INVALID;
    flops_host[0] = h->flops[0]; flops_host[1] = h->flops[1];
    return DMK_OK;
}

int dmk_dfjk_free(dmk_dfjk *h) {
    if (!h) return DMK_ERR_INVALID;
    dfjk_release(h);
    return DMK_OK;
}

}  // extern "C"
