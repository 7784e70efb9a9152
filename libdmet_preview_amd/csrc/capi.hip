// C ABI of libdmetk: context, memory, k-mesh bookkeeping (host, integer), ERI plan, folds, generic batched products.
// The ERI pipeline (dmk_eri_*) is eri_engine.hip; kernel launchers live in the sibling .hip files; this file holds no
// device code except tiny utility kernels (split-K reduce, transpose, restore, row gather).
#include "common.h"
#include "kmesh.h"
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <algorithm>
#include <chrono>
#include <thread>

// =============================================================================================
// context / errors / memory
// =============================================================================================

int dmk_fail(dmk_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else fprintf(stderr, "libdmetk: %s\n", buf);
    return code;
}

static thread_local std::string g_noctx_err;

// `a` is recorded exactly once, on the stream the launch goes to (ctx->stream unless the caller names another one)
FamScope::FamScope(dmk_ctx *c, int f, hipStream_t stream) : ctx(c), fam(f), on(stream) {
    on_set = ctx && stream != ctx->stream;
    begin();
}
FamScope::FamScope(dmk_ctx *c, int f) : ctx(c), fam(f), on(nullptr) { begin(); }
void FamScope::begin() {
    if (ctx && ctx->profile) {
        auto get = [&]() {
            hipEvent_t e;
            if (!ctx->event_pool.empty()) { e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
            else if (hipEventCreate(&e) != hipSuccess) e = nullptr;
            return e;
        };
        a = get(); b = get();
        if (a) (void)hipEventRecord(a, on_set ? on : ctx->stream);
    }
    if (ctx) ctx->fam_launches[fam] += 1;
}
FamScope::~FamScope() {
    if (ctx && ctx->profile && a && b) {
        (void)hipEventRecord(b, on_set ? on : ctx->stream);
        ctx->pending.push_back({fam, a, b, fam2, share});
    }
}

static void drain_pending(dmk_ctx *ctx) {
    for (auto &p : ctx->pending) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess)
        {
            ctx->fam_ms[p.fam] += p.fam2 >= 0 ? ms * p.share : ms;
            if (p.fam2 >= 0) ctx->fam_ms[p.fam2] += ms * (1.0 - p.share);
        }
        ctx->event_pool.push_back(p.a);
        ctx->event_pool.push_back(p.b);
    }
    ctx->pending.clear();
}

extern "C" {

const char *dmk_version(void) { return "libdmetk 0.1 (gfx950)"; }

int dmk_init(int device, void *stream, dmk_ctx **out) {
    if (!out) return DMK_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        fprintf(stderr, "libdmetk: no HIP device available (%s)\n", hipGetErrorString(e));
        return DMK_ERR_HIP;
    }
    if (device < 0 || device >= ndev) return DMK_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return DMK_ERR_HIP;
    dmk_ctx *c = new dmk_ctx();
    c->device = device;
    c->stream = reinterpret_cast<hipStream_t>(stream);
    if (hipEventCreate(&c->t0) != hipSuccess || hipEventCreate(&c->t1) != hipSuccess) {
        delete c;
        return DMK_ERR_HIP;
    }
    *out = c;
    return DMK_OK;
}

int dmk_destroy(dmk_ctx *ctx) {
    if (!ctx) return DMK_OK;
    (void)hipStreamSynchronize(ctx->stream);
    drain_pending(ctx);
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    for (auto &p : ctx->phases) (void)hipFree(p.dev);
    for (auto &t : ctx->tile_tables) (void)hipFree(t.dev);
    for (auto &t : ctx->step2_tables) (void)hipFree(t.dev);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->scratch2) (void)hipFree(ctx->scratch2);
    for (int w = 0; w < 3; ++w)
        if (ctx->eri_ws[w]) (void)hipFree(ctx->eri_ws[w]);
    (void)hipEventDestroy(ctx->t0);
    (void)hipEventDestroy(ctx->t1);
    delete ctx;
    return DMK_OK;
}

int dmk_set_stream(dmk_ctx *ctx, void *stream) {
    if (!ctx) return DMK_ERR_INVALID;
    ctx->stream = reinterpret_cast<hipStream_t>(stream);
    return DMK_OK;
}

int dmk_mem_info(dmk_ctx *ctx, size_t *free_bytes, size_t *total_bytes) {
    if (!ctx || !free_bytes || !total_bytes) return DMK_ERR_INVALID;
    DMK_HIP(ctx, hipMemGetInfo(free_bytes, total_bytes));
    // hipFree returns before the driver has given every page back: a block freed just before the call can still count as used
    // (measured: 18 MiB of a freed 17.8 MB block, back about 1 ms later with nothing done in between).  The figure handed out is
    // the one that two readings 2 ms apart agree on, at most ten readings.
    for (int k = 0; k < 10; ++k) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        size_t again = 0;
        DMK_HIP(ctx, hipMemGetInfo(&again, total_bytes));
        const bool settled = again == *free_bytes;
        *free_bytes = again;
        if (settled) break;
    }
    return DMK_OK;
}

int dmk_set_oom_hook(dmk_ctx *ctx, void (*hook)(void *), void *user) {
    if (!ctx) return DMK_ERR_INVALID;
    ctx->oom_hook = hook;
    ctx->oom_user = user;
    return DMK_OK;
}

int dmk_sync(dmk_ctx *ctx) {
    if (!ctx) return DMK_ERR_INVALID;
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

const char *dmk_last_error(const dmk_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int dmk_malloc(dmk_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out) return DMK_ERR_INVALID;
    *out = nullptr;
    if (bytes == 0) return DMK_OK;
    hipError_t e = dmk_dev_alloc(ctx, out, bytes);
    if (e != hipSuccess) return dmk_fail(ctx, DMK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return DMK_OK;
}
int dmk_free(dmk_ctx *ctx, void *p) {
    if (!ctx) return DMK_ERR_INVALID;
    if (p) {
        // work enqueued on the context stream may still read the buffer: drain it first
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        DMK_HIP(ctx, hipFree(p));
    }
    return DMK_OK;
}
int dmk_host_alloc(dmk_ctx *ctx, size_t bytes, void **out) {
    if (!ctx || !out) return DMK_ERR_INVALID;
    *out = nullptr;
    DMK_HIP(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return DMK_OK;
}
int dmk_host_free(dmk_ctx *ctx, void *p) {
    if (!ctx) return DMK_ERR_INVALID;
    if (p) DMK_HIP(ctx, hipHostFree(p));
    return DMK_OK;
}
int dmk_memset(dmk_ctx *ctx, void *p, int value, size_t bytes) {
    if (!ctx) return DMK_ERR_INVALID;
    if (bytes) DMK_HIP(ctx, hipMemsetAsync(p, value, bytes, ctx->stream));
    return DMK_OK;
}
int dmk_memcpy_h2d(dmk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return DMK_ERR_INVALID;
    if (bytes) {
        DMK_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DMK_OK;
}
int dmk_memcpy_d2h(dmk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return DMK_ERR_INVALID;
    if (bytes) {
        DMK_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DMK_OK;
}
int dmk_memcpy_d2d(dmk_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return DMK_ERR_INVALID;
    if (bytes) DMK_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return DMK_OK;
}

int dmk_timer_start(dmk_ctx *ctx) {
    if (!ctx) return DMK_ERR_INVALID;
    DMK_HIP(ctx, hipEventRecord(ctx->t0, ctx->stream));
    return DMK_OK;
}
int dmk_timer_stop(dmk_ctx *ctx, double *ms_out) {
    if (!ctx || !ms_out) return DMK_ERR_INVALID;
    DMK_HIP(ctx, hipEventRecord(ctx->t1, ctx->stream));
    DMK_HIP(ctx, hipEventSynchronize(ctx->t1));
    float ms = 0.f;
    DMK_HIP(ctx, hipEventElapsedTime(&ms, ctx->t0, ctx->t1));
    *ms_out = ms;
    return DMK_OK;
}

int dmk_profile(dmk_ctx *ctx, int enable) {
    if (!ctx) return DMK_ERR_INVALID;
    if (!enable && ctx->profile) { (void)hipStreamSynchronize(ctx->stream); drain_pending(ctx); }
    ctx->profile = enable != 0;
    return DMK_OK;
}
int dmk_profile_read(dmk_ctx *ctx, double *ms, int64_t *launches, int reset) {
    if (!ctx) return DMK_ERR_INVALID;
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drain_pending(ctx);
    for (int i = 0; i < DMK_FAM_COUNT; ++i) {
        if (ms) ms[i] = ctx->fam_ms[i];
        if (launches) launches[i] = ctx->fam_launches[i];
        if (reset) { ctx->fam_ms[i] = 0; ctx->fam_launches[i] = 0; }
    }
    return DMK_OK;
}
int dmk_profile_read_flops(dmk_ctx *ctx, double *flops, int reset) {
    if (!ctx) return DMK_ERR_INVALID;
    for (int i = 0; i < DMK_FAM_COUNT; ++i) {
        if (flops) flops[i] = ctx->fam_mfma_flops[i];
        if (reset) ctx->fam_mfma_flops[i] = 0;
    }
    return DMK_OK;
}

}  // extern "C"

hipError_t dmk_dev_alloc(dmk_ctx *ctx, void **out, size_t bytes) {
    hipError_t e = hipMalloc(out, bytes);
    if (e == hipSuccess || !ctx) return e;
    bool parked = false;
    for (int w = 0; w < 3; ++w) parked = parked || ctx->eri_ws[w] != nullptr;
    if (!parked && !ctx->oom_hook) return e;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);      // parked blocks may still be read by queued work
    // the workspaces the last ERI pipeline left in the context (plane stack: tens of GB) are only a cache
    for (int w = 0; w < 3; ++w)
        if (ctx->eri_ws[w]) {
            (void)hipFree(ctx->eri_ws[w]);
            ctx->eri_ws[w] = nullptr;
            ctx->eri_ws_bytes[w] = 0;
        }
    if (ctx->oom_hook) ctx->oom_hook(ctx->oom_user);
    e = hipMalloc(out, bytes);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

int dmk_scratch(dmk_ctx *ctx, size_t bytes, void **out) {
    if (bytes > ctx->scratch_bytes) {
        if (ctx->scratch) {
            DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            DMK_HIP(ctx, hipFree(ctx->scratch));
            ctx->scratch = nullptr;
            ctx->scratch_bytes = 0;
        }
        hipError_t e = dmk_dev_alloc(ctx, &ctx->scratch, bytes);
        if (e != hipSuccess) return dmk_fail(ctx, DMK_ERR_NOMEM, "scratch hipMalloc(%zu) failed", bytes);
        ctx->scratch_bytes = bytes;
    }
    *out = ctx->scratch;
    return DMK_OK;
}

int dmk_scratch2(dmk_ctx *ctx, size_t bytes, void **out) {
    if (bytes > ctx->scratch2_bytes) {
        if (ctx->scratch2) {
            DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            DMK_HIP(ctx, hipFree(ctx->scratch2));
            ctx->scratch2 = nullptr;
            ctx->scratch2_bytes = 0;
        }
        hipError_t e = dmk_dev_alloc(ctx, &ctx->scratch2, bytes);
        if (e != hipSuccess) return dmk_fail(ctx, DMK_ERR_NOMEM, "scratch2 hipMalloc(%zu) failed", bytes);
        ctx->scratch2_bytes = bytes;
    }
    *out = ctx->scratch2;
    return DMK_OK;
}

// =============================================================================================
// a1 / a2 / a15 : integer mesh bookkeeping (host; Mesh and tr_weights: kmesh.h)
// =============================================================================================

extern "C" {

int dmk_kmesh_tables(const int mesh[3], int32_t *kint, int32_t *minus_k, int32_t *weights) {
    Mesh m(mesh);
    if (!m.ok()) return DMK_ERR_INVALID;
    std::vector<int> w;
    tr_weights(m, 1, w);
    for (int i = 0; i < m.nk; ++i) {
        if (kint) { int a[3]; m.ints(i, a); kint[3 * i] = a[0]; kint[3 * i + 1] = a[1]; kint[3 * i + 2] = a[2]; }
        if (minus_k) minus_k[i] = m.minus(i);
        if (weights) weights[i] = w[i];
    }
    return DMK_OK;
}

int dmk_kconserv_table(const int mesh[3], int32_t *out) {
    Mesh m(mesh);
    if (!m.ok() || !out) return DMK_ERR_INVALID;
    for (int kL = 0; kL < m.nk; ++kL)
        for (int i = 0; i < m.nk; ++i) out[(size_t)kL * m.nk + i] = m.combine(i, kL, -1);
    return DMK_OK;
}

int dmk_cell_add_table(const int mesh[3], int sign, int32_t *out) {
    Mesh m(mesh);
    if (!m.ok() || !out || (sign != 1 && sign != -1)) return DMK_ERR_INVALID;
    for (int i = 0; i < m.nk; ++i)
        for (int j = 0; j < m.nk; ++j) out[(size_t)i * m.nk + j] = m.combine(i, j, sign);
    return DMK_OK;
}

int dmk_kpts_scaled(const int mesh[3], double *kpts) {
    Mesh m(mesh);
    if (!m.ok() || !kpts) return DMK_ERR_INVALID;
    for (int i = 0; i < m.nk; ++i) {
        int a[3];
        m.ints(i, a);
        for (int d = 0; d < 3; ++d) {
            const double val = 1.0 / ((double)m.n[d] * 1.0);      // numpy fftfreq: results * (1/(n*d))
            kpts[3 * i + d] = (double)Mesh::freq(a[d], m.n[d]) * val;
        }
    }
    return DMK_OK;
}

int dmk_kpt_member(const int mesh[3], const double kpt[3], double tol) {
    Mesh m(mesh);
    if (!m.ok() || !kpt) return DMK_ERR_INVALID;
    std::vector<double> ks((size_t)3 * m.nk);
    dmk_kpts_scaled(mesh, ks.data());
    for (int i = 0; i < m.nk; ++i) {
        double s = 0.0;
        for (int d = 0; d < 3; ++d) {
            double dk = ks[3 * i + d] - kpt[d];
            dk -= nearbyint(dk);
            s += dk * dk;
        }
        if (sqrt(s) < tol) return i;
    }
    return -1;
}

// basis_transform/eri_transform.py:1409-1427 (get_mask_kptij_lst) on mesh indices: pair p' = (-ki, -kj) of pair p.
// mask[p] = index of the time-reversed partner (first later pair), -2 for a pair already claimed, -1 otherwise.
int dmk_kptij_mask(const int mesh[3], int npairs, const int32_t *pairs, int32_t *mask) {
    Mesh m(mesh);
    if (!m.ok() || npairs < 0 || (npairs > 0 && (!pairs || !mask))) return DMK_ERR_INVALID;
    for (int p = 0; p < npairs; ++p) {
        if (pairs[2 * p] < 0 || pairs[2 * p] >= m.nk || pairs[2 * p + 1] < 0 || pairs[2 * p + 1] >= m.nk) return DMK_ERR_INVALID;
        mask[p] = -1;
    }
    for (int i = 0; i < npairs; ++i) {
        if (mask[i] != -1) continue;
        const int na = m.minus(pairs[2 * i]), nb = m.minus(pairs[2 * i + 1]);
        for (int j = i + 1; j < npairs; ++j) {
            if (pairs[2 * j] == na && pairs[2 * j + 1] == nb) {
                mask[i] = j;
                mask[j] = -2;
                break;
            }
        }
    }
    return DMK_OK;
}

int dmk_eri_plan(const int mesh[3], int tr, int32_t *plan, int64_t capacity, int64_t *nrec) {
    Mesh m(mesh);
    if (!m.ok() || !nrec) return DMK_ERR_INVALID;
    std::vector<int> w;
    tr_weights(m, tr, w);
    std::vector<char> visited(m.nk);
    int64_t n = 0;
    for (int kL = 0; kL < m.nk; ++kL) {
        if (w[kL] <= 0) continue;
        std::fill(visited.begin(), visited.end(), 0);
        for (int i = 0; i < m.nk; ++i) {
            if (visited[i]) continue;
            visited[i] = 1;
            const int j = m.combine(i, kL, -1);
            int jm = -1, sym = 0;
            if (tr) {
                jm = m.minus(j);
                sym = visited[jm] ? 0 : 1;
            }
            if (plan) {
                if (n >= capacity) return DMK_ERR_INVALID;
                int32_t *r = plan + 5 * n;
                r[0] = kL; r[1] = i; r[2] = j; r[3] = jm; r[4] = sym;
            }
            ++n;
            if (tr) visited[jm] = 1;
        }
    }
    *nrec = n;
    return DMK_OK;
}

int dmk_assign_workload(const int mesh[3], int tr, int nranks, int rank, int32_t *kl, int *n_out) {
    Mesh m(mesh);
    if (!m.ok() || nranks <= 0 || rank < 0 || rank >= nranks || !n_out) return DMK_ERR_INVALID;
    std::vector<int> w, idx1, idx2;
    tr_weights(m, tr, w);
    for (int i = 0; i < m.nk; ++i) {
        if (w[i] == 1) idx1.push_back(i);
        else if (w[i] == 2) idx2.push_back(i);
    }
    const int nibz = (int)(idx1.size() + idx2.size());
    const int neach = nibz / nranks, extras = nibz % nranks;
    std::vector<std::vector<int>> kids(nranks);
    for (size_t i = 0; i < idx1.size(); ++i) kids[i % nranks].push_back(idx1[i]);
    size_t start = 0;
    for (int r = 0; r < nranks; ++r) {
        const int ns = neach + (r < extras ? 1 : 0);
        long long want = (long long)ns - (long long)kids[r].size();
        // python slice semantics of idx_2[start:end] (end may fall below start -> empty)
        long long end = (long long)start + want;
        long long s = std::min<long long>((long long)start, (long long)idx2.size());
        long long e2 = std::min<long long>(std::max<long long>(end, 0), (long long)idx2.size());
        for (long long t = s; t < e2; ++t) kids[r].push_back(idx2[(size_t)t]);
        start = (size_t)std::max<long long>(end, 0);
    }
    *n_out = (int)kids[rank].size();
    if (kl) for (size_t t = 0; t < kids[rank].size(); ++t) kl[t] = kids[rank][t];
    return DMK_OK;
}

}  // extern "C"

// =============================================================================================
// a6 : folds -- full meshes through fold.hip (fused mixed-radix pass); the DFT as a complex GEMM against a cached twiddle
//      matrix below serves k subsets (multi-rank partial folds), axes longer than 16 and DMK_FOLD_FFT=0
// =============================================================================================

namespace {

// P[r][k] = exp(-2 pi i sum_d a_d(k) a_d(r) / n_d), symmetric in (r, k); rows optionally
// restricted to `subset`.
int get_phase(dmk_ctx *ctx, const Mesh &m, const int32_t *subset, int nsub, void **dev) {
    for (auto &p : ctx->phases) {
        if (p.mesh[0] == m.n[0] && p.mesh[1] == m.n[1] && p.mesh[2] == m.n[2] && p.nsub == nsub &&
            (nsub == 0 || std::equal(p.subset.begin(), p.subset.end(), subset))) {
            *dev = p.dev;
            return DMK_OK;
        }
    }
    // common denominator D = lcm(n0, n1, n2)
    auto gcd = [](long long a, long long b) { while (b) { long long t = a % b; a = b; b = t; } return a; };
    long long D = m.n[0];
    D = D / gcd(D, m.n[1]) * m.n[1];
    D = D / gcd(D, m.n[2]) * m.n[2];
    const int rows = nsub > 0 ? nsub : m.nk;
    std::vector<double> tw((size_t)2 * D);
    for (long long t = 0; t < D; ++t) {
        const long double ang = -2.0L * 3.141592653589793238462643383279502884L * (long double)t / (long double)D;
        tw[2 * t] = (double)cosl(ang);
        tw[2 * t + 1] = (double)sinl(ang);
    }
    // exact values on the axes
    for (long long t = 0; t < D; ++t) {
        if ((4 * t) % D == 0) {
            const int q = (int)((4 * t) / D);   // angle = -q*pi/2
            const double c[4] = {1, 0, -1, 0}, s[4] = {0, -1, 0, 1};
            tw[2 * t] = c[q]; tw[2 * t + 1] = s[q];
        }
    }
    std::vector<double> host((size_t)2 * rows * m.nk);
    for (int rr = 0; rr < rows; ++rr) {
        const int r = nsub > 0 ? subset[rr] : rr;
        if (r < 0 || r >= m.nk) return dmk_fail(ctx, DMK_ERR_INVALID, "fold: k subset index out of range");
        int a[3];
        m.ints(r, a);
        for (int k = 0; k < m.nk; ++k) {
            int b[3];
            m.ints(k, b);
            long long t = 0;
            for (int d = 0; d < 3; ++d) t += (long long)a[d] * b[d] % m.n[d] * (D / m.n[d]);
            t %= D;
            host[2 * ((size_t)rr * m.nk + k)] = tw[2 * t];
            host[2 * ((size_t)rr * m.nk + k) + 1] = tw[2 * t + 1];
        }
    }
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, host.size() * sizeof(double));
    if (e != hipSuccess) return dmk_fail(ctx, DMK_ERR_NOMEM, "fold: phase allocation failed");
    DMK_HIP(ctx, hipMemcpyAsync(d, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    dmk_ctx::Phase ph;
    ph.mesh[0] = m.n[0]; ph.mesh[1] = m.n[1]; ph.mesh[2] = m.n[2];
    ph.dir = 0; ph.nsub = nsub;
    if (nsub > 0) ph.subset.assign(subset, subset + nsub);
    ph.dev = d;
    ctx->phases.push_back(ph);
    *dev = d;
    return DMK_OK;
}

}  // namespace

extern "C" {

int dmk_fold_R2k(dmk_ctx *ctx, const int mesh[3], int64_t ncol, int batch, const void *in_R, int in_is_complex,
                 void *out_k) {
    if (!ctx) return DMK_ERR_INVALID;
    Mesh m(mesh);
    if (!m.ok() || ncol <= 0 || batch <= 0 || !in_R || !out_k || ncol > 0x7fffffffLL)
        return dmk_fail(ctx, DMK_ERR_INVALID, "fold_R2k: bad arguments");
    {
        int rf = launch_fold_fft(ctx, m.n, ncol, batch, in_R, in_is_complex ? 0 : 1, out_k, 0, 0, nullptr);
        if (rf != 0) return rf < 0 ? rf : DMK_OK;
    }
    void *P = nullptr;
    int rc = get_phase(ctx, m, nullptr, 0, &P);
    if (rc) return rc;
    ZGemm g;
    g.M = m.nk; g.N = (int)ncol; g.K = m.nk; g.batch = batch; g.nseg = 1;
    g.seg[0].A = P; g.seg[0].lda = m.nk; g.seg[0].strideA = 0; g.seg[0].a_kmajor = 1;   // A[kdim=R][m=k] = P[R][k]
    g.seg[0].B = in_R; g.seg[0].ldb = ncol; g.seg[0].strideB = (int64_t)m.nk * ncol; g.seg[0].b_kmajor = 1;
    g.seg[0].b_real = in_is_complex ? 0 : 1;
    g.alpha = 1.0; g.epi = ZEPI_STORE; g.C = out_k; g.ldc = ncol; g.strideC = (int64_t)m.nk * ncol;
    return launch_zgemm(ctx, g, DMK_FAM_FOLD);
}

static int fold_k2R_impl(dmk_ctx *ctx, const int mesh[3], int64_t ncol, int batch, const void *in_k, void *out,
                         int real_out, double *imag_max, const int32_t *subset, int nsub) {
    if (!ctx) return DMK_ERR_INVALID;
    Mesh m(mesh);
    if (!m.ok() || ncol <= 0 || batch <= 0 || !in_k || !out || ncol > 0x7fffffffLL || nsub < 0 || nsub > m.nk)
        return dmk_fail(ctx, DMK_ERR_INVALID, "fold_k2R: bad arguments");
    if (imag_max) DMK_HIP(ctx, hipMemsetAsync(imag_max, 0, sizeof(double), ctx->stream));
    if (!(subset && nsub > 0)) {                 // a full mesh: the fused mixed-radix kernel; a k subset is not a mesh
        int rf = launch_fold_fft(ctx, m.n, ncol, batch, in_k, 0, out, real_out, 1, imag_max);
        if (rf != 0) return rf < 0 ? rf : DMK_OK;
    }
    void *P = nullptr;
    int rc = get_phase(ctx, m, subset, subset ? nsub : 0, &P);
    if (rc) return rc;
    const int kin = (subset && nsub > 0) ? nsub : m.nk;
    ZGemm g;
    g.M = m.nk; g.N = (int)ncol; g.K = kin; g.batch = batch; g.nseg = 1;
    // out[R] = (1/N) sum_k conj(P[k][R]) in[k]  ->  A[kdim=k][m=R] = conj(P[k][R])
    g.seg[0].A = P; g.seg[0].lda = m.nk; g.seg[0].strideA = 0; g.seg[0].a_kmajor = 1; g.seg[0].conjA = 1;
    g.seg[0].B = in_k; g.seg[0].ldb = ncol; g.seg[0].strideB = (int64_t)kin * ncol; g.seg[0].b_kmajor = 1;
    g.alpha = 1.0 / (double)m.nk;
    g.epi = real_out ? ZEPI_STORE_REAL : ZEPI_STORE;
    g.C = out; g.ldc = ncol; g.strideC = (int64_t)m.nk * ncol; g.imag_max = imag_max;
    return launch_zgemm(ctx, g, DMK_FAM_FOLD);
}

int dmk_fold_k2R(dmk_ctx *ctx, const int mesh[3], int64_t ncol, int batch, const void *in_k, double *out_R,
                 double *imag_max_dev, const int32_t *k_subset_host, int nsub) {
    return fold_k2R_impl(ctx, mesh, ncol, batch, in_k, out_R, 1, imag_max_dev, k_subset_host, nsub);
}
int dmk_fold_k2R_complex(dmk_ctx *ctx, const int mesh[3], int64_t ncol, int batch, const void *in_k, void *out_R) {
    return fold_k2R_impl(ctx, mesh, ncol, batch, in_k, out_R, 0, nullptr, nullptr, 0);
}

// =============================================================================================
// a9 / a10 : generic batched complex product
// =============================================================================================

namespace {
// C[e] = alpha * sum_s part[s][e]: the reduction of a split-K product (fixed order: deterministic)
__global__ void splitk_reduce_kernel(long long nelem, int nsplit, double alpha, const double2 *__restrict__ part, double2 *__restrict__ C) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nelem; e += (long long)gridDim.x * blockDim.x) {
        double re = 0.0, im = 0.0;
        for (int sidx = 0; sidx < nsplit; ++sidx) {
            const double2 v = part[(long long)sidx * nelem + e];
            re += v.x;
            im += v.y;
        }
        C[e] = make_double2(alpha * re, alpha * im);
    }
}
}  // namespace

int dmk_zgemm_batched(dmk_ctx *ctx, int opA, int opB, int M, int N, int K, int batch, double alpha, const void *A,
                      int64_t strideA, const void *B, int64_t strideB, void *C, int64_t strideC) {
    if (!ctx) return DMK_ERR_INVALID;
    if (opA < 0 || opA > 2 || opB < 0 || opB > 2 || M < 0 || N < 0 || K < 0 || batch < 0)
        return dmk_fail(ctx, DMK_ERR_INVALID, "zgemm_batched: bad arguments");
    if (M == 0 || N == 0 || batch == 0) return DMK_OK;
    // SPLIT-K for the long-K folds (1/nk) sum_k B_k^H T_k written as ONE product with K = nk * nlo (slater.py:682-704): at C5
    // M = N = 256, K = 43 200, two spins -- 32 workgroups of 64 x 64 tiles on 256 CUs, 5.6 ms per call.  K is cut into `ns` equal
    // chunks that become the batch of one launch per original batch element (partial products in the context's second scratch),
    // then summed in a fixed order.  Only for K-major operands (op(A) = T | C, op(B) = N) and few, small output matrices.
    if (opA != 0 && opB == 0 && K >= 4096 && batch <= 4 && (long long)M * N <= (1 << 18)) {
        int ns = 0;
        for (int cand = 128; cand >= 8; --cand)
            if (K % cand == 0 && K / cand >= 128) { ns = cand; break; }
        void *part = nullptr;
        if (ns && dmk_scratch2(ctx, (size_t)ns * M * N * sizeof(double2), &part) == DMK_OK) {
            const int kc = K / ns;
            const long long nelem = (long long)M * N;
            for (int b = 0; b < batch; ++b) {
                ZGemm gs;
                gs.M = M; gs.N = N; gs.K = kc; gs.batch = ns; gs.nseg = 1;
                ZSeg &ss = gs.seg[0];
                ss.A = reinterpret_cast<const double2 *>(A) + (long long)b * strideA; ss.a_kmajor = 1; ss.lda = M; ss.conjA = (opA == 2);
                ss.strideA = (int64_t)kc * M;
                ss.B = reinterpret_cast<const double2 *>(B) + (long long)b * strideB; ss.b_kmajor = 1; ss.ldb = N;
                ss.strideB = (int64_t)kc * N;
                gs.alpha = 1.0; gs.epi = ZEPI_STORE; gs.C = part; gs.ldc = N; gs.strideC = nelem;
                int rc = launch_zgemm(ctx, gs, DMK_FAM_ZGEMM_SMALL);
                if (rc) return rc;
                FamScope fs(ctx, DMK_FAM_ZGEMM_SMALL);
                hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)std::min<long long>((nelem + 255) / 256, 1024)), dim3(256), 0,
                                   ctx->stream, nelem, ns, alpha, reinterpret_cast<const double2 *>(part),
                                   reinterpret_cast<double2 *>(C) + (long long)b * strideC);
                DMK_CHECK_LAUNCH(ctx);
            }
            return DMK_OK;
        }
    }
    ZGemm g;
    g.M = M; g.N = N; g.K = K; g.batch = batch; g.nseg = 1;
    ZSeg &s = g.seg[0];
    s.A = A; s.B = B; s.strideA = strideA; s.strideB = strideB;
    if (opA == 0) { s.a_kmajor = 0; s.lda = K; } else { s.a_kmajor = 1; s.lda = M; s.conjA = (opA == 2); }
    if (opB == 0) { s.b_kmajor = 1; s.ldb = N; } else { s.b_kmajor = 0; s.ldb = K; s.conjB = (opB == 2); }
    g.alpha = alpha; g.epi = ZEPI_STORE; g.C = C; g.ldc = N; g.strideC = strideC;
    if (K == 0) {
        DMK_HIP(ctx, hipMemsetAsync(C, 0, (size_t)16 * ((size_t)(batch - 1) * strideC + (size_t)M * N), ctx->stream));
        return DMK_OK;
    }
    return launch_zgemm(ctx, g, DMK_FAM_ZGEMM_SMALL);
}

int dmk_occ_density(dmk_ctx *ctx, int n, int batch, const void *Vt, const double *occ, void *rho) {
    if (!ctx) return DMK_ERR_INVALID;
    if (n <= 0 || batch <= 0 || !Vt || !occ || !rho) return dmk_fail(ctx, DMK_ERR_INVALID, "occ_density: bad arguments");
    // rho[i][j] = sum_m Vt[m][i] occ[m] conj(Vt[m][j])   (routine/mfd.py:357)
    ZGemm g;
    g.M = n; g.N = n; g.K = n; g.batch = batch; g.nseg = 1;
    ZSeg &s = g.seg[0];
    s.A = Vt; s.lda = n; s.strideA = (int64_t)n * n; s.a_kmajor = 1;
    s.B = Vt; s.ldb = n; s.strideB = (int64_t)n * n; s.b_kmajor = 1; s.conjB = 1; s.kscaleB = occ;
    g.alpha = 1.0; g.epi = ZEPI_STORE; g.C = rho; g.ldc = n; g.strideC = (int64_t)n * n;
    return launch_zgemm(ctx, g, DMK_FAM_ZGEMM_SMALL);
}

int dmk_dgemm_tn_acc(dmk_ctx *ctx, int N, int K, double alpha, const double *X, const double *Y, int64_t ldxy,
                     double *C, int64_t ldc) {
    if (!ctx) return DMK_ERR_INVALID;
    if (N < 0 || K < 0 || !X || !Y || !C) return dmk_fail(ctx, DMK_ERR_INVALID, "dgemm_tn_acc: bad arguments");
    return dmk_dgemm_tn_acc_skip(ctx, N, N, K, alpha, X, ldxy, Y, ldxy, C, ldc, 0);
}

int dmk_dgemm_tn_acc_rect(dmk_ctx *ctx, int M, int N, int K, double alpha, const double *X, int64_t ldx,
                          const double *Y, int64_t ldy, double *C, int64_t ldc) {
    if (!ctx) return DMK_ERR_INVALID;
    if (M < 0 || N < 0 || K < 0 || !X || !Y || !C) return dmk_fail(ctx, DMK_ERR_INVALID, "dgemm_tn_acc_rect: bad arguments");
    return dmk_dgemm_tn_acc_skip(ctx, M, N, K, alpha, X, ldx, Y, ldy, C, ldc, 0);
}

int dmk_dgemm_tn_acc_skip(dmk_ctx *ctx, int M, int N, int K, double alpha, const double *X, int64_t ldx, const double *Y,
                          int64_t ldy, double *C, int64_t ldc, int skip_tiles) {
    if (!ctx) return DMK_ERR_INVALID;
    if (M < 0 || N < 0 || K < 0 || !X || !Y || !C || skip_tiles < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "dgemm_tn_acc_skip: bad arguments");
    DgemmTn g;
    g.M = M; g.N = N; g.K = K; g.alpha = alpha;
    g.X = X; g.ldx = ldx; g.Y = Y; g.ldy = ldy; g.C = C; g.ldc = ldc; g.skip_tiles = skip_tiles;
    return launch_dgemm_tn_acc(ctx, g);
}

int dmk_df_block_philox(dmk_ctx *ctx, uint64_t seed, int ki, int kj, int naux, int nao, void *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (naux <= 0 || nao <= 0 || !out || ki < 0 || kj < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "df_block_philox: bad arguments");
    return launch_philox_block(ctx, seed, ki, kj, naux, nao, out);
}

int dmk_df_blocks_philox_on(dmk_ctx *ctx, void *stream, uint64_t seed, int nblk, const int32_t *ij, int naux, int nao, void *out,
                            int64_t stride_bytes) {
    if (!ctx) return DMK_ERR_INVALID;
    if (naux <= 0 || nao <= 0 || !out || !ij || nblk < 0 || stride_bytes < (int64_t)naux * nao * nao * 16 || (stride_bytes & 15))
        return dmk_fail(ctx, DMK_ERR_INVALID, "df_blocks_philox_on: bad arguments");
    for (int b = 0; b < 2 * nblk; ++b)
        if (ij[b] < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "df_blocks_philox_on: negative k-point index");
    return launch_philox_blocks_on(ctx, reinterpret_cast<hipStream_t>(stream), seed, nblk, ij, naux, nao, out, stride_bytes);
}

int dmk_df_block_philox_on(dmk_ctx *ctx, void *stream, uint64_t seed, int ki, int kj, int naux, int nao, void *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (naux <= 0 || nao <= 0 || !out || ki < 0 || kj < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "df_block_philox_on: bad arguments");
    return launch_philox_block_on(ctx, reinterpret_cast<hipStream_t>(stream), seed, ki, kj, naux, nao, out);
}

}  // extern "C"

// =============================================================================================
// small utility kernels: transpose, restore
// =============================================================================================

namespace {

__global__ void transpose_c128_kernel(int rows, int cols, const double2 *__restrict__ in, double2 *__restrict__ out) {
    __shared__ double2 tile[32][33];
    const size_t boff = (size_t)blockIdx.z * rows * cols;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int y = threadIdx.y; y < 32; y += blockDim.y) {
        const int r = r0 + y, c = c0 + threadIdx.x;
        if (r < rows && c < cols) tile[y][threadIdx.x] = in[boff + (size_t)r * cols + c];
    }
    __syncthreads();
    for (int y = threadIdx.y; y < 32; y += blockDim.y) {
        const int c = c0 + y, r = r0 + threadIdx.x;
        if (r < rows && c < cols) out[boff + (size_t)c * rows + r] = tile[threadIdx.x][y];
    }
}

// 4-fold (npair x npair) -> 1-fold (n^4): out[i][j][k][l] = eri4[pair(i,j)][pair(k,l)]
__global__ void restore_4to1_kernel(int n, const double *__restrict__ e4, double *__restrict__ out) {
    const long long total = (long long)n * n * n * n;
    const long long npair = (long long)n * (n + 1) / 2;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int l = (int)(t % n), k = (int)((t / n) % n), j = (int)((t / ((long long)n * n)) % n),
                  i = (int)(t / ((long long)n * n * n));
        const long long ij = i >= j ? (long long)i * (i + 1) / 2 + j : (long long)j * (j + 1) / 2 + i;
        const long long kl = k >= l ? (long long)k * (k + 1) / 2 + l : (long long)l * (l + 1) / 2 + k;
        out[t] = e4[ij * npair + kl];
    }
}

// 4-fold -> 8-fold: out[p(p+1)/2 + q] = eri4[p][q], p >= q
__global__ void restore_4to8_kernel(long long npair, const double *__restrict__ e4, double *__restrict__ out) {
    const long long total = npair * (npair + 1) / 2;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        int p, q;
        dmk_tril_rc(t, p, q);
        out[t] = e4[(long long)p * npair + q];
    }
}

}  // namespace

extern "C" {

int dmk_transpose_c128(dmk_ctx *ctx, int rows, int cols, int batch, const void *in, void *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (rows <= 0 || cols <= 0 || batch <= 0 || !in || !out || batch > 65535)
        return dmk_fail(ctx, DMK_ERR_INVALID, "transpose: bad arguments");
    FamScope fs(ctx, DMK_FAM_MISC);
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch), block(32, 8);
    hipLaunchKernelGGL(transpose_c128_kernel, grid, block, 0, ctx->stream, rows, cols,
                       reinterpret_cast<const double2 *>(in), reinterpret_cast<double2 *>(out));
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

int dmk_eri_restore(dmk_ctx *ctx, int nemb, int symmetry, const double *eri4, double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (nemb <= 0 || !eri4 || !out) return dmk_fail(ctx, DMK_ERR_INVALID, "eri_restore: bad arguments");
    const long long npair = (long long)nemb * (nemb + 1) / 2;
    FamScope fs(ctx, DMK_FAM_MISC);
    if (symmetry == 4) {
        DMK_HIP(ctx, hipMemcpyAsync(out, eri4, (size_t)npair * npair * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    } else if (symmetry == 1) {
        hipLaunchKernelGGL(restore_4to1_kernel, dim3(2048), dim3(256), 0, ctx->stream, nemb, eri4, out);
        DMK_CHECK_LAUNCH(ctx);
    } else if (symmetry == 8) {
        hipLaunchKernelGGL(restore_4to8_kernel, dim3(2048), dim3(256), 0, ctx->stream, npair, eri4, out);
        DMK_CHECK_LAUNCH(ctx);
    } else {
        return dmk_fail(ctx, DMK_ERR_INVALID, "eri_restore: symmetry must be 1, 4 or 8");
    }
    return DMK_OK;
}

}  // extern "C"

// ---- row gather / scatter (k-sharded mean field: this rank's k rows of the resident Fock batch; eigenvalues of a shard
//      placed into the all-k table before the all-reduce) ------------------------------------------------------------
namespace {
__global__ void copy_rows_kernel(long long nrows, long long row_len, const int *__restrict__ idx, const double *__restrict__ in,
                                 double *__restrict__ out, int scatter) {
    const long long total = nrows * row_len;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long r = t / row_len, c = t - r * row_len;
        const long long far = (long long)idx[r] * row_len + c;
        if (scatter) out[far] = in[t];
        else out[t] = in[far];
    }
}
}  // namespace

extern "C" int dmk_copy_rows_f64(dmk_ctx *ctx, int64_t nrows, int64_t row_len, const int32_t *idx_dev, const double *in, double *out,
                                 int scatter) {
    if (!ctx) return DMK_ERR_INVALID;
    if (nrows < 0 || row_len < 0 || !idx_dev || !in || !out) return dmk_fail(ctx, DMK_ERR_INVALID, "copy_rows: bad arguments");
    if (nrows == 0 || row_len == 0) return DMK_OK;
    const long long total = (long long)nrows * row_len;
    const unsigned grid = (unsigned)std::min<long long>((total + 255) / 256, 65536);
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(copy_rows_kernel, dim3(grid), dim3(256), 0, ctx->stream, (long long)nrows, (long long)row_len, idx_dev, in, out,
                       scatter ? 1 : 0);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}
