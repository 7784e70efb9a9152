// K18 -- embedded Hartree-Fock on the device: the SCF driver.
//
// Replaces the PySCF kernel behind the reference's SCF.HF (solver/scf.py:954-1043: RIHF / UIHF, :231-253, :354-460).
//
// dmk_scf           the handle owns h1, overlap, S^-1/2, densities, Fock matrices, orbitals and the DIIS ring (one allocation); the
//                   ERI blocks are borrowed.  An iteration reads back ONE record (two energy sums and the new row of the DIIS
//                   matrix, at most DIIS_MAX + 2 doubles); nothing of size n^2 crosses to the host inside the loop.
// Fock build        scf_veff calls dmk_fock_s4 (jk.hip: J and K of a block from one pass over it), or two dmk_jk_s4 passes per block
//                   under DMK_SCF_TWO_PASS; the alpha-beta block needs J only and goes through dmk_jk_s4 either way.
// This file holds the driver, the DIIS arithmetic (dmk_diis_coeffs, host) and the small elementwise kernels around them.
#include "devres.h"
#include <algorithm>
#include <cmath>
#include <new>

namespace {

constexpr int NT = 256;
constexpr int DIIS_MAX = 12;
constexpr int NDOT_MAX = DIIS_MAX + 2;

// out = c0 p0 + c1 p1 + c2 p2 (null pointers contribute nothing)
__global__ void scf_lin3_kernel(long long N, double c0, const double *p0, double c1, const double *p1, double c2, const double *p2,
                                double *out) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        if (p0) s = c0 * p0[t];
        if (p1) s = fma(c1, p1[t], s);
        if (p2) s = fma(c2, p2[t], s);
        out[t] = s;
    }
}

// out[b][i][j] = T[b][i][j] - T[b][j][i]
__global__ void scf_antisym_kernel(int n, int batch, const double *__restrict__ T, double *__restrict__ out) {
    const long long nn = (long long)n * n, total = nn * batch;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / nn, e = t % nn;
        const int i = (int)(e / n), j = (int)(e % n);
        out[t] = T[t] - T[b * nn + (long long)j * n + i];
    }
}

struct DotList { int count; const double *a[NDOT_MAX]; const double *b[NDOT_MAX]; };
// out[q] = <a[q], b[q]> over N elements: one workgroup per product, per-thread strided sums combined in a fixed order
__global__ __launch_bounds__(NT) void scf_dots_kernel(long long N, DotList L, double *__restrict__ out) {
    __shared__ double red[NT];
    const double *a = L.a[blockIdx.x], *b = L.b[blockIdx.x];
    double s = 0.0;
    for (long long t = threadIdx.x; t < N; t += NT) s = fma(a[t], b[t], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

struct Combo { int count; double c[DIIS_MAX]; int slot[DIIS_MAX]; };
// out = sum_q c[q] ring[slot[q]]
__global__ void scf_combine_kernel(long long N, Combo C, const double *__restrict__ ring, double *__restrict__ out) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < N; t += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int q = 0; q < C.count; ++q) s = fma(C.c[q], ring[(long long)C.slot[q] * N + t], s);
        out[t] = s;
    }
}

// symmetric eigenproblem of a small matrix by cyclic Jacobi (host): A (m x m, destroyed) -> w, V (columns)
void host_jacobi(int m, double *A, double *w, double *V) {
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) V[i * m + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < i; ++j) off += A[i * m + j] * A[i * m + j];
        if (off < 1e-300) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[p * m + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * m + q] - A[p * m + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < m; ++k) {
                    const double akp = A[k * m + p], akq = A[k * m + q];
                    A[k * m + p] = c * akp - s * akq;
                    A[k * m + q] = s * akp + c * akq;
                }
                for (int k = 0; k < m; ++k) {
                    const double apk = A[p * m + k], aqk = A[q * m + k];
                    A[p * m + k] = c * apk - s * aqk;
                    A[q * m + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < m; ++k) {
                    const double vkp = V[k * m + p], vkq = V[k * m + q];
                    V[k * m + p] = c * vkp - s * vkq;
                    V[k * m + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < m; ++i) w[i] = A[i * m + i];
}

}  // namespace

struct dmk_scf {
    dmk_ctx *ctx = nullptr;
    int n = 0, ns = 1, nx = 0, diis_dim = DIIS_MAX, flags = 0;
    const double *eri[3] = {nullptr, nullptr, nullptr};
    int64_t ld = 0;
    DevMem mem;
    // all (ns, n, n) unless noted
    double *h1 = nullptr, *h1e = nullptr, *S = nullptr, *X = nullptr;      // S, X: (nx, n, n)
    double *D = nullptr, *F = nullptr, *V = nullptr, *Fx = nullptr, *C = nullptr, *T1 = nullptr, *T2 = nullptr;
    double *w = nullptr;                                                   // (ns, n)
    double *vj = nullptr, *vk = nullptr;                                   // (4, n, n), (2, n, n)
    double *ringF = nullptr, *ringE = nullptr;                             // (diis_dim, ns, n, n)
    double *rec = nullptr;                                                 // NDOT_MAX doubles
    long long nn() const { return (long long)n * n; }
    long long N() const { return nn() * ns; }
};

namespace {

int scf_lin3(dmk_scf *h, long long N, double c0, const double *p0, double c1, const double *p1, double c2, const double *p2, double *out) {
    hipLaunchKernelGGL(scf_lin3_kernel, dim3(dmk_grid1d(N, 4096)), dim3(256), 0, h->ctx->stream, N, c0, p0, c1, p1, c2, p2, out);
    DMK_CHECK_LAUNCH(h->ctx);
    return DMK_OK;
}

// batched n x n product over the spin channels; a stride of 0 shares one matrix
int scf_mm(dmk_scf *h, int opA, int opB, const double *A, long long sA, const double *B, long long sB, double *Cm) {
    const int n = h->n;
    return dmk_dgemm_batched(h->ctx, opA, opB, n, n, n, h->ns, 1.0, A, n, sA, B, n, sB, 0.0, Cm, n, h->nn());
}

// V = veff(Dm) with exchange scaled by alpha: RHF vj - alpha/2 vk of the spin-traced density, UHF vj_s + vj_s' - alpha vk_s
int scf_veff(dmk_scf *h, const double *Dm, double alpha, double *V) {
    dmk_ctx *ctx = h->ctx;
    const int n = h->n;
    const long long nn = h->nn();
    const bool fused = !(h->flags & DMK_SCF_TWO_PASS);
    int rc;
    for (int s = 0; s < h->ns; ++s) {
        const double *d = Dm + s * nn;
        double *j = h->vj + s * nn, *k = h->vk + s * nn;
        if (fused) rc = dmk_fock_s4(ctx, n, h->eri[s], h->ld, d, d, j, k);
        else {
            rc = dmk_jk_s4(ctx, n, h->eri[s], h->ld, d, nullptr, nullptr, j, nullptr, nullptr);
            if (!rc) rc = dmk_jk_s4(ctx, n, h->eri[s], h->ld, nullptr, nullptr, d, nullptr, nullptr, k);
        }
        if (rc) return rc;
    }
    if (h->ns == 1) return scf_lin3(h, nn, 1.0, h->vj, -0.5 * alpha, h->vk, 0.0, nullptr, V);
    // the alpha-beta block, both directions in one stream: J on alpha from D_b (rows), J on beta from D_a (columns)
    rc = dmk_jk_s4(ctx, n, h->eri[2], h->ld, Dm + nn, Dm, nullptr, h->vj + 2 * nn, h->vj + 3 * nn, nullptr);
    if (rc) return rc;
    for (int s = 0; s < 2; ++s) {
        rc = scf_lin3(h, nn, 1.0, h->vj + s * nn, 1.0, h->vj + (2 + s) * nn, -alpha, h->vk + s * nn, V + s * nn);
        if (rc) return rc;
    }
    return DMK_OK;
}

// orbitals of Fm: C rows = eigenvectors (generalised problem through X = S^-1/2), w ascending
int scf_eig(dmk_scf *h, const double *Fm) {
    dmk_ctx *ctx = h->ctx;
    const long long sx = h->nx == 2 ? h->nn() : 0;
    int rc;
    if (!h->nx) return dmk_eigh_batched_real(ctx, h->n, h->ns, Fm, h->w, h->C);
    if ((rc = scf_mm(h, 0, 0, Fm, h->nn(), h->X, sx, h->T1))) return rc;
    if ((rc = scf_mm(h, 1, 0, h->X, sx, h->T1, h->nn(), h->T2))) return rc;
    if ((rc = dmk_eigh_batched_real(ctx, h->n, h->ns, h->T2, h->w, h->T1))) return rc;
    return scf_mm(h, 0, 1, h->T1, h->nn(), h->X, sx, h->C);          // rows: (X c)^T = c^T X^T
}

// D[s] = f sum_{m < nocc[s]} c_m c_m^T
int scf_density(dmk_scf *h, const int *nocc) {
    const int n = h->n;
    const double f = h->ns == 1 ? 2.0 : 1.0;
    for (int s = 0; s < h->ns; ++s) {
        double *D = h->D + s * h->nn();
        if (nocc[s] == 0) { DMK_HIP(h->ctx, hipMemsetAsync(D, 0, (size_t)h->nn() * 8, h->ctx->stream)); continue; }
        const double *Cs = h->C + s * h->nn();
        int rc = dmk_dgemm_batched(h->ctx, 1, 0, n, n, nocc[s], 1, f, Cs, n, 0, Cs, n, 0, 0.0, D, n, 0);
        if (rc) return rc;
    }
    return DMK_OK;
}

// out = X^T (F D S - S D F) X per spin (the commutator in the orthonormal basis); uses T1, T2
int scf_error(dmk_scf *h, double *out) {
    const long long nn = h->nn(), sx = h->nx == 2 ? nn : 0;
    int rc;
    if ((rc = scf_mm(h, 0, 0, h->F, nn, h->D, nn, h->T1))) return rc;
    double *fds = h->T1, *other = h->T2;
    if (h->nx) {
        if ((rc = scf_mm(h, 0, 0, h->T1, nn, h->S, sx, h->T2))) return rc;
        fds = h->T2; other = h->T1;
    }
    double *comm = h->nx ? other : out;
    hipLaunchKernelGGL(scf_antisym_kernel, dim3(dmk_grid1d(h->N(), 4096)), dim3(256), 0, h->ctx->stream, h->n, h->ns, fds, comm);
    DMK_CHECK_LAUNCH(h->ctx);
    if (!h->nx) return DMK_OK;
    if ((rc = scf_mm(h, 0, 0, comm, nn, h->X, sx, fds))) return rc;
    return scf_mm(h, 1, 0, h->X, sx, fds, nn, out);
}

}  // namespace

extern "C" {

int dmk_diis_coeffs(int m, const double *B_host, double *c_host) {
    if (m <= 0 || m > DIIS_MAX || !B_host || !c_host) return DMK_ERR_INVALID;
    const int d = m + 1;
    double scale = 0.0;
    for (int i = 0; i < m; ++i) scale = std::max(scale, std::fabs(B_host[i * m + i]));
    if (!(scale > 0.0) || !std::isfinite(scale)) {          // no error left (or nothing usable): the newest matrix alone
        for (int i = 0; i < m; ++i) c_host[i] = 0.0;
        c_host[m - 1] = 1.0;
        return DMK_OK;
    }
    double A[(DIIS_MAX + 1) * (DIIS_MAX + 1)], V[(DIIS_MAX + 1) * (DIIS_MAX + 1)], w[DIIS_MAX + 1];
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) A[i * d + j] = 0.5 * (B_host[i * m + j] + B_host[j * m + i]) / scale;
    for (int i = 0; i < m; ++i) A[i * d + m] = A[m * d + i] = 1.0;
    A[m * d + m] = 0.0;
    host_jacobi(d, A, w, V);
    // pseudo-inverse applied to (0, ..., 0, 1): directions with |w| <= 1e-13 (of a matrix scaled to unit diagonal) are dropped
    for (int i = 0; i < m; ++i) c_host[i] = 0.0;
    for (int k = 0; k < d; ++k) {
        if (std::fabs(w[k]) <= 1e-13) continue;
        const double g = V[m * d + k] / w[k];
        for (int i = 0; i < m; ++i) c_host[i] += V[i * d + k] * g;
    }
    double sum = 0.0;
    for (int i = 0; i < m; ++i) sum += c_host[i];
    if (!std::isfinite(sum) || std::fabs(sum) < 1e-8) return DMK_ERR_NOCONV;
    for (int i = 0; i < m; ++i) c_host[i] /= sum;
    return DMK_OK;
}

int dmk_scf_create(dmk_ctx *ctx, int n, int nspin, const double *h1, const double *h1_energy, const double *ovlp, const double *xorth,
                   int novlp, const double *eri_aa, const double *eri_bb, const double *eri_ab, int64_t ld, int diis_dim, int flags,
                   dmk_scf **out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (out) *out = nullptr;
    const long long npair = (long long)n * (n + 1) / 2;
    if (!out || n <= 0 || n > 512 || (nspin != 1 && nspin != 2) || !h1 || !eri_aa || ld < npair)
        return dmk_fail(ctx, DMK_ERR_INVALID, "scf_create: bad arguments (1 <= n <= 512, nspin 1 | 2, h1, the aa block, ld >= npair)");
    if (nspin == 2 && (!eri_bb || !eri_ab)) return dmk_fail(ctx, DMK_ERR_INVALID, "scf_create: UHF needs the bb and ab blocks");
    if (novlp < 0 || novlp > nspin || (novlp > 0 && (!ovlp || !xorth)) )
        return dmk_fail(ctx, DMK_ERR_INVALID, "scf_create: novlp overlap matrices (0: identity, 1, or one per spin) with their S^-1/2");
    if (diis_dim < 1 || diis_dim > DIIS_MAX) return dmk_fail(ctx, DMK_ERR_INVALID, "scf_create: 1 <= diis_dim <= %d", DIIS_MAX);
    dmk_scf *h = new (std::nothrow) dmk_scf;
    if (!h) return dmk_fail(ctx, DMK_ERR_NOMEM, "scf_create: host allocation failed");
    h->ctx = ctx; h->n = n; h->ns = nspin; h->nx = novlp; h->diis_dim = diis_dim; h->flags = flags;
    h->eri[0] = eri_aa; h->eri[1] = eri_bb; h->eri[2] = eri_ab; h->ld = ld;
    const size_t nn = (size_t)n * n, N = nn * nspin;
    // every array starts on a 256-byte boundary of the one allocation; a first pass over a null base gives the size
    auto carve = [&](double *base) {
        double *p = base;
        auto take = [&](size_t cnt) { double *q = p; p += (cnt + 31) & ~(size_t)31; return q; };
        h->h1 = take(N); h->h1e = take(N); h->D = take(N); h->F = take(N); h->V = take(N); h->Fx = take(N); h->C = take(N);
        h->T1 = take(N); h->T2 = take(N);
        h->ringF = take(N * diis_dim); h->ringE = take(N * diis_dim);
        h->S = take(nn * novlp); h->X = take(nn * novlp);
        h->w = take((size_t)nspin * n); h->vj = take(4 * nn); h->vk = take(2 * nn); h->rec = take(64);
        return (size_t)(p - base);
    };
    const size_t total = carve(nullptr);
    if (h->mem.alloc(ctx, total * 8) != hipSuccess) {
        (void)hipGetLastError();
        delete h;
        return dmk_fail(ctx, DMK_ERR_NOMEM, "scf_create: no device memory for %zu bytes", total * 8);
    }
    carve(h->mem.get<double>());
    auto copy = [&](double *dst, const double *src, size_t cnt) {
        return cnt ? hipMemcpyAsync(dst, src, cnt * 8, hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess; };
    hipError_t e = copy(h->h1, h1, N);
    if (e == hipSuccess) e = copy(h->h1e, h1_energy ? h1_energy : h1, N);
    if (e == hipSuccess) e = copy(h->S, ovlp, nn * novlp);
    if (e == hipSuccess) e = copy(h->X, xorth, nn * novlp);
    if (e == hipSuccess) e = hipMemsetAsync(h->D, 0, N * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->w, 0, (size_t)nspin * n * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->C, 0, N * 8, ctx->stream);
    if (e == hipSuccess) e = copy(h->F, h1, N);
    if (e == hipSuccess) e = hipMemsetAsync(h->V, 0, N * 8, ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        delete h;
        return dmk_fail(ctx, DMK_ERR_HIP, "scf_create: copying the inputs failed: %s", hipGetErrorString(e));
    }
    *out = h;
    return DMK_OK;
}

int dmk_scf_free(dmk_scf *h) {
    if (!h) return DMK_OK;
    (void)hipStreamSynchronize(h->ctx->stream);      // work that reads the handle's memory may still be queued
    delete h;
    return DMK_OK;
}

int dmk_scf_veff(dmk_scf *h, const double *dm, double alpha, double *veff_out) {
    if (!h) return DMK_ERR_INVALID;
    if (!dm || !veff_out) return dmk_fail(h->ctx, DMK_ERR_INVALID, "scf_veff: bad arguments");
    return scf_veff(h, dm, alpha, veff_out);
}

int dmk_scf_get(dmk_scf *h, int what, double *out) {
    if (!h) return DMK_ERR_INVALID;
    const double *src[] = {h->D, h->F, h->V, h->C, h->w};
    if (what < 0 || what > 4 || !out) return dmk_fail(h->ctx, DMK_ERR_INVALID, "scf_get: what must be one of DMK_SCF_DM .. DMK_SCF_MO_ENERGY");
    const size_t cnt = what == DMK_SCF_MO_ENERGY ? (size_t)h->ns * h->n : (size_t)h->N();
    DMK_HIP(h->ctx, hipMemcpyAsync(out, src[what], cnt * 8, hipMemcpyDeviceToDevice, h->ctx->stream));
    return DMK_OK;
}

int dmk_scf_run(dmk_scf *h, const int *nocc_host, const double *dm0, double alpha, double e_const, int max_iter, double tol,
                double tol_grad, int use_diis, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    const int ns = h->ns, n = h->n;
    if (!nocc_host || !result_host || max_iter < 0 || !(tol > 0.0) || !(tol_grad > 0.0))
        return dmk_fail(ctx, DMK_ERR_INVALID, "scf_run: bad arguments");
    for (int s = 0; s < ns; ++s)
        if (nocc_host[s] < 0 || nocc_host[s] > n) return dmk_fail(ctx, DMK_ERR_INVALID, "scf_run: %d occupied orbitals of %d", nocc_host[s], n);
    const long long N = h->N();
    int rc;
    if (dm0) DMK_HIP(ctx, hipMemcpyAsync(h->D, dm0, (size_t)N * 8, hipMemcpyDeviceToDevice, ctx->stream));
    else {                                              // core-Hamiltonian guess (init_guess_by_1e)
        if ((rc = scf_eig(h, h->h1))) return rc;
        if ((rc = scf_density(h, nocc_host))) return rc;
    }
    if ((rc = scf_veff(h, h->D, alpha, h->V))) return rc;
    double B[DIIS_MAX * DIIS_MAX] = {0.0}, rec[NDOT_MAX];
    double E = 0.0, E_prev = 0.0, gnorm = 0.0;
    int pushed = 0, it = 0;
    bool converged = false;
    for (it = 0;; ++it) {
        if ((rc = scf_lin3(h, N, 1.0, h->h1, 1.0, h->V, 0.0, nullptr, h->F))) return rc;
        const int slot = pushed % h->diis_dim, m = std::min(pushed + 1, h->diis_dim);
        double *eslot = h->ringE + (long long)slot * N;
        if ((rc = scf_error(h, eslot))) return rc;
        DotList L;
        L.count = 2 + (use_diis ? m : 1);
        L.a[0] = h->h1e; L.b[0] = h->D;
        L.a[1] = h->V;   L.b[1] = h->D;
        if (use_diis) {
            DMK_HIP(ctx, hipMemcpyAsync(h->ringF + (long long)slot * N, h->F, (size_t)N * 8, hipMemcpyDeviceToDevice, ctx->stream));
            for (int q = 0; q < m; ++q) { L.a[2 + q] = eslot; L.b[2 + q] = h->ringE + (long long)q * N; }
        } else { L.a[2] = eslot; L.b[2] = eslot; }
        hipLaunchKernelGGL(scf_dots_kernel, dim3(L.count), dim3(NT), 0, ctx->stream, N, L, h->rec);
        DMK_CHECK_LAUNCH(ctx);
        // the one read-back of the iteration: two energy sums and the new row of the DIIS matrix
        DMK_HIP(ctx, hipMemcpyAsync(rec, h->rec, (size_t)L.count * 8, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        E = rec[0] + 0.5 * rec[1] + e_const;
        const double ee = use_diis ? rec[2 + slot] : rec[2];
        gnorm = std::sqrt(std::max(ee, 0.0) * 0.5);
        if (!std::isfinite(E) || !std::isfinite(gnorm)) return dmk_fail(ctx, DMK_ERR_NOCONV, "scf_run: non-finite energy in iteration %d", it);
        if (it > 0 && std::fabs(E - E_prev) < tol && gnorm < tol_grad) { converged = true; break; }
        if (it >= max_iter) break;
        const double *Fd = h->F;
        if (use_diis) {
            for (int q = 0; q < m; ++q) B[slot * DIIS_MAX + q] = B[q * DIIS_MAX + slot] = rec[2 + q];
            ++pushed;
            if (m > 1) {
                double Bm[DIIS_MAX * DIIS_MAX];
                Combo cb;
                for (int a = 0; a < m; ++a)
                    for (int b = 0; b < m; ++b) Bm[a * m + b] = B[a * DIIS_MAX + b];
                if (dmk_diis_coeffs(m, Bm, cb.c) == DMK_OK) {
                    cb.count = m;
                    for (int q = 0; q < m; ++q) cb.slot[q] = q;
                    hipLaunchKernelGGL(scf_combine_kernel, dim3(dmk_grid1d(N, 4096)), dim3(256), 0, ctx->stream, N, cb, h->ringF, h->Fx);
                    DMK_CHECK_LAUNCH(ctx);
                    Fd = h->Fx;
                } else pushed = 0;                       // a subspace without a usable solution is started afresh
            }
        }
        if ((rc = scf_eig(h, Fd))) return rc;
        if ((rc = scf_density(h, nocc_host))) return rc;
        if ((rc = scf_veff(h, h->D, alpha, h->V))) return rc;
        E_prev = E;
    }
    // the state handed back is consistent: canonical orbitals of the last Fock matrix, THEIR density, its veff, Fock matrix and
    // energy (PySCF's closing cycle, scf/hf.py kernel) -- one more pass over the blocks
    const double E_loop = E;
    if ((rc = scf_eig(h, h->F))) return rc;
    if ((rc = scf_density(h, nocc_host))) return rc;
    if ((rc = scf_veff(h, h->D, alpha, h->V))) return rc;
    if ((rc = scf_lin3(h, N, 1.0, h->h1, 1.0, h->V, 0.0, nullptr, h->F))) return rc;
    {
        DotList L;
        L.count = 2;
        L.a[0] = h->h1e; L.b[0] = h->D;
        L.a[1] = h->V;   L.b[1] = h->D;
        hipLaunchKernelGGL(scf_dots_kernel, dim3(L.count), dim3(NT), 0, ctx->stream, N, L, h->rec);
        DMK_CHECK_LAUNCH(ctx);
        DMK_HIP(ctx, hipMemcpyAsync(rec, h->rec, 2 * 8, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        E = rec[0] + 0.5 * rec[1] + e_const;
        if (!std::isfinite(E)) return dmk_fail(ctx, DMK_ERR_NOCONV, "scf_run: non-finite final energy");
        E_prev = E_loop;
    }
    result_host[0] = E;
    result_host[1] = converged ? 1.0 : 0.0;
    result_host[2] = (double)it;
    result_host[3] = gnorm;
    result_host[4] = it > 0 ? E - E_prev : 0.0;
    return DMK_OK;
}

}  // extern "C"
