// K1L -- real symmetric eigensolver for ONE large matrix spread over the whole GPU (dmk_eighl_*).
//
// Replaces scipy.linalg.eigh at routine/slater.py:278 and routine/spinless.py:166-275 (eig-flavoured bath: env-env block of the
// density matrix) and routine/spinless.py:274-349 (bath_opt: the full lattice dimension) above the n = 2000 limit of the
// one-workgroup-per-matrix kernel (eigh.hip).  Both callers need SELECTED eigenpairs only, hence the handle: dmk_eighl_factor
// returns every eigenvalue, the host picks indices with the reference's own comparisons, dmk_eighl_vectors delivers exactly those.
//
//   1. Householder tridiagonalisation, the dsytd2 recurrence of eigh.hip with one kernel boundary per dependency: per column k a
//      one-workgroup kernel (house_kernel) finishes w_{k-1}, applies the pending rank-2 update to row k only and forms the
//      reflector v_k; a grid-wide kernel (update_matvec_kernel) then applies the pending update A -= v w^T + w v^T to the trailing
//      block and, in the same pass over it, forms y = A v_k.  A wave owns whole rows (four at a time, lanes along the row, 16-byte
//      loads), so every y_i is summed in one fixed order: no atomics, bit-reproducible.  No device-wide barrier, no host
//      synchronisation inside the column loop.  The working copy of A (full symmetric storage) ends up holding the reflectors,
//      v_k in row k.  Traffic: the trailing block is read and written once per column, 16 (n - k)^2 bytes.
//   2. all eigenvalues: T is cut into unreduced blocks (host, O(n)), one lane per eigenvalue bisects on the Sturm count
//      (tridiag_eig.h), the host sorts.
//   3. selected eigenvectors of T: one lane per vector runs inverse iteration (pivoted elimination of T - lam I kept lane-major
//      in scratch, hashed start that depends on the eigenvalue's position only, three solves); eigenvalues of a block chained by
//      gaps <= 1e-3 |T| (dstein's criterion) form a cluster, owned by one workgroup: row by row classical Gram-Schmidt applied twice
//      (with further solves where the projection leaves less than half of a vector: degenerate clusters), then a third pass that
//      MEASURES the orthogonality.  Every vector is verified (|T z - lam z|_inf <= 64 n eps |T|, |z| = 1); a
//      rejected one is rebuilt the way dstein does it (perturbed shift, fresh start, re-orthogonalisation inside the iteration);
//      a second failure, like NaN / Inf in the input, is reported as DMK_ERR_NOCONV.
//   4. back-transformation of the m selected vectors: panels of NB = 32 reflectors in compact WY form, Y -= V T (V^T Y), every
//      product a C += alpha X^T Y contraction on the f64 matrix cores (dgemm_tn.hip); O(n^2 m).
#include "common.h"
#include "tridiag_eig.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <vector>

struct dmk_eighl {
    dmk_ctx *ctx = nullptr;
    int n = 0;
    int64_t ld = 0;                 // even leading dimension of the working copy
    double *W = nullptr;            // n x ld: reflector k in row k, columns > k
    double *vec = nullptr;          // d | e | e2 | tau | lam | bnorm | wbuf | ybuf  (8 arrays of ld doubles)
    int *ivec = nullptr;            // bs | be  (2 arrays of n ints) | status[4]
    std::vector<double> lam, bnorm; // host copies (by position in T)
    std::vector<int> bs, be, perm, clus;   // perm[rank] = position; clus[position] = cluster id (chain of close eigenvalues of a block)
};

namespace {

constexpr int NB = 32;            // reflectors per compact-WY panel
constexpr int HNT = 1024;         // threads of the one-workgroup kernels
constexpr int HNW = HNT / 64;
constexpr int UNT = 256;          // threads of the trailing-block kernel
constexpr int ROWS = 4;           // rows per wave and pass
constexpr int MAXGRID = 2048;

// sum over the workgroup, every thread gets it; partials are combined in wave order (deterministic)
template <int NWAVES>
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = dmk_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NWAVES; ++q) s += red[q];
    return s;
}

// W = symmetric completion of the lower triangle of A; the padding column (odd n) is zero
__global__ void init_kernel(int n, const double *__restrict__ A, int64_t lda, double *__restrict__ W, int64_t ld) {
    const size_t total = (size_t)n * ld;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const size_t i = t / ld, j = t % ld;
        double v = 0.0;
        if (j < (size_t)n) v = i >= j ? A[i * lda + j] : A[j * lda + i];
        W[t] = v;
    }
}

// Step k, one workgroup.  (A) k >= 1: w_{k-1} = p + alpha v, p = tau y, alpha = -tau/2 p.v on the indices >= k.  (B) row k with the
// pending update applied on the fly, d[k], and for k < n - 1 the reflector v_k (written over row k), tau[k], e[k].
__global__ __launch_bounds__(HNT) void house_kernel(int n, int k, double *__restrict__ W, int64_t ld, double *__restrict__ d,
                                                    double *__restrict__ e, double *__restrict__ tau, double *__restrict__ wbuf,
                                                    const double *__restrict__ ybuf) {
    __shared__ double red[HNW];
    __shared__ double wk_s;
    const int tid = threadIdx.x;
    double *rowk = W + (size_t)k * ld;
    const double *vp = k >= 1 ? W + (size_t)(k - 1) * ld : nullptr;      // v_{k-1}, entries at columns >= k
    if (k >= 1) {
        const double tp = tau[k - 1];
        double part = 0.0;
        for (int i = k + tid; i < n; i += HNT) part += tp * ybuf[i] * vp[i];
        const double alpha = -0.5 * tp * block_sum<HNW>(part, red);
        for (int i = k + tid; i < n; i += HNT) {
            const double wi = tp * ybuf[i] + alpha * vp[i];
            wbuf[i] = wi;
            if (i == k) wk_s = wi;
        }
        __syncthreads();
    }
    const double wk = k >= 1 ? wk_s : 0.0;
    // x[j] = W[k][j] - v[k] w[j] - w[k] v[j], v[k] = 1  (each thread keeps re-deriving its own entries: nothing is stored)
    auto xval = [&](int j) {
        double x = rowk[j];
        if (k >= 1) x -= wbuf[j] + wk * vp[j];
        return x;
    };
    if (k == n - 1) {
        if (tid == 0) { d[k] = xval(k); e[k] = 0.0; tau[k] = 0.0; }
        return;
    }
    double part = 0.0;
    for (int j = k + 2 + tid; j < n; j += HNT) { const double x = xval(j); part += x * x; }
    const double xnorm2 = block_sum<HNW>(part, red);
    const double alpha = xval(k + 1);
    double tk = 0.0, scale = 0.0, beta = alpha;
    if (xnorm2 != 0.0) {
        const double nrm = sqrt(alpha * alpha + xnorm2);
        beta = alpha >= 0.0 ? -nrm : nrm;
        tk = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    const double dk = xval(k);
    __syncthreads();                                   // every read of row k is done before it is overwritten
    for (int j = k + 1 + tid; j < n; j += HNT) {
        double x = rowk[j];
        if (k >= 1) x -= wbuf[j] + wk * vp[j];
        rowk[j] = (j == k + 1) ? 1.0 : x * scale;
    }
    if (tid == 0) { d[k] = dk; e[k] = beta; tau[k] = tk; }
}

// Rows i > k of the trailing block: A[i][j] -= vp[i] wp[j] + wp[i] vp[j] (the update of step k - 1; vp = wp = zeros at k = 0), then
// y[i] = sum_{j > k} A[i][j] v[j] with v = v_k (row k).  Columns are walked in aligned pairs; the column k of a pair that straddles
// the boundary is left alone.
__global__ __launch_bounds__(UNT) void update_matvec_kernel(int n, int k, double *__restrict__ W, int64_t ld, const double *__restrict__ vp,
                                                            const double *__restrict__ wp, double *__restrict__ ybuf) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * (UNT / 64) + (threadIdx.x >> 6), nwaves = gridDim.x * (UNT / 64);
    const double2 *v2 = reinterpret_cast<const double2 *>(W + (size_t)k * ld);
    const double2 *vp2 = reinterpret_cast<const double2 *>(vp);
    const double2 *wp2 = reinterpret_cast<const double2 *>(wp);
    const int c_lo = (k + 1) >> 1, c_hi = (int)(ld >> 1);
    const bool odd = ((k + 1) & 1) != 0;              // pair c_lo starts at column k
    for (int i0 = k + 1 + gw * ROWS; i0 < n; i0 += nwaves * ROWS) {
        double2 *row[ROWS];
        double vi[ROWS], wi[ROWS], acc[ROWS];
        bool live[ROWS];
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            live[u] = i0 + u < n;
            const int i = live[u] ? i0 + u : n - 1;
            row[u] = reinterpret_cast<double2 *>(W + (size_t)i * ld);
            vi[u] = vp[i];
            wi[u] = wp[i];
            acc[u] = 0.0;
        }
        for (int c = c_lo + lane; c < c_hi; c += 64) {
            double2 v = v2[c], pv = vp2[c], pw = wp2[c];
            const bool edge = odd && c == c_lo;
            if (edge) { v.x = 0.0; pv.x = 0.0; pw.x = 0.0; }
            double2 a[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) a[u] = row[u][c];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                a[u].x -= vi[u] * pw.x + wi[u] * pv.x;
                a[u].y -= vi[u] * pw.y + wi[u] * pv.y;
                acc[u] += a[u].x * v.x + a[u].y * v.y;
                if (live[u]) row[u][c] = a[u];
            }
        }
#pragma unroll
        for (int u = 0; u < ROWS; ++u) {
            const double s = dmk_wave_sum(acc[u]);
            if (lane == 0 && live[u]) ybuf[i0 + u] = s;
        }
    }
}

// status[0] |= 1 when d or e holds a non-finite value
__global__ void finite_kernel(int n, const double *__restrict__ d, const double *__restrict__ e, int *__restrict__ status) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!(fabs(d[i]) <= 1.7e308) || !(fabs(e[i]) <= 1.7e308)) status[0] = 1;
}

// lam[j] = eigenvalue number j - bs[j] of the block of position j
__global__ void bisect_kernel(int n, const double *__restrict__ d, const double *__restrict__ e, const double *__restrict__ e2,
                              const int *__restrict__ bs, const int *__restrict__ be, const double *__restrict__ bnorm,
                              double *__restrict__ lam) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int s0 = bs[j], t0 = be[j];
    lam[j] = t0 - s0 == 1 ? d[s0] : dmk_bisect_eigenvalue(d, e, e2, s0, t0, j - s0, bnorm[j]);
}

// first pass: one lane per selected vector (row r of Z, position pos[r] in T), three solves from the hashed start
__global__ void invit_kernel(int n, int m, const int *__restrict__ pos, const double *__restrict__ dl, const double *__restrict__ el,
                             const int *__restrict__ bs, const int *__restrict__ be, const double *__restrict__ bnorm,
                             const double *__restrict__ lam, double *__restrict__ ws, double *__restrict__ Z) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int j = pos[r];
    double *z = Z + (size_t)r * n;
    if (be[j] - bs[j] == 1) { z[bs[j]] = 1.0; return; }
    InvIt<true> it(n, m, r, j, dl, el, bs, be, bnorm, ws);
    it.factor(lam[j]);
    double xm = it.seed(0, j, 0ull);
    for (int iter = 0; iter < 3; ++iter) xm = it.solve(xm);
    it.store(xm, z);
}

// One workgroup per cluster (rows r0 .. r0 + cnt of Z, all of one block), the rows one after another as in LAPACK's dstein: classical
// Gram-Schmidt twice against the rows before, renormalise.  When the projection took away more than half of the vector -- a (nearly)
// degenerate cluster, where independently iterated vectors come out almost parallel and what is left is amplified rounding noise that
// every later row would inherit -- the projected vector goes through one more solve with its factorisation of T - lam I (still in
// the scratch of the first pass; thread 0) and is projected again, up to four times.  A third pass then MEASURES the overlaps.
// bad[row] = 1 when a vector vanishes, does not settle or keeps an overlap above otol: it goes to the repair pass.
__global__ __launch_bounds__(HNT) void cluster_kernel(int n, int m, const int *__restrict__ cl_r0, const int *__restrict__ cl_cnt,
                                                      const int *__restrict__ pos, const double *__restrict__ dl, const double *__restrict__ el,
                                                      const int *__restrict__ bs, const int *__restrict__ be, const double *__restrict__ bnorm,
                                                      double *__restrict__ ws, double *__restrict__ Z, double *__restrict__ dots, double otol,
                                                      int *__restrict__ bad) {
    __shared__ double red[HNW];
    const int r0 = cl_r0[blockIdx.x], cnt = cl_cnt[blockIdx.x];
    const int s0 = bs[pos[r0]], t0 = be[pos[r0]];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *dt = dots + r0;
    auto overlaps = [&](const double *zq, const int q) {            // dt[p] = z_p . z_q for the rows before q
        for (int p = wave; p < q; p += HNW) {
            const double *zp = Z + (size_t)(r0 + p) * n;
            double s = 0.0;
            for (int i = s0 + lane; i < t0; i += 64) s += zp[i] * zq[i];
            s = dmk_wave_sum(s);
            if (lane == 0) dt[p] = s;
        }
        __syncthreads();
    };
    for (int q = 1; q < cnt; ++q) {
        double *zq = Z + (size_t)(r0 + q) * n;
        double kept = 0.0;                                            // |z|^2 the two projections left of the unit vector
        for (int round = 0; round < 5; ++round) {
            for (int pass = 0; pass < 2; ++pass) {
                overlaps(zq, q);
                for (int i = s0 + tid; i < t0; i += HNT) {
                    double acc = 0.0;
#pragma unroll 8
                    for (int p = 0; p < q; ++p) acc += dt[p] * Z[(size_t)(r0 + p) * n + i];
                    zq[i] -= acc;
                }
                __syncthreads();
            }
            double s = 0.0;
            for (int i = s0 + tid; i < t0; i += HNT) s += zq[i] * zq[i];
            kept = block_sum<HNW>(s, red);
            const double inv = kept > 0.0 ? 1.0 / sqrt(kept) : 0.0;
            for (int i = s0 + tid; i < t0; i += HNT) zq[i] *= inv;
            __syncthreads();
            if (!(kept < 0.5) || round == 4) break;                   // uniform: every thread holds the same sum
            if (tid == 0) {
                const int r = r0 + q;
                InvIt<true> it(n, m, r, pos[r], dl, el, bs, be, bnorm, ws);
                double xm = 0.0;
                for (int i = s0; i < t0; ++i) { const double v = zq[i]; it.x[(size_t)i * it.sm] = v; xm = fmax(xm, fabs(v)); }
                xm = it.solve(xm);
                it.store(xm, zq);
            }
            __syncthreads();
        }
        if (!(kept >= 0.5) && tid == 0) bad[r0 + q] = 1;
        overlaps(zq, q);
        double mx = 0.0;
        for (int p = tid; p < q; p += HNT) mx = fmax(mx, fabs(dt[p]));
        if (!(mx <= otol)) bad[r0 + q] = 1;
        __syncthreads();
    }
}

// one wave per vector: bad[r] = 1 when the vector fails the acceptance test; status[1] counts the flagged rows
__global__ __launch_bounds__(256) void verify_kernel(int n, int m, const int *__restrict__ pos, const double *__restrict__ dl,
                                                     const double *__restrict__ el, const int *__restrict__ bs, const int *__restrict__ be,
                                                     const double *__restrict__ bnorm, const double *__restrict__ lam,
                                                     const double *__restrict__ Z, double rtol, int *__restrict__ bad,
                                                     double *__restrict__ ratio, int *__restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    const int j = pos[r], s0 = bs[j], t0 = be[j];
    const double tn = bnorm[j];
    double res = 0.0;
    const bool ok = t0 - s0 == 1 || dmk_tri_accept(lane, s0, t0, dl, el, tn, lam[j], Z + (size_t)r * n, rtol, &res);
    const double rt = res / fmax(tn, 1e-300);          // the residual in units of |T|
    if (lane == 0) {
        const int b = (ok && !bad[r]) ? 0 : 1;         // a row the cluster pass flagged stays flagged
        bad[r] = b;
        ratio[r] = rt;
        if (b) atomicAdd(status + 1, 1);
    }
}

// Repair of the vectors verify_kernel rejected, the way LAPACK's dstein builds a vector: perturbed shift, fresh start, and the
// re-orthogonalisation against the ACCEPTED members of its cluster (rows cl_lo[r] .. cl_hi[r]) inside the iteration; accepted as soon
// as it passes the acceptance test and its overlaps with those members are below otol.  One wave, the rejected rows one after
// another (they are rare); status[0] = 2 when a vector cannot be repaired.
__global__ __launch_bounds__(64) void repair_kernel(int n, int m, const int *__restrict__ pos, const int *__restrict__ cl_lo,
                                                    const int *__restrict__ cl_hi, const double *__restrict__ dl, const double *__restrict__ el,
                                                    const int *__restrict__ bs, const int *__restrict__ be, const double *__restrict__ bnorm,
                                                    const double *__restrict__ lam, double *__restrict__ ws, double *__restrict__ Z, double rtol,
                                                    double otol, int *__restrict__ bad, int *__restrict__ status) {
    const int lane = threadIdx.x;
    for (int r = 0; r < m; ++r) {
        if (!bad[r]) continue;
        const int j = pos[r], s0 = bs[j], t0 = be[j];
        const double tn = bnorm[j], lj = lam[j];
        double *zj = Z + (size_t)r * n;
        InvIt<true> it(n, m, r, j, dl, el, bs, be, bnorm, ws);
        bool fixed = false;
        for (int attempt = 1; attempt <= 3 && !fixed; ++attempt) {
            double xm = 0.0;
            if (lane == 0) {
                it.factor(lj + ((attempt & 1) ? 4.0 : -4.0) * attempt * DMK_EPS * tn);
                xm = it.seed(0, j, (unsigned long long)attempt);
            }
            for (int iter = 0; iter < 5 && !fixed; ++iter) {
                if (lane == 0) {
                    xm = it.solve(xm);
                    it.store(xm, zj);
                }
                __threadfence_block();
                double worst = 0.0;
                for (int pass = 0; pass < 3; ++pass) {            // two projections, then the overlaps that remain
                    worst = 0.0;
                    for (int p = cl_lo[r]; p < cl_hi[r]; ++p) {
                        if (p == r || bad[p]) continue;
                        const double *zp = Z + (size_t)p * n;
                        double dot = 0.0;
                        for (int i = s0 + lane; i < t0; i += 64) dot += zp[i] * zj[i];
                        dot = dmk_wave_sum(dot);
                        worst = fmax(worst, fabs(dot));
                        if (pass < 2) for (int i = s0 + lane; i < t0; i += 64) zj[i] -= dot * zp[i];
                    }
                    if (pass == 1) {
                        double nr = 0.0;
                        for (int i = s0 + lane; i < t0; i += 64) nr += zj[i] * zj[i];
                        nr = dmk_wave_sum(nr);
                        const double inv = nr > 0.0 ? 1.0 / sqrt(nr) : 0.0;
                        for (int i = s0 + lane; i < t0; i += 64) {
                            const double v = zj[i] * inv;
                            zj[i] = v;
                            it.x[(size_t)i * it.sm] = v;              // fed back: the next solve starts from the projected vector
                        }
                    }
                    __threadfence_block();
                }
                xm = 1.0;
                fixed = iter >= 1 && worst <= otol && dmk_tri_accept(lane, s0, t0, dl, el, tn, lj, zj, rtol);
            }
        }
        if (lane == 0) {
            if (fixed) bad[r] = 0;
            else status[0] = 2;
        }
        __threadfence_block();
    }
}

// out[c][dst ? dst[r] : r] = in[r][c]  (in: rows x cols, ld_in; out: cols x ld_out)
__global__ void transpose_kernel(int rows, int cols, const double *__restrict__ in, int64_t ld_in, double *__restrict__ out,
                                 int64_t ld_out, const int *__restrict__ dst) {
    __shared__ double tile[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int rr = threadIdx.y; rr < 32; rr += blockDim.y) {
        const int r = r0 + rr, c = c0 + threadIdx.x;
        tile[rr][threadIdx.x] = (r < rows && c < cols) ? in[(size_t)r * ld_in + c] : 0.0;
    }
    __syncthreads();
    for (int cc = threadIdx.y; cc < 32; cc += blockDim.y) {
        const int c = c0 + cc, r = r0 + threadIdx.x;
        if (r < rows && c < cols) out[(size_t)c * ld_out + (dst ? dst[r] : r)] = tile[threadIdx.x][cc];
    }
}

// panel of nbp reflectors k0 .. k0 + nbp: V (nbp x n, rows = reflectors, zero up to the diagonal) and its transpose Vt (n x NB)
__global__ void panel_kernel(int n, int k0, int nbp, const double *__restrict__ W, int64_t ld, double *__restrict__ V,
                             double *__restrict__ Vt) {
    const size_t total = (size_t)nbp * n;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(t / n), c = (int)(t % n);
        const double v = c > k0 + j ? W[(size_t)(k0 + j) * ld + c] : 0.0;
        V[t] = v;
        Vt[(size_t)c * NB + j] = v;
    }
}

// T of the compact WY form Q = I - V T V^T (forward, columnwise; dlarft): thread j owns row j of the upper triangle,
// T[j][i] = -tau_i sum_{j <= l < i} T[j][l] G[l][i], T[i][i] = tau_i, G = V V^T.  Then U = T S (nbp x m).
__global__ __launch_bounds__(256) void wy_apply_t_kernel(int nbp, int m, const double *__restrict__ tau, const double *__restrict__ G,
                                                         const double *__restrict__ S, double *__restrict__ U) {
    __shared__ double T[NB][NB + 1];
    const int tid = threadIdx.x;
    if (tid < nbp) {
        const int j = tid;
        for (int i = 0; i < j; ++i) T[j][i] = 0.0;
        T[j][j] = tau[j];
        for (int i = j + 1; i < nbp; ++i) {
            double s = 0.0;
            for (int l = j; l < i; ++l) s += T[j][l] * G[(size_t)l * NB + i];
            T[j][i] = -tau[i] * s;
        }
    }
    __syncthreads();
    for (int c = blockIdx.x * blockDim.x + tid; c < m; c += gridDim.x * blockDim.x)
        for (int j = 0; j < nbp; ++j) {
            double s = 0.0;
            for (int l = j; l < nbp; ++l) s += T[j][l] * S[(size_t)l * m + c];
            U[(size_t)j * m + c] = s;
        }
}


int alloc_or_refuse(dmk_ctx *ctx, void **out, size_t bytes, const char *what, int n) {
    if (dmk_dev_alloc(ctx, out, bytes) != hipSuccess) {
        *out = nullptr;
        return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_large: n = %d needs %zu bytes of device memory for %s, which the device cannot provide",
                        n, bytes, what);
    }
    return DMK_OK;
}

void release(dmk_eighl *h) {
    if (!h) return;
    if (h->W) (void)hipFree(h->W);
    if (h->vec) (void)hipFree(h->vec);
    if (h->ivec) (void)hipFree(h->ivec);
    delete h;
}

int factor(dmk_ctx *ctx, int n, const double *A, int64_t lda, double *w, dmk_eighl *h) {
    hipStream_t st = ctx->stream;
    h->ctx = ctx;
    h->n = n;
    const int64_t ld = h->ld = ((int64_t)n + 1) & ~(int64_t)1;
    int rc;
    if ((rc = alloc_or_refuse(ctx, reinterpret_cast<void **>(&h->W), (size_t)n * ld * 8, "the working copy of the matrix", n))) return rc;
    if ((rc = alloc_or_refuse(ctx, reinterpret_cast<void **>(&h->vec), (size_t)8 * ld * 8, "its vectors", n))) return rc;
    if ((rc = alloc_or_refuse(ctx, reinterpret_cast<void **>(&h->ivec), ((size_t)2 * n + 4) * 4, "its index tables", n))) return rc;
    double *d = h->vec, *e = d + ld, *e2 = e + ld, *tau = e2 + ld, *lam = tau + ld, *bnorm = lam + ld, *wbuf = bnorm + ld, *ybuf = wbuf + ld;
    int *bs = h->ivec, *be = bs + n, *status = be + n;
    DMK_HIP(ctx, hipMemsetAsync(h->vec, 0, (size_t)8 * ld * 8, st));
    DMK_HIP(ctx, hipMemsetAsync(status, 0, 16, st));
    {
        const size_t total = (size_t)n * ld;
        const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(init_kernel, dim3(grid), dim3(256), 0, st, n, A, lda, h->W, ld);
        DMK_CHECK_LAUNCH(ctx);
    }
    // ---- phase 1: two launches per column, ordered by the stream
    for (int k = 0; k < n; ++k) {
        hipLaunchKernelGGL(house_kernel, dim3(1), dim3(HNT), 0, st, n, k, h->W, ld, d, e, tau, wbuf, ybuf);
        if (k == n - 1) break;
        const int rows = n - k - 1, per_wg = ROWS * (UNT / 64);
        const int grid = std::min(MAXGRID, (rows + per_wg - 1) / per_wg);
        const double *vp = k >= 1 ? h->W + (size_t)(k - 1) * ld : wbuf;        // k = 0: wbuf is still all zeros
        hipLaunchKernelGGL(update_matvec_kernel, dim3(grid), dim3(UNT), 0, st, n, k, h->W, ld, vp, wbuf, ybuf);
    }
    DMK_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(finite_kernel, dim3(std::min(1024, (n + 255) / 256)), dim3(256), 0, st, n, d, e, status);
    DMK_CHECK_LAUNCH(ctx);
    std::vector<double> hd(n), he(n), he2(n);
    int hstatus = 0;
    DMK_HIP(ctx, hipMemcpyAsync(hd.data(), d, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    DMK_HIP(ctx, hipMemcpyAsync(he.data(), e, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    DMK_HIP(ctx, hipMemcpyAsync(&hstatus, status, 4, hipMemcpyDeviceToHost, st));
    DMK_HIP(ctx, hipStreamSynchronize(st));
    if (hstatus != 0)
        return dmk_fail(ctx, DMK_ERR_NOCONV, "eigh_large: the tridiagonal form of the %d x %d matrix is not finite (NaN / Inf in the input?)", n, n);
    // ---- phase 2: unreduced blocks (negligible couplings are set to zero), bisection, sort
    h->bs.assign(n, 0); h->be.assign(n, 0); h->bnorm.assign(n, 0.0);
    dmk_tri_split(n, hd.data(), he.data(), h->bs.data(), h->be.data(), h->bnorm.data());
    for (int i = 0; i < n; ++i) he2[i] = he[i] * he[i];
    DMK_HIP(ctx, hipMemcpyAsync(e, he.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(e2, he2.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(bnorm, h->bnorm.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(bs, h->bs.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(be, h->be.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(bisect_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, d, e, e2, bs, be, bnorm, lam);
    DMK_CHECK_LAUNCH(ctx);
    h->lam.resize(n);
    DMK_HIP(ctx, hipMemcpyAsync(h->lam.data(), lam, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    DMK_HIP(ctx, hipStreamSynchronize(st));
    h->perm.resize(n);
    std::iota(h->perm.begin(), h->perm.end(), 0);
    const std::vector<double> &L = h->lam;
    std::stable_sort(h->perm.begin(), h->perm.end(), [&L](int a, int b) { return L[a] < L[b]; });
    std::vector<double> hw(n);
    for (int r = 0; r < n; ++r) hw[r] = L[h->perm[r]];
    DMK_HIP(ctx, hipMemcpyAsync(w, hw.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipStreamSynchronize(st));             // hw goes out of scope
    // clusters: eigenvalues of one block (ascending by position) chained by gaps <= 1e-3 |T_block|
    h->clus.assign(n, 0);
    for (int j = 0, c = -1; j < n; ++j) {
        if (j == h->bs[j] || L[j] - L[j - 1] > 1e-3 * h->bnorm[j]) ++c;
        h->clus[j] = c;
    }
    return DMK_OK;
}

int vectors(dmk_eighl *h, int m, const int32_t *idx, double *Vt) {
    dmk_ctx *ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int n = h->n;
    const int64_t ld = h->ld;
    // rows of Z in the order of the positions in T: the members of a cluster are then consecutive
    std::vector<int> order(m), pos(m), rowq(m), cl_lo(m), cl_hi(m), cl_r0, cl_cnt;
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return h->perm[idx[a]] < h->perm[idx[b]]; });
    for (int r = 0; r < m; ++r) { rowq[r] = order[r]; pos[r] = h->perm[idx[order[r]]]; }
    for (int r = 0; r < m;) {
        int r1 = r + 1;
        while (r1 < m && h->clus[pos[r1]] == h->clus[pos[r]]) ++r1;
        if (r1 - r >= 2) { cl_r0.push_back(r); cl_cnt.push_back(r1 - r); }
        for (int q = r; q < r1; ++q) { cl_lo[q] = r; cl_hi[q] = r1; }
        r = r1;
    }
    const int ncl = (int)cl_r0.size();
    // workspace: Z (m n) | Y (n m) | scratch of the inverse iteration (7 n m) | V, Vt panels | G, S, U | tables
    const size_t mn = (size_t)m * n;
    const size_t b_Z = dmk_align256(mn * 8), b_Y = b_Z, b_ws = dmk_align256(7 * mn * 8), b_V = dmk_align256((size_t)NB * n * 8),
                 b_G = dmk_align256((size_t)NB * NB * 8), b_S = dmk_align256((size_t)NB * m * 8), b_dots = dmk_align256((size_t)m * 8),
                 b_int = dmk_align256((size_t)m * 4);
    const size_t total = b_Z + b_Y + b_ws + 2 * b_V + b_G + 2 * b_S + b_dots + 7 * b_int;
    if (total > ctx->scratch_bytes) {
        size_t fr = 0, tot = 0;
        DMK_HIP(ctx, hipMemGetInfo(&fr, &tot));
        if (total > tot)
            return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_large: %d vectors of dimension %d need %zu bytes of workspace, the device has %zu", m, n,
                            total, tot);
    }
    void *base = nullptr;
    if (dmk_scratch(ctx, total, &base))
        return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_large: %d vectors of dimension %d need %zu bytes of workspace, which the device cannot provide",
                        m, n, total);
    char *p = reinterpret_cast<char *>(base);
    double *Z = reinterpret_cast<double *>(p); p += b_Z;
    double *Y = reinterpret_cast<double *>(p); p += b_Y;
    double *ws = reinterpret_cast<double *>(p); p += b_ws;
    double *V = reinterpret_cast<double *>(p); p += b_V;
    double *VT = reinterpret_cast<double *>(p); p += b_V;
    double *G = reinterpret_cast<double *>(p); p += b_G;
    double *S = reinterpret_cast<double *>(p); p += b_S;
    double *U = reinterpret_cast<double *>(p); p += b_S;
    double *dots = reinterpret_cast<double *>(p); p += b_dots;
    int *d_pos = reinterpret_cast<int *>(p); p += b_int;
    int *d_rowq = reinterpret_cast<int *>(p); p += b_int;
    int *d_r0 = reinterpret_cast<int *>(p); p += b_int;
    int *d_cnt = reinterpret_cast<int *>(p); p += b_int;
    int *d_lo = reinterpret_cast<int *>(p); p += b_int;
    int *d_hi = reinterpret_cast<int *>(p); p += b_int;
    int *d_bad = reinterpret_cast<int *>(p); p += b_int;
    double *d = h->vec, *e = d + ld, *tau = d + 3 * ld, *lam = d + 4 * ld, *bnorm = d + 5 * ld;
    int *bs = h->ivec, *be = bs + n, *status = be + n;

    DMK_HIP(ctx, hipMemcpyAsync(d_pos, pos.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(d_rowq, rowq.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(d_lo, cl_lo.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemcpyAsync(d_hi, cl_hi.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
    DMK_HIP(ctx, hipMemsetAsync(d_bad, 0, (size_t)m * 4, st));
    if (ncl) {
        DMK_HIP(ctx, hipMemcpyAsync(d_r0, cl_r0.data(), (size_t)ncl * 4, hipMemcpyHostToDevice, st));
        DMK_HIP(ctx, hipMemcpyAsync(d_cnt, cl_cnt.data(), (size_t)ncl * 4, hipMemcpyHostToDevice, st));
    }
    DMK_HIP(ctx, hipMemsetAsync(status, 0, 16, st));
    DMK_HIP(ctx, hipMemsetAsync(Z, 0, mn * 8, st));
    // ---- phase 3
    hipLaunchKernelGGL(invit_kernel, dim3((m + 63) / 64), dim3(64), 0, st, n, m, d_pos, d, e, bs, be, bnorm, lam, ws, Z);
    DMK_CHECK_LAUNCH(ctx);
    const double otol = 64.0 * DMK_EPS * std::sqrt((double)n), rtol = 64.0 * n * DMK_EPS;
    if (ncl) {
        hipLaunchKernelGGL(cluster_kernel, dim3(ncl), dim3(HNT), 0, st, n, m, d_r0, d_cnt, d_pos, d, e, bs, be, bnorm, ws, Z, dots, otol, d_bad);
        DMK_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL(verify_kernel, dim3((m + 3) / 4), dim3(256), 0, st, n, m, d_pos, d, e, bs, be, bnorm, lam, Z, rtol, d_bad, dots, status);
    DMK_CHECK_LAUNCH(ctx);
    if (getenv("DMK_EIGHL_DEBUG")) {            // which vectors the first pass did not deliver (diagnostics; synchronises)
        std::vector<int> hb(m);
        std::vector<double> hr(m);
        DMK_HIP(ctx, hipMemcpyAsync(hb.data(), d_bad, (size_t)m * 4, hipMemcpyDeviceToHost, st));
        DMK_HIP(ctx, hipMemcpyAsync(hr.data(), dots, (size_t)m * 8, hipMemcpyDeviceToHost, st));
        DMK_HIP(ctx, hipStreamSynchronize(st));
        for (int r = 0; r < m; ++r)
            if (hb[r]) {
                const int j = pos[r];
                fprintf(stderr, "[eigh_large n=%d m=%d] row %d (position %d, block [%d, %d), cluster rows [%d, %d)) rejected: lam %.17g, "
                                "|T z - lam z| / |T| = %.3e (limit %.3e), |T_block| %.3e\n", n, m, r, j, h->bs[j], h->be[j], cl_lo[r], cl_hi[r],
                        h->lam[j], hr[r], rtol, h->bnorm[j]);
            }
    }
    hipLaunchKernelGGL(repair_kernel, dim3(1), dim3(64), 0, st, n, m, d_pos, d_lo, d_hi, d, e, bs, be, bnorm, lam, ws, Z, rtol, otol, d_bad, status);
    DMK_CHECK_LAUNCH(ctx);
    // ---- phase 4: Y (n x m, column q = vector of idx[q]) <- H_0 ... H_{n-2} Z^T, panel by panel from the last
    {
        const dim3 tg((n + 31) / 32, (m + 31) / 32), tb(32, 8);
        hipLaunchKernelGGL(transpose_kernel, tg, tb, 0, st, m, n, Z, (int64_t)n, Y, (int64_t)m, d_rowq);
        DMK_CHECK_LAUNCH(ctx);
    }
    const int nref = n - 1;
    for (int pnl = (nref + NB - 1) / NB - 1; pnl >= 0; --pnl) {
        const int k0 = pnl * NB, nbp = std::min(NB, nref - k0), lo = k0 + 1, K = n - lo;
        const size_t tot = (size_t)nbp * n;
        hipLaunchKernelGGL(panel_kernel, dim3((unsigned)std::min<size_t>((tot + 255) / 256, 4096)), dim3(256), 0, st, n, k0, nbp, h->W, ld, V, VT);
        DMK_CHECK_LAUNCH(ctx);
        DMK_HIP(ctx, hipMemsetAsync(G, 0, (size_t)NB * NB * 8, st));
        DMK_HIP(ctx, hipMemsetAsync(S, 0, (size_t)NB * m * 8, st));
        int rc;
        // G = V V^T and S = V Y over the rows below the panel's first diagonal (the reflectors vanish above)
        DgemmTn vv, vy;
        vv.M = vv.N = nbp; vv.K = K; vv.X = vv.Y = VT + (size_t)lo * NB; vv.ldx = vv.ldy = NB; vv.C = G; vv.ldc = NB;
        vy.M = nbp; vy.N = m; vy.K = K; vy.X = vv.X; vy.ldx = NB; vy.Y = Y + (size_t)lo * m; vy.ldy = m; vy.C = S; vy.ldc = m;
        if ((rc = launch_dgemm_tn_acc(ctx, vv))) return rc;
        if ((rc = launch_dgemm_tn_acc(ctx, vy))) return rc;
        hipLaunchKernelGGL(wy_apply_t_kernel, dim3(std::min(256, (m + 255) / 256)), dim3(256), 0, st, nbp, m, tau + k0, G, S, U);
        DMK_CHECK_LAUNCH(ctx);
        // Y[lo:, :] -= V[:, lo:]^T U
        DgemmTn vu;
        vu.M = K; vu.N = m; vu.K = nbp; vu.alpha = -1.0; vu.X = V + lo; vu.ldx = n; vu.Y = U; vu.ldy = m; vu.C = Y + (size_t)lo * m; vu.ldc = m;
        if ((rc = launch_dgemm_tn_acc(ctx, vu))) return rc;
    }
    {
        const dim3 tg((m + 31) / 32, (n + 31) / 32), tb(32, 8);
        hipLaunchKernelGGL(transpose_kernel, tg, tb, 0, st, n, m, Y, (int64_t)m, Vt, (int64_t)n, (const int *)nullptr);
        DMK_CHECK_LAUNCH(ctx);
    }
    int hstatus = 0;
    DMK_HIP(ctx, hipMemcpyAsync(&hstatus, status, 4, hipMemcpyDeviceToHost, st));
    DMK_HIP(ctx, hipStreamSynchronize(st));
    if (hstatus != 0)
        return dmk_fail(ctx, DMK_ERR_NOCONV, "eigh_large: an eigenvector of the tridiagonal form failed the residual test |T z - lam z| <= 64 n eps |T| "
                                            "or the orthogonality test inside its cluster after three repair attempts (n = %d, %d vectors)", n, m);
    return DMK_OK;
}

}  // namespace

// all eigenpairs of one matrix: the n > 2000 route of dmk_eigh_batched_real (eigh.hip)
int launch_eigh_large_all(dmk_ctx *ctx, int n, const double *A, double *w, double *Vt) {
    dmk_eighl *h = nullptr;
    int rc = dmk_eighl_factor(ctx, n, A, n, w, &h);
    if (rc) return rc;
    std::vector<int32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    rc = dmk_eighl_vectors(h, n, idx.data(), Vt);
    dmk_eighl_free(h);
    return rc;
}

extern "C" {

int dmk_eighl_factor(dmk_ctx *ctx, int n, const double *A, int64_t lda, double *w, dmk_eighl **out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (out) *out = nullptr;
    if (n < 2 || !A || !w || !out || lda < n) return dmk_fail(ctx, DMK_ERR_INVALID, "eighl_factor: bad arguments (n >= 2, lda >= n)");
    dmk_eighl *h = new dmk_eighl;
    const int rc = factor(ctx, n, A, lda, w, h);
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        release(h);
        return rc;
    }
    *out = h;
    return DMK_OK;
}

int dmk_eighl_vectors(dmk_eighl *h, int m, const int32_t *idx_host, double *Vt) {
    if (!h || !h->ctx) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (m < 0 || m > h->n || (m > 0 && (!idx_host || !Vt))) return dmk_fail(ctx, DMK_ERR_INVALID, "eighl_vectors: bad arguments");
    for (int q = 0; q < m; ++q)
        if (idx_host[q] < 0 || idx_host[q] >= h->n || (q > 0 && idx_host[q] <= idx_host[q - 1]))
            return dmk_fail(ctx, DMK_ERR_INVALID, "eighl_vectors: idx must be strictly ascending in [0, %d) (entry %d is %d)", h->n, q,
                            (int)idx_host[q]);
    if (m == 0) return DMK_OK;
    return vectors(h, m, idx_host, Vt);
}

int dmk_eighl_free(dmk_eighl *h) {
    if (!h) return DMK_OK;
    if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
    release(h);
    return DMK_OK;
}

}  // extern "C"
