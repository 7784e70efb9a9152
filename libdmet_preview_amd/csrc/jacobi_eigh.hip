// K13 -- low-latency symmetric eigensolver for a FEW small real matrices: parallel block Jacobi over several CUs.
//
// routine/slater.py:1075, 1098 call la.eigh(embHeff[s], ovlp_emb[s]) once per objective / gradient evaluation of the
// vcor fit, hundreds to thousands of times in sequence on a (spin, nemb, nemb) stack (2 x 256 x 256 at C5).  The
// batched Householder + QL kernel (eigh.hip) is built for throughput -- one workgroup per matrix, 27 ms of latency
// at n = 256 -- and its QL phase is a sequential recurrence.  Here latency is what counts:
//
//   * one-sided (Hestenes) Jacobi on M = A + c I (c >= |A|_F makes M positive definite, so the singular vectors of M
//     ARE the eigenvectors and nothing mixes +l with -l): rows g_j of G = V M are rotated in pairs until they are
//     mutually orthogonal; then g_j = (l_j + c) v_j, l_j = g_j . v_j - c.
//   * the n vectors are cut into blocks of 16; a workgroup owns a PAIR of blocks for one step (both blocks of G and V
//     in LDS, 128 KB at n = 256), rotates all cross pairs (16 inner steps of 16 disjoint pairs, one pair per wave at a
//     time, lanes along the vector, DPP reductions), and the block pairs follow a round-robin tournament: n/32
//     workgroups per matrix, n/16 - 1 device-wide hand-overs per sweep instead of n - 1.
//   * WARM START: successive fit matrices differ by a line-search step, so the previous eigenvectors V0 make
//     G = V0 M almost orthogonal already and 2-3 sweeps (instead of 8-10) reach the same tolerance.
//
// Hand-over between workgroups of one matrix is an agent-scope release / acquire on a monotonic counter
// (__threadfence: L2 write-back + invalidate, the XCDs do not share an L2).  All workgroups of the launch are
// co-resident (batch * n/32 <= 256 CUs is checked).  Bit-reproducible: fixed pair order, no atomics on data.
#include "common.h"

namespace {

constexpr int JT = 256;
constexpr int JWV = JT / 64;

struct JacArgs {
    int n;            // padded dimension (multiple of 2 b)
    int batch, b, nb, max_sweeps;
    double *G, *V;    // batch x n x n, row j = vector j
    unsigned *bar;    // one monotonic counter per matrix
    int *abort_flag;  // set when a hand-over timed out
    int *flags;       // batch x max_sweeps: "a rotation happened in this sweep"
    int *sweeps_done; // batch
    double tol;
};

// Returns false when the hand-over timed out (a workgroup of the matrix is not running: the launch was not co-resident).
__device__ __forceinline__ bool matrix_barrier(unsigned *bar, unsigned target, int *abort_flag) {
    __shared__ int ok;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();                                   // release: this workgroup's rows are visible device-wide
        atomicAdd(bar, 1u);
        long long spins = 0;
        int good = 1;
        while (atomicAdd(bar, 0u) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1LL << 26) || atomicOr(abort_flag, 0)) {
                atomicOr(abort_flag, 1);
                good = 0;
                break;
            }
        }
        __threadfence();                                   // acquire
        ok = good;
    }
    __syncthreads();
    return ok != 0;
}

__device__ __forceinline__ double fast_rsqrt(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    return y;
}

// NP Hestenes rotations of disjoint row pairs (rp[k], rq[k]) by one wave, lanes along the vectors (LDS images Gs / Vs,
// leading dimension n).  The 3 NP dot products and their DPP reductions are issued together so that the reductions and
// the sqrt / div chains of the NP pairs overlap.  Returns true if any pair was rotated.
template <int NP>
__device__ __forceinline__ bool rotate_pairs(double *Gs, double *Vs, int n, const int (&rp)[NP], const int (&rq)[NP], double tol,
                                             int lane) {
    double a[NP], b[NP], c[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) a[k] = b[k] = c[k] = 0.0;
    for (int i = lane; i < n; i += 64) {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const double x = Gs[(size_t)rp[k] * n + i], y = Gs[(size_t)rq[k] * n + i];
            a[k] = fma(x, x, a[k]);
            b[k] = fma(y, y, b[k]);
            c[k] = fma(x, y, c[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        a[k] = dmk_wave_sum(a[k]);
        b[k] = dmk_wave_sum(b[k]);
        c[k] = dmk_wave_sum(c[k]);
    }
    double cs[NP], sn[NP];
    bool rot[NP], any = false;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        // |c| > tol sqrt(a b)  <=>  c^2 > tol^2 a b ; reciprocals and reciprocal square roots from the hardware
        // approximations + two Newton steps (full double precision, a fraction of the IEEE division / sqrt sequences)
        rot[k] = (c[k] * c[k] > tol * tol * (a[k] * b[k])) && c[k] != 0.0;
        const double cc = rot[k] ? c[k] : 1.0;
        const double zeta = 0.5 * (b[k] - a[k]) * dmk_rcp_nr2(cc);
        const double h2 = fma(zeta, zeta, 1.0);
        const double hyp = h2 * fast_rsqrt(h2);                 // sqrt(1 + zeta^2)
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) * dmk_rcp_nr2(fabs(zeta) + hyp);
        cs[k] = fast_rsqrt(fma(t, t, 1.0));
        sn[k] = cs[k] * t;
        any |= rot[k];
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        if (!rot[k]) continue;                               // wave-uniform
        double *gp = Gs + (size_t)rp[k] * n, *gq = Gs + (size_t)rq[k] * n;
        double *vp = Vs + (size_t)rp[k] * n, *vq = Vs + (size_t)rq[k] * n;
        for (int i = lane; i < n; i += 64) {
            const double x = gp[i], y = gq[i];
            gp[i] = cs[k] * x - sn[k] * y;
            gq[i] = sn[k] * x + cs[k] * y;
            const double u = vp[i], w = vq[i];
            vp[i] = cs[k] * u - sn[k] * w;
            vq[i] = sn[k] * u + cs[k] * w;
        }
    }
    return any;
}

template <int B>
__global__ __launch_bounds__(JT) void jacobi_eigh_kernel(JacArgs g) {
    extern __shared__ double sh[];
    constexpr int b = B, NP = B / JWV;
    const int n = g.n, nb = g.nb, nwg = nb / 2;
    double *Gs = sh;                       // [2b][n]
    double *Vs = sh + (size_t)2 * b * n;   // [2b][n]
    const int mat = blockIdx.x / nwg, w = blockIdx.x % nwg;
    double *G = g.G + (size_t)mat * n * n, *V = g.V + (size_t)mat * n * n;
    unsigned *bar = g.bar + mat;
    int *flags = g.flags + (size_t)mat * g.max_sweeps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned epoch = 0;

    auto load_blocks = [&](int P, int Q) {
        const size_t rows = (size_t)b * n;
        for (size_t t = tid; t < rows; t += JT) {
            Gs[t] = G[(size_t)P * rows + t];
            Gs[rows + t] = G[(size_t)Q * rows + t];
            Vs[t] = V[(size_t)P * rows + t];
            Vs[rows + t] = V[(size_t)Q * rows + t];
        }
        __syncthreads();
    };
    auto store_blocks = [&](int P, int Q) {
        __syncthreads();
        const size_t rows = (size_t)b * n;
        for (size_t t = tid; t < rows; t += JT) {
            G[(size_t)P * rows + t] = Gs[t];
            G[(size_t)Q * rows + t] = Gs[rows + t];
            V[(size_t)P * rows + t] = Vs[t];
            V[(size_t)Q * rows + t] = Vs[rows + t];
        }
    };

    int sweep = 0;
    for (; sweep < g.max_sweeps; ++sweep) {
        bool rotated = false;
        // ---- pairs inside the two blocks this workgroup starts with (round robin inside each block) ----
        load_blocks(2 * w, 2 * w + 1);
        for (int r = 0; r < b - 1; ++r) {
            int rp[NP], rq[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) {                 // b/2 pairs per block, two blocks: b pairs, NP per wave
                const int pi = wave + JWV * k;
                const int blk = pi / (b / 2), q0 = pi % (b / 2);
                int p, q;
                if (q0 == 0) { p = b - 1; q = r; }
                else { p = (r + q0) % (b - 1); q = (r - q0 + (b - 1)) % (b - 1); }
                rp[k] = blk * b + p;
                rq[k] = blk * b + q;
            }
            rotated |= rotate_pairs<NP>(Gs, Vs, n, rp, rq, g.tol, lane);
            __syncthreads();
        }
        store_blocks(2 * w, 2 * w + 1);
        ++epoch;
        if (!matrix_barrier(bar, epoch * nwg, g.abort_flag)) return;
        // ---- cross pairs: round-robin tournament over the blocks ----
        for (int t = 0; t < nb - 1; ++t) {
            int P, Q;
            if (w == 0) { P = nb - 1; Q = t; }
            else { P = (t + w) % (nb - 1); Q = (t - w + (nb - 1)) % (nb - 1); }
            load_blocks(P, Q);
            for (int s = 0; s < b; ++s) {
                int rp[NP], rq[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int i = wave + JWV * k;
                    rp[k] = i;
                    rq[k] = b + (i + s) % b;
                }
                rotated |= rotate_pairs<NP>(Gs, Vs, n, rp, rq, g.tol, lane);
                __syncthreads();
            }
            store_blocks(P, Q);
            if (t == nb - 2 && __syncthreads_or(rotated ? 1 : 0) && tid == 0) atomicOr(&flags[sweep], 1);
            ++epoch;
            if (!matrix_barrier(bar, epoch * nwg, g.abort_flag)) return;
        }
        int any = 0;
        if (tid == 0) any = atomicOr(&flags[sweep], 0);
        any = __syncthreads_or(any);
        if (!any) { ++sweep; break; }
    }
    if (w == 0 && tid == 0) g.sweeps_done[mat] = sweep;
}

// Shift c >= spectral radius of the symmetric matrix Bm (n0 x n0): min(Gershgorin row sum, Frobenius norm), rigorous.
// from_lower: only the lower triangle of Bm is valid (cold start on A); otherwise Bm = V0 A V0^T is stored in full and is
// nearly diagonal, which makes the bound tight (a tight shift keeps the eigenvector error at eps |A| instead of eps |A|_F).
__global__ __launch_bounds__(JT) void jacobi_shift_kernel(int n0, int from_lower, const double *__restrict__ Bm,
                                                          double *__restrict__ cshift) {
    __shared__ double red[2 * JWV];
    const int mat = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *a = Bm + (size_t)mat * n0 * n0;
    double fro = 0.0, gmax = 0.0;
    for (int r = wave; r < n0; r += JWV) {
        double rs = 0.0;
        for (int c = lane; c < n0; c += 64) {
            const double v = from_lower ? a[(size_t)(r >= c ? r : c) * n0 + (r >= c ? c : r)] : a[(size_t)r * n0 + c];
            rs += fabs(v);
            fro = fma(v, v, fro);
        }
        rs = dmk_wave_sum(rs);
        gmax = fmax(gmax, rs);
    }
    fro = dmk_wave_sum(fro);
    if (lane == 0) { red[wave] = fro; red[JWV + wave] = gmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double f = sqrt((red[0] + red[1]) + (red[2] + red[3]));
        const double gsh = fmax(fmax(red[JWV], red[JWV + 1]), fmax(red[JWV + 2], red[JWV + 3]));
        const double bound = fmin(f, gsh);
        cshift[mat] = bound > 0.0 ? 1.015625 * bound : 1.0;
    }
}

__global__ void jacobi_init_kernel(int n0, int n, int batch, const double *__restrict__ A, const double *__restrict__ V0A,
                                   const double *__restrict__ V0, const double *__restrict__ cshift, double *__restrict__ G,
                                   double *__restrict__ V) {
    const long long total = (long long)batch * n * n;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int mat = (int)(t / ((long long)n * n));
        const int r = (int)((t / n) % n), col = (int)(t % n);
        const double c = cshift[mat];
        double gv, vv;
        if (r < n0 && col < n0) {
            const size_t o = (size_t)mat * n0 * n0 + (size_t)r * n0 + col;
            if (V0) {
                vv = V0[o];
                gv = V0A[o] + c * vv;                      // row r of V0 (A + c I)
            } else {
                vv = (r == col) ? 1.0 : 0.0;
                gv = A[(size_t)mat * n0 * n0 + (size_t)(r >= col ? r : col) * n0 + (r >= col ? col : r)] + (r == col ? c : 0.0);
            }
        } else {
            vv = (r == col) ? 1.0 : 0.0;
            gv = (r == col) ? c : 0.0;
        }
        G[t] = gv;
        V[t] = vv;
    }
}

// Vu (n0 x n0, contiguous) = the converged vectors without the padding
__global__ void jacobi_gather_kernel(int n0, int n, int batch, const double *__restrict__ V, double *__restrict__ Vu) {
    const long long total = (long long)batch * n0 * n0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int mat = (int)(t / ((long long)n0 * n0));
        const int r = (int)((t / n0) % n0), c = (int)(t % n0);
        Vu[t] = V[(size_t)mat * n * n + (size_t)r * n + c];
    }
}

// eigenvalues as Rayleigh quotients l_j = (v_j A) . v_j (error eps |A|, second order in the vector error), ascending
// stable rank, sorted output (rows of Vt = eigenvectors)
__global__ __launch_bounds__(JT) void jacobi_finish_kernel(int n0, const double *__restrict__ Vu, const double *__restrict__ VA,
                                                           double *__restrict__ w, double *__restrict__ Vt, int *__restrict__ bad) {
    extern __shared__ double ev[];           // [n0] + ranks
    const int mat = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *Vm = Vu + (size_t)mat * n0 * n0, *Tm = VA + (size_t)mat * n0 * n0;
    double *inrm = ev + n0;                  // 1 / |v_j|: thousands of rotations leave |v_j| = 1 + O(1e-13)
    for (int j = wave; j < n0; j += JWV) {
        double s = 0.0, q = 0.0;
        for (int i = lane; i < n0; i += 64) {
            const double v = Vm[(size_t)j * n0 + i];
            s = fma(Tm[(size_t)j * n0 + i], v, s);
            q = fma(v, v, q);
        }
        s = dmk_wave_sum(s);
        q = dmk_wave_sum(q);
        if (lane == 0) {
            ev[j] = s / q;
            inrm[j] = 1.0 / sqrt(q);
            if (!(fabs(s / q) <= 1.7e308)) atomicOr(bad, 1);     // NaN / Inf input: the rotation test is false for NaN, so
        }                                                        // the sweeps "converge" at once -- caught here
    }
    __syncthreads();
    int *rank = reinterpret_cast<int *>(ev + 2 * n0);
    for (int j = threadIdx.x; j < n0; j += JT) {
        const double dj = ev[j];
        int rk = 0;
        for (int q = 0; q < n0; ++q) rk += (ev[q] < dj || (ev[q] == dj && q < j)) ? 1 : 0;
        w[(size_t)mat * n0 + rk] = dj;
        rank[j] = rk;
    }
    __syncthreads();
    for (int j = wave; j < n0; j += JWV) {
        const size_t orow = (size_t)mat * n0 * n0 + (size_t)rank[j] * n0;
        for (int i = lane; i < n0; i += 64) Vt[orow + i] = Vm[(size_t)j * n0 + i] * inrm[j];
    }
}

// full symmetric copy of a lower-triangle-valid matrix
__global__ void jacobi_symm_kernel(int n0, int batch, const double *__restrict__ A, double *__restrict__ Af) {
    const long long total = (long long)batch * n0 * n0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const long long mat = t / ((long long)n0 * n0);
        const int r = (int)((t / n0) % n0), c = (int)(t % n0);
        Af[t] = A[mat * n0 * n0 + (size_t)(r >= c ? r : c) * n0 + (r >= c ? c : r)];
    }
}


// ---- warm-start fast path: Newton-like refinement of an approximate eigenbasis on the matrix cores ----------------------------
// A line search moves the fit matrix by a small step, so the rows of V0 are eigenvectors up to angles theta << 1.  Instead of
// rotating pairs (three sweeps = 48 device-wide hand-overs, 3 ms at n = 256) the basis is corrected as a whole
// (Ogita & Aishima, Japan J. Indust. Appl. Math. 35 (2018) 1007, Algorithm 1, here in row form):
//     G = V V^T,  S = V A V^T,  l_i = s_ii / g_ii,  R = I - G,  delta = 2 (|S - D|_F + |A| |R|_F)
//     f_ab = (s_ab + l_a r_ab) / (l_a - l_b)   if |l_a - l_b| > delta,   r_ab / 2 otherwise (clusters: only re-orthogonalised)
//     V <- V + F V
// which squares the error per pass (theta -> O(theta^2)) and is four n^3 products on v_mfma_f64_16x16x4_f64 plus one
// elementwise pass -- about 8 us per launch at n = 256 instead of a latency chain.  Every decision is taken on the device
// (per-matrix state word), the host reads the verdict once:
//     state 0 running | 1 converged: residual max|s_ab + l_a r_ab| and orthogonality max|r_ab| of THIS V verified against
//           4 sqrt(n) eps |A| resp. 16 sqrt(n) eps; nothing is accepted on the strength of an expected contraction
//           2 failed (|F| not small, no contraction, or unresolved cluster) -> the caller falls back to the Jacobi sweeps.
constexpr int RF_T = 256;
constexpr int RF_STAT = 8;
constexpr int RF_SPLIT = 16;  // workgroups per matrix in the analysis pass   // doubles per (matrix, pass): max|F|, max|s + l r|, max|r|, delta, anorm

struct RfGemm {
    int n, batch, nprob;
    const double *A[2], *B[2], *Cadd[2];
    double *C[2];
    const int *state;
    int pass;                // state 3 | (p << 8) ("settled by the update of pass p"): runs like state 0 in pass p, like state 1 later
    int run_mask;            // bit s set: matrices in state s take part
    int copy_mask;           // bit s set: matrices in state s get C = Cadd (the basis is carried to the other buffer)
    double *sq_part[2];      // optional [batch][nt16][nt16]: per-tile sums of squares for the norms of the analysis pass --
    int sq_mode[2];          //   mode 1: off-diagonal entries of C, mode 2: entries of I - C; a mirrored tile counts twice
    int symm[2];             // the product is symmetric: only 16 x 16 tiles on / below the diagonal are computed, each written
                             // together with its mirror image -- the two images of an off-diagonal tile agree to the last bit
};

// C = (Cadd +) A op(B), n x n row-major contiguous, one 16 x 16 tile per wave (2 x 2 waves per workgroup).  The k index is
// permuted identically in both operands: lane (x, q) owns k0 + 16 q .. + 15 of a 64-wide chunk and the t-th MFMA of the chunk
// contracts element t of the four q groups -- so NT operands are read as 128 contiguous bytes per lane.
template <bool NN>
__global__ __launch_bounds__(RF_T) void rf_gemm_kernel(RfGemm g) {
    // One 16 x 16 tile of C per WORKGROUP, the four waves split K (wave w takes the 64-wide chunks w, w + 4, ...) and the
    // partial tiles are added through LDS in the fixed order ((w0 + w1) + (w2 + w3)): at n = 256 every wave runs ONE chunk -- a
    // single round trip to L2 and 16 MFMAs -- where the one-tile-per-wave form walked four chunks in sequence (11 us per
    // launch, latency bound; round 5: these products are 2/3 of the vcor fit's kernel time).
    __shared__ double part[3][4][64];
    const int n = g.n;
    const int prob = blockIdx.z / g.batch, mat = blockIdx.z % g.batch;
    int st = g.state ? g.state[mat] : 0;
    if ((st & 0xff) == 3) st = ((st >> 8) == g.pass) ? 0 : 1;
    const bool run = (g.run_mask >> st) & 1, copy = (g.copy_mask >> st) & 1;
    if (!run && !copy) return;
    const size_t nn = (size_t)n * n;
    const double *A = g.A[prob] + mat * nn, *B = g.B[prob] + mat * nn;
    const double *Cadd = g.Cadd[prob] ? g.Cadd[prob] + mat * nn : nullptr;
    double *C = g.C[prob] + mat * nn;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const bool symm = g.symm[prob] != 0;
    if (symm && m0 < n0) return;
    if (!run) {                                            // pass-through of a finished matrix
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + q + 4 * r, col = n0 + x;
                if (row < n && col < n) C[(size_t)row * n + col] = Cadd[(size_t)row * n + col];
            }
        }
        return;
    }
    const int am = m0 + x, bn = n0 + x;
    const bool a_ok = am < n, b_ok = bn < n;
    const bool even = (n & 1) == 0;
    const double *arow = A + (size_t)(a_ok ? am : 0) * n;
    const double *brow = NN ? B + (b_ok ? bn : 0) : B + (size_t)(b_ok ? bn : 0) * n;

    auto load_row16 = [&](const double *row, bool ok, int k0, double (&r)[16]) {     // 16 consecutive k of one row
        if (ok && even && k0 + 16 <= n) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const double2 v = *reinterpret_cast<const double2 *>(row + k0 + 2 * t);
                r[2 * t] = v.x;
                r[2 * t + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 16; ++t) r[t] = (ok && k0 + t < n) ? row[k0 + t] : 0.0;
        }
    };
    auto load_col16 = [&](const double *col, bool ok, int k0, double (&r)[16]) {     // 16 consecutive k of one column
#pragma unroll
        for (int t = 0; t < 16; ++t) r[t] = (ok && k0 + t < n) ? col[(size_t)(k0 + t) * n] : 0.0;
    };

    d4_t acc = d4_t{0.0, 0.0, 0.0, 0.0};
    const int nchunk = (n + 63) / 64;
    if (wave < nchunk) {
        double a[2][16], b[2][16];
        load_row16(arow, a_ok, wave * 64 + 16 * q, a[0]);
        if (NN) load_col16(brow, b_ok, wave * 64 + 16 * q, b[0]); else load_row16(brow, b_ok, wave * 64 + 16 * q, b[0]);
#pragma unroll 1
        for (int c = wave; c < nchunk; c += 8) {
            if (c + 4 < nchunk) {
                load_row16(arow, a_ok, (c + 4) * 64 + 16 * q, a[1]);
                if (NN) load_col16(brow, b_ok, (c + 4) * 64 + 16 * q, b[1]); else load_row16(brow, b_ok, (c + 4) * 64 + 16 * q, b[1]);
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0][t], b[0][t], acc, 0, 0, 0);
            if (c + 4 < nchunk) {
                if (c + 8 < nchunk) {
                    load_row16(arow, a_ok, (c + 8) * 64 + 16 * q, a[0]);
                    if (NN) load_col16(brow, b_ok, (c + 8) * 64 + 16 * q, b[0]); else load_row16(brow, b_ok, (c + 8) * 64 + 16 * q, b[0]);
                }
#pragma unroll
                for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1][t], b[1][t], acc, 0, 0, 0);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = (acc[r] + part[0][r][lane]) + (part[1][r][lane] + part[2][r][lane]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = m0 + q + 4 * r;
        if (row < n && bn < n) {
            const size_t o = (size_t)row * n + bn;
            C[o] = Cadd ? Cadd[o] + acc[r] : acc[r];
            if (symm && m0 != n0) C[(size_t)bn * n + row] = acc[r];
        }
    }
    if (g.sq_part[prob]) {
        const int mode = g.sq_mode[prob];
        double sq = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = m0 + q + 4 * r;
            if (row < n && bn < n) {
                const double v = mode == 1 ? (row != bn ? acc[r] : 0.0) : (row == bn ? 1.0 : 0.0) - acc[r];
                sq = fma(v, v, sq);
            }
        }
        sq = dmk_wave_sum(sq);
        const int nt16 = (n + 15) / 16;
        if (lane == 0) g.sq_part[prob][((size_t)mat * nt16 + (m0 >> 4)) * nt16 + (n0 >> 4)] = (symm && m0 != n0) ? 2.0 * sq : sq;
    }
}


// |A|_2 bound of a FULL symmetric matrix: min(max column sum, Frobenius norm).  Thread <-> column (column sums equal row sums),
// four row groups per column: no wave reductions in the loop, every load coalesced and independent.  Also resets the state word.
__global__ __launch_bounds__(1024) void rf_norm_kernel(int n, const double *__restrict__ A, double *__restrict__ anorm,
                                                        int *__restrict__ state, unsigned *__restrict__ arrive, int raw) {
    __shared__ double cs[4][256];
    __shared__ double red[2][16];
    const int mat = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *a = A + (size_t)mat * n * n;
    const int grp = tid >> 8, c0 = tid & 255;
    double fro = 0.0, gmax = 0.0;
    for (int cb = 0; cb < n; cb += 256) {
        const int c = cb + c0;
        double sum = 0.0;
        if (c < n) {
#pragma unroll 8
            for (int r = grp; r < n; r += 4) {
                const double v = a[(size_t)r * n + c];
                sum += fabs(v);
                fro = fma(v, v, fro);
            }
        }
        cs[grp][c0] = sum;
        __syncthreads();
        if (grp == 0 && c < n) gmax = fmax(gmax, (cs[0][c0] + cs[1][c0]) + (cs[2][c0] + cs[3][c0]));
        __syncthreads();
    }
    fro = dmk_wave_sum(fro);
    for (int o = 32; o > 0; o >>= 1) gmax = fmax(gmax, __shfl_xor(gmax, o, 64));
    if (lane == 0) { red[0][wave] = fro; red[1][wave] = gmax; }
    __syncthreads();
    if (tid == 0) {
        double f = 0.0, gm = 0.0;
        for (int w = 0; w < 16; ++w) { f += red[0][w]; gm = fmax(gm, red[1][w]); }
        const double bound = fmin(sqrt(f), gm);
        if (raw) { anorm[mat] = bound; return; }  // dmk_sym_norm_bound: the bound itself, nothing else
        anorm[mat] = bound > 0.0 ? 1.015625 * bound : 1.0;
        state[mat] = 0;
        state[gridDim.x + mat] = -1;              // settling pass: none yet
        arrive[mat] = 0;
    }
}

// Sorted, normalised output of a verified basis: w = l (ascending, stable), row rank(j) of Vt = v_j / |v_j|.
// l_j = s_jj / g_jj are the Rayleigh quotients the analysis pass computed; |v_j|^2 = g_jj.  16 rows per workgroup.
// ASYNCHRONOUS use (`state` given): the host has not looked at the verdicts -- a matrix whose state is not 1 (verified) is left
// alone (w, Vt untouched) and every matrix's (state, settling pass) goes to `verdict_out` [2][batch] for the caller to read
// together with whatever it enqueued behind this launch.
__global__ __launch_bounds__(256) void rf_finish_kernel(int n, const double *__restrict__ V, const double *__restrict__ G,
                                                         const double *__restrict__ lam, double *__restrict__ w,
                                                         double *__restrict__ Vt, const int *__restrict__ state, int batch,
                                                         int *__restrict__ verdict_out, int no_renorm) {
    extern __shared__ double ls[];               // [n]
    __shared__ int rank_s[16];
    const int mat = blockIdx.y, j0 = blockIdx.x * 16, tid = threadIdx.x;
    const int st = state[mat] & 0xff;            // 1 verified, 3 settled by prediction (state 3 | pass << 8)
    if (verdict_out) {
        if (blockIdx.x == 0 && tid == 0) {
            verdict_out[mat] = st;
            verdict_out[batch + mat] = state[batch + mat];
        }
        if (st != 1 && st != 3) return;           // uniform over the workgroup
    }
    // V + F V is not the basis g_aa was measured on: a predicted state (3), and EVERY state of the fused analysis + update pass
    const bool renorm = st != 3 && !no_renorm;
    const double *l = lam + (size_t)mat * n;
    for (int i = tid; i < n; i += 256) ls[i] = l[i];
    __syncthreads();
    {
        const int jr = tid >> 4, part = tid & 15, j = j0 + jr;          // 16 threads count for one row
        int cnt = 0;
        if (j < n) {
            const double dj = ls[j];
            for (int q = part; q < n; q += 16) cnt += (ls[q] < dj || (ls[q] == dj && q < j)) ? 1 : 0;
        }
        cnt += __shfl_xor(cnt, 1, 64);
        cnt += __shfl_xor(cnt, 2, 64);
        cnt += __shfl_xor(cnt, 4, 64);
        cnt += __shfl_xor(cnt, 8, 64);
        if (part == 0) rank_s[jr] = cnt;
    }
    __syncthreads();
    const size_t base = (size_t)mat * n * n;
    for (int jr = tid >> 6; jr < 16; jr += 4) {
        const int j = j0 + jr;
        if (j >= n) break;
        const int rk = rank_s[jr];
        const double inrm = renorm ? 1.0 / sqrt(G[base + (size_t)j * n + j]) : 1.0;
        if ((tid & 63) == 0) w[(size_t)mat * n + rk] = ls[j];
        for (int i = tid & 63; i < n; i += 64) Vt[base + (size_t)rk * n + i] = V[base + (size_t)j * n + i] * inrm;
    }
}

struct RfAnalyse {
    int n, batch, pass, last;
    const double *S, *G, *anorm;     // anorm: bound on |A|_2 per matrix (the Jacobi shift)
    double *F, *lam, *stats;         // stats: [batch][pass][RF_STAT]
    const double *sqS, *sqG;         // [batch][nt16][nt16] per-tile sums of squares from the product kernels (lower tile triangle)
    double *part;                    // [batch][RF_SPLIT][4] partial maxima of this pass
    unsigned *arrive;                // [batch] arrival counters (zero between launches)
    int *state;
    double tol;
    int predict;                     // accept V + F V unmeasured when max|F| <= RF_PREDICT_F (see there)
};

// Settled BY PREDICTION (state 3 | pass << 8).  The correction is quadratically convergent: with every rotated pair's gap above
// delta, V' = (I + F) V has errors c max|F|^2 with c = 0.49 - 0.54 measured over the fit's whole range of steps (max|F| 1e-4 ...
// 3e-3 -> next pass 5e-9 ... 3e-6) -- so once a MEASURED max|F| is below 5e-8 the updated basis is good to 1.3e-15, ten times
// inside the 4 sqrt(n) eps budget the verification itself applies, provided the pairs that are only re-orthogonalised (gap <=
// delta) already meet that budget (m3).  Such a matrix skips the measurement pass that would confirm it -- four n^3 products,
// a third of a fit evaluation; its Rayleigh quotients l = s_aa / g_aa are those of V (error O(F^2 |A|)), and the finish kernel
// does not renormalise V' with the stale g_aa (V' is orthonormal to O(F^2) as it stands).  DMK_EIGH_PREDICT=0 switches it off.
constexpr double RF_PREDICT_F = 5.0e-8;

// One pass of the analysis, RF_SPLIT workgroups per matrix: each one forms l and delta for itself (the norms from the per-tile
// sums of the product kernels, added in a fixed order, so all of them hold the same delta) and then a slice of F; the last workgroup of a matrix to arrive
// folds the partial maxima (max is exact in any order) into the verdict.
__global__ __launch_bounds__(1024) void rf_analyse_kernel(RfAnalyse g) {
    extern __shared__ double lam[];                // [n]
    __shared__ double red[4][16];
    __shared__ double delta_s;
    __shared__ int last_s;
    const int mat = blockIdx.x / RF_SPLIT, split = blockIdx.x % RF_SPLIT;
    const int n = g.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (g.state[mat] != 0) return;                 // written only by the last workgroup of a matrix, after everyone has read it
    const size_t nn = (size_t)n * n;
    const double *__restrict__ S = g.S + mat * nn;
    const double *__restrict__ G = g.G + mat * nn;
    double *__restrict__ F = g.F + mat * nn;
    for (int i = tid; i < n; i += 1024) {
        const double l = S[(size_t)i * n + i] / G[(size_t)i * n + i];
        lam[i] = l;
        if (split == 0) g.lam[(size_t)mat * n + i] = l;
    }
    // |S - D|_F^2 and |R|_F^2 from the per-tile sums the product kernels left behind (fixed summation order)
    double ssd = 0.0, srr = 0.0;
    {
        const int nt16 = (n + 15) / 16;
        const double *pS = g.sqS + (size_t)mat * nt16 * nt16, *pG = g.sqG + (size_t)mat * nt16 * nt16;
        for (int t = tid; t < nt16 * nt16; t += 1024) {
            if (t / nt16 >= t % nt16) { ssd += pS[t]; srr += pG[t]; }
        }
    }
    ssd = dmk_wave_sum(ssd);
    srr = dmk_wave_sum(srr);
    if (lane == 0) { red[0][wave] = ssd; red[1][wave] = srr; }
    __syncthreads();
    if (tid == 0) {
        double s0 = 0.0, s1 = 0.0;
        for (int w = 0; w < 16; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
        // pairs closer than delta are only re-orthogonalised.  The floor sqrt(eps) |A| keeps the rounding noise of S
        // (~ eps |A|) from being amplified by 1 / gap into rotations whose SQUARE would show up in the orthogonality.
        delta_s = fmax(2.0 * (sqrt(s0) + g.anorm[mat] * sqrt(s1)), 1.4901161193847656e-08 * g.anorm[mat]);
    }
    __syncthreads();
    const double delta = delta_s;
    double maxf = 0.0, maxres = 0.0, maxr = 0.0, maxresc = 0.0;      // maxresc: residual of the pairs that are NOT rotated (gap <= delta)
    // rows of this workgroup: 16-row groups split, split + RF_SPLIT, ...; wave <-> row inside a group, lanes along b
    for (int a = split * 16 + wave; a < n; a += 16 * RF_SPLIT) {
        const double la = lam[a];
#pragma unroll 4
        for (int b = lane; b < n; b += 64) {
            const double r = (a == b ? 1.0 : 0.0) - G[(size_t)a * n + b];
            double f;
            if (a == b) {
                f = 0.5 * r;
            } else {
                // S comes out of the product kernel with bit-identical mirror images except inside the 16 x 16 diagonal
                // tiles; there the lower image serves both (a, b) and (b, a): F + F^T = R then holds to rounding of the
                // quotient and the update cannot spoil the orthogonality at first order
                const bool up_diag = (a >> 4) == (b >> 4) && a < b;
                const double sv = up_diag ? S[(size_t)b * n + a] : S[(size_t)a * n + b];
                const double gap = la - lam[b];
                const double num = fma(la, r, sv);
                maxres = (fabs(num) <= 1.7e308) ? fmax(maxres, fabs(num)) : INFINITY;     // NaN / Inf must not vanish in fmax
                if (fabs(gap) > delta) {
                    f = num * dmk_rcp_nr2(gap);
                } else {
                    f = 0.5 * r;
                    maxresc = fmax(maxresc, fabs(num));
                }
            }
            maxr = (fabs(r) <= 1.7e308) ? fmax(maxr, fabs(r)) : INFINITY;
            maxf = fmax(maxf, fabs(f));
            F[(size_t)a * n + b] = f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        maxf = fmax(maxf, __shfl_xor(maxf, o, 64));
        maxres = fmax(maxres, __shfl_xor(maxres, o, 64));
        maxr = fmax(maxr, __shfl_xor(maxr, o, 64));
        maxresc = fmax(maxresc, __shfl_xor(maxresc, o, 64));
    }
    __syncthreads();
    if (lane == 0) { red[0][wave] = maxf; red[1][wave] = maxres; red[2][wave] = maxr; red[3][wave] = maxresc; }
    __syncthreads();
    if (tid == 0) {
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
        for (int w = 0; w < 16; ++w) {
            m0 = fmax(m0, red[0][w]); m1 = fmax(m1, red[1][w]); m2 = fmax(m2, red[2][w]); m3 = fmax(m3, red[3][w]);
        }
        double *mine = g.part + ((size_t)mat * RF_SPLIT + split) * 4;
        mine[0] = m0; mine[1] = m1; mine[2] = m2; mine[3] = m3;
        __threadfence();
        const unsigned before = atomicAdd(&g.arrive[mat], 1u);
        last_s = (before == RF_SPLIT - 1) ? 1 : 0;
    }
    __syncthreads();
    if (last_s && wave == 0) {
        // the last workgroup of the matrix folds the RF_SPLIT x 4 partial maxima: one load per lane (they were 64 dependent
        // volatile loads of one thread), a shuffle maximum over the lanes that hold the same quantity (lane & 3)
        static_assert(RF_SPLIT * 4 <= 64, "one partial maximum per lane of a wave");
        __threadfence();
        double v = (lane < RF_SPLIT * 4) ? __hip_atomic_load(g.part + (size_t)mat * RF_SPLIT * 4 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        for (int o = 4; o < 64; o <<= 1) {
            const double u = __shfl_xor(v, o, 64);
            v = (fabs(u) <= 1.7e308 && fabs(v) <= 1.7e308) ? fmax(v, u) : INFINITY;        // NaN / Inf must not vanish in fmax
        }
        const double m0 = __shfl(v, 0, 64), m1 = __shfl(v, 1, 64), m2 = __shfl(v, 2, 64), m3 = __shfl(v, 3, 64);
        if (lane == 0) {
            const double an = g.anorm[mat];
            double *st = g.stats + ((size_t)mat * 8 + g.pass) * RF_STAT;
            st[0] = m0; st[1] = m1; st[2] = m2; st[3] = delta; st[4] = an;
            const bool finite = (delta == delta) && (delta < 1.0e300) && (m1 < 1.0e300) && (m2 < 1.0e300);
            int verdict = 0;
            if (!finite) verdict = 2;
            else if (m1 <= g.tol * an && m2 <= 4.0 * g.tol) verdict = 1;      // this V is verified: residual and orthogonality
            else if (g.predict && m0 <= RF_PREDICT_F && m3 <= g.tol * an) verdict = 3 | (g.pass << 8);
            else if (m0 > 0.125) verdict = 2;
            else if (g.pass >= 4) {
                // a close pair is first only re-orthogonalised (gap < delta) and resolved one or two passes later, when delta
                // has followed the residual down: the residual is flat for a pass and then falls quadratically.  Stagnation
                // after that is a genuine failure (a cluster the refinement cannot split): leave it to the sweeps.
                // (a resolving pass leaves |r| ~ F^2 behind, which lifts delta over the gap once more: such a pair advances
                // every other pass, so the comparison is with the residual two passes back)
                const double prev = g.stats[((size_t)mat * 8 + g.pass - 2) * RF_STAT + 1];
                if (m1 > 0.5 * prev) verdict = 2;
            }
            if (verdict == 0 && g.last) verdict = 2;
            g.arrive[mat] = 0;
            if (verdict != 0) g.state[g.batch + mat] = g.pass;       // the measurement pass that settled this matrix
            g.state[mat] = verdict;
        }
    }
}

// ---- analysis + update of one refinement pass in ONE launch (round 5) ---------------------------------------------------------
// rf_analyse_kernel writes F, a fourth product launch forms V + F V: two dependent launches per pass, 16 + 8 us at n = 256 where
// the whole pass is 40.  Here a workgroup owns one 16 x 16 tile of the new basis: it forms the 16 rows of F it needs straight
// into LDS (l from the diagonals of S and G, delta from the per-tile sums the product kernels left, every workgroup with the
// same fixed-order sums -> the same delta), multiplies them with V on the matrix cores (the four waves split k) and adds the
// old tile; the partial maxima of its F rows go to a table that the LAST workgroup of a matrix to arrive folds into the verdict.
// The update is therefore applied in the pass that settles a matrix as well: V + F V of a VERIFIED V is the same basis to
// O(max|F|^2), so nothing downstream renormalises with the g_aa of the measured V any more (rf_finish_kernel), and "settled by
// prediction" (RF_PREDICT_F) needs no state of its own.
struct RfUpdate {
    int n, batch, pass, last, predict, ldf;
    const double *S, *G, *anorm, *V;
    double *Vnew, *lam, *stats, *part;     // part: [batch][tiles][4]
    const double *sqS, *sqG;
    unsigned *arrive;
    int *state;
    double tol;
};

__global__ __launch_bounds__(RF_T) void rf_update_kernel(RfUpdate g) {
    extern __shared__ double dyn[];                 // lam[n] | Fs[16][ldf]
    __shared__ double red4[4][4];
    __shared__ double accp[3][4][64];
    __shared__ double delta_s;
    const int n = g.n, mat = blockIdx.z, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t nn = (size_t)n * n;
    const double *__restrict__ V = g.V + mat * nn;
    double *__restrict__ Vn = g.Vnew + mat * nn;
    const int m0 = blockIdx.y * 16, n0 = blockIdx.x * 16;
    const int x = lane & 15, q = lane >> 4;
    if (g.state[mat] != 0) {                         // settled or failed earlier: the basis is carried to the other buffer
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + q + 4 * r, col = n0 + x;
                if (row < n && col < n) Vn[(size_t)row * n + col] = V[(size_t)row * n + col];
            }
        }
        return;
    }
    const double *__restrict__ S = g.S + mat * nn;
    const double *__restrict__ G = g.G + mat * nn;
    double *lam = dyn, *Fs = dyn + ((n + 1) & ~1);
    const int ldf = g.ldf;
    for (int i = tid; i < n; i += RF_T) {
        const double l = S[(size_t)i * n + i] / G[(size_t)i * n + i];
        lam[i] = l;
        if (blockIdx.x == 0 && blockIdx.y == 0) g.lam[(size_t)mat * n + i] = l;
    }
    // |S - D|_F^2 and |R|_F^2 from the per-tile sums of the product kernels, in a fixed order (identical in every workgroup)
    double ssd = 0.0, srr = 0.0;
    {
        const int nt16 = (n + 15) / 16;
        const double *pS = g.sqS + (size_t)mat * nt16 * nt16, *pG = g.sqG + (size_t)mat * nt16 * nt16;
        for (int t = tid; t < nt16 * nt16; t += RF_T) {
            if (t / nt16 >= t % nt16) { ssd += pS[t]; srr += pG[t]; }
        }
    }
    ssd = dmk_wave_sum(ssd);
    srr = dmk_wave_sum(srr);
    if (lane == 0) { red4[0][wave] = ssd; red4[1][wave] = srr; }
    __syncthreads();
    if (tid == 0) {
        const double s0 = (red4[0][0] + red4[0][1]) + (red4[0][2] + red4[0][3]);
        const double s1 = (red4[1][0] + red4[1][1]) + (red4[1][2] + red4[1][3]);
        delta_s = fmax(2.0 * (sqrt(s0) + g.anorm[mat] * sqrt(s1)), 1.4901161193847656e-08 * g.anorm[mat]);
    }
    __syncthreads();
    const double delta = delta_s;
    // the 16 rows m0 .. m0 + 15 of F (all columns): wave <-> 4 rows, lanes along the columns
    double maxf = 0.0, maxres = 0.0, maxr = 0.0, maxresc = 0.0;
    for (int rr = 0; rr < 4; ++rr) {
        const int a = m0 + wave * 4 + rr;
        double *frow = Fs + (size_t)(wave * 4 + rr) * ldf;
        if (a >= n) {
            for (int b = lane; b < n; b += 64) frow[b] = 0.0;
            continue;
        }
        const double la = lam[a];
#pragma unroll 4
        for (int b = lane; b < n; b += 64) {
            const double r = (a == b ? 1.0 : 0.0) - G[(size_t)a * n + b];
            double f;
            if (a == b) {
                f = 0.5 * r;
            } else {
                const bool up_diag = (a >> 4) == (b >> 4) && a < b;          // see rf_analyse_kernel: one image of S per pair
                const double sv = up_diag ? S[(size_t)b * n + a] : S[(size_t)a * n + b];
                const double gap = la - lam[b];
                const double num = fma(la, r, sv);
                maxres = (fabs(num) <= 1.7e308) ? fmax(maxres, fabs(num)) : INFINITY;
                if (fabs(gap) > delta) {
                    f = num * dmk_rcp_nr2(gap);
                } else {
                    f = 0.5 * r;
                    maxresc = fmax(maxresc, fabs(num));
                }
            }
            maxr = (fabs(r) <= 1.7e308) ? fmax(maxr, fabs(r)) : INFINITY;
            maxf = fmax(maxf, fabs(f));
            frow[b] = f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        maxf = fmax(maxf, __shfl_xor(maxf, o, 64));
        maxres = fmax(maxres, __shfl_xor(maxres, o, 64));
        maxr = fmax(maxr, __shfl_xor(maxr, o, 64));
        maxresc = fmax(maxresc, __shfl_xor(maxresc, o, 64));
    }
    if (lane == 0) { red4[0][wave] = maxf; red4[1][wave] = maxres; red4[2][wave] = maxr; red4[3][wave] = maxresc; }
    __syncthreads();                                 // F rows and the maxima are in LDS
    // V' tile = V tile + sum_k F[m0 + x][k] V[k][n0 + x']: A from LDS (rows of F), B strided from V; wave w takes chunks w, w + 4, ..
    d4_t acc = d4_t{0.0, 0.0, 0.0, 0.0};
    {
        const int bn = n0 + x;
        const bool b_ok = bn < n;
        const double *fa = Fs + (size_t)x * ldf;
        const double *bcol = V + (b_ok ? bn : 0);
        const int nchunk = (n + 63) / 64;
#pragma unroll 1
        for (int c = wave; c < nchunk; c += 4) {
            double a[16], b[16];
            const int k0 = c * 64 + 16 * q;
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int k = k0 + t;
                a[t] = k < n ? fa[k] : 0.0;
                b[t] = (b_ok && k < n) ? bcol[(size_t)k * n] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < 16; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b[t], acc, 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) accp[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double v = (acc[r] + accp[0][r][lane]) + (accp[1][r][lane] + accp[2][r][lane]);
        const int row = m0 + q + 4 * r, col = n0 + x;
        if (row < n && col < n) Vn[(size_t)row * n + col] = V[(size_t)row * n + col] + v;
    }
    // verdict: partial maxima -> table, last workgroup of this matrix folds it (max is exact in any order)
    const int ntile = gridDim.x * gridDim.y, me = blockIdx.y * gridDim.x + blockIdx.x;
    int is_last = 0;
    if (lane == 0) {
        double *mine = g.part + ((size_t)mat * ntile + me) * 4;
        mine[0] = fmax(fmax(red4[0][0], red4[0][1]), fmax(red4[0][2], red4[0][3]));
        mine[1] = fmax(fmax(red4[1][0], red4[1][1]), fmax(red4[1][2], red4[1][3]));
        mine[2] = fmax(fmax(red4[2][0], red4[2][1]), fmax(red4[2][2], red4[2][3]));
        mine[3] = fmax(fmax(red4[3][0], red4[3][1]), fmax(red4[3][2], red4[3][3]));
        __threadfence();
        const unsigned before = atomicAdd(&g.arrive[mat], 1u);
        is_last = (before == (unsigned)ntile - 1u) ? 1 : 0;
    }
    is_last = __shfl(is_last, 0, 64);                // wave 0 only from here on
    if (!is_last) return;
    __threadfence();
    double m0v = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
    for (int t = lane; t < ntile; t += 64) {
        const volatile double *o = g.part + ((size_t)mat * ntile + t) * 4;
        m0v = fmax(m0v, o[0]); m1 = fmax(m1, o[1]); m2 = fmax(m2, o[2]); m3 = fmax(m3, o[3]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        m0v = fmax(m0v, __shfl_xor(m0v, o, 64));
        m1 = fmax(m1, __shfl_xor(m1, o, 64));
        m2 = fmax(m2, __shfl_xor(m2, o, 64));
        m3 = fmax(m3, __shfl_xor(m3, o, 64));
    }
    if (lane == 0) {
        const double an = g.anorm[mat];
        double *st = g.stats + ((size_t)mat * 8 + g.pass) * RF_STAT;
        st[0] = m0v; st[1] = m1; st[2] = m2; st[3] = delta; st[4] = an;
        const bool finite = (delta == delta) && (delta < 1.0e300) && (m1 < 1.0e300) && (m2 < 1.0e300);
        int verdict = 0;
        if (!finite) verdict = 2;
        else if (m1 <= g.tol * an && m2 <= 4.0 * g.tol) verdict = 1;          // the measured V is verified (and was updated once more)
        else if (g.predict && m0v <= RF_PREDICT_F && m3 <= g.tol * an) verdict = 3;   // settled by this update (RF_PREDICT_F)
        else if (m0v > 0.125) verdict = 2;
        else if (g.pass >= 4) {
            const double prev = g.stats[((size_t)mat * 8 + g.pass - 2) * RF_STAT + 1];
            if (m1 > 0.5 * prev) verdict = 2;                                 // stagnation: see rf_analyse_kernel
        }
        if (verdict == 0 && g.last) verdict = 2;
        g.arrive[mat] = 0;
        if (verdict != 0) g.state[g.batch + mat] = g.pass;
        g.state[mat] = verdict;
    }
}

}  // namespace

int launch_dgemm_small_nn(dmk_ctx *ctx, int M, int N, int K, int batch, const double *A, const double *B, double *C);

// Warm-start refinement driver: *ok = 1 when every matrix of the batch converged (w, Vt written), 0 when the caller has to run
// the Jacobi sweeps (nothing written).  V0 may alias Vt.
// `async_verdict` (device, [2][batch] ints) selects the ASYNCHRONOUS form used by the fused fit objective (dmk_fit_objective):
// exactly `async_passes` passes are enqueued, nothing is read back, the finish launch writes w / Vt only for verified matrices
// and leaves (state, settling pass) in `async_verdict`; *ok is then 1 and means "enqueued", not "converged".
// The scratch layout of the refinement (one dmk_scratch block): also handed to the kernel of fit.hip that leaves |A| in it.
int rf_workspace(dmk_ctx *ctx, int n, int batch, RfWorkspace *W) {
    const size_t nn = (size_t)n * n;
    const size_t b_mat = ((nn * 8 * batch) + 255) & ~(size_t)255;
    const int nt16 = (n + 15) / 16;
    const size_t b_small = (((size_t)batch * 8 * RF_STAT * 8) + (size_t)batch * n * 8 +
                            (size_t)batch * std::max(RF_SPLIT, nt16 * nt16) * 32 +
                            (size_t)2 * batch * nt16 * nt16 * 8 + (size_t)batch * 32 + 1023) & ~(size_t)255;
    void *ws = nullptr;
    int rc = dmk_scratch(ctx, 6 * b_mat + b_small, &ws);
    if (rc) return rc;
    char *p = static_cast<char *>(ws);
    W->Vb[0] = reinterpret_cast<double *>(p); p += b_mat;
    W->Vb[1] = reinterpret_cast<double *>(p); p += b_mat;
    W->T1 = reinterpret_cast<double *>(p); p += b_mat;
    W->S = reinterpret_cast<double *>(p); p += b_mat;
    W->G = reinterpret_cast<double *>(p); p += b_mat;
    W->F = reinterpret_cast<double *>(p); p += b_mat;
    W->stats = reinterpret_cast<double *>(p); p += (size_t)batch * 8 * RF_STAT * 8;
    W->lam = reinterpret_cast<double *>(p); p += (size_t)batch * n * 8;
    W->anorm = reinterpret_cast<double *>(p); p += (size_t)batch * 8;
    const int ntile16 = nt16 * nt16;
    W->part = reinterpret_cast<double *>(p); p += (size_t)batch * std::max(RF_SPLIT, ntile16) * 32;
    W->sqS = reinterpret_cast<double *>(p); p += (size_t)batch * nt16 * nt16 * 8;
    W->sqG = reinterpret_cast<double *>(p); p += (size_t)batch * nt16 * nt16 * 8;
    W->state = reinterpret_cast<int *>(p); p += (size_t)batch * 8;         // [2][batch]: verdict, settling pass
    W->arrive = reinterpret_cast<unsigned *>(p);
    return DMK_OK;
}

static int eigh_refine_try(dmk_ctx *ctx, int n, int batch, const double *A, const double *V0, double *w, double *Vt, int *ok,
                           int *passes_out, int *async_verdict = nullptr, int async_passes = 0, bool norm_done = false) {
    *ok = 0;
    const size_t nn = (size_t)n * n;
    RfWorkspace W;
    int rc = rf_workspace(ctx, n, batch, &W);
    if (rc) return rc;
    double *Vb[2] = {W.Vb[0], W.Vb[1]};
    double *T1 = W.T1, *S = W.S, *G = W.G, *F = W.F, *stats = W.stats, *lam = W.lam, *anorm = W.anorm, *part = W.part, *sqS = W.sqS,
           *sqG = W.sqG;
    int *state = W.state;
    unsigned *arrive = W.arrive;
    const int nt16 = (n + 15) / 16;
    // (norm_done: the caller has left a bound on |A|, the cleared state words and arrival counters in this workspace already --
    // dmk_fit_objective on a line-search ray, where |H0 + t V1| <= |H0| + |t| |V1| with the two bounds computed once per ray)
    if (!norm_done) hipLaunchKernelGGL(rf_norm_kernel, dim3(batch), dim3(1024), 0, ctx->stream, n, A, anorm, state, arrive, 0);
    const dim3 tiles((n + 15) / 16, (n + 15) / 16, 1);             // one 16 x 16 tile per workgroup, K split over its waves
    int cur = 0, pass = 0;
    auto gemm = [&](bool nn_mode, int nprob, const double *a0, const double *b0, const double *add0, double *c0, const double *a1,
                    const double *b1, double *c1, int run_mask, int copy_mask, bool masked, int symm0 = 0, int symm1 = 0) {
        RfGemm g;
        g.symm[0] = symm0; g.symm[1] = symm1;
        g.sq_part[0] = g.sq_part[1] = nullptr; g.sq_mode[0] = g.sq_mode[1] = 0;
        if (symm1) { g.sq_part[1] = sqG; g.sq_mode[1] = 2; }        // G = V V^T
        else if (symm0) { g.sq_part[0] = sqS; g.sq_mode[0] = 1; }   // S
        g.n = n; g.batch = batch; g.nprob = nprob;
        g.A[0] = a0; g.B[0] = b0; g.Cadd[0] = add0; g.C[0] = c0;
        g.A[1] = a1; g.B[1] = b1; g.Cadd[1] = nullptr; g.C[1] = c1;
        g.state = masked ? state : nullptr; g.run_mask = run_mask; g.copy_mask = copy_mask; g.pass = pass;
        const dim3 grid(tiles.x, tiles.y, (unsigned)(batch * nprob));
        if (nn_mode) hipLaunchKernelGGL(rf_gemm_kernel<true>, grid, dim3(RF_T), 0, ctx->stream, g);
        else hipLaunchKernelGGL(rf_gemm_kernel<false>, grid, dim3(RF_T), 0, ctx->stream, g);
    };
    const double tol = 4.0 * sqrt((double)n) * 2.220446049250313e-16;
    static const bool predict_on = !(getenv("DMK_EIGH_PREDICT") && atoi(getenv("DMK_EIGH_PREDICT")) == 0);
    const double *Vc = V0;
    std::vector<int> st(batch);
    // measured (round 5, C5 fit: 2 x 256^2): the fused analysis + update launch takes 33 us where rf_analyse_kernel + the update
    // product take 16 + 8 -- every one of the 16 column tiles of a row block recomputes the same 16 rows of F and pays the
    // preamble (diagonals, per-tile sums) again; converged fit 0.98 s against 0.89 s.  Kept behind DMK_EIGH_FUSED_UPDATE=1.
    static const bool fused_update = getenv("DMK_EIGH_FUSED_UPDATE") && atoi(getenv("DMK_EIGH_FUSED_UPDATE")) != 0;
    const int ldf = ((n + 15) & ~15) + 2;                      // LDS row stride of the F rows (bank spread)
    const size_t upd_lds = ((size_t)((n + 1) & ~1) + (size_t)16 * ldf) * sizeof(double);
    const bool use_fused = fused_update && upd_lds <= 96 * 1024;
    if (use_fused && upd_lds > 48 * 1024)
        DMK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(rf_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)upd_lds));
    auto enqueue_pass = [&](bool last) {
        gemm(false, 2, Vc, A, nullptr, T1, Vc, Vc, G, 1 << 0, 0, true, 0, 1);      // T1 = V A (A symmetric), G = V V^T
        gemm(false, 1, T1, Vc, nullptr, S, nullptr, nullptr, nullptr, 1 << 0, 0, true, 1);   // S = T1 V^T
        if (use_fused) {
            RfUpdate u;
            u.n = n; u.batch = batch; u.pass = pass; u.last = last ? 1 : 0; u.predict = predict_on ? 1 : 0; u.ldf = ldf;
            u.S = S; u.G = G; u.anorm = anorm; u.V = Vc; u.Vnew = Vb[cur]; u.lam = lam; u.stats = stats; u.part = part;
            u.sqS = sqS; u.sqG = sqG; u.arrive = arrive; u.state = state; u.tol = tol;
            hipLaunchKernelGGL(rf_update_kernel, dim3(tiles.x, tiles.y, batch), dim3(RF_T), upd_lds, ctx->stream, u);
            Vc = Vb[cur];
            cur ^= 1;
            ++pass;
            return;
        }
        RfAnalyse a;
        a.n = n; a.batch = batch; a.pass = pass; a.last = last ? 1 : 0;
        a.S = S; a.G = G; a.anorm = anorm; a.F = F; a.lam = lam; a.stats = stats; a.state = state; a.tol = tol;
        a.predict = predict_on ? 1 : 0;
        a.part = part; a.arrive = arrive; a.sqS = sqS; a.sqG = sqG;
        hipLaunchKernelGGL(rf_analyse_kernel, dim3(batch * RF_SPLIT), dim3(1024), (size_t)n * 8, ctx->stream, a);
        gemm(true, 1, F, Vc, Vc, Vb[cur], nullptr, nullptr, nullptr, 1 << 0, (1 << 1) | (1 << 2), true);   // V + F V
        Vc = Vb[cur];
        cur ^= 1;
        ++pass;
    };
    auto all_done = [&](bool *good) {
        bool done = true;
        *good = true;
        for (int i = 0; i < batch; ++i) {
            if (st[i] == 0) done = false;
            if ((st[i] & 0xff) == 2) *good = false;
        }
        return done;
    };
    if (async_verdict) {
        const int np = std::max(1, std::min(async_passes, 8));
        for (int i = 0; i < np; ++i) enqueue_pass(i == 7);
        hipLaunchKernelGGL(rf_finish_kernel, dim3((n + 15) / 16, batch), dim3(256), (size_t)n * 8, ctx->stream, n, Vc, G, lam, w, Vt,
                           state, batch, async_verdict, use_fused ? 1 : 0);
        DMK_CHECK_LAUNCH(ctx);
        if (passes_out) *passes_out = pass;
        *ok = 1;
        return DMK_OK;
    }
    bool good = true, done = false;
    const int plan[3] = {3, 4, 1};                 // passes before the first / second / third look at the verdict
    for (int round = 0; round < 3 && !done; ++round) {
        for (int i = 0; i < plan[round]; ++i) enqueue_pass(round == 2 && i == plan[round] - 1);
        DMK_CHECK_LAUNCH(ctx);
        DMK_HIP(ctx, hipMemcpyAsync(st.data(), state, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
        DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        done = all_done(&good);
        if (!good) break;
    }
    if (passes_out) *passes_out = pass;
    static const bool debug = getenv("DMK_EIGH_REFINE_DEBUG") != nullptr;
    if (debug) {
        std::vector<double> hs((size_t)batch * 8 * RF_STAT);
        DMK_HIP(ctx, hipMemcpy(hs.data(), stats, hs.size() * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < batch; ++i)
            for (int q = 0; q < pass && q < 8; ++q) {
                const double *h = &hs[((size_t)i * 8 + q) * RF_STAT];
                fprintf(stderr, "[refine] mat %d pass %d: max|F| %.3e  max|s+lr| %.3e  max|r| %.3e  delta %.3e  |A| %.3e  -> state %d\n",
                        i, q, h[0], h[1], h[2], h[3], h[4], st[i]);
            }
    }
    if (!done || !good) return DMK_OK;
    hipLaunchKernelGGL(rf_finish_kernel, dim3((n + 15) / 16, batch), dim3(256), (size_t)n * 8, ctx->stream, n, Vc, G, lam, w, Vt,
                       (const int *)state, batch, (int *)nullptr, use_fused ? 1 : 0);
    DMK_CHECK_LAUNCH(ctx);
    *ok = 1;
    return DMK_OK;
}

// Internal entry for csrc/fit.hip: warm refinement of `batch` n x n symmetric matrices from the basis V0, ENQUEUED only (see
// eigh_refine_try).  verdict_dev [2][batch]: state (1 verified: w, Vt written; 0 not yet settled after `npass` passes; 2 failed)
// and the measurement pass that settled it.
int dmk_eigh_refine_enqueue(dmk_ctx *ctx, int n, int batch, const double *A, const double *V0, double *w, double *Vt, int npass,
                            int *verdict_dev, int norm_done) {
    if (!ctx || n <= 0 || batch <= 0 || !A || !V0 || !w || !Vt || !verdict_dev) return DMK_ERR_INVALID;
    FamScope fs(ctx, DMK_FAM_EIGH);
    int ok = 0;
    return eigh_refine_try(ctx, n, batch, A, V0, w, Vt, &ok, nullptr, verdict_dev, npass, norm_done != 0);
}

// The bound on |A|_2 the refinement uses, min(max column sum, Frobenius norm) of full symmetric matrices, WITHOUT its safety factor:
// out[batch].  For callers that know how their matrix family moves (a line-search ray H0 + t V1) and bound it once.
int dmk_sym_norm_bound(dmk_ctx *ctx, int n, int batch, const double *A, double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (n <= 0 || batch <= 0 || !A || !out) return dmk_fail(ctx, DMK_ERR_INVALID, "sym_norm_bound: bad arguments");
    FamScope fs(ctx, DMK_FAM_EIGH);
    hipLaunchKernelGGL(rf_norm_kernel, dim3(batch), dim3(1024), 0, ctx->stream, n, A, out, nullptr, nullptr, 1);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

extern "C" {

int dmk_eigh_jacobi_real(dmk_ctx *ctx, int n, int batch, const double *A, const double *V0, double *w, double *Vt,
                         int *sweeps_out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (n <= 0 || batch <= 0 || !A || !w || !Vt) return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_jacobi: bad arguments");
    int b = 16;
    int npad = ((n + 2 * b - 1) / (2 * b)) * (2 * b);
    if ((size_t)4 * b * npad * 8 > 144 * 1024) {
        b = 8;
        npad = ((n + 2 * b - 1) / (2 * b)) * (2 * b);
    }
    const size_t lds = (size_t)4 * b * npad * sizeof(double);
    if (lds > 144 * 1024) return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_jacobi: n = %d exceeds the supported maximum of 576", n);
    const int nb = npad / b, nwg = nb / 2;
    if ((long long)batch * nwg > 256)
        return dmk_fail(ctx, DMK_ERR_INVALID, "eigh_jacobi: batch * n/32 = %lld workgroups would not be co-resident; use "
                        "dmk_eigh_batched_real for large batches", (long long)batch * nwg);
    FamScope fs(ctx, DMK_FAM_EIGH);
    static const bool refine_on = !(getenv("DMK_EIGH_REFINE") && atoi(getenv("DMK_EIGH_REFINE")) == 0);
    if (V0 && refine_on) {
        // a caller whose matrices keep failing the fast path (exactly degenerate levels that every step splits anew) stops
        // paying for the attempt: after three failures in a row the next eight calls go straight to the sweeps
        if (ctx->refine_skip > 0) {
            --ctx->refine_skip;
        } else {
            int ok = 0;
            const int rcr = eigh_refine_try(ctx, n, batch, A, V0, w, Vt, &ok, nullptr);
            if (rcr) return rcr;
            if (ok) {
                ctx->refine_streak = 0;
                ++ctx->refine_ok;
                if (sweeps_out) *sweeps_out = 0;
                return DMK_OK;
            }
            ++ctx->refine_failed;
            if (++ctx->refine_streak >= 3) {
                ctx->refine_streak = 0;
                ctx->refine_skip = 8;
            }
        }
    }
    const int max_sweeps = 40;
    const size_t nn = (size_t)npad * npad;
    const size_t b_mat = ((nn * 8 * batch) + 255) & ~(size_t)255;
    const size_t b_tmp = (((size_t)n * n * 8 * batch) + 255) & ~(size_t)255;
    void *ws = nullptr;
    int rc = dmk_scratch(ctx, 2 * b_mat + 3 * b_tmp + 8192 + (size_t)batch * (max_sweeps + 4) * 8, &ws);
    if (rc) return rc;
    char *p = static_cast<char *>(ws);
    double *G = reinterpret_cast<double *>(p); p += b_mat;
    double *V = reinterpret_cast<double *>(p); p += b_mat;
    double *T1 = reinterpret_cast<double *>(p); p += b_tmp;      // V0 A, later Vu
    double *T2 = reinterpret_cast<double *>(p); p += b_tmp;      // V0 A V0^T, later Vu A
    double *Af = reinterpret_cast<double *>(p); p += b_tmp;      // full symmetric A (cold start)
    double *cshift = reinterpret_cast<double *>(p); p += ((size_t)batch * 8 + 255) & ~(size_t)255;
    unsigned *bar = reinterpret_cast<unsigned *>(p); p += ((size_t)batch * 4 + 255) & ~(size_t)255;
    int *sweeps_done = reinterpret_cast<int *>(p); p += ((size_t)batch * 4 + 255) & ~(size_t)255;
    int *abort_flag = reinterpret_cast<int *>(p); p += 256;
    int *flags = reinterpret_cast<int *>(p);
    DMK_HIP(ctx, hipMemsetAsync(bar, 0, (size_t)(p - reinterpret_cast<char *>(bar)) + (size_t)batch * max_sweeps * 4, ctx->stream));
    const long long tot0 = (long long)batch * n * n;
    const unsigned g0 = (unsigned)std::min<long long>((tot0 + 255) / 256, 8192);
    const double *Afull = A;
    if (V0) {
        rc = launch_dgemm_small_nn(ctx, n, n, n, batch, V0, A, T1);        // rows of V0 A  (A symmetric, full storage)
        if (rc) return rc;
        rc = dmk_dgemm_batched(ctx, 0, 1, n, n, n, batch, 1.0, T1, n, (int64_t)n * n, V0, n, (int64_t)n * n, 0.0, T2, n,
                               (int64_t)n * n);                           // V0 A V0^T: nearly diagonal
        if (rc) return rc;
        hipLaunchKernelGGL(jacobi_shift_kernel, dim3(batch), dim3(JT), 0, ctx->stream, n, 0, T2, cshift);
    } else {
        hipLaunchKernelGGL(jacobi_symm_kernel, dim3(g0), dim3(256), 0, ctx->stream, n, batch, A, Af);
        Afull = Af;
        hipLaunchKernelGGL(jacobi_shift_kernel, dim3(batch), dim3(JT), 0, ctx->stream, n, 1, A, cshift);
    }
    const long long total = (long long)batch * nn;
    hipLaunchKernelGGL(jacobi_init_kernel, dim3((unsigned)std::min<long long>((total + 255) / 256, 8192)), dim3(256), 0, ctx->stream,
                       n, npad, batch, A, V0 ? T1 : (const double *)nullptr, V0, cshift, G, V);
    DMK_CHECK_LAUNCH(ctx);
    JacArgs g;
    g.n = npad; g.batch = batch; g.b = b; g.nb = nb; g.max_sweeps = max_sweeps;
    g.G = G; g.V = V; g.bar = bar; g.flags = flags; g.sweeps_done = sweeps_done; g.abort_flag = abort_flag;
    g.tol = sqrt((double)npad) * 2.220446049250313e-16;
    if (b == 16) {
        DMK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(jacobi_eigh_kernel<16>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(jacobi_eigh_kernel<16>, dim3(batch * nwg), dim3(JT), lds, ctx->stream, g);
    } else {
        DMK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(jacobi_eigh_kernel<8>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(jacobi_eigh_kernel<8>, dim3(batch * nwg), dim3(JT), lds, ctx->stream, g);
    }
    DMK_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(jacobi_gather_kernel, dim3(g0), dim3(256), 0, ctx->stream, n, npad, batch, V, T1);
    rc = launch_dgemm_small_nn(ctx, n, n, n, batch, T1, Afull, T2);        // rows v_j A
    if (rc) return rc;
    hipLaunchKernelGGL(jacobi_finish_kernel, dim3(batch), dim3(JT), (size_t)n * 16 + (size_t)n * 4 + 16, ctx->stream, n, T1, T2, w, Vt,
                       abort_flag + 1);
    DMK_CHECK_LAUNCH(ctx);
    std::vector<int> sw(batch);
    int aborted = 0, nonfinite = 0;
    DMK_HIP(ctx, hipMemcpyAsync(&nonfinite, abort_flag + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipMemcpyAsync(sw.data(), sweeps_done, (size_t)batch * 4, hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipMemcpyAsync(&aborted, abort_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (aborted) return dmk_fail(ctx, DMK_ERR_STATE, "eigh_jacobi: workgroup hand-over timed out (launch not co-resident)");
    if (nonfinite) return dmk_fail(ctx, DMK_ERR_NOCONV, "eigh_jacobi: the matrix contains NaN / Inf");
    int worst = 0;
    for (int i = 0; i < batch; ++i) worst = std::max(worst, sw[i]);
    if (sweeps_out) *sweeps_out = worst;
    if (worst >= max_sweeps) return dmk_fail(ctx, DMK_ERR_NOCONV, "eigh_jacobi: no convergence in %d sweeps", max_sweeps);
    return DMK_OK;
}

}  // extern "C"
