// K23 -- full configuration interaction (FCI) of a small impurity on the device, restricted (one h1, one ERI block) or unrestricted
// (h1[2]; blocks aa, ab, bb).  Replaces PySCF's direct_spin1 / direct_uhf behind the reference's solver/fci.py.  DESIGN.md K23.
//
// Determinants |Ia Ib> = prod_{p in Ia} a+_p,alpha prod_{q in Ib} a+_q,beta |0>, orbitals ascending; strings are bit masks ordered by
// integer value; the vector is c[Ia][Ib], row-major, Nb fastest.  With E_pq = a+_p a_q of one spin
//     H = H0 + sum_s h~s_pq Es_pq + 1/2 sum_st g^st_pqrs Es_pq Et_rs,      h~s_pq = hs_pq - 1/2 sum_r g^ss_prrq.
// sigma = H c by N-resolution over slabs [j0, j1) of alpha rows:
//   fci_d_kernel    D^t[rs][J] = (Et_rs c)(J) for every determinant J of the slab, through the DENSE link table of each spin
//                   (entry [rs][J]: the one string K with <J|E_rs|K> != 0, and the sign; 0 where there is none), so every element of
//                   D is written exactly once and nothing is zeroed beforehand.  Alpha links copy whole contiguous rows c[Ka][:]; beta
//                   links gather inside the row c[Ja][:], which a workgroup stages in LDS where it fits.  The last row of D is c.
//   dmk_dgemm_batched   G = 1/2 A D, with A the supermatrix [g^st[pq][rs] | 2 h~s_pq] made at create (the one-body term rides in
//                   the last column against the row c of D).
//   fci_s_kernel    sigma(I) += sum_{s,pq} <I|Es_pq|J> G[(s,pq)][J]: every sigma element is owned by one thread, which walks the
//                   element's own link lists (sorted by target string: a fixed order of additions); of the alpha links of row Ia
//                   only those whose target row lies in the slab contribute, beta links stay inside the slab.  No atomics.
// The densities of a vector are one Gram product of [D^a; D^b; c] with itself, accumulated over the same slabs in a fixed order.
// Davidson for the lowest root with a diagonal preconditioner; basis and H basis stay on the device, every dot product and linear
// combination is a fixed-grid reduction, the small eigenproblem (<= 16) is solved on the host.
#include "devres.h"
#include <cmath>
#include <limits>

namespace {

constexpr int NT = 256, RED_GRID = 512, LDS_NB = 4096, MAX_SPACE = 16, NORB_MAX = 32;

long long binom(int n, int k) {
    if (k < 0 || k > n) return 0;
    long long r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return r;
}

// ---- host: strings and link tables of one spin ---------------------------------------------------------------------------------
struct Strings {
    int n = 0, ne = 0, nlink = 0;
    long long ns = 0;
    std::vector<uint32_t> mask;       // ascending
    std::vector<int32_t> dense;       // [n n][ns]: sign * (K + 1) of <J|E_pq|K>, 0: none
    std::vector<int32_t> lpq, ltgt;   // [nlink][ns]: pair index, sign * (target + 1); sorted by target within a string
};

long long rank_of(uint32_t m) {        // position of a mask among the masks of its popcount, in integer order
    long long r = 0;
    int i = 0;
    for (int p = 0; p < 32; ++p)
        if (m >> p & 1u) r += binom(p, ++i);
    return r;
}

void build_strings(int n, int ne, Strings &S) {
    S.n = n; S.ne = ne; S.ns = binom(n, ne); S.nlink = ne * (n - ne + 1);
    S.mask.resize((size_t)S.ns);
    if (ne == 0) S.mask[0] = 0;
    else {
        uint64_t m = (1ull << ne) - 1;
        for (long long i = 0; i < S.ns; ++i) {
            S.mask[(size_t)i] = (uint32_t)m;
            const uint64_t c = m & (~m + 1), r = m + c;       // next mask with the same popcount
            m = (((r ^ m) >> 2) / c) | r;
        }
    }
    S.dense.assign((size_t)n * n * S.ns, 0);
    S.lpq.assign((size_t)std::max(S.nlink, 1) * S.ns, 0);
    S.ltgt.assign((size_t)std::max(S.nlink, 1) * S.ns, 0);
    std::vector<std::pair<long long, int>> row;     // (target, signed pair)
    for (long long j = 0; j < S.ns; ++j) {
        const uint32_t J = S.mask[(size_t)j];
        row.clear();
        // <J|E_pq|K> != 0: p in J, (q not in J or q == p), K = J - p + q
        for (int p = 0; p < n; ++p) {
            if (!(J >> p & 1u)) continue;
            for (int q = 0; q < n; ++q) {
                if (q != p && (J >> q & 1u)) continue;
                const uint32_t K = (J & ~(1u << p)) | (1u << q);
                const int lo = std::min(p, q), hi = std::max(p, q);
                const uint32_t between = hi - lo > 1 ? (J & (((1u << hi) - 1u) & ~((2u << lo) - 1u))) : 0u;
                const int sgn = (__builtin_popcount(between) & 1) ? -1 : 1;
                const long long k = rank_of(K);
                S.dense[(size_t)(p * n + q) * S.ns + j] = (int32_t)(sgn * (k + 1));
                row.push_back({k, sgn * (p * n + q + 1)});
            }
        }
        std::sort(row.begin(), row.end(), [](const std::pair<long long, int> &a, const std::pair<long long, int> &b) {
            return a.first != b.first ? a.first < b.first : std::abs(a.second) < std::abs(b.second); });
        for (size_t l = 0; l < row.size(); ++l) {
            const int sp = row[l].second, sgn = sp < 0 ? -1 : 1;
            S.lpq[l * S.ns + j] = std::abs(sp) - 1;
            S.ltgt[l * S.ns + j] = (int32_t)(sgn * (row[l].first + 1));
        }
    }
}

// ---- device ---------------------------------------------------------------------------------------------------------------------
struct DArgs {
    int n2, split;                  // split 0: D[rs] = D^a + D^b (n2 rows); 1: D^a rows [0, n2), D^b rows [n2, 2 n2); then the row c
    long long Na, Nb, j0, cols;     // cols = (j1 - j0) Nb: the leading dimension of D
    const int32_t *denseA, *denseB;
    const double *c;
    double *D;
};

__global__ __launch_bounds__(NT) void fci_d_kernel(DArgs g) {
    __shared__ double crow[LDS_NB];
    const long long r = blockIdx.x, Ja = g.j0 + r, Nb = g.Nb;
    const double *cJ = g.c + Ja * Nb;
    const bool staged = Nb <= LDS_NB;
    if (staged) {
        for (long long b = threadIdx.x; b < Nb; b += NT) crow[b] = cJ[b];
        __syncthreads();
    }
    const long long step = (long long)gridDim.y * NT;
    for (long long Jb = (long long)blockIdx.y * NT + threadIdx.x; Jb < Nb; Jb += step) {
        double *Dc = g.D + r * Nb + Jb;
        for (int pq = 0; pq < g.n2; ++pq) {
            const int ea = g.denseA[(long long)pq * g.Na + Ja];         // the same for the whole workgroup
            const int eb = g.denseB[(long long)pq * Nb + Jb];
            double va = 0.0, vb = 0.0;
            if (ea) { const double x = g.c[(long long)(abs(ea) - 1) * Nb + Jb]; va = ea < 0 ? -x : x; }
            if (eb) { const int k = abs(eb) - 1; const double x = staged ? crow[k] : cJ[k]; vb = eb < 0 ? -x : x; }
            if (g.split) {
                Dc[(long long)pq * g.cols] = va;
                Dc[(long long)(g.n2 + pq) * g.cols] = vb;
            } else Dc[(long long)pq * g.cols] = va + vb;
        }
        Dc[(long long)(g.split ? 2 * g.n2 : g.n2) * g.cols] = staged ? crow[Jb] : cJ[Jb];
    }
}

struct SArgs {
    int nlA, nlB, offB, first;      // offB: first row of G of the beta pairs (0 for one spin block); first: sigma is overwritten
    long long Na, Nb, j0, j1, cols;
    const int32_t *lpqA, *ltgtA, *lpqB, *ltgtB;
    const double *G;
    double *sigma;
};

__global__ __launch_bounds__(NT) void fci_s_kernel(SArgs g) {
    const long long Ia = blockIdx.x, Nb = g.Nb;
    const bool inslab = Ia >= g.j0 && Ia < g.j1;
    const long long step = (long long)gridDim.y * NT;
    for (long long Ib = (long long)blockIdx.y * NT + threadIdx.x; Ib < Nb; Ib += step) {
        double acc = 0.0;
        bool touched = inslab;
        for (int l = 0; l < g.nlA; ++l) {
            const int t = g.ltgtA[(long long)l * g.Na + Ia];            // the same for the whole workgroup
            const long long K = abs(t) - 1;
            if (K < g.j0 || K >= g.j1) continue;
            touched = true;
            const double x = g.G[(long long)g.lpqA[(long long)l * g.Na + Ia] * g.cols + (K - g.j0) * Nb + Ib];
            acc += t < 0 ? -x : x;
        }
        if (inslab) {
            const double *Gr = g.G + (Ia - g.j0) * Nb;
            for (int l = 0; l < g.nlB; ++l) {
                const int t = g.ltgtB[(long long)l * Nb + Ib];
                const double x = Gr[(long long)(g.offB + g.lpqB[(long long)l * Nb + Ib]) * g.cols + (abs(t) - 1)];
                acc += t < 0 ? -x : x;
            }
        }
        double *s = g.sigma + Ia * Nb + Ib;
        if (g.first) *s = acc;
        else if (touched) *s += acc;
    }
}

struct HdArgs {
    int n;
    long long Na, Nb;
    const uint32_t *strA, *strB;
    const double *tab;              // ha[n], hb[n], then n x n each: Jaa - Kaa, Jbb - Kbb, Jab
    double *hdiag;
};

__global__ __launch_bounds__(NT) void fci_hdiag_kernel(HdArgs g) {
    const int n = g.n;
    const double *ha = g.tab, *hb = ha + n, *Aaa = hb + n, *Abb = Aaa + n * n, *Jab = Abb + n * n;
    const long long nd = g.Na * g.Nb;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < nd; e += (long long)gridDim.x * NT) {
        const uint32_t a = g.strA[e / g.Nb], b = g.strB[e % g.Nb];
        double s = 0.0;
        for (int p = 0; p < n; ++p) {
            const bool pa = a >> p & 1u, pb = b >> p & 1u;
            if (!pa && !pb) continue;
            if (pa) s += ha[p];
            if (pb) s += hb[p];
            for (int q = 0; q < n; ++q) {
                const bool qa = a >> q & 1u, qb = b >> q & 1u;
                if (pa && qa) s += 0.5 * Aaa[p * n + q];
                if (pb && qb) s += 0.5 * Abb[p * n + q];
                if (pa && qb) s += Jab[p * n + q];
            }
        }
        g.hdiag[e] = s;
    }
}

// part[k][block] = the block's share of x . Y_k (k < nv, Y_k = Y + k stride); a fixed grid, a fixed tree
__global__ __launch_bounds__(NT) void fci_dot_kernel(long long n, const double *__restrict__ x, const double *__restrict__ Y, long long stride,
                                                     double *__restrict__ part) {
    __shared__ double red[NT];
    const double *y = Y + (long long)blockIdx.y * stride;
    double s = 0.0;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) s += x[e] * y[e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}
__global__ __launch_bounds__(NT) void fci_dotsum_kernel(int nblk, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double red[NT];
    double s = 0.0;
    for (int e = threadIdx.x; e < nblk; e += NT) s += part[(long long)blockIdx.x * nblk + e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

struct Coef { double a[MAX_SPACE]; };
// y = sy y + sum_k a_k X_k (sy == 0: y is not read)
__global__ __launch_bounds__(NT) void fci_comb_kernel(long long n, double sy, double *__restrict__ y, int nv, const double *__restrict__ X,
                                                      long long stride, Coef a) {
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        double s = sy != 0.0 ? sy * y[e] : 0.0;
        for (int k = 0; k < nv; ++k) s += a.a[k] * X[(long long)k * stride + e];
        y[e] = s;
    }
}
// r = (w - theta x) and t = r / |hdiag - theta|: w holds H x on entry, r on exit; t goes to `t`.  The absolute value keeps the
// preconditioner positive definite: from a start high in the spectrum (theta above part of the diagonal) the signed quotient steers
// towards the eigenvalue nearest theta and can settle on an excited state; below the diagonal the two are the same.
__global__ __launch_bounds__(NT) void fci_resid_kernel(long long n, double theta, const double *__restrict__ x, double *__restrict__ w,
                                                       const double *__restrict__ hdiag, double *__restrict__ t) {
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT) {
        const double r = w[e] - theta * x[e];
        const double d = fmax(fabs(hdiag[e] - theta), 1e-8);
        w[e] = r;
        t[e] = r / d;
    }
}
// (value, index) of the minimum of the block's share, ties to the lower index
__global__ __launch_bounds__(NT) void fci_argmin_kernel(long long n, const double *__restrict__ x, double *__restrict__ pv, long long *__restrict__ pi) {
    __shared__ double rv[NT];
    __shared__ long long ri[NT];
    double v = std::numeric_limits<double>::infinity();
    long long i = -1;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < n; e += (long long)gridDim.x * NT)
        if (x[e] < v) { v = x[e]; i = e; }
    rv[threadIdx.x] = v; ri[threadIdx.x] = i;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            const double v2 = rv[threadIdx.x + w];
            const long long i2 = ri[threadIdx.x + w];
            if (i2 >= 0 && (ri[threadIdx.x] < 0 || v2 < rv[threadIdx.x] || (v2 == rv[threadIdx.x] && i2 < ri[threadIdx.x]))) {
                rv[threadIdx.x] = v2; ri[threadIdx.x] = i2;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { pv[blockIdx.x] = rv[0]; pi[blockIdx.x] = ri[0]; }
}
__global__ void fci_unit_kernel(double *c, long long at) { c[at] = 1.0; }

// the densities out of the Gram matrix P of [D^a; D^b; c] (m = 2 n2 + 1 rows):
//   what 0: out (2, n, n), g^s_pq = P[c][(s, pq)]
//   what 1, spin 1: out (n^4) = sum_st <Es_pq Et_rs> - d_qr g_ps;  spin 2: out (3, n^4), blocks aa, ab, bb
__global__ __launch_bounds__(NT) void fci_rdm_kernel(int n, int spin, int what, const double *__restrict__ P, double *__restrict__ out) {
    const long long n2 = (long long)n * n, m = 2 * n2 + 1, n4 = n2 * n2;
    const long long total = what == 0 ? 2 * n2 : (spin == 1 ? n4 : 3 * n4);
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        if (what == 0) { out[e] = P[(m - 1) * m + e]; continue; }
        const long long blk = e / n4, f = e % n4;
        const int p = (int)(f / (n2 * n)), q = (int)(f / n2 % n), r = (int)(f / n % n), s = (int)(f % n);
        const long long qp = (long long)q * n + p, rs = (long long)r * n + s, ps = (long long)p * n + s;
        const double aa = P[qp * m + rs] - (q == r ? P[(m - 1) * m + ps] : 0.0);
        const double bb = P[(n2 + qp) * m + n2 + rs] - (q == r ? P[(m - 1) * m + n2 + ps] : 0.0);
        const double ab = P[qp * m + n2 + rs], ba = P[(n2 + qp) * m + rs];
        out[e] = spin == 1 ? (aa + bb) + (ab + ba) : blk == 0 ? aa : blk == 1 ? ab : bb;
    }
}

int grid_of(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + NT - 1) / NT, RED_GRID)); }

// symmetric eigenproblem of the projected matrix (m <= 16) on the host: cyclic Jacobi; the lowest pair
void host_lowest(int m, const double *H, double *theta, double *y) {
    double A[MAX_SPACE][MAX_SPACE], V[MAX_SPACE][MAX_SPACE];
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) { A[i][j] = 0.5 * (H[i * MAX_SPACE + j] + H[j * MAX_SPACE + i]); V[i][j] = i == j; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) (i == j ? dia : off) += A[i][j] * A[i][j];
        if (off <= 1e-34 * dia || off == 0.0) break;
        for (int p = 0; p < m; ++p)
            for (int q = p + 1; q < m; ++q) {
                if (A[p][q] == 0.0) continue;
                const double tau = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int k = 0; k < m; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < m; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < m; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int best = 0;
    for (int i = 1; i < m; ++i)
        if (A[i][i] < A[best][best]) best = i;
    *theta = A[best][best];
    double nrm = 0.0;
    for (int k = 0; k < m; ++k) nrm += V[k][best] * V[k][best];
    nrm = std::sqrt(nrm);
    int big = 0;
    for (int k = 1; k < m; ++k)
        if (std::fabs(V[k][best]) > std::fabs(V[big][best])) big = k;
    const double sg = V[big][best] < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < m; ++k) y[k] = sg * V[k][best] / nrm;
}

struct Plan { long long Na, Nb, ndet, mrows, drows, fixed, per_row; };

// fixed: c, hdiag, one work vector, basis and H basis, the tables, the supermatrix, the Gram matrix; per alpha row: its columns of D, G
int make_plan(int n, int na, int nb, int spin, int max_space, Plan *P) {
    if (n < 1 || n > NORB_MAX || na < 0 || nb < 0 || na > n || nb > n || spin < 1 || spin > 2 || max_space < 2 || max_space > MAX_SPACE)
        return DMK_ERR_INVALID;
    P->Na = binom(n, na); P->Nb = binom(n, nb);
    if (P->Na > 0x7fffffffLL || P->Nb > 0x7fffffffLL || P->Na > (1LL << 40) / P->Nb) return DMK_ERR_INVALID;
    P->ndet = P->Na * P->Nb;
    const long long n2 = (long long)n * n;
    P->mrows = spin * n2;            // rows of G
    P->drows = 2 * n2 + 1;           // rows of D: enough for the split form of the densities (spin 1 sigma uses n2 + 1 of them)
    const long long vec = (long long)dmk_align256((size_t)P->ndet * 8);
    long long f = (3 + 2LL * max_space) * vec;
    const long long nla = std::max(na * (n - na + 1), 1), nlb = std::max(nb * (n - nb + 1), 1);
    f += (long long)dmk_align256((size_t)(n2 * P->Na * 4)) + 2 * (long long)dmk_align256((size_t)(nla * P->Na * 4)) + (long long)dmk_align256((size_t)P->Na * 4);
    f += (long long)dmk_align256((size_t)(n2 * P->Nb * 4)) + 2 * (long long)dmk_align256((size_t)(nlb * P->Nb * 4)) + (long long)dmk_align256((size_t)P->Nb * 4);
    f += (long long)dmk_align256((size_t)(P->mrows * (P->mrows + 1) * 8));     // supermatrix
    f += (long long)dmk_align256((size_t)(P->drows * P->drows * 8));           // Gram matrix
    f += (long long)dmk_align256((size_t)((2 * n + 3 * n2) * 8));              // hdiag tables
    f += (long long)dmk_align256((size_t)(RED_GRID * (MAX_SPACE + 1) * 16)) + 4096;
    P->fixed = f;
    P->per_row = (P->drows + P->mrows) * P->Nb * 8;
    return DMK_OK;
}

}  // namespace

struct dmk_fci {
    dmk_ctx *ctx = nullptr;
    int n = 0, na = 0, nb = 0, spin = 1, max_space = 0, nlA = 0, nlB = 0;
    long long Na = 0, Nb = 0, ndet = 0, rows = 0, vec = 0;      // rows: alpha rows in flight; vec: doubles between two vectors
    Plan plan;
    DevMem mem, ws;
    double h0 = 0.0;
    double *c = nullptr, *hdiag = nullptr, *w1 = nullptr, *V = nullptr, *HV = nullptr, *A = nullptr, *P = nullptr, *tab = nullptr, *part = nullptr,
           *res = nullptr;
    int32_t *denseA = nullptr, *lpqA = nullptr, *ltgtA = nullptr, *denseB = nullptr, *lpqB = nullptr, *ltgtB = nullptr;
    uint32_t *strA = nullptr, *strB = nullptr;
    double *D = nullptr, *G = nullptr;
};

namespace {

int fci_d(dmk_fci *h, const double *c, long long j0, long long j1, int split) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    const DArgs g{h->n * h->n, split, h->Na, h->Nb, j0, (j1 - j0) * h->Nb, h->denseA, h->denseB, c, h->D};
    const unsigned ny = (unsigned)std::max<long long>(1, std::min<long long>((h->Nb + NT - 1) / NT, 8));
    hipLaunchKernelGGL(fci_d_kernel, dim3((unsigned)(j1 - j0), ny), dim3(NT), 0, ctx->stream, g);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// sigma = (H - H0) c; c and sigma: device, ndet doubles, not overlapping
int fci_sigma(dmk_fci *h, const double *c, double *sigma) {
    dmk_ctx *ctx = h->ctx;
    const int n2 = h->n * h->n, M = h->spin * n2, Kd = M + 1;
    const unsigned ny = (unsigned)std::max<long long>(1, std::min<long long>((h->Nb + NT - 1) / NT, 8));
    for (long long j0 = 0; j0 < h->Na; j0 += h->rows) {
        const long long j1 = std::min(h->Na, j0 + h->rows), cols = (j1 - j0) * h->Nb;
        int rc;
        if ((rc = fci_d(h, c, j0, j1, h->spin == 2))) return rc;
        if ((rc = dmk_dgemm_batched(ctx, 0, 0, M, (int)cols, Kd, 1, 0.5, h->A, Kd, 0, h->D, cols, 0, 0.0, h->G, cols, 0))) return rc;
        FamScope fs(ctx, DMK_FAM_MISC);
        const SArgs g{h->nlA, h->nlB, h->spin == 2 ? n2 : 0, j0 == 0, h->Na, h->Nb, j0, j1, cols, h->lpqA, h->ltgtA, h->lpqB, h->ltgtB, h->G, sigma};
        hipLaunchKernelGGL(fci_s_kernel, dim3((unsigned)h->Na, ny), dim3(NT), 0, ctx->stream, g);
        DMK_CHECK_LAUNCH(ctx);
    }
    return DMK_OK;
}

// out_host[k] = x . Y_k, k < nv (synchronises)
int fci_dots(dmk_fci *h, const double *x, const double *Y, long long stride, int nv, double *out_host) {
    dmk_ctx *ctx = h->ctx;
    const int grid = grid_of(h->ndet);
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(fci_dot_kernel, dim3(grid, nv), dim3(NT), 0, ctx->stream, h->ndet, x, Y, stride, h->part);
        hipLaunchKernelGGL(fci_dotsum_kernel, dim3(nv), dim3(NT), 0, ctx->stream, grid, h->part, h->res);
        DMK_CHECK_LAUNCH(ctx);
    }
    DMK_HIP(ctx, hipMemcpyAsync(out_host, h->res, (size_t)nv * 8, hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

int fci_comb(dmk_fci *h, double sy, double *y, int nv, const double *X, long long stride, const double *a) {
    dmk_ctx *ctx = h->ctx;
    Coef cf;
    for (int k = 0; k < MAX_SPACE; ++k) cf.a[k] = k < nv ? a[k] : 0.0;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(fci_comb_kernel, dim3(grid_of(h->ndet)), dim3(NT), 0, ctx->stream, h->ndet, sy, y, nv, X, stride, cf);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// the Gram matrix of [D^a; D^b; c] of the current vector, summed over the slabs in their order
int fci_gram(dmk_fci *h) {
    dmk_ctx *ctx = h->ctx;
    const int m = (int)h->plan.drows;
    for (long long j0 = 0; j0 < h->Na; j0 += h->rows) {
        const long long j1 = std::min(h->Na, j0 + h->rows), cols = (j1 - j0) * h->Nb;
        int rc;
        if ((rc = fci_d(h, h->c, j0, j1, 1))) return rc;
        if ((rc = dmk_dgemm_batched(ctx, 0, 1, m, m, (int)cols, 1, 1.0, h->D, cols, 0, h->D, cols, 0, j0 == 0 ? 0.0 : 1.0, h->P, m, 0))) return rc;
    }
    return DMK_OK;
}

template <class T> T *carve(char *&p, size_t count) {
    T *r = reinterpret_cast<T *>(p);
    p += dmk_align256(count * sizeof(T));
    return r;
}

}  // namespace

extern "C" {

int dmk_fci_plan(int norb, int na, int nb, int spin, int max_space, int64_t *bytes_host) {
    Plan P;
    if (!bytes_host || make_plan(norb, na, nb, spin, max_space, &P)) return DMK_ERR_INVALID;
    bytes_host[0] = P.fixed; bytes_host[1] = P.per_row; bytes_host[2] = P.ndet;
    return DMK_OK;
}

int dmk_fci_create(dmk_ctx *ctx, int norb, int na, int nb, int spin, const double *h1, const double *eri_aa, const double *eri_ab,
                   const double *eri_bb, double h0, int max_space, int64_t max_bytes, dmk_fci **out) {
    if (!ctx) return DMK_ERR_INVALID;
    Plan P;
    if (!out || !h1 || !eri_aa || (spin == 2 && (!eri_ab || !eri_bb)) || make_plan(norb, na, nb, spin, max_space, &P))
        return dmk_fail(ctx, DMK_ERR_INVALID, "fci_create: bad arguments (1 <= norb <= %d, 0 <= na, nb <= norb, spin 1 | 2, 2 <= max_space <= %d, "
                        "at most 2^31 - 1 strings per spin)", NORB_MAX, MAX_SPACE);
    *out = nullptr;
    long long budget = max_bytes;
    if (budget <= 0) {          // "what is free": three quarters of it, the rest stays for the caller
        size_t fr = 0, tot = 0;
        DMK_HIP(ctx, hipMemGetInfo(&fr, &tot));
        budget = (long long)(fr / 4 * 3);
    }
    if (P.fixed + P.per_row > budget)
        return dmk_fail(ctx, DMK_ERR_NOMEM, "fci_create: norb = %d, (%d, %d) electrons, %lld determinants need %lld bytes + %lld per alpha row "
                        "in flight, the budget is %lld bytes", norb, na, nb, P.ndet, P.fixed, P.per_row, budget);
    const int n = norb, n2 = n * n;
    const long long n4 = (long long)n2 * n2;
    // the integrals come back to the host once: the supermatrix and the tables of the diagonal are made here (n <= 32)
    std::vector<double> hh((size_t)spin * n2), g[3];
    const double *gsrc[3] = {eri_aa, spin == 2 ? eri_ab : eri_aa, spin == 2 ? eri_bb : eri_aa};
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    DMK_HIP(ctx, hipMemcpy(hh.data(), h1, hh.size() * 8, hipMemcpyDeviceToHost));
    for (int b = 0; b < (spin == 2 ? 3 : 1); ++b) {
        g[b].resize((size_t)n4);
        DMK_HIP(ctx, hipMemcpy(g[b].data(), gsrc[b], (size_t)n4 * 8, hipMemcpyDeviceToHost));
    }
    const double *ha = hh.data(), *hb = spin == 2 ? hh.data() + n2 : hh.data();
    const double *gaa = g[0].data(), *gab = spin == 2 ? g[1].data() : g[0].data(), *gbb = spin == 2 ? g[2].data() : g[0].data();
    auto G4 = [&](const double *gg, int p, int q, int r, int s) { return gg[(((long long)p * n + q) * n + r) * n + s]; };
    const int M = spin * n2, Kd = M + 1;
    std::vector<double> A((size_t)M * Kd);
    for (int s = 0; s < spin; ++s) {
        const double *hs = s ? hb : ha, *gs = s ? gbb : gaa;
        for (int p = 0; p < n; ++p)
            for (int q = 0; q < n; ++q) {
                double ht = hs[p * n + q];
                for (int r = 0; r < n; ++r) ht -= 0.5 * G4(gs, p, r, r, q);
                double *row = A.data() + (size_t)(s * n2 + p * n + q) * Kd;
                row[Kd - 1] = 2.0 * ht;
                for (int t = 0; t < spin; ++t)
                    for (int r = 0; r < n; ++r)
                        for (int u = 0; u < n; ++u)
                            row[t * n2 + r * n + u] = s == t ? G4(gs, p, q, r, u) : s == 0 ? G4(gab, p, q, r, u) : G4(gab, r, u, p, q);
            }
    }
    std::vector<double> tab((size_t)(2 * n + 3 * n2));
    for (int p = 0; p < n; ++p) {
        tab[p] = ha[p * n + p]; tab[n + p] = hb[p * n + p];
        for (int q = 0; q < n; ++q) {
            tab[2 * n + p * n + q] = G4(gaa, p, p, q, q) - G4(gaa, p, q, q, p);
            tab[2 * n + n2 + p * n + q] = G4(gbb, p, p, q, q) - G4(gbb, p, q, q, p);
            tab[2 * n + 2 * n2 + p * n + q] = G4(gab, p, p, q, q);
        }
    }
    Strings SA, SB;
    build_strings(n, na, SA);
    build_strings(n, nb, SB);

    dmk_fci *h = new dmk_fci;
    h->ctx = ctx; h->n = n; h->na = na; h->nb = nb; h->spin = spin; h->max_space = max_space; h->h0 = h0;
    h->Na = P.Na; h->Nb = P.Nb; h->ndet = P.ndet; h->plan = P; h->nlA = SA.nlink; h->nlB = SB.nlink;
    h->rows = std::min(std::min(P.Na, (budget - P.fixed) / P.per_row), 0x7fffffffLL / P.Nb);
    if (h->mem.alloc(ctx, (size_t)P.fixed) != hipSuccess || h->ws.alloc(ctx, (size_t)(h->rows * P.per_row)) != hipSuccess) {
        (void)hipGetLastError();
        const long long want = P.fixed + h->rows * P.per_row;
        delete h;
        return dmk_fail(ctx, DMK_ERR_NOMEM, "fci_create: no device memory for %lld bytes", want);
    }
    char *p = h->mem.get<char>();
    h->vec = (long long)(dmk_align256((size_t)P.ndet * 8) / 8);
    h->c = carve<double>(p, (size_t)P.ndet);
    h->hdiag = carve<double>(p, (size_t)P.ndet);
    h->w1 = carve<double>(p, (size_t)P.ndet);
    h->V = reinterpret_cast<double *>(p);  p += (size_t)max_space * h->vec * 8;
    h->HV = reinterpret_cast<double *>(p); p += (size_t)max_space * h->vec * 8;
    h->denseA = carve<int32_t>(p, SA.dense.size());
    h->lpqA = carve<int32_t>(p, SA.lpq.size());
    h->ltgtA = carve<int32_t>(p, SA.ltgt.size());
    h->strA = carve<uint32_t>(p, SA.mask.size());
    h->denseB = carve<int32_t>(p, SB.dense.size());
    h->lpqB = carve<int32_t>(p, SB.lpq.size());
    h->ltgtB = carve<int32_t>(p, SB.ltgt.size());
    h->strB = carve<uint32_t>(p, SB.mask.size());
    h->A = carve<double>(p, A.size());
    h->P = carve<double>(p, (size_t)(P.drows * P.drows));
    h->tab = carve<double>(p, tab.size());
    h->part = carve<double>(p, (size_t)RED_GRID * (MAX_SPACE + 1) * 2);
    h->res = carve<double>(p, 64);
    h->D = h->ws.get<double>();
    h->G = h->D + P.drows * h->rows * P.Nb;
    auto fail = [&](int code) { (void)hipStreamSynchronize(ctx->stream); delete h; return code; };
    auto up = [&](void *dst, const void *src, size_t bytes) { return bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    if (!up(h->denseA, SA.dense.data(), SA.dense.size() * 4) || !up(h->lpqA, SA.lpq.data(), SA.lpq.size() * 4) ||
        !up(h->ltgtA, SA.ltgt.data(), SA.ltgt.size() * 4) || !up(h->strA, SA.mask.data(), SA.mask.size() * 4) ||
        !up(h->denseB, SB.dense.data(), SB.dense.size() * 4) || !up(h->lpqB, SB.lpq.data(), SB.lpq.size() * 4) ||
        !up(h->ltgtB, SB.ltgt.data(), SB.ltgt.size() * 4) || !up(h->strB, SB.mask.data(), SB.mask.size() * 4) ||
        !up(h->A, A.data(), A.size() * 8) || !up(h->tab, tab.data(), tab.size() * 8))
        return fail(dmk_fail(ctx, DMK_ERR_HIP, "fci_create: upload failed"));
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(fci_hdiag_kernel, dim3(grid_of(h->ndet)), dim3(NT), 0, ctx->stream, HdArgs{n, h->Na, h->Nb, h->strA, h->strB, h->tab, h->hdiag});
        long long *pi = reinterpret_cast<long long *>(h->part + RED_GRID);
        const int grid = grid_of(h->ndet);
        hipLaunchKernelGGL(fci_argmin_kernel, dim3(grid), dim3(NT), 0, ctx->stream, h->ndet, h->hdiag, h->part, pi);
        if (hipGetLastError() != hipSuccess) return fail(dmk_fail(ctx, DMK_ERR_HIP, "fci_create: kernel launch failed"));
        std::vector<double> pv((size_t)grid);
        std::vector<long long> pidx((size_t)grid);
        if (hipMemcpyAsync(pv.data(), h->part, (size_t)grid * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(pidx.data(), pi, (size_t)grid * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess)
            return fail(dmk_fail(ctx, DMK_ERR_HIP, "fci_create: read-back failed"));
        long long at = -1;
        double best = 0.0;
        for (int b = 0; b < grid; ++b)
            if (pidx[b] >= 0 && (at < 0 || pv[b] < best || (pv[b] == best && pidx[b] < at))) { at = pidx[b]; best = pv[b]; }
        if (at < 0) return fail(dmk_fail(ctx, DMK_ERR_NOCONV, "fci_create: the diagonal is not finite"));
        if (hipMemsetAsync(h->c, 0, (size_t)h->ndet * 8, ctx->stream) != hipSuccess) return fail(dmk_fail(ctx, DMK_ERR_HIP, "fci_create: memset failed"));
        hipLaunchKernelGGL(fci_unit_kernel, dim3(1), dim3(1), 0, ctx->stream, h->c, at);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return fail(dmk_fail(ctx, DMK_ERR_HIP, "fci_create: kernel launch failed"));
    }
    *out = h;
    return DMK_OK;
}

int dmk_fci_free(dmk_fci *h) {
    if (!h) return DMK_OK;
    (void)hipStreamSynchronize(h->ctx->stream);      // work that reads the handle's memory may still be queued
    delete h;
    return DMK_OK;
}

int dmk_fci_set(dmk_fci *h, const double *c_dev) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!c_dev) return dmk_fail(ctx, DMK_ERR_INVALID, "fci_set: NULL vector");
    DMK_HIP(ctx, hipMemcpyAsync(h->c, c_dev, (size_t)h->ndet * 8, hipMemcpyDeviceToDevice, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

int dmk_fci_get(dmk_fci *h, int what, double *out_dev) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!out_dev || (what != DMK_FCI_C && what != DMK_FCI_HDIAG)) return dmk_fail(ctx, DMK_ERR_INVALID, "fci_get: bad arguments");
    DMK_HIP(ctx, hipMemcpyAsync(out_dev, what == DMK_FCI_C ? h->c : h->hdiag, (size_t)h->ndet * 8, hipMemcpyDeviceToDevice, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

int dmk_fci_info(dmk_fci *h, int64_t *info_host) {
    if (!h || !info_host) return DMK_ERR_INVALID;
    info_host[0] = h->Na; info_host[1] = h->Nb; info_host[2] = h->rows; info_host[3] = (h->Na + h->rows - 1) / h->rows;
    return DMK_OK;
}

int dmk_fci_sigma(dmk_fci *h, const double *c_dev, double *sigma_dev) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!c_dev || !sigma_dev || c_dev == sigma_dev) return dmk_fail(ctx, DMK_ERR_INVALID, "fci_sigma: two distinct device vectors are needed");
    const int rc = fci_sigma(h, c_dev, sigma_dev);
    if (rc) return rc;
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

int dmk_fci_run(dmk_fci *h, int max_iter, double tol_e, double tol_r, int max_space, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!result_host || max_iter < 0 || max_space < 2 || max_space > h->max_space || !(tol_e > 0.0) || !(tol_r > 0.0))
        return dmk_fail(ctx, DMK_ERR_INVALID, "fci_run: bad arguments (max_iter >= 0, tolerances > 0, 2 <= max_space <= %d of create)", h->max_space);
    const long long vs = h->vec;
    double Hs[MAX_SPACE * MAX_SPACE] = {0.0}, y[MAX_SPACE], d[MAX_SPACE + 1];
    double theta = std::numeric_limits<double>::quiet_NaN(), rnorm = theta, dE = theta, e_prev = theta;
    int rc, m = 0, it = 0, conv = 0;
    // the start: the current vector, normalised
    if ((rc = fci_dots(h, h->c, h->c, 0, 1, d))) return rc;
    if (!(d[0] > 0.0) || !std::isfinite(d[0])) return dmk_fail(ctx, DMK_ERR_STATE, "fci_run: the start vector is zero or not finite");
    if (max_iter > 0) {
        const double s = 1.0 / std::sqrt(d[0]);
        if ((rc = fci_comb(h, 0.0, h->V, 1, h->c, 0, &s))) return rc;
    }
    for (it = 0; it < max_iter;) {
        // H times the newest basis vector, and its row of the projected matrix
        if ((rc = fci_sigma(h, h->V + m * vs, h->HV + m * vs))) return rc;
        if ((rc = fci_dots(h, h->HV + m * vs, h->V, vs, m + 1, d))) return rc;
        for (int k = 0; k <= m; ++k) Hs[k * MAX_SPACE + m] = Hs[m * MAX_SPACE + k] = d[k];
        ++m; ++it;
        host_lowest(m, Hs, &theta, y);
        if (it == 1) e_prev = theta;
        // Ritz vector into c, H x into w1
        if ((rc = fci_comb(h, 0.0, h->c, m, h->V, vs, y))) return rc;
        if ((rc = fci_comb(h, 0.0, h->w1, m, h->HV, vs, y))) return rc;
        const bool collapse = m == max_space;
        if (collapse) {
            const double one = 1.0;
            if ((rc = fci_comb(h, 0.0, h->V, 1, h->c, 0, &one))) return rc;
            if ((rc = fci_comb(h, 0.0, h->HV, 1, h->w1, 0, &one))) return rc;
            m = 1;
            Hs[0] = theta;
        }
        double *t = h->V + m * vs;          // the next basis vector is made in its slot
        {
            FamScope fs(ctx, DMK_FAM_MISC);
            hipLaunchKernelGGL(fci_resid_kernel, dim3(grid_of(h->ndet)), dim3(NT), 0, ctx->stream, h->ndet, theta, h->c, h->w1, h->hdiag, t);
            DMK_CHECK_LAUNCH(ctx);
        }
        if ((rc = fci_dots(h, h->w1, h->w1, 0, 1, d))) return rc;
        rnorm = std::sqrt(d[0]);
        dE = theta - e_prev;
        e_prev = theta;
        if (!std::isfinite(theta) || !std::isfinite(rnorm)) return dmk_fail(ctx, DMK_ERR_NOCONV, "fci_run: not finite in iteration %d", it);
        if (std::fabs(dE) < tol_e && rnorm < tol_r) { conv = 1; break; }
        if (it == max_iter) break;
        // orthogonalise the correction against the basis (twice), normalise
        double nrm = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            if ((rc = fci_dots(h, t, h->V, vs, m, d))) return rc;
            for (int k = 0; k < m; ++k) d[k] = -d[k];
            if ((rc = fci_comb(h, 1.0, t, m, h->V, vs, d))) return rc;
        }
        if ((rc = fci_dots(h, t, t, 0, 1, d))) return rc;
        nrm = std::sqrt(d[0]);
        // nothing new to add: the space is exhausted (Ndet or a symmetry sector reached, or an exact start).  The Ritz pair cannot
        // improve, and dE is still the last real step (the residual vanished on the step that completed the space): the residual
        // alone decides.  The correction is r over an energy difference, so the absolute 1e-14 does not depend on the scale of H.
        if (!(nrm > 1e-14)) { conv = rnorm < tol_r; break; }
        const double s = 1.0 / nrm;
        if ((rc = fci_comb(h, s, t, 0, h->V, vs, d))) return rc;
    }
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    result_host[0] = theta + h->h0;
    result_host[1] = (double)conv;
    result_host[2] = (double)it;
    result_host[3] = rnorm;
    result_host[4] = dE;
    return DMK_OK;
}

int dmk_fci_rdm1(dmk_fci *h, double *out_dev) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!out_dev) return dmk_fail(ctx, DMK_ERR_INVALID, "fci_rdm1: NULL output");
    int rc;
    if ((rc = fci_gram(h))) return rc;
    const long long n2 = (long long)h->n * h->n;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(fci_rdm_kernel, dim3(grid_of(2 * n2)), dim3(NT), 0, ctx->stream, h->n, 2, 0, h->P, out_dev);
    DMK_CHECK_LAUNCH(ctx);
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

int dmk_fci_rdm2(dmk_fci *h, double *out_dev) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!out_dev) return dmk_fail(ctx, DMK_ERR_INVALID, "fci_rdm2: NULL output");
    int rc;
    if ((rc = fci_gram(h))) return rc;
    const long long n2 = (long long)h->n * h->n;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(fci_rdm_kernel, dim3(grid_of((h->spin == 1 ? 1 : 3) * n2 * n2)), dim3(NT), 0, ctx->stream, h->n, h->spin, 1, h->P, out_dev);
    DMK_CHECK_LAUNCH(ctx);
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

}  // extern "C"
