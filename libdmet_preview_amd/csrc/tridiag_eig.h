// Eigenpairs of a real symmetric tridiagonal matrix T = (dl, el): the building blocks shared by the three solvers --
// phase 2 of eigh_kernel (eigh.hip), tri_eigpairs_kernel (eigh_tripairs.hip) and the many-workgroup solver (eigh_large.hip).
//
// el[i] couples i and i + 1, e2[i] = el[i]^2.  A block is the rows [s0, t0) of an unreduced piece of T; bs[i] / be[i] / bnorm[i]
// are the first row, one past the last row and the 1-norm of the block of row i.  The arrays may live in LDS or in global memory.
#pragma once

constexpr double DMK_EPS = 2.220446049250313e-16;

// Cuts T into unreduced blocks at the negligible couplings |e_i| <= eps (|d_i| + |d_i+1|), which are set to zero (serial: one
// thread, or the host)
__host__ __device__ __forceinline__ void dmk_tri_split(const int n, const double *dl, double *el, int *bs, int *be, double *bnorm) {
    int s0 = 0;
    for (int i = 0; i < n; ++i) {
        const bool cut = (i == n - 1) || fabs(el[i]) <= DMK_EPS * (fabs(dl[i]) + fabs(dl[i + 1]));
        if (!cut) continue;
        el[i] = 0.0;
        double nrm = 0.0;
        for (int q = s0; q <= i; ++q)
            nrm = fmax(nrm, fabs(dl[q]) + (q > s0 ? fabs(el[q - 1]) : 0.0) + (q < i ? fabs(el[q]) : 0.0));
        for (int q = s0; q <= i; ++q) { bs[q] = s0; be[q] = i + 1; bnorm[q] = nrm; }
        s0 = i + 1;
    }
}

// number of eigenvalues of the block below `x`: negative pivots of the LDL^T recurrence of T - x I
__device__ __forceinline__ int dmk_sturm_count(const double *dl, const double *e2, const int s0, const int t0, const double x,
                                               const double pivmin) {
    int cnt = 0;
    double q = dl[s0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0 ? 1 : 0;
#pragma unroll 4
    for (int i = s0 + 1; i < t0; ++i) {
        // the count only needs the SIGN of the pivots to be right up to perturbations of a few ulp of |T|, which is the
        // accuracy bisection delivers anyway
        q = (dl[i] - x) - e2[i - 1] * dmk_rcp_nr2(q);
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0 ? 1 : 0;
    }
    return cnt;
}

// eigenvalue number kk (0-based, ascending) of the block, to the last bits bisection can resolve; tn = 1-norm of the block
__device__ __forceinline__ double dmk_bisect_eigenvalue(const double *dl, const double *el, const double *e2, const int s0, const int t0,
                                                        const int kk, const double tn) {
    const int m = t0 - s0;
    // Gershgorin interval
    double emax2 = 0.0, lo = dl[s0], hi = dl[s0];
    for (int i = s0; i < t0; ++i) {
        const double rad = (i > s0 ? fabs(el[i - 1]) : 0.0) + (i + 1 < t0 ? fabs(el[i]) : 0.0);
        lo = fmin(lo, dl[i] - rad);
        hi = fmax(hi, dl[i] + rad);
        if (i + 1 < t0) emax2 = fmax(emax2, el[i] * el[i]);
    }
    const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax2);
    lo -= 2.0 * DMK_EPS * tn * m + 2.0 * pivmin;
    hi += 2.0 * DMK_EPS * tn * m + 2.0 * pivmin;
    // plain bisection (measured: a quadrisection with three interleaved Sturm recurrences per lane is SLOWER, 0.75 vs 0.67 ms per
    // 200 x 200 matrix -- the loop is bound by f64 instruction issue (v_rcp_f64 + two Newton steps per pivot), not by latency)
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        const int cnt = dmk_sturm_count(dl, e2, s0, t0, mid, pivmin);
        if (cnt > kk) hi = mid; else lo = mid;
        if (hi - lo <= DMK_EPS * (fabs(lo) + fabs(hi)) + 2.0 * pivmin) break;
    }
    return 0.5 * (lo + hi);
}

// ---- inverse iteration for one vector, run by ONE lane: Gaussian elimination with partial pivoting of the shifted block (three
// upper diagonals, multipliers, swap flags), a hashed start, forward / backward solves.  Scratch is lane-major: element i of
// array a of row r at ws[a n m + i m + r] (arrays: U0, U1, U2, multipliers, swap flags, x, y).  How many solves make a vector is
// the caller's business.
// FUSE_X1: which product of u1 x1 + u2 x2 in the backward solve is fused onto the other, rounded one.  Written as `u1 * x1 +
// u2 * x2` the compiler chose: fma(u2, x2, u1 * x1) in eigh_kernel (false), fma(u1, x1, u2 * x2) in the kernels of eigh_large.hip
// (true).  The parameter keeps the vectors of both solvers bit for bit what they were; a change that may move them in the last
// place can settle on one order and drop it.
template <bool FUSE_X1>
struct InvIt {
    int s0, t0;
    size_t sm;
    double *U0, *U1, *U2, *Lm, *Pv, *x, *yv;
    const double *dl, *el;
    double pert;
    __device__ __forceinline__ InvIt(int n, int m, int r, int j, const double *dl_, const double *el_, const int *bs, const int *be,
                                     const double *bnorm, double *ws)
        : s0(bs[j]), t0(be[j]), sm((size_t)m), dl(dl_), el(el_) {
        const size_t nm = (size_t)n * m;
        U0 = ws + r; U1 = U0 + nm; U2 = U1 + nm; Lm = U2 + nm; Pv = Lm + nm; x = Pv + nm; yv = x + nm;
        pert = fmax(DMK_EPS * bnorm[j], 1e-300);
    }
    // elimination with partial pivoting of T - lm I; tiny pivots -> eps |T|
    __device__ __forceinline__ void factor(const double lm) {
        double cd = dl[s0] - lm, cu = el[s0];
        for (int i = s0; i + 1 < t0; ++i) {
            const double sub = el[i], nd = dl[i + 1] - lm, nu = (i + 2 < t0) ? el[i + 1] : 0.0;
            const size_t o = (size_t)i * sm;
            if (fabs(cd) >= fabs(sub)) {
                if (fabs(cd) < pert) cd = cd >= 0.0 ? pert : -pert;
                const double mlt = sub / cd;
                U0[o] = cd; U1[o] = cu; U2[o] = 0.0; Lm[o] = mlt; Pv[o] = 0.0;
                cd = nd - mlt * cu;
                cu = nu;
            } else {
                const double mlt = cd / sub;
                U0[o] = sub; U1[o] = nd; U2[o] = nu; Lm[o] = mlt; Pv[o] = 1.0;
                cd = cu - mlt * nd;
                cu = -mlt * nu;
            }
        }
        if (fabs(cd) < pert) cd = cd >= 0.0 ? pert : -pert;
        U0[(size_t)(t0 - 1) * sm] = cd;
    }
    // start vector: hashed uniform numbers in (-1, 1), a function of the matrix b, the position j, the row index and the attempt
    // only (a vector does not depend on which other vectors were asked for); returns max |x|
    __device__ __forceinline__ double seed(const int b, const int j, const unsigned long long salt) {
        unsigned long long h = ((unsigned long long)b * 0x9E3779B97F4A7C15ull) ^ ((unsigned long long)(j + 1) * 0xC2B2AE3D27D4EB4Full) ^
                               (salt * 0xD6E8FEB86659FD93ull);
        double xm = 0.0;
        for (int i = s0; i < t0; ++i) {
            h += 0x9E3779B97F4A7C15ull;
            unsigned long long q = h;
            q = (q ^ (q >> 30)) * 0xBF58476D1CE4E5B9ull;
            q = (q ^ (q >> 27)) * 0x94D049BB133111EBull;
            q ^= q >> 31;
            const double v = (double)(long long)(q >> 11) * (2.0 / 9007199254740992.0) - 1.0;
            x[(size_t)i * sm] = v;
            xm = fmax(xm, fabs(v));
        }
        return xm;
    }
    // one solve (T - lm I) x_new = x / xm_in; returns max |x_new|, the scale of the next right-hand side.  It reads one array and
    // writes another (forward x -> y, backward y -> x), so the loads of a pass do not alias its stores and the compiler may run
    // several rows ahead of the recurrence.  Bounds, stride and pointers are taken into locals first: with the members themselves
    // eigh_kernel<32, 2> came out with 44 bytes more scratch per lane (1448 against 1404).
    __device__ __forceinline__ double solve(const double xm_in) {
        const int s0 = this->s0, t0 = this->t0;
        const size_t sm = this->sm;
        const double *U0 = this->U0, *U1 = this->U1, *U2 = this->U2, *Lm = this->Lm, *Pv = this->Pv;
        double *x = this->x;
        double *__restrict__ y = yv;
        const double sc = xm_in > 0.0 ? 1.0 / xm_in : 1.0;
        double cur = x[(size_t)s0 * sm] * sc;
#pragma unroll 4
        for (int i = s0; i + 1 < t0; ++i) {                // forward: row swaps and multipliers
            const size_t o = (size_t)i * sm;
            double nxt = x[o + sm] * sc;
            const double pv = Pv[o], ml = Lm[o];
            if (pv != 0.0) { const double tsw = cur; cur = nxt; nxt = tsw; }
            y[o] = cur;
            cur = nxt - ml * cur;
        }
        y[(size_t)(t0 - 1) * sm] = cur;
        double x1 = 0.0, x2 = 0.0, xm = 0.0;
#pragma unroll 4
        for (int i = t0 - 1; i >= s0; --i) {               // backward: three upper diagonals
            const size_t o = (size_t)i * sm;
            const double u0 = U0[o], u1 = U1[o], u2 = U2[o];
            double rr = y[o];
            if (i + 1 < t0) rr -= FUSE_X1 ? fma(u1, x1, u2 * x2) : fma(u2, x2, u1 * x1);
            rr /= u0;
            x[o] = rr;
            xm = fmax(xm, fabs(rr));
            x2 = x1;
            x1 = rr;
        }
        return xm;
    }
    // normalised copy into z (a row of Z)
    __device__ __forceinline__ void store(const double xm, double *z) {
        const double sc = xm > 0.0 ? 1.0 / xm : 1.0;
        double nr = 0.0;
        for (int i = s0; i < t0; ++i) { const double v = x[(size_t)i * sm] * sc; nr += v * v; }
        const double inv = sc / sqrt(nr);
        for (int i = s0; i < t0; ++i) z[i] = x[(size_t)i * sm] * inv;
    }
};

// Acceptance test of one vector z of the block [s0, t0) by one wave: |T z - lam z|_inf <= rtol |T| and | |z|^2 - 1 | <= 1e-8 (NaN
// fails both).  tn = 1-norm of the block.  Every lane returns the verdict; *res (optional) gets the residual norm and *znorm2
// (optional) |z|^2.  This is what keeps a wrong eigenvector out of rho, the bath and the vcor fit: every solver accepts by this
// rule and no other.  The unit vector of a 1 x 1 block is exact; the callers do not bring it here.
__device__ __forceinline__ bool dmk_tri_accept(const int lane, const int s0, const int t0, const double *dl, const double *el,
                                               const double tn, const double lj, const double *z, const double rtol,
                                               double *res = nullptr, double *znorm2 = nullptr) {
    double r = 0.0, zn = 0.0;
    for (int i = s0 + lane; i < t0; i += 64) {
        const double zi = z[i];
        double t = (dl[i] - lj) * zi;
        if (i > s0) t += el[i - 1] * z[i - 1];
        if (i + 1 < t0) t += el[i] * z[i + 1];
        r = fmax(r, fabs(t));
        if (!(fabs(t) <= 1.7e308)) r = 1.7e308;            // NaN / Inf: fmax would drop a NaN
        zn += zi * zi;
    }
    r = dmk_wave_max(r);
    zn = dmk_wave_sum(zn);
    if (res) *res = r;
    if (znorm2) *znorm2 = zn;
    return r <= rtol * fmax(tn, 1e-300) && fabs(zn - 1.0) <= 1e-8;
}

// Clusters: eigenvalues of one block (lam ascending inside a block) closer than 1e-3 |T| form a cluster whose vectors (rows of Zt,
// row length n) are re-orthogonalised -- modified Gram-Schmidt, twice -- by one wave per cluster, members in ascending order:
// independently computed vectors of a (near-)degenerate group span the right invariant subspace but are not orthogonal to each
// other.  Called by every wave of the workgroup.
template <int NWAVES>
__device__ __forceinline__ void dmk_tri_cluster_mgs(const int n, const int lane, const int wave, const int *bs, const int *be,
                                                    const double *lam, const double *bnorm, double *Zt) {
    int cluster = -1;
    for (int j = 0; j < n; ++j) {
        const bool first = (j == bs[j]) || (lam[j] - lam[j - 1] > 1e-3 * bnorm[j]);
        if (!first) continue;
        ++cluster;
        if (cluster % NWAVES != wave) continue;
        const int s0 = bs[j], t0 = be[j];
        int last = j;
        while (last + 1 < t0 && lam[last + 1] - lam[last] <= 1e-3 * bnorm[j]) ++last;
        for (int q = j + 1; q <= last; ++q) {
            double *zq = Zt + (size_t)q * n;
            for (int pass = 0; pass < 2; ++pass)
                for (int p = j; p < q; ++p) {
                    const double *zp = Zt + (size_t)p * n;
                    double dot = 0.0;
                    for (int i = s0 + lane; i < t0; i += 64) dot += zp[i] * zq[i];
                    dot = dmk_wave_sum(dot);
                    for (int i = s0 + lane; i < t0; i += 64) zq[i] -= dot * zp[i];
                }
            double nr = 0.0;
            for (int i = s0 + lane; i < t0; i += 64) nr += zq[i] * zq[i];
            nr = dmk_wave_sum(nr);
            const double inv = nr > 0.0 ? 1.0 / sqrt(nr) : 0.0;
            for (int i = s0 + lane; i < t0; i += 64) zq[i] *= inv;
        }
    }
}

// Stable ascending rank sort of the n eigenvalues `key`, one thread per eigenvalue: w[rank] = key[j]; rank goes to rank_a[j] and
// rank_b[j] (either may be null)
template <int NTHREADS>
__device__ __forceinline__ void dmk_tri_rank_sort(const int n, const int tid, const double *key, double *w, int *rank_a, int *rank_b) {
    for (int j = tid; j < n; j += NTHREADS) {
        const double dj = key[j];
        int rk = 0;
        for (int q = 0; q < n; ++q) {
            const double dq = key[q];
            rk += (dq < dj || (dq == dj && q < j)) ? 1 : 0;
        }
        w[rk] = dj;
        if (rank_a) rank_a[j] = rk;
        if (rank_b) rank_b[j] = rk;
    }
}
