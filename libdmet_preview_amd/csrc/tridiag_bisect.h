// Sturm count and bisection for one unreduced block of a real symmetric tridiagonal matrix (device functions shared by the
// one-workgroup solver, eigh.hip, and the many-workgroup solver, eigh_large.hip).
//
// Block = rows [s0, t0) of T = (dl, el); el[i] couples i and i + 1, e2[i] = el[i]^2.  The arrays may live in LDS or in
// global memory.
#pragma once

// number of eigenvalues of the block below `x`: negative pivots of the LDL^T recurrence of T - x I
__device__ __forceinline__ int dmk_sturm_count(const double *dl, const double *e2, const int s0, const int t0, const double x,
                                               const double pivmin) {
    int cnt = 0;
    double q = dl[s0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0 ? 1 : 0;
#pragma unroll 4
    for (int i = s0 + 1; i < t0; ++i) {
        // 1 / q from v_rcp_f64 and two Newton steps (the count only needs the SIGN of the pivots to be right
        // up to perturbations of a few ulp of |T|, which is the accuracy bisection delivers anyway)
        double r = __builtin_amdgcn_rcp(q);
        r = r * (2.0 - q * r);
        r = r * (2.0 - q * r);
        q = (dl[i] - x) - e2[i - 1] * r;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0 ? 1 : 0;
    }
    return cnt;
}

// eigenvalue number kk (0-based, ascending) of the block, to the last bits bisection can resolve; tn = 1-norm of the block
__device__ __forceinline__ double dmk_bisect_eigenvalue(const double *dl, const double *el, const double *e2, const int s0, const int t0,
                                                        const int kk, const double tn) {
    const double eps = 2.220446049250313e-16;
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
    lo -= 2.0 * eps * tn * m + 2.0 * pivmin;
    hi += 2.0 * eps * tn * m + 2.0 * pivmin;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        const int cnt = dmk_sturm_count(dl, e2, s0, t0, mid, pivmin);
        if (cnt > kk) hi = mid; else lo = mid;
        if (hi - lo <= eps * (fabs(lo) + fabs(hi)) + 2.0 * pivmin) break;
    }
    return 0.5 * (lo + hi);
}
