// K21 -- restricted (closed-shell) CCSD on the device: the T1 / T2 amplitude equations with a general, non-canonical Fock matrix
// and the correlation energy, over the MO blocks that dmk_ao2mo_s4 writes.  Replaces cc.CCSD(mf).kernel() behind the reference's
// CCSD.run (solver/cc.py:905-906, :1029) for a restricted Hamiltonian.  The equations are stated in DESIGN.md K21.
//
// The ladder kernel, the permute kernels, the element-wise helpers, the contraction engine and the DIIS iteration are in cc_engine.h,
// which csrc/uccsd.hip (K24, unrestricted) includes as well; what they are:
//
// cc_ladder_kernel   THE HOT KERNEL, the particle-particle ladder out[r][a][b] (+)= sum_cd tau[r][c][d] (ac|bd), the only
//                    O(o^2 v^4) term, on the 4-fold PACKED (vv|vv) block (rows pair(a,c), columns pair(b,d)); the v^4 tensor is never
//                    unpacked to memory.  For fixed a (the batch) it is a GEMM  M = rows r, N = b, K = (c, d)  whose B operand
//                    B[(c,d)][b] = row pair(a,c) at pair(max(b,d), min(b,d)) the loader expands from the packed triangle on the fly
//                    through LDS.  The tile geometry is the one of ao2mo.hip (K19): 64 x 64 workgroup tile, K tile 16, four waves of
//                    2 x 2 v_mfma_f64_16x16x4_f64 accumulators, k-major LDS tiles of pitch 81 doubles, two stages, one barrier per K
//                    tile.  K runs over c (outer) and 16-wide chunks of d (inner), so c and the chunk are workgroup-uniform and the
//                    loader divides nothing.  Where the chunk of d lies at or above the tile's b (d >= b: the triangle is contiguous
//                    along b) the lanes of a load run along b, elsewhere along d.  Fixed-order sums, no atomics.
// cc_perm_*_kernel   out = alpha perm(in) + beta out for any order of up to four indices: 32 x 32 transposes through LDS between
//                    the fastest index of the source and the fastest index of the destination (256-byte runs on both sides), or a
//                    plain strided copy where the two are the same index.
// Contract           every other term: a two-operand contraction named by its index letters is  permute (only where the operand is
//                    not already [free, summed] or [summed, free])  ->  dmk_dgemm_batched  ->  permute-accumulate (only where the
//                    product's index order differs from the destination's).  No host loops over elements, no host round trips.
// dmk_rccsd          the handle, a Core of cc_engine.h: the (t1 | t2) vector with its DIIS ring and the intermediates (one allocation)
//                    and the contraction workspace (another).  The layout (Parts) and the ring (Ring) are the types the Lambda
//                    iteration and uccsd.hip use as well.
// Lambda             ("Lambda") the Lambda equations as the REVERSE SWEEP of the amplitude equations (lambda_update: the
//                    adjoint of every line of cc_rod in the reverse order, the (vv|vv) term being cc_ladder_kernel itself on the adjoint
//                    of R), the one-particle density (cc_rdm1_kernel assembles it), the residual without a division (cc_resid_kernel)
//                    and the Lagrangian E_corr + <l~, r> of a probe handle; their state (a second Ring and the kept intermediates) is a
//                    third allocation, made on first use.
#include "devres.h"
#include "ccsd_view.h"
#include "cc_engine.h"

namespace {

// out = in - D t with the D of cc_div_kernel: the projected residual R_od - d t, nothing divided (in and out may be the same array)
__global__ __launch_bounds__(NT) void cc_resid_kernel(int o, int v, int two, const double *in, const double *__restrict__ t,
                                                      const double *__restrict__ eo, const double *__restrict__ ev, double *out) {
    const long long vv = two ? (long long)v * v : v, total = (two ? (long long)o * o : o) * vv;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < total; e += (long long)gridDim.x * NT) {
        const long long ij = e / vv, ab = e % vv;
        double d;
        if (two) d = (eo[ij / o] + eo[ij % o]) - (ev[ab / v] + ev[ab % v]);
        else d = eo[ij] - ev[ab];
        out[e] = in[e] - d * t[e];
    }
}

// gamma (n x n, [occ | vir]) = [[doo + doo^T + 2 1, dov + dvo^T], [(dov + dvo^T)^T, dvv + dvv^T]]; dvo is handed over as (i, a)
__global__ __launch_bounds__(NT) void cc_rdm1_kernel(int o, int v, const double *__restrict__ doo, const double *__restrict__ dvv,
                                                     const double *__restrict__ dov, const double *__restrict__ dvo_ia,
                                                     double *__restrict__ gamma) {
    const int n = o + v;
    for (long long e = (long long)blockIdx.x * NT + threadIdx.x; e < (long long)n * n; e += (long long)gridDim.x * NT) {
        const int p = (int)(e / n), q = (int)(e % n);
        double x;
        if (p < o && q < o) x = doo[(long long)p * o + q] + doo[(long long)q * o + p] + (p == q ? 2.0 : 0.0);
        else if (p >= o && q >= o) x = dvv[(long long)(p - o) * v + q - o] + dvv[(long long)(q - o) * v + p - o];
        else {
            const long long ia = p < o ? (long long)p * v + q - o : (long long)q * v + p - o;
            x = dov[ia] + dvo_ia[ia];
        }
        gamma[e] = x;
    }
}

}  // namespace

struct dmk_rccsd : Core {
    int o, v;
    const double *oooo = nullptr, *ovoo = nullptr, *ovov = nullptr, *oovv = nullptr, *ovvo = nullptr, *ovvv = nullptr, *vvvv = nullptr;
    long long ld_vvvv = 0;
    double *Lovov, *Lt, *tau, *tau2, *R, *S, *Wvoov, *Wvovo, *Woooo, *Y, *Q;
    double *foo, *Foo, *Loo, *X1, *X2, *fvv, *Fvv, *Lvv, *fov, *Fov, *n1, *eo, *ev;

    // the vector: t1 | t2, t1 padded with zeros to a multiple of 32 doubles, t2 not
    dmk_rccsd(dmk_ctx *c, int nocc, int nvir, int diis_dim) : Core(c, nocc, nvir, nocc, nvir, diis_dim), o(nocc), v(nvir) {
        P = Parts({ext("ov"), ext("oovv")}, false);
    }
    // what the carve lays out; with a null base: the bytes
    size_t carve(void *base) {
        Carver c(base);
        T.carve(c, P.nx, diis);
        const Slot tab[] = {
            {&Lovov, "oovv"}, {&Lt, "oovv"}, {&tau, "oovv"}, {&tau2, "oovv"}, {&R, "oovv"}, {&S, "oovv"}, {&Wvoov, "oovv"}, {&Wvovo, "oovv"},
            {&Woooo, "oooo"}, {&Y, "ooov"}, {&Q, "ooov"}, {&foo, "oo"}, {&Foo, "oo"}, {&Loo, "oo"}, {&X1, "oo"}, {&X2, "oo"},
            {&fvv, "vv"}, {&Fvv, "vv"}, {&Lvv, "vv"}, {&fov, "ov"}, {&Fov, "ov"}, {&n1, "ov"}, {&eo, "o"}, {&ev, "v"}};
        take(c, tab);
        part = c.take(2048); rec = c.take(16);
        return (size_t)(c.p - static_cast<char *>(base));
    }

    // ---- Lambda ("Lambda"): a second allocation, made by the first Lambda call ------------------------------------
    // L: the vector (l1 | l2) and its ring, as T; k*: the T-only intermediates of cc_rod at the current t, kept across sweeps; *b: the
    // adjoints that have no home in the first allocation (those of R, S, tau, tau2, Wvoov, Wvovo, Woooo live in the buffers of those
    // names, which hold nothing between two applications of cc_rod); g1 the t1 gradient of the energy; d* / xt*: density pieces.
    DevMem lmem;
    Ring L;
    double *ktau, *ktau2, *kWvoov, *kWvovo, *kWoooo, *kFov, *kFoo, *kFvv, *kLoo, *kLvv, *kX1, *kX2;
    double *t2b, *Qb, *Yb, *t1b, *n1b, *Fovb, *Foob, *Loob, *X1b, *X2b, *Fvvb, *Lvvb, *g1;
    double *doo, *dvv, *dvo, *xt1, *xt2;
    bool have_l = false, kept = false;          // kept: the k* arrays belong to the amplitudes in T.x

    size_t lambda_carve(void *base) {
        Carver c(base);
        L.carve(c, P.nx, diis);
        const Slot tab[] = {
            {&ktau, "oovv"}, {&ktau2, "oovv"}, {&kWvoov, "oovv"}, {&kWvovo, "oovv"}, {&t2b, "oovv"}, {&kWoooo, "oooo"}, {&Qb, "ooov"}, {&Yb, "ooov"},
            {&kFoo, "oo"}, {&kLoo, "oo"}, {&kX1, "oo"}, {&kX2, "oo"}, {&Foob, "oo"}, {&Loob, "oo"}, {&X1b, "oo"}, {&X2b, "oo"}, {&doo, "oo"}, {&xt1, "oo"},
            {&kFvv, "vv"}, {&kLvv, "vv"}, {&Fvvb, "vv"}, {&Lvvb, "vv"}, {&dvv, "vv"}, {&xt2, "vv"},
            {&kFov, "ov"}, {&Fovb, "ov"}, {&t1b, "ov"}, {&n1b, "ov"}, {&g1, "ov"}, {&dvo, "ov"}};
        take(c, tab);
        return (size_t)(c.p - static_cast<char *>(base));
    }
};

namespace {

int cc_tau(dmk_rccsd *h, double c2, double c1, const double *amp, double *out) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(cc_tau_kernel, dim3(grid_of(h->P.cnt[1])), dim3(NT), 0, ctx->stream, h->o, h->o, h->v, h->v, c2, c1, amp,
                       amp, amp + h->P.off[1], out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

int cc_div(dmk_rccsd *h, int two, const double *in, double *out) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(cc_div_kernel, dim3(grid_of(h->P.cnt[two])), dim3(NT), 0, ctx->stream,
                       Denoms{h->o, h->o, h->v, h->v, h->eo, h->eo, h->ev, h->ev}, two, in, out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// *e_dev = 2 f_ia t_ia + sum (2 (ia|jb) - (ib|ja)) tau_ij^ab of the amplitude vector `amp` (h->tau is overwritten)
int cc_energy(dmk_rccsd *h, const double *amp, double *e_dev) {
    int rc;
    if ((rc = cc_tau(h, 1.0, 1.0, amp, h->tau))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[0], h->fov, amp, 2.0, 0, e_dev))) return rc;
    return cc_dot(h, h->P.cnt[1], h->Lt, h->tau, 1.0, 1, e_dev);
}

#define CT(alpha, A, sa, B, sb, beta, C, sc) do { if ((rc = E.contract(alpha, A, sa, B, sb, beta, C, sc))) return rc; } while (0)
#define PM(alpha, in, si, beta, out, so) do { if ((rc = E.perm(alpha, in, si, beta, out, so))) return rc; } while (0)

// the right-hand sides of the amplitude equations at the vector `src`, before the division: R_od of t1 into h->n1,
// of t2 into h->R.  Every intermediate named in the handle is left as the equations define it at `src`.
int cc_rod(dmk_rccsd *h, const double *src) {
    const Engine &E = h->E;
    const double *t1 = src, *t2 = src + h->P.off[1];
    const double *oooo = h->oooo, *ovoo = h->ovoo, *ovov = h->ovov, *oovv = h->oovv, *ovvo = h->ovvo, *ovvv = h->ovvv;
    double *tau = h->tau, *tau2 = h->tau2, *R = h->R, *S = h->S, *Wvoov = h->Wvoov, *Wvovo = h->Wvovo, *Woooo = h->Woooo, *Y = h->Y, *Q = h->Q;
    double *Foo = h->Foo, *Loo = h->Loo, *X1 = h->X1, *X2 = h->X2, *Fvv = h->Fvv, *Lvv = h->Lvv, *Fov = h->Fov, *n1 = h->n1;
    const double *fov = h->fov, *L = h->Lovov;
    int rc;
    if ((rc = cc_tau(h, 1.0, 1.0, src, tau))) return rc;
    if ((rc = cc_tau(h, 0.5, 1.0, src, tau2))) return rc;
    // Fock-like intermediates (the diagonals of f_oo / f_vv are on the other side: the denominators)
    PM(1.0, fov, "kc", 0.0, Fov, "kc");       CT(1.0, L, "kcld", t1, "ld", 1.0, Fov, "kc");
    PM(1.0, h->foo, "ki", 0.0, Foo, "ki");    CT(1.0, L, "kcld", tau, "ilcd", 1.0, Foo, "ki");
    PM(1.0, h->fvv, "ac", 0.0, Fvv, "ac");    CT(-1.0, L, "kcld", tau, "klad", 1.0, Fvv, "ac");
    CT(1.0, fov, "kc", t1, "ic", 0.0, X1, "ki");
    PM(1.0, Foo, "ki", 0.0, Loo, "ki");       PM(1.0, X1, "ki", 1.0, Loo, "ki");
    CT(2.0, ovoo, "lcki", t1, "lc", 1.0, Loo, "ki");    CT(-1.0, ovoo, "kcli", t1, "lc", 1.0, Loo, "ki");
    PM(1.0, Fvv, "ac", 0.0, Lvv, "ac");       CT(-1.0, fov, "kc", t1, "ka", 1.0, Lvv, "ac");
    CT(2.0, ovvv, "kdac", t1, "kd", 1.0, Lvv, "ac");    CT(-1.0, ovvv, "kcad", t1, "kd", 1.0, Lvv, "ac");
    CT(1.0, Fov, "kc", t1, "ic", 0.0, X2, "ki");
    // T1
    PM(1.0, fov, "ia", 0.0, n1, "ia");
    CT(-2.0, X1, "ki", t1, "ka", 1.0, n1, "ia");
    CT(1.0, Fvv, "ac", t1, "ic", 1.0, n1, "ia");
    CT(-1.0, Foo, "ki", t1, "ka", 1.0, n1, "ia");
    CT(2.0, Fov, "kc", t2, "kica", 1.0, n1, "ia");      CT(-1.0, Fov, "kc", t2, "ikca", 1.0, n1, "ia");
    CT(1.0, X2, "ki", t1, "ka", 1.0, n1, "ia");
    CT(2.0, ovvo, "kcai", t1, "kc", 1.0, n1, "ia");     CT(-1.0, oovv, "kiac", t1, "kc", 1.0, n1, "ia");
    CT(2.0, ovvv, "kdac", tau, "ikcd", 1.0, n1, "ia");  CT(-1.0, ovvv, "kcad", tau, "ikcd", 1.0, n1, "ia");
    CT(-2.0, ovoo, "lcki", tau, "klac", 1.0, n1, "ia"); CT(1.0, ovoo, "kcli", tau, "klac", 1.0, n1, "ia");
    // T2: R holds the terms that are symmetric under (i a) <-> (j b) as they stand, S those that are symmetrised at the end
    PM(1.0, ovov, "iajb", 0.0, R, "ijab");
    CT(1.0, ovvv, "iacb", t1, "jc", 0.0, S, "ijab");
    CT(1.0, oovv, "kibc", t1, "jc", 0.0, Q, "kibj");    CT(-1.0, Q, "kibj", t1, "ka", 1.0, S, "ijab");
    CT(-1.0, ovoo, "iajk", t1, "kb", 1.0, S, "ijab");
    CT(1.0, ovvo, "kcai", t1, "jc", 0.0, Q, "akij");    CT(-1.0, Q, "akij", t1, "kb", 1.0, S, "ijab");
    PM(1.0, oooo, "kilj", 0.0, Woooo, "klij");
    CT(1.0, ovoo, "lcki", t1, "jc", 1.0, Woooo, "klij"); CT(1.0, ovoo, "kclj", t1, "ic", 1.0, Woooo, "klij");
    CT(1.0, ovov, "kcld", tau, "ijcd", 1.0, Woooo, "klij");
    CT(1.0, Woooo, "klij", tau, "klab", 1.0, R, "ijab");                                  // hole-hole ladder
    Ladder lad{(long long)h->o * h->o, h->v, h->v, h->vvvv, h->ld_vvvv, tau, 1.0, 1.0, R};         // particle-particle ladder
    if ((rc = ladder_launch(h->ctx, lad))) return rc;
    CT(1.0, ovvv, "kcbd", tau, "ijcd", 0.0, Y, "ijkb"); CT(-1.0, t1, "ka", Y, "ijkb", 1.0, S, "ijab");
    CT(1.0, Lvv, "ac", t2, "ijcb", 1.0, S, "ijab");
    CT(-1.0, Loo, "ki", t2, "kjab", 1.0, S, "ijab");
    PM(1.0, ovvo, "kcai", 0.0, Wvoov, "akic");
    CT(1.0, ovvv, "kcad", t1, "id", 1.0, Wvoov, "akic");  CT(-1.0, ovoo, "kcli", t1, "la", 1.0, Wvoov, "akic");
    CT(-1.0, ovov, "ldkc", tau2, "ilda", 1.0, Wvoov, "akic"); CT(0.5, L, "ldkc", t2, "ilad", 1.0, Wvoov, "akic");
    PM(1.0, oovv, "kiac", 0.0, Wvovo, "akci");
    CT(1.0, ovvv, "kdac", t1, "id", 1.0, Wvovo, "akci");  CT(-1.0, ovoo, "lcki", t1, "la", 1.0, Wvovo, "akci");
    CT(-1.0, ovov, "lckd", tau2, "ilda", 1.0, Wvovo, "akci");
    CT(2.0, Wvoov, "akic", t2, "kjcb", 1.0, S, "ijab");   CT(-1.0, Wvovo, "akci", t2, "kjcb", 1.0, S, "ijab");
    CT(-1.0, Wvoov, "akic", t2, "kjbc", 1.0, S, "ijab");
    CT(-1.0, Wvovo, "bkci", t2, "kjac", 1.0, S, "ijab");
    PM(1.0, S, "ijab", 1.0, R, "ijab");
    PM(1.0, S, "jiba", 1.0, R, "ijab");
    return DMK_OK;
}

// one application of the amplitude equations to the vector `src`, the new amplitudes into `dst`
int cc_update(dmk_rccsd *h, const double *src, double *dst) {
    int rc;
    if ((rc = cc_rod(h, src))) return rc;
    if ((rc = cc_div(h, 0, h->n1, dst))) return rc;
    return cc_div(h, 1, h->R, dst + h->P.off[1]);
}

int cc_init(dmk_rccsd *h) {
    const Engine &E = h->E;
    int rc;
    if ((rc = cc_div(h, 0, h->fov, h->T.x))) return rc;
    PM(1.0, h->ovov, "iajb", 0.0, h->R, "ijab");
    if ((rc = cc_div(h, 1, h->R, h->T.x + h->P.off[1]))) return rc;
    // E(MP2) = sum (2 (ia|jb) - (ib|ja)) t_ij^ab: the doubles alone, as PySCF's init_amps reports it
    if ((rc = cc_dot(h, h->P.cnt[1], h->Lt, h->T.x + h->P.off[1], 1.0, 0, h->rec + 15))) return rc;
    h->have_amps = true;
    return DMK_OK;
}

// ---- Lambda -----------------------------------------------------------------------------------------------------------------------
int cc_resid(dmk_rccsd *h, int two, const double *in, const double *t, double *out) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(cc_resid_kernel, dim3(grid_of(h->P.cnt[two])), dim3(NT), 0, ctx->stream, h->o, h->v, two, in, t, h->eo, h->ev, out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// r1 = R_od - d t1 into h->n1, r2 into h->R, of the current amplitudes
int cc_residual(dmk_rccsd *h) {
    int rc;
    if ((rc = cc_rod(h, h->T.x))) return rc;
    if ((rc = cc_resid(h, 0, h->n1, h->T.x, h->n1))) return rc;
    return cc_resid(h, 1, h->R, h->T.x + h->P.off[1], h->R);
}

int lambda_alloc(dmk_rccsd *h) {
    if (h->lmem.get<void>()) return DMK_OK;
    dmk_ctx *ctx = h->ctx;
    const size_t bytes = h->lambda_carve(nullptr);
    if (h->lmem.alloc(ctx, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "rccsd_lambda: no device memory for %lld bytes", (long long)bytes);
    }
    h->lambda_carve(h->lmem.get<void>());
    DMK_HIP(ctx, hipMemsetAsync(h->lmem.get<void>(), 0, bytes, ctx->stream));
    return DMK_OK;
}

// the T-only quantities of the reverse sweep, once per set of amplitudes: the intermediates of cc_rod at t, and
// g1_ia = 2 f_ia + 2 sum_jb (2 (ia|jb) - (ib|ja)) t_jb
int lambda_prepare(dmk_rccsd *h) {
    if (h->kept) return DMK_OK;
    dmk_ctx *ctx = h->ctx;
    const Engine &E = h->E;
    int rc;
    if ((rc = cc_rod(h, h->T.x))) return rc;
    const long long oo = (long long)h->o * h->o, vv = (long long)h->v * h->v, ov = (long long)h->o * h->v, t2n = oo * vv;
    const struct { double *dst; const double *src; long long n; } keep[] = {
        {h->ktau, h->tau, t2n}, {h->ktau2, h->tau2, t2n}, {h->kWvoov, h->Wvoov, t2n}, {h->kWvovo, h->Wvovo, t2n}, {h->kWoooo, h->Woooo, oo * oo},
        {h->kFov, h->Fov, ov}, {h->kFoo, h->Foo, oo}, {h->kFvv, h->Fvv, vv}, {h->kLoo, h->Loo, oo}, {h->kLvv, h->Lvv, vv},
        {h->kX1, h->X1, oo}, {h->kX2, h->X2, oo}};
    for (const auto &k : keep) DMK_HIP(ctx, hipMemcpyAsync(k.dst, k.src, (size_t)k.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PM(2.0, h->fov, "ia", 0.0, h->g1, "ia");
    CT(2.0, h->Lovov, "iajb", h->T.x, "jb", 1.0, h->g1, "ia");
    h->kept = true;
    return DMK_OK;
}

#define LADDER(in, b, dst) do { if ((rc = ladder_launch(h->ctx, Ladder{(long long)h->o * h->o, h->v, h->v, h->vvvv, h->ld_vvvv, in, 1.0, b, dst}))) return rc; } while (0)

// one application of the Lambda equations to the vector `src` = (l1, l2), the new (l1, l2) into `dst`: the weights
// l~1 = 2 l1, l~2 = 2 l2 - l2^T(ab) go BACKWARDS through cc_rod (every CT(alpha, A, B -> C) gives Ab += alpha Cb . B and
// Bb += alpha Cb . A for the operands that depend on t, in the reverse order; a buffer's adjoint starts with beta = 0 where it is
// first written), then l~ = (z + g) / d and l from l~.  lambda_prepare must have run for the amplitudes in h->T.x.
int lambda_update(dmk_rccsd *h, const double *src, double *dst) {
    const Engine &E = h->E;
    const double *t1 = h->T.x, *t2 = h->T.x + h->P.off[1], *l1 = src, *l2 = src + h->P.off[1];
    const double *ovoo = h->ovoo, *ovov = h->ovov, *oovv = h->oovv, *ovvo = h->ovvo, *ovvv = h->ovvv;
    const double *fov = h->fov, *Lovov = h->Lovov;
    const double *ktau = h->ktau, *kWvoov = h->kWvoov, *kWvovo = h->kWvovo, *kWoooo = h->kWoooo, *kFov = h->kFov, *kFoo = h->kFoo,
                 *kFvv = h->kFvv, *kLoo = h->kLoo, *kLvv = h->kLvv, *kX1 = h->kX1, *kX2 = h->kX2;
    double *Rb = h->R, *Sb = h->S, *taub = h->tau, *tau2b = h->tau2, *Wvoovb = h->Wvoov, *Wvovob = h->Wvovo, *Woooob = h->Woooo;
    double *Q = h->Q, *Y = h->Y, *Qb = h->Qb, *Yb = h->Yb, *t1b = h->t1b, *t2b = h->t2b, *n1b = h->n1b;
    double *Fovb = h->Fovb, *Foob = h->Foob, *Loob = h->Loob, *X1b = h->X1b, *X2b = h->X2b, *Fvvb = h->Fvvb, *Lvvb = h->Lvvb;
    int rc;
    PM(2.0, l1, "ia", 0.0, n1b, "ia");
    PM(2.0, l2, "ijab", 0.0, Rb, "ijab");
    PM(-1.0, l2, "ijba", 1.0, Rb, "ijab");
    // R += S + S^T
    PM(1.0, Rb, "ijab", 0.0, Sb, "jiba");
    PM(1.0, Rb, "ijab", 1.0, Sb, "ijab");
    // the ring terms and their W
    CT(-1.0, Sb, "ijab", t2, "kjac", 0.0, Wvovob, "bkci");
    CT(-1.0, kWvovo, "bkci", Sb, "ijab", 0.0, t2b, "kjac");
    CT(-1.0, Sb, "ijab", t2, "kjbc", 0.0, Wvoovb, "akic");
    CT(-1.0, kWvoov, "akic", Sb, "ijab", 1.0, t2b, "kjbc");
    CT(-1.0, Sb, "ijab", t2, "kjcb", 1.0, Wvovob, "akci");
    CT(-1.0, kWvovo, "akci", Sb, "ijab", 1.0, t2b, "kjcb");
    CT(2.0, Sb, "ijab", t2, "kjcb", 1.0, Wvoovb, "akic");
    CT(2.0, kWvoov, "akic", Sb, "ijab", 1.0, t2b, "kjcb");
    CT(-1.0, ovov, "lckd", Wvovob, "akci", 0.0, tau2b, "ilda");
    CT(-1.0, ovoo, "lcki", Wvovob, "akci", 0.0, t1b, "la");
    CT(1.0, Wvovob, "akci", ovvv, "kdac", 1.0, t1b, "id");
    CT(0.5, Lovov, "ldkc", Wvoovb, "akic", 1.0, t2b, "ilad");
    CT(-1.0, ovov, "ldkc", Wvoovb, "akic", 1.0, tau2b, "ilda");
    CT(-1.0, ovoo, "kcli", Wvoovb, "akic", 1.0, t1b, "la");
    CT(1.0, ovvv, "kcad", Wvoovb, "akic", 1.0, t1b, "id");
    // Loo, Lvv
    CT(-1.0, t2, "kjab", Sb, "ijab", 0.0, Loob, "ki");
    CT(-1.0, kLoo, "ki", Sb, "ijab", 1.0, t2b, "kjab");
    CT(1.0, Sb, "ijab", t2, "ijcb", 0.0, Lvvb, "ac");
    CT(1.0, kLvv, "ac", Sb, "ijab", 1.0, t2b, "ijcb");
    // Y (made again: it is not kept), the two ladders, Woooo
    CT(1.0, ovvv, "kcbd", ktau, "ijcd", 0.0, Y, "ijkb");
    CT(-1.0, Y, "ijkb", Sb, "ijab", 1.0, t1b, "ka");
    CT(-1.0, t1, "ka", Sb, "ijab", 0.0, Yb, "ijkb");
    CT(1.0, Yb, "ijkb", ovvv, "kcbd", 0.0, taub, "ijcd");
    LADDER(Rb, 1.0, taub);                                                                   // (ac|bd) = (ca|db): its own adjoint
    CT(1.0, ktau, "klab", Rb, "ijab", 0.0, Woooob, "klij");
    CT(1.0, kWoooo, "klij", Rb, "ijab", 1.0, taub, "klab");
    CT(1.0, Woooob, "klij", ovov, "kcld", 1.0, taub, "ijcd");
    CT(1.0, Woooob, "klij", ovoo, "kclj", 1.0, t1b, "ic");
    CT(1.0, Woooob, "klij", ovoo, "lcki", 1.0, t1b, "jc");
    // the t1 terms of S (Q made again, twice)
    CT(1.0, ovvo, "kcai", t1, "jc", 0.0, Q, "akij");
    CT(-1.0, Sb, "ijab", t1, "kb", 0.0, Qb, "akij");
    CT(-1.0, Q, "akij", Sb, "ijab", 1.0, t1b, "kb");
    CT(1.0, Qb, "akij", ovvo, "kcai", 1.0, t1b, "jc");
    CT(-1.0, ovoo, "iajk", Sb, "ijab", 1.0, t1b, "kb");
    CT(1.0, oovv, "kibc", t1, "jc", 0.0, Q, "kibj");
    CT(-1.0, Sb, "ijab", t1, "ka", 0.0, Qb, "kibj");
    CT(-1.0, Q, "kibj", Sb, "ijab", 1.0, t1b, "ka");
    CT(1.0, Qb, "kibj", oovv, "kibc", 1.0, t1b, "jc");
    CT(1.0, Sb, "ijab", ovvv, "iacb", 1.0, t1b, "jc");
    // T1
    CT(1.0, ovoo, "kcli", n1b, "ia", 1.0, taub, "klac");
    CT(-2.0, ovoo, "lcki", n1b, "ia", 1.0, taub, "klac");
    CT(-1.0, n1b, "ia", ovvv, "kcad", 1.0, taub, "ikcd");
    CT(2.0, ovvv, "kdac", n1b, "ia", 1.0, taub, "ikcd");
    CT(-1.0, oovv, "kiac", n1b, "ia", 1.0, t1b, "kc");
    CT(2.0, ovvo, "kcai", n1b, "ia", 1.0, t1b, "kc");
    CT(1.0, t1, "ka", n1b, "ia", 0.0, X2b, "ki");
    CT(1.0, kX2, "ki", n1b, "ia", 1.0, t1b, "ka");
    CT(-1.0, n1b, "ia", t2, "ikca", 0.0, Fovb, "kc");
    CT(-1.0, kFov, "kc", n1b, "ia", 1.0, t2b, "ikca");
    CT(2.0, n1b, "ia", t2, "kica", 1.0, Fovb, "kc");
    CT(2.0, kFov, "kc", n1b, "ia", 1.0, t2b, "kica");
    CT(-1.0, t1, "ka", n1b, "ia", 0.0, Foob, "ki");
    CT(-1.0, kFoo, "ki", n1b, "ia", 1.0, t1b, "ka");
    CT(1.0, n1b, "ia", t1, "ic", 0.0, Fvvb, "ac");
    CT(1.0, n1b, "ia", kFvv, "ac", 1.0, t1b, "ic");
    CT(-2.0, t1, "ka", n1b, "ia", 0.0, X1b, "ki");
    CT(-2.0, kX1, "ki", n1b, "ia", 1.0, t1b, "ka");
    // the Fock-like intermediates
    CT(1.0, X2b, "ki", t1, "ic", 1.0, Fovb, "kc");
    CT(1.0, X2b, "ki", kFov, "kc", 1.0, t1b, "ic");
    CT(-1.0, Lvvb, "ac", ovvv, "kcad", 1.0, t1b, "kd");
    CT(2.0, ovvv, "kdac", Lvvb, "ac", 1.0, t1b, "kd");
    CT(-1.0, fov, "kc", Lvvb, "ac", 1.0, t1b, "ka");
    PM(1.0, Lvvb, "ac", 1.0, Fvvb, "ac");
    CT(-1.0, ovoo, "kcli", Loob, "ki", 1.0, t1b, "lc");
    CT(2.0, ovoo, "lcki", Loob, "ki", 1.0, t1b, "lc");
    PM(1.0, Loob, "ki", 1.0, X1b, "ki");
    PM(1.0, Loob, "ki", 1.0, Foob, "ki");
    CT(1.0, X1b, "ki", fov, "kc", 1.0, t1b, "ic");
    CT(-1.0, Lovov, "kcld", Fvvb, "ac", 1.0, taub, "klad");
    CT(1.0, Lovov, "kcld", Foob, "ki", 1.0, taub, "ilcd");
    CT(1.0, Lovov, "kcld", Fovb, "kc", 1.0, t1b, "ld");
    // tau = t2 + t1 t1, tau2 = t2 / 2 + t1 t1
    PM(1.0, taub, "ijab", 1.0, t2b, "ijab");
    PM(0.5, tau2b, "ijab", 1.0, t2b, "ijab");
    PM(1.0, tau2b, "ijab", 1.0, taub, "ijab");
    CT(1.0, taub, "ijab", t1, "jb", 1.0, t1b, "ia");
    CT(1.0, taub, "jiba", t1, "jb", 1.0, t1b, "ia");
    // z2 onto the symmetry of t2, plus g; l~ -> l (the denominators are symmetric under a <-> b, so the division comes last)
    PM(1.0, h->Lt, "ijab", 0.0, Sb, "ijab");
    PM(0.5, t2b, "ijab", 1.0, Sb, "ijab");
    PM(0.5, t2b, "jiba", 1.0, Sb, "ijab");
    PM(2.0 / 3.0, Sb, "ijab", 0.0, Rb, "ijab");
    PM(1.0 / 3.0, Sb, "ijba", 1.0, Rb, "ijab");
    PM(0.5, t1b, "ia", 0.0, n1b, "ia");
    PM(0.5, h->g1, "ia", 1.0, n1b, "ia");
    if ((rc = cc_div(h, 0, n1b, dst))) return rc;
    return cc_div(h, 1, Rb, dst + h->P.off[1]);
}

// gamma (n x n) of the current (t, l) into gamma_dev: DESIGN.md K21, "Lambda"
int lambda_rdm1(dmk_rccsd *h, double *gamma_dev) {
    dmk_ctx *ctx = h->ctx;
    const Engine &E = h->E;
    const double *t1 = h->T.x, *t2 = h->T.x + h->P.off[1], *l1 = h->L.x, *l2 = h->L.x + h->P.off[1];
    double *th = h->S, *doo = h->doo, *dvv = h->dvv, *dvo = h->dvo, *xt1 = h->xt1, *xt2 = h->xt2, *X = h->X1b;
    int rc;
    PM(2.0, t2, "ijab", 0.0, th, "ijab");
    PM(-1.0, t2, "ijba", 1.0, th, "ijab");
    CT(1.0, l2, "mnef", th, "inef", 0.0, xt1, "mi");
    CT(1.0, th, "mnef", l2, "mnaf", 0.0, xt2, "ea");
    CT(-1.0, l1, "ia", t1, "ja", 0.0, doo, "ij");
    PM(-1.0, xt1, "ij", 1.0, doo, "ij");
    CT(1.0, t1, "ia", l1, "ib", 0.0, dvv, "ab");
    PM(1.0, xt2, "ab", 1.0, dvv, "ab");
    PM(1.0, t1, "ia", 0.0, dvo, "ia");
    CT(1.0, t1, "ie", l1, "me", 0.0, X, "im");
    CT(-1.0, X, "im", t1, "ma", 1.0, dvo, "ia");
    CT(1.0, th, "imae", l1, "me", 1.0, dvo, "ia");
    CT(-1.0, xt1, "mi", t1, "ma", 1.0, dvo, "ia");
    CT(-1.0, t1, "ie", xt2, "ae", 1.0, dvo, "ia");
    FamScope fs(ctx, DMK_FAM_MISC);
    const int n = h->o + h->v;
    hipLaunchKernelGGL(cc_rdm1_kernel, dim3(grid_of((long long)n * n)), dim3(NT), 0, ctx->stream, h->o, h->v, doo, dvv, l1, dvo, gamma_dev);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

#undef LADDER
#undef CT
#undef PM

}  // namespace

// ---- what csrc/ccsd_t.hip (K22) reads of a handle (ccsd_view.h) -------------------------------------------------------------------
int dmk_rccsd_view(dmk_rccsd *h, RccsdView *out) {
    *out = RccsdView{h->ctx, h->o, h->v, h->have_amps, h->ovoo, h->ovov, h->ovvv, h->fov, h->eo, h->ev, h->T.x, h->T.x + h->P.off[1]};
    return DMK_OK;
}

int dmk_cc_perm(dmk_ctx *ctx, int o, int v, double alpha, const double *in, const char *si, double beta, double *out, const char *so) {
    Engine E;
    E.ctx = ctx; E.extents(o, v, o, v);
    return E.perm(alpha, in, si, beta, out, so);
}

extern "C" {

int dmk_cc_ladder_s4(dmk_ctx *ctx, int64_t m, int nvir, const double *vvvv_s4, int64_t ld, const double *tau, double alpha, double beta,
                     double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (m < 1 || nvir < 1 || nvir > 512 || !vvvv_s4 || !tau || !out)
        return dmk_fail(ctx, DMK_ERR_INVALID, "cc_ladder_s4: bad arguments (m >= 1, 1 <= nvir <= 512; block, tau and out)");
    if (ld < pair_of(nvir)) return dmk_fail(ctx, DMK_ERR_INVALID, "cc_ladder_s4: row pitch %lld below npair = %lld", (long long)ld, pair_of(nvir));
    return ladder_launch(ctx, Ladder{(long long)m, nvir, nvir, vvvv_s4, (long long)ld, tau, alpha, beta, out});
}

int dmk_cc_ladder_s4_ab(dmk_ctx *ctx, int64_t m, int nvir_a, int nvir_b, const double *vvVV_s4, int64_t ld, const double *tau, double alpha,
                        double beta, double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (m < 1 || nvir_a < 1 || nvir_a > 512 || nvir_b < 1 || nvir_b > 512 || !vvVV_s4 || !tau || !out)
        return dmk_fail(ctx, DMK_ERR_INVALID, "cc_ladder_s4_ab: bad arguments (m >= 1, 1 <= nvir_a, nvir_b <= 512; block, tau and out)");
    if (ld < pair_of(nvir_b))
        return dmk_fail(ctx, DMK_ERR_INVALID, "cc_ladder_s4_ab: row pitch %lld below npair_b = %lld", (long long)ld, pair_of(nvir_b));
    return ladder_launch(ctx, Ladder{(long long)m, nvir_a, nvir_b, vvVV_s4, (long long)ld, tau, alpha, beta, out});
}

int dmk_rccsd_plan(int nocc, int nvir, int diis_dim, int64_t *bytes_host) {
    if (!bytes_host || nocc < 1 || nvir < 1 || nvir > 512 || nocc > 512 || diis_dim < 0 || diis_dim > DIIS_MAX) return DMK_ERR_INVALID;
    dmk_rccsd h(nullptr, nocc, nvir, diis_dim);
    bytes_host[0] = (int64_t)h.carve(nullptr);
    bytes_host[1] = h.ws_bytes();
    return DMK_OK;
}

int dmk_rccsd_create(dmk_ctx *ctx, int nocc, int nvir, const double *fock_mo, const double *oooo, const double *ovoo, const double *ovov,
                     const double *oovv, const double *ovvo, const double *ovvv, const double *vvvv_s4, int64_t ld_vvvv, int diis_dim,
                     dmk_rccsd **out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (!out || nocc < 1 || nvir < 1 || nocc > 512 || nvir > 512 || !fock_mo || !oooo || !ovoo || !ovov || !oovv || !ovvo || !ovvv || !vvvv_s4)
        return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_create: bad arguments (1 <= nocc, nvir <= 512; Fock matrix and seven blocks)");
    if (diis_dim < 0 || diis_dim > DIIS_MAX) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_create: diis_dim %d outside [0, %d]", diis_dim, DIIS_MAX);
    if (ld_vvvv < pair_of(nvir)) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_create: pitch of the (vv|vv) block below npair");
    *out = nullptr;
    dmk_rccsd *h = new dmk_rccsd(ctx, nocc, nvir, diis_dim);
    h->oooo = oooo; h->ovoo = ovoo; h->ovov = ovov; h->oovv = oovv; h->ovvo = ovvo; h->ovvv = ovvv; h->vvvv = vvvv_s4; h->ld_vvvv = ld_vvvv;
    return cc_create(h, "rccsd_create", [&]() -> int {
        {
            FamScope fs(ctx, DMK_FAM_MISC);
            const int n = nocc + nvir;
            hipLaunchKernelGGL(cc_fock_split_kernel, dim3(grid_of((long long)n * n)), dim3(NT), 0, ctx->stream, nocc, nvir, fock_mo, h->foo, h->fvv,
                               h->fov, h->eo, h->ev);
            if (hipGetLastError() != hipSuccess) return dmk_fail(ctx, DMK_ERR_HIP, "rccsd_create: kernel launch failed");
        }
        // L_kcld = 2 (kc|ld) - (kd|lc), and the same in (k, l, c, d) order for the energy
        int rc;
        if ((rc = h->E.perm(2.0, ovov, "kcld", 0.0, h->Lovov, "kcld"))) return rc;
        if ((rc = h->E.perm(-1.0, ovov, "kdlc", 1.0, h->Lovov, "kcld"))) return rc;
        return h->E.perm(1.0, h->Lovov, "iajb", 0.0, h->Lt, "ijab");
    }, out);
}

int dmk_rccsd_free(dmk_rccsd *h) { return cc_free(h); }

int dmk_rccsd_init(dmk_rccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    h->kept = false;
    return h->synced([h] { return cc_init(h); });
}

int dmk_rccsd_set(dmk_rccsd *h, const double *t1, const double *t2) {
    if (!h) return DMK_ERR_INVALID;
    if (!t1 || !t2) return dmk_fail(h->ctx, DMK_ERR_INVALID, "rccsd_set: NULL amplitudes");
    h->kept = false;
    const double *src[2] = {t1, t2};
    return h->set(src, h->T.x, &h->have_amps);
}

int dmk_rccsd_energy(dmk_rccsd *h, double *e_dev) {
    if (!h) return DMK_ERR_INVALID;
    if (!e_dev || !h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_energy: no amplitudes yet (init or set first), or a NULL result");
    return h->synced([=] { return cc_energy(h, h->T.x, e_dev); });
}

int dmk_rccsd_update(dmk_rccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    if (!h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_update: no amplitudes yet (init or set first)");
    h->kept = false;
    return h->step(h->T, [h](const double *from, double *to) { return cc_update(h, from, to); });
}

int dmk_rccsd_run(dmk_rccsd *h, int max_iter, double tol_e, double tol_normt, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!result_host || max_iter < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_run: bad arguments");
    int rc;
    if (!h->have_amps && (rc = cc_init(h))) return rc;
    h->kept = false;
    // without a ring the step is kept in n1 / tau2, free between updates
    const Iterate s{&h->T, {h->n1, h->tau2}, true, "rccsd_run"};
    return cc_iterate(h, s, max_iter, tol_e, tol_normt, [h](const double *from, double *to) { return cc_update(h, from, to); },
                      [h](const double *amp, double *e_dev) { return cc_energy(h, amp, e_dev); }, result_host);
}

int dmk_rccsd_lambda_plan(int nocc, int nvir, int diis_dim, int64_t *bytes_host) {
    if (!bytes_host || nocc < 1 || nvir < 1 || nvir > 512 || nocc > 512 || diis_dim < 0 || diis_dim > DIIS_MAX) return DMK_ERR_INVALID;
    dmk_rccsd h(nullptr, nocc, nvir, diis_dim);
    bytes_host[0] = (int64_t)h.lambda_carve(nullptr);
    return DMK_OK;
}

int dmk_rccsd_lambda_init(dmk_rccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!h->have_amps) return dmk_fail(ctx, DMK_ERR_STATE, "rccsd_lambda_init: no amplitudes yet (run, init or set first)");
    int rc;
    if ((rc = lambda_alloc(h))) return rc;
    DMK_HIP(ctx, hipMemcpyAsync(h->L.x, h->T.x, (size_t)h->P.nx * 8, hipMemcpyDeviceToDevice, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    h->have_l = true;
    return DMK_OK;
}

int dmk_rccsd_lambda_set(dmk_rccsd *h, const double *l1, const double *l2) {
    if (!h) return DMK_ERR_INVALID;
    if (!l1 || !l2) return dmk_fail(h->ctx, DMK_ERR_INVALID, "rccsd_lambda_set: NULL amplitudes");
    int rc;
    if ((rc = lambda_alloc(h))) return rc;
    const double *src[2] = {l1, l2};
    return h->set(src, h->L.x, &h->have_l);
}

int dmk_rccsd_lambda_update(dmk_rccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    if (!h->have_amps || !h->have_l)
        return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_lambda_update: needs amplitudes and Lambda amplitudes (lambda_init or lambda_set first)");
    int rc;
    if ((rc = lambda_prepare(h))) return rc;
    return h->step(h->L, [h](const double *from, double *to) { return lambda_update(h, from, to); });
}

int dmk_rccsd_lambda_run(dmk_rccsd *h, int max_iter, double tol_normt, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!result_host || max_iter < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_lambda_run: bad arguments");
    if (!h->have_amps) return dmk_fail(ctx, DMK_ERR_STATE, "rccsd_lambda_run: no amplitudes yet (run, init or set first)");
    int rc;
    if (!h->have_l && (rc = dmk_rccsd_lambda_init(h))) return rc;
    if ((rc = lambda_prepare(h))) return rc;
    // without a ring the step is kept in the adjoints of n1 / tau2, free between sweeps
    const Iterate s{&h->L, {h->n1b, h->tau2}, false, "rccsd_lambda_run"};
    double res[5];
    if ((rc = cc_iterate(h, s, max_iter, 1.0, tol_normt, [h](const double *from, double *to) { return lambda_update(h, from, to); },
                         [](const double *, double *) { return (int)DMK_OK; }, res)))
        return rc;
    result_host[0] = res[1]; result_host[1] = res[2]; result_host[2] = res[3];
    return DMK_OK;
}

int dmk_rccsd_rdm1(dmk_rccsd *h, double *gamma_dev) {
    if (!h) return DMK_ERR_INVALID;
    if (!gamma_dev) return dmk_fail(h->ctx, DMK_ERR_INVALID, "rccsd_rdm1: NULL result");
    if (!h->have_amps || !h->have_l) return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_rdm1: needs amplitudes and Lambda amplitudes");
    return h->synced([=] { return lambda_rdm1(h, gamma_dev); });
}

int dmk_rccsd_residual(dmk_rccsd *h, double *r1_dev, double *r2_dev) {
    if (!h) return DMK_ERR_INVALID;
    if (!r1_dev || !r2_dev) return dmk_fail(h->ctx, DMK_ERR_INVALID, "rccsd_residual: NULL result");
    if (!h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_residual: no amplitudes yet (init or set first)");
    return h->synced([=]() -> int {
        const int rc = cc_residual(h);
        if (rc) return rc;
        const double *src[2] = {h->n1, h->R};
        double *dst[2] = {r1_dev, r2_dev};
        return h->parts_out(src, dst);
    });
}

int dmk_rccsd_lagrangian(dmk_rccsd *h, const double *l1, const double *l2, double *out_dev) {
    if (!h) return DMK_ERR_INVALID;
    if (!l1 || !l2 || !out_dev) return dmk_fail(h->ctx, DMK_ERR_INVALID, "rccsd_lagrangian: NULL argument");
    if (!h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "rccsd_lagrangian: no amplitudes yet (init or set first)");
    return h->synced([=]() -> int {
        int rc;
        if ((rc = cc_residual(h))) return rc;
        // l~2 = 2 l2 - l2^T(ab) into S, free after cc_rod; the energy overwrites tau alone
        if ((rc = h->E.perm(2.0, l2, "ijab", 0.0, h->S, "ijab"))) return rc;
        if ((rc = h->E.perm(-1.0, l2, "ijba", 1.0, h->S, "ijab"))) return rc;
        if ((rc = cc_energy(h, h->T.x, out_dev))) return rc;
        if ((rc = cc_dot(h, h->P.cnt[0], l1, h->n1, 2.0, 1, out_dev))) return rc;
        return cc_dot(h, h->P.cnt[1], h->S, h->R, 1.0, 1, out_dev);
    });
}

int dmk_rccsd_get(dmk_rccsd *h, int what, double *out) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!out || what < DMK_RCCSD_T1 || what > DMK_RCCSD_L2) return dmk_fail(ctx, DMK_ERR_INVALID, "rccsd_get: bad arguments");
    if (what == DMK_RCCSD_L1 || what == DMK_RCCSD_L2) {
        if (!h->have_l) return dmk_fail(ctx, DMK_ERR_STATE, "rccsd_get: no Lambda amplitudes yet (lambda_init, lambda_set or lambda_run first)");
        return h->get(h->L.x, what - DMK_RCCSD_L1, out);
    }
    if (!h->have_amps) return dmk_fail(ctx, DMK_ERR_STATE, "rccsd_get: no amplitudes yet (init or set first)");
    return h->get(h->T.x, what, out);          // DMK_RCCSD_T1, _T2, _EMP2 = 0, 1, 2: the parts, then E(MP2)
}

}  // extern "C"
