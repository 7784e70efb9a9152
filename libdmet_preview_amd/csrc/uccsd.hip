// K24 -- unrestricted CCSD on the device: the T1 / T2 amplitude equations with general (non-canonical) Fock matrices and the correlation
// energy over two sets of orbitals, on the MO blocks that dmk_ao2mo_s4 writes from the three ERI blocks of the device UHF.  Replaces
// UICCSD(mf).kernel() behind the reference's CCSD.run (solver/cc.py:227, :912).  The equations are stated in DESIGN.md K24: the
// spin-orbital equations of Stanton, Gauss, Watts, Bartlett (1991) resolved into spin blocks over chemists' integrals.
//
// Everything that computes is in cc_engine.h, shared with ccsd.hip (K21): the three O(o^2 v^4) terms are cc_ladder_kernel on the packed
// (vv|vv), (VV|VV) and (vv|VV) blocks -- the only reader of those blocks --, every other term is a CT / PM line over the contraction
// engine, whose upper-case letters run over the beta extents.  The iteration is cc_iterate.  Amplitudes: ONE vector of five parts
// t1a | t1b | t2aa | t2ab | t2bb, each padded with zeros to a multiple of 32 doubles; t2aa and t2bb are stored in full.  The handle is
// a Core of cc_engine.h, its layout and ring the Parts and Ring that ccsd.hip's T and Lambda iterations use.
#include "devres.h"
#include "cc_engine.h"

struct dmk_uccsd : Core {
    int oa, va, ob, vb;
    dmk_uccsd_ints I{};
    // the intermediates of uc_rod, by the names DESIGN.md K24 gives them
    double *X2aa, *X2ab, *X2bb, *tauaa, *tauab, *taubb, *tataa, *tatab, *tatbb, *Fvva, *Fvvb, *Fooa, *Foob, *Fova, *Fovb, *Wooaa,
           *Wooab, *Woobb, *W_aaaa, *W_abab, *W_abba, *W_baab, *W_baba, *W_bbbb, *n1a, *n1b, *Gvva, *Gvvb, *Gooa, *Goob, *Q_aaaa,
           *Q_abab, *Q_abba, *Q_baab, *Q_baba, *Q_bbbb, *Y_aaaa, *Y_abab, *Y_baab, *Y_bbbb, *Raa, *Rab, *Rbb;
    // Fock pieces (off-diagonal f_oo / f_vv, f_ov, the diagonals), <ij||ab> as the energy reads it
    double *fooa, *foob, *fvva, *fvvb, *fova, *fovb, *eoa, *eob, *eva, *evb, *Gaa, *Gab, *Gbb;

    // the vector: t1a | t1b | t2aa | t2ab | t2bb, every part padded with zeros to a multiple of 32 doubles
    dmk_uccsd(dmk_ctx *c, int nocc_a, int nvir_a, int nocc_b, int nvir_b, int diis_dim)
        : Core(c, nocc_a, nvir_a, nocc_b, nvir_b, diis_dim), oa(nocc_a), va(nvir_a), ob(nocc_b), vb(nvir_b) {
        P = Parts({ext("ov"), ext("OV"), ext("oovv"), ext("oOvV"), ext("OOVV")}, true);
    }
    // what the carve lays out; with a null base: the bytes
    size_t carve(void *base) {
        Carver c(base);
        T.carve(c, P.nx, diis);
        const Slot tab[] = {
            {&X2aa, "oovv"}, {&X2ab, "oOvV"}, {&X2bb, "OOVV"}, {&tauaa, "oovv"}, {&tauab, "oOvV"}, {&taubb, "OOVV"},
            {&tataa, "oovv"}, {&tatab, "oOvV"}, {&tatbb, "OOVV"}, {&Fvva, "vv"}, {&Fvvb, "VV"}, {&Fooa, "oo"},
            {&Foob, "OO"}, {&Fova, "ov"}, {&Fovb, "OV"}, {&Wooaa, "oooo"}, {&Wooab, "oOoO"}, {&Woobb, "OOOO"},
            {&W_aaaa, "ovvo"}, {&W_abab, "oVvO"}, {&W_abba, "oVVo"}, {&W_baab, "OvvO"}, {&W_baba, "OvVo"},
            {&W_bbbb, "OVVO"}, {&n1a, "ov"}, {&n1b, "OV"}, {&Gvva, "vv"}, {&Gvvb, "VV"}, {&Gooa, "oo"}, {&Goob, "OO"},
            {&Q_aaaa, "ovoo"}, {&Q_abab, "oVoO"}, {&Q_abba, "oVOo"}, {&Q_baab, "OvoO"}, {&Q_baba, "OvOo"},
            {&Q_bbbb, "OVOO"}, {&Y_aaaa, "ovoo"}, {&Y_abab, "oVoO"}, {&Y_baab, "OvoO"}, {&Y_bbbb, "OVOO"}, {&Raa, "oovv"},
            {&Rab, "oOvV"}, {&Rbb, "OOVV"},
            {&fooa, "oo"}, {&foob, "OO"}, {&fvva, "vv"}, {&fvvb, "VV"}, {&fova, "ov"}, {&fovb, "OV"},
            {&eoa, "o"}, {&eob, "O"}, {&eva, "v"}, {&evb, "V"}, {&Gaa, "oovv"}, {&Gab, "oOvV"}, {&Gbb, "OOVV"}};
        take(c, tab);
        part = c.take(2048); rec = c.take(16);
        return (size_t)(c.p - static_cast<char *>(base));
    }
};

namespace {

bool extents_ok(int oa, int va, int ob, int vb) {
    for (int e : {oa, va, ob, vb})
        if (e < 1 || e > 512) return false;
    return true;
}

// out[i][j][a][b] = c2 t2[i][j][a][b] + c1 t1[i][a] t1'[j][b] of the vector `src`; si, sj: the spins (0 alpha, 1 beta) of (i, a), (j, b)
int uc_tau(dmk_uccsd *h, double c2, double c1, int si, int sj, const double *src, double *out) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    const int oi = si ? h->ob : h->oa, vi = si ? h->vb : h->va, oj = sj ? h->ob : h->oa, vj = sj ? h->vb : h->va;
    hipLaunchKernelGGL(cc_tau_kernel, dim3(grid_of((long long)oi * oj * vi * vj)), dim3(NT), 0, ctx->stream, oi, oj, vi, vj, c2, c1,
                       src + h->P.off[si], src + h->P.off[sj], src + h->P.off[2 + si + sj], out);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// part p of the vector dst = part p of the right-hand side / its Fock-diagonal denominators
int uc_div(dmk_uccsd *h, int p, const double *in, double *dst) {
    dmk_ctx *ctx = h->ctx;
    FamScope fs(ctx, DMK_FAM_MISC);
    const Denoms A{h->oa, h->oa, h->va, h->va, h->eoa, h->eoa, h->eva, h->eva}, B{h->ob, h->ob, h->vb, h->vb, h->eob, h->eob, h->evb, h->evb},
        AB{h->oa, h->ob, h->va, h->vb, h->eoa, h->eob, h->eva, h->evb};
    const Denoms &D = (p == 0 || p == 2) ? A : (p == 1 || p == 4) ? B : AB;
    hipLaunchKernelGGL(cc_div_kernel, dim3(grid_of(h->P.cnt[p])), dim3(NT), 0, ctx->stream, D, p >= 2, in, dst + h->P.off[p]);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

#define CT(alpha, A, sa, B, sb, beta, C, sc) do { if ((rc = E.contract(alpha, A, sa, B, sb, beta, C, sc))) return rc; } while (0)
#define PM(alpha, in, si, beta, out, so) do { if ((rc = E.perm(alpha, in, si, beta, out, so))) return rc; } while (0)
#define TAU(c2, c1, si, sj, out) do { if ((rc = uc_tau(h, c2, c1, si, sj, src, out))) return rc; } while (0)
#define LADDER(m, v1, v2, W, ld, in, dst) do { if ((rc = ladder_launch(h->ctx, Ladder{(long long)(m), v1, v2, W, ld, in, 1.0, 1.0, dst}))) return rc; } while (0)

// tau_ij^ab = t_ij^ab + t_i^a t_j^b - t_i^b t_j^a of the vector `src` into tauaa / tauab / taubb (X2aa / X2bb are overwritten)
int uc_tau_of(dmk_uccsd *h, const double *src) {
    const Engine &E = h->E;
    int rc;
    TAU(0.5, 1.0, 0, 0, h->X2aa);
    TAU(0.5, 1.0, 1, 1, h->X2bb);
    PM(1.0, h->X2aa, "ijab", 0.0, h->tauaa, "ijab");
    PM(-1.0, h->X2aa, "ijba", 1.0, h->tauaa, "ijab");
    PM(1.0, h->X2bb, "IJAB", 0.0, h->taubb, "IJAB");
    PM(-1.0, h->X2bb, "IJBA", 1.0, h->taubb, "IJAB");
    TAU(1.0, 1.0, 0, 1, h->tauab);
    return DMK_OK;
}

// *e_dev = f_ia t_ia (both spins) + 1/4 <ij||ab> tau_ij^ab (aa, bb) + (ia|JB) tau_iJ^aB of the amplitude vector `amp`
int uc_energy(dmk_uccsd *h, const double *amp, double *e_dev) {
    int rc;
    if ((rc = uc_tau_of(h, amp))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[0], h->fova, amp + h->P.off[0], 1.0, 0, e_dev))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[1], h->fovb, amp + h->P.off[1], 1.0, 1, e_dev))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[2], h->Gaa, h->tauaa, 0.25, 1, e_dev))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[3], h->Gab, h->tauab, 1.0, 1, e_dev))) return rc;
    return cc_dot(h, h->P.cnt[4], h->Gbb, h->taubb, 0.25, 1, e_dev);
}

// the right-hand sides of the amplitude equations (line by line) at the vector `src`, before the division: of t1 into
// n1a / n1b, of t2 into Raa / Rab / Rbb
int uc_rod(dmk_uccsd *h, const double *src) {
    const Engine &E = h->E;
    const dmk_uccsd_ints &I = h->I;
    const int oa = h->oa, ob = h->ob, va = h->va, vb = h->vb;
    const double *t1a = src + h->P.off[0], *t1b = src + h->P.off[1], *t2aa = src + h->P.off[2], *t2ab = src + h->P.off[3], *t2bb = src + h->P.off[4];
    const double *oooo = I.oooo, *ovoo = I.ovoo, *ovov = I.ovov, *oovv = I.oovv, *ovvv = I.ovvv;
    const double *OOOO = I.OOOO, *OVOO = I.OVOO, *OVOV = I.OVOV, *OOVV = I.OOVV, *OVVV = I.OVVV;
    const double *ooOO = I.ooOO, *ovOO = I.ovOO, *ovOV = I.ovOV, *ooVV = I.ooVV, *ovVV = I.ovVV, *OVoo = I.OVoo, *OOvv = I.OOvv, *OVvv = I.OVvv;
    const double *fooa = h->fooa, *foob = h->foob, *fvva = h->fvva, *fvvb = h->fvvb, *fova = h->fova, *fovb = h->fovb;
    double *X2aa = h->X2aa, *X2ab = h->X2ab, *X2bb = h->X2bb, *tauaa = h->tauaa, *tauab = h->tauab, *taubb = h->taubb, *tataa =
           h->tataa, *tatab = h->tatab, *tatbb = h->tatbb, *Fvva = h->Fvva, *Fvvb = h->Fvvb, *Fooa = h->Fooa, *Foob = h->Foob,
           *Fova = h->Fova, *Fovb = h->Fovb, *Wooaa = h->Wooaa, *Wooab = h->Wooab, *Woobb = h->Woobb, *W_aaaa = h->W_aaaa, *W_abab
           = h->W_abab, *W_abba = h->W_abba, *W_baab = h->W_baab, *W_baba = h->W_baba, *W_bbbb = h->W_bbbb, *n1a = h->n1a, *n1b =
           h->n1b, *Gvva = h->Gvva, *Gvvb = h->Gvvb, *Gooa = h->Gooa, *Goob = h->Goob, *Q_aaaa = h->Q_aaaa, *Q_abab = h->Q_abab,
           *Q_abba = h->Q_abba, *Q_baab = h->Q_baab, *Q_baba = h->Q_baba, *Q_bbbb = h->Q_bbbb, *Y_aaaa = h->Y_aaaa, *Y_abab =
           h->Y_abab, *Y_baab = h->Y_baab, *Y_bbbb = h->Y_bbbb, *Raa = h->Raa, *Rab = h->Rab, *Rbb = h->Rbb;
    int rc;
    // tau = t2 + t1 t1 - (a <-> b), tat = t2 + (t1 t1 - (a <-> b)) / 2, X2 = t2 / 2 + t1 t1
    TAU(0.5, 1.0, 0, 0, X2aa);
    TAU(0.5, 1.0, 0, 1, X2ab);
    TAU(0.5, 1.0, 1, 1, X2bb);
    PM(1.0, X2aa, "ijab", 0.0, tauaa, "ijab");
    PM(-1.0, X2aa, "ijba", 1.0, tauaa, "ijab");
    PM(1.0, X2bb, "IJAB", 0.0, taubb, "IJAB");
    PM(-1.0, X2bb, "IJBA", 1.0, taubb, "IJAB");
    TAU(1.0, 1.0, 0, 1, tauab);
    PM(0.5, t2aa, "ijab", 0.0, tataa, "ijab");
    PM(0.5, tauaa, "ijab", 1.0, tataa, "ijab");
    PM(0.5, t2bb, "IJAB", 0.0, tatbb, "IJAB");
    PM(0.5, taubb, "IJAB", 1.0, tatbb, "IJAB");
    TAU(1.0, 0.5, 0, 1, tatab);
    // F_ae
    PM(1.0, fvva, "ac", 0.0, Fvva, "ac");
    CT(-0.5, fova, "kc", t1a, "ka", 1.0, Fvva, "ac");
    CT(1.0, t1a, "kd", ovvv, "kdac", 1.0, Fvva, "ac");
    CT(-1.0, t1a, "kd", ovvv, "kcad", 1.0, Fvva, "ac");
    CT(1.0, t1b, "KD", OVvv, "KDac", 1.0, Fvva, "ac");
    CT(-0.5, tataa, "klad", ovov, "kcld", 1.0, Fvva, "ac");
    CT(0.5, tataa, "klad", ovov, "kdlc", 1.0, Fvva, "ac");
    CT(-1.0, tatab, "kLaD", ovOV, "kcLD", 1.0, Fvva, "ac");
    PM(1.0, fvvb, "AC", 0.0, Fvvb, "AC");
    CT(-0.5, fovb, "KC", t1b, "KA", 1.0, Fvvb, "AC");
    CT(1.0, t1a, "kd", ovVV, "kdAC", 1.0, Fvvb, "AC");
    CT(1.0, t1b, "KD", OVVV, "KDAC", 1.0, Fvvb, "AC");
    CT(-1.0, t1b, "KD", OVVV, "KCAD", 1.0, Fvvb, "AC");
    CT(-1.0, tatab, "kLdA", ovOV, "kdLC", 1.0, Fvvb, "AC");
    CT(-0.5, tatbb, "KLAD", OVOV, "KCLD", 1.0, Fvvb, "AC");
    CT(0.5, tatbb, "KLAD", OVOV, "KDLC", 1.0, Fvvb, "AC");
    // F_mi
    PM(1.0, fooa, "ki", 0.0, Fooa, "ki");
    CT(0.5, t1a, "ic", fova, "kc", 1.0, Fooa, "ki");
    CT(1.0, t1a, "lc", ovoo, "lcki", 1.0, Fooa, "ki");
    CT(-1.0, t1a, "lc", ovoo, "kcli", 1.0, Fooa, "ki");
    CT(1.0, t1b, "LC", OVoo, "LCki", 1.0, Fooa, "ki");
    CT(0.5, tataa, "ilcd", ovov, "kcld", 1.0, Fooa, "ki");
    CT(-0.5, tataa, "ilcd", ovov, "kdlc", 1.0, Fooa, "ki");
    CT(1.0, tatab, "iLcD", ovOV, "kcLD", 1.0, Fooa, "ki");
    PM(1.0, foob, "KI", 0.0, Foob, "KI");
    CT(0.5, t1b, "IC", fovb, "KC", 1.0, Foob, "KI");
    CT(1.0, t1a, "lc", ovOO, "lcKI", 1.0, Foob, "KI");
    CT(1.0, t1b, "LC", OVOO, "LCKI", 1.0, Foob, "KI");
    CT(-1.0, t1b, "LC", OVOO, "KCLI", 1.0, Foob, "KI");
    CT(1.0, tatab, "lIcD", ovOV, "lcKD", 1.0, Foob, "KI");
    CT(0.5, tatbb, "ILCD", OVOV, "KCLD", 1.0, Foob, "KI");
    CT(-0.5, tatbb, "ILCD", OVOV, "KDLC", 1.0, Foob, "KI");
    // F_me
    PM(1.0, fova, "kc", 0.0, Fova, "kc");
    CT(1.0, t1a, "ld", ovov, "kcld", 1.0, Fova, "kc");
    CT(-1.0, t1a, "ld", ovov, "kdlc", 1.0, Fova, "kc");
    CT(1.0, t1b, "LD", ovOV, "kcLD", 1.0, Fova, "kc");
    PM(1.0, fovb, "KC", 0.0, Fovb, "KC");
    CT(1.0, t1a, "ld", ovOV, "ldKC", 1.0, Fovb, "KC");
    CT(1.0, t1b, "LD", OVOV, "KCLD", 1.0, Fovb, "KC");
    CT(-1.0, t1b, "LD", OVOV, "KDLC", 1.0, Fovb, "KC");
    // W_mnij, with the whole tau tau <mn||ef> term (one half of it is W_abef's in the paper)
    PM(1.0, oooo, "kilj", 0.0, Wooaa, "klij");
    PM(-1.0, oooo, "kjli", 1.0, Wooaa, "klij");
    CT(1.0, t1a, "jc", ovoo, "lcki", 1.0, Wooaa, "klij");
    CT(-1.0, t1a, "jc", ovoo, "kcli", 1.0, Wooaa, "klij");
    CT(-1.0, t1a, "ic", ovoo, "lckj", 1.0, Wooaa, "klij");
    CT(1.0, t1a, "ic", ovoo, "kclj", 1.0, Wooaa, "klij");
    CT(0.5, tauaa, "ijcd", ovov, "kcld", 1.0, Wooaa, "klij");
    CT(-0.5, tauaa, "ijcd", ovov, "kdlc", 1.0, Wooaa, "klij");
    PM(1.0, ooOO, "kiLJ", 0.0, Wooab, "kLiJ");
    CT(1.0, t1b, "JC", OVoo, "LCki", 1.0, Wooab, "kLiJ");
    CT(1.0, t1a, "ic", ovOO, "kcLJ", 1.0, Wooab, "kLiJ");
    CT(1.0, tauab, "iJcD", ovOV, "kcLD", 1.0, Wooab, "kLiJ");
    PM(1.0, OOOO, "KILJ", 0.0, Woobb, "KLIJ");
    PM(-1.0, OOOO, "KJLI", 1.0, Woobb, "KLIJ");
    CT(1.0, t1b, "JC", OVOO, "LCKI", 1.0, Woobb, "KLIJ");
    CT(-1.0, t1b, "JC", OVOO, "KCLI", 1.0, Woobb, "KLIJ");
    CT(-1.0, t1b, "IC", OVOO, "LCKJ", 1.0, Woobb, "KLIJ");
    CT(1.0, t1b, "IC", OVOO, "KCLJ", 1.0, Woobb, "KLIJ");
    CT(0.5, taubb, "IJCD", OVOV, "KCLD", 1.0, Woobb, "KLIJ");
    CT(-0.5, taubb, "IJCD", OVOV, "KDLC", 1.0, Woobb, "KLIJ");
    // W_mbej, six spin patterns
    PM(-1.0, oovv, "kjbc", 0.0, W_aaaa, "kbcj");
    PM(1.0, ovov, "kcjb", 1.0, W_aaaa, "kbcj");
    CT(1.0, t1a, "jd", ovvv, "kcbd", 1.0, W_aaaa, "kbcj");
    CT(-1.0, t1a, "jd", ovvv, "kdbc", 1.0, W_aaaa, "kbcj");
    CT(1.0, t1a, "lb", ovoo, "lckj", 1.0, W_aaaa, "kbcj");
    CT(-1.0, t1a, "lb", ovoo, "kclj", 1.0, W_aaaa, "kbcj");
    CT(-1.0, X2aa, "jldb", ovov, "kcld", 1.0, W_aaaa, "kbcj");
    CT(1.0, X2aa, "jldb", ovov, "kdlc", 1.0, W_aaaa, "kbcj");
    CT(0.5, t2ab, "jLbD", ovOV, "kcLD", 1.0, W_aaaa, "kbcj");
    PM(1.0, ovOV, "kcJB", 0.0, W_abab, "kBcJ");
    CT(1.0, t1b, "JD", ovVV, "kcBD", 1.0, W_abab, "kBcJ");
    CT(-1.0, t1b, "LB", ovOO, "kcLJ", 1.0, W_abab, "kBcJ");
    CT(0.5, t2ab, "lJdB", ovov, "kcld", 1.0, W_abab, "kBcJ");
    CT(-0.5, t2ab, "lJdB", ovov, "kdlc", 1.0, W_abab, "kBcJ");
    CT(-1.0, X2bb, "JLDB", ovOV, "kcLD", 1.0, W_abab, "kBcJ");
    PM(-1.0, ooVV, "kjBC", 0.0, W_abba, "kBCj");
    CT(-1.0, t1a, "jd", ovVV, "kdBC", 1.0, W_abba, "kBCj");
    CT(1.0, t1b, "LB", OVoo, "LCkj", 1.0, W_abba, "kBCj");
    CT(1.0, X2ab, "jLdB", ovOV, "kdLC", 1.0, W_abba, "kBCj");
    PM(-1.0, OOvv, "KJbc", 0.0, W_baab, "KbcJ");
    CT(-1.0, t1b, "JD", OVvv, "KDbc", 1.0, W_baab, "KbcJ");
    CT(1.0, t1a, "lb", ovOO, "lcKJ", 1.0, W_baab, "KbcJ");
    CT(1.0, X2ab, "lJbD", ovOV, "lcKD", 1.0, W_baab, "KbcJ");
    PM(1.0, ovOV, "jbKC", 0.0, W_baba, "KbCj");
    CT(1.0, t1a, "jd", OVvv, "KCbd", 1.0, W_baba, "KbCj");
    CT(-1.0, t1a, "lb", OVoo, "KClj", 1.0, W_baba, "KbCj");
    CT(-1.0, X2aa, "jldb", ovOV, "ldKC", 1.0, W_baba, "KbCj");
    CT(0.5, t2ab, "jLbD", OVOV, "KCLD", 1.0, W_baba, "KbCj");
    CT(-0.5, t2ab, "jLbD", OVOV, "KDLC", 1.0, W_baba, "KbCj");
    PM(-1.0, OOVV, "KJBC", 0.0, W_bbbb, "KBCJ");
    PM(1.0, OVOV, "KCJB", 1.0, W_bbbb, "KBCJ");
    CT(1.0, t1b, "JD", OVVV, "KCBD", 1.0, W_bbbb, "KBCJ");
    CT(-1.0, t1b, "JD", OVVV, "KDBC", 1.0, W_bbbb, "KBCJ");
    CT(1.0, t1b, "LB", OVOO, "LCKJ", 1.0, W_bbbb, "KBCJ");
    CT(-1.0, t1b, "LB", OVOO, "KCLJ", 1.0, W_bbbb, "KBCJ");
    CT(0.5, t2ab, "lJdB", ovOV, "ldKC", 1.0, W_bbbb, "KBCJ");
    CT(-1.0, X2bb, "JLDB", OVOV, "KCLD", 1.0, W_bbbb, "KBCJ");
    CT(1.0, X2bb, "JLDB", OVOV, "KDLC", 1.0, W_bbbb, "KBCJ");
    // T1
    PM(1.0, fova, "ia", 0.0, n1a, "ia");
    CT(1.0, t1a, "ic", Fvva, "ac", 1.0, n1a, "ia");
    CT(-1.0, t1a, "ka", Fooa, "ki", 1.0, n1a, "ia");
    CT(1.0, t2aa, "ikac", Fova, "kc", 1.0, n1a, "ia");
    CT(1.0, t2ab, "iKaC", Fovb, "KC", 1.0, n1a, "ia");
    CT(-1.0, t1a, "ld", oovv, "liad", 1.0, n1a, "ia");
    CT(1.0, t1a, "ld", ovov, "ldia", 1.0, n1a, "ia");
    CT(1.0, t1b, "LD", ovOV, "iaLD", 1.0, n1a, "ia");
    CT(-0.5, t2aa, "ikcd", ovvv, "kcad", 1.0, n1a, "ia");
    CT(0.5, t2aa, "ikcd", ovvv, "kdac", 1.0, n1a, "ia");
    CT(1.0, t2ab, "iKcD", OVvv, "KDac", 1.0, n1a, "ia");
    CT(0.5, t2aa, "klac", ovoo, "kcli", 1.0, n1a, "ia");
    CT(-0.5, t2aa, "klac", ovoo, "lcki", 1.0, n1a, "ia");
    CT(-1.0, t2ab, "kLaC", OVoo, "LCki", 1.0, n1a, "ia");
    PM(1.0, fovb, "IA", 0.0, n1b, "IA");
    CT(1.0, t1b, "IC", Fvvb, "AC", 1.0, n1b, "IA");
    CT(-1.0, t1b, "KA", Foob, "KI", 1.0, n1b, "IA");
    CT(1.0, t2ab, "kIcA", Fova, "kc", 1.0, n1b, "IA");
    CT(1.0, t2bb, "IKAC", Fovb, "KC", 1.0, n1b, "IA");
    CT(1.0, t1a, "ld", ovOV, "ldIA", 1.0, n1b, "IA");
    CT(-1.0, t1b, "LD", OOVV, "LIAD", 1.0, n1b, "IA");
    CT(1.0, t1b, "LD", OVOV, "LDIA", 1.0, n1b, "IA");
    CT(1.0, t2ab, "kIcD", ovVV, "kcAD", 1.0, n1b, "IA");
    CT(-0.5, t2bb, "IKCD", OVVV, "KCAD", 1.0, n1b, "IA");
    CT(0.5, t2bb, "IKCD", OVVV, "KDAC", 1.0, n1b, "IA");
    CT(-1.0, t2ab, "kLcA", ovOO, "kcLI", 1.0, n1b, "IA");
    CT(0.5, t2bb, "KLAC", OVOO, "KCLI", 1.0, n1b, "IA");
    CT(-0.5, t2bb, "KLAC", OVOO, "LCKI", 1.0, n1b, "IA");
    // F_be - t F_me / 2, F_mj + t F_me / 2
    PM(1.0, Fvva, "bc", 0.0, Gvva, "bc");
    CT(-0.5, t1a, "kb", Fova, "kc", 1.0, Gvva, "bc");
    PM(1.0, Fvvb, "BC", 0.0, Gvvb, "BC");
    CT(-0.5, t1b, "KB", Fovb, "KC", 1.0, Gvvb, "BC");
    PM(1.0, Fooa, "kj", 0.0, Gooa, "kj");
    CT(0.5, t1a, "jc", Fova, "kc", 1.0, Gooa, "kj");
    PM(1.0, Foob, "KJ", 0.0, Goob, "KJ");
    CT(0.5, t1b, "JC", Fovb, "KC", 1.0, Goob, "KJ");
    // Q_mbji = t_i^e <mb||je>
    CT(1.0, t1a, "ic", oovv, "kjbc", 0.0, Q_aaaa, "kbji");
    CT(-1.0, t1a, "ic", ovov, "kcjb", 1.0, Q_aaaa, "kbji");
    CT(1.0, t1b, "IC", ooVV, "kjBC", 0.0, Q_abab, "kBjI");
    CT(-1.0, t1a, "ic", ovOV, "kcJB", 0.0, Q_abba, "kBJi");
    CT(-1.0, t1b, "IC", ovOV, "jbKC", 0.0, Q_baab, "KbjI");
    CT(1.0, t1a, "ic", OOvv, "KJbc", 0.0, Q_baba, "KbJi");
    CT(1.0, t1b, "IC", OOVV, "KJBC", 0.0, Q_bbbb, "KBJI");
    CT(-1.0, t1b, "IC", OVOV, "KCJB", 1.0, Q_bbbb, "KBJI");
    // Y_mbij = tau_ij^ef <mb||ef> / 2: the t1 dressing of W_abef
    CT(0.5, tauaa, "ijcd", ovvv, "kcbd", 0.0, Y_aaaa, "kbij");
    CT(-0.5, tauaa, "ijcd", ovvv, "kdbc", 1.0, Y_aaaa, "kbij");
    CT(1.0, tauab, "iJcD", ovVV, "kcBD", 0.0, Y_abab, "kBiJ");
    CT(-1.0, tauab, "iJcD", OVvv, "KDbc", 0.0, Y_baab, "KbiJ");
    CT(0.5, taubb, "IJCD", OVVV, "KCBD", 0.0, Y_bbbb, "KBIJ");
    CT(-0.5, taubb, "IJCD", OVVV, "KDBC", 1.0, Y_bbbb, "KBIJ");
    // T2, alpha-alpha
    PM(1.0, ovov, "iajb", 0.0, Raa, "ijab");
    PM(-1.0, ovov, "ibja", 1.0, Raa, "ijab");
    CT(1.0, t2aa, "ijac", Gvva, "bc", 1.0, Raa, "ijab");
    CT(-1.0, t2aa, "ijbc", Gvva, "ac", 1.0, Raa, "ijab");
    CT(-1.0, t2aa, "ikab", Gooa, "kj", 1.0, Raa, "ijab");
    CT(1.0, t2aa, "jkab", Gooa, "ki", 1.0, Raa, "ijab");
    CT(0.5, tauaa, "klab", Wooaa, "klij", 1.0, Raa, "ijab");
    CT(1.0, t1a, "kb", Y_aaaa, "kaij", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "ka", Y_aaaa, "kbij", 1.0, Raa, "ijab");
    CT(1.0, t2aa, "ikac", W_aaaa, "kbcj", 1.0, Raa, "ijab");
    CT(1.0, t2ab, "iKaC", W_baba, "KbCj", 1.0, Raa, "ijab");
    CT(1.0, t1a, "ka", Q_aaaa, "kbji", 1.0, Raa, "ijab");
    CT(-1.0, t2aa, "jkac", W_aaaa, "kbci", 1.0, Raa, "ijab");
    CT(-1.0, t2ab, "jKaC", W_baba, "KbCi", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "ka", Q_aaaa, "kbij", 1.0, Raa, "ijab");
    CT(-1.0, t2aa, "ikbc", W_aaaa, "kacj", 1.0, Raa, "ijab");
    CT(-1.0, t2ab, "iKbC", W_baba, "KaCj", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "kb", Q_aaaa, "kaji", 1.0, Raa, "ijab");
    CT(1.0, t2aa, "jkbc", W_aaaa, "kaci", 1.0, Raa, "ijab");
    CT(1.0, t2ab, "jKbC", W_baba, "KaCi", 1.0, Raa, "ijab");
    CT(1.0, t1a, "kb", Q_aaaa, "kaij", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "ic", ovvv, "jacb", 1.0, Raa, "ijab");
    CT(1.0, t1a, "ic", ovvv, "jbca", 1.0, Raa, "ijab");
    CT(1.0, t1a, "jc", ovvv, "iacb", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "jc", ovvv, "ibca", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "ka", ovoo, "jbik", 1.0, Raa, "ijab");
    CT(1.0, t1a, "ka", ovoo, "ibjk", 1.0, Raa, "ijab");
    CT(1.0, t1a, "kb", ovoo, "jaik", 1.0, Raa, "ijab");
    CT(-1.0, t1a, "kb", ovoo, "iajk", 1.0, Raa, "ijab");
    LADDER(oa * oa, va, va, I.vvvv, I.ld_vvvv, tauaa, Raa);
    // T2, alpha-beta
    PM(1.0, ovOV, "iaJB", 0.0, Rab, "iJaB");
    CT(1.0, t2ab, "iJaC", Gvvb, "BC", 1.0, Rab, "iJaB");
    CT(1.0, t2ab, "iJcB", Gvva, "ac", 1.0, Rab, "iJaB");
    CT(-1.0, t2ab, "iKaB", Goob, "KJ", 1.0, Rab, "iJaB");
    CT(-1.0, t2ab, "kJaB", Gooa, "ki", 1.0, Rab, "iJaB");
    CT(1.0, tauab, "kLaB", Wooab, "kLiJ", 1.0, Rab, "iJaB");
    CT(1.0, t1b, "KB", Y_baab, "KaiJ", 1.0, Rab, "iJaB");
    CT(-1.0, t1a, "ka", Y_abab, "kBiJ", 1.0, Rab, "iJaB");
    CT(1.0, t2aa, "ikac", W_abab, "kBcJ", 1.0, Rab, "iJaB");
    CT(1.0, t2ab, "iKaC", W_bbbb, "KBCJ", 1.0, Rab, "iJaB");
    CT(1.0, t1a, "ka", Q_abba, "kBJi", 1.0, Rab, "iJaB");
    CT(1.0, t2ab, "kJaC", W_abba, "kBCi", 1.0, Rab, "iJaB");
    CT(-1.0, t1a, "ka", Q_abab, "kBiJ", 1.0, Rab, "iJaB");
    CT(1.0, t2ab, "iKcB", W_baab, "KacJ", 1.0, Rab, "iJaB");
    CT(-1.0, t1b, "KB", Q_baba, "KaJi", 1.0, Rab, "iJaB");
    CT(1.0, t2ab, "kJcB", W_aaaa, "kaci", 1.0, Rab, "iJaB");
    CT(1.0, t2bb, "JKBC", W_baba, "KaCi", 1.0, Rab, "iJaB");
    CT(1.0, t1b, "KB", Q_baab, "KaiJ", 1.0, Rab, "iJaB");
    CT(1.0, t1a, "ic", OVvv, "JBca", 1.0, Rab, "iJaB");
    CT(1.0, t1b, "JC", ovVV, "iaCB", 1.0, Rab, "iJaB");
    CT(-1.0, t1a, "ka", OVoo, "JBik", 1.0, Rab, "iJaB");
    CT(-1.0, t1b, "KB", ovOO, "iaJK", 1.0, Rab, "iJaB");
    LADDER(oa * ob, va, vb, I.vvVV, I.ld_vvVV, tauab, Rab);
    // T2, beta-beta
    PM(1.0, OVOV, "IAJB", 0.0, Rbb, "IJAB");
    PM(-1.0, OVOV, "IBJA", 1.0, Rbb, "IJAB");
    CT(1.0, t2bb, "IJAC", Gvvb, "BC", 1.0, Rbb, "IJAB");
    CT(-1.0, t2bb, "IJBC", Gvvb, "AC", 1.0, Rbb, "IJAB");
    CT(-1.0, t2bb, "IKAB", Goob, "KJ", 1.0, Rbb, "IJAB");
    CT(1.0, t2bb, "JKAB", Goob, "KI", 1.0, Rbb, "IJAB");
    CT(0.5, taubb, "KLAB", Woobb, "KLIJ", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "KB", Y_bbbb, "KAIJ", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "KA", Y_bbbb, "KBIJ", 1.0, Rbb, "IJAB");
    CT(1.0, t2ab, "kIcA", W_abab, "kBcJ", 1.0, Rbb, "IJAB");
    CT(1.0, t2bb, "IKAC", W_bbbb, "KBCJ", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "KA", Q_bbbb, "KBJI", 1.0, Rbb, "IJAB");
    CT(-1.0, t2ab, "kJcA", W_abab, "kBcI", 1.0, Rbb, "IJAB");
    CT(-1.0, t2bb, "JKAC", W_bbbb, "KBCI", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "KA", Q_bbbb, "KBIJ", 1.0, Rbb, "IJAB");
    CT(-1.0, t2ab, "kIcB", W_abab, "kAcJ", 1.0, Rbb, "IJAB");
    CT(-1.0, t2bb, "IKBC", W_bbbb, "KACJ", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "KB", Q_bbbb, "KAJI", 1.0, Rbb, "IJAB");
    CT(1.0, t2ab, "kJcB", W_abab, "kAcI", 1.0, Rbb, "IJAB");
    CT(1.0, t2bb, "JKBC", W_bbbb, "KACI", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "KB", Q_bbbb, "KAIJ", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "IC", OVVV, "JACB", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "IC", OVVV, "JBCA", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "JC", OVVV, "IACB", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "JC", OVVV, "IBCA", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "KA", OVOO, "JBIK", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "KA", OVOO, "IBJK", 1.0, Rbb, "IJAB");
    CT(1.0, t1b, "KB", OVOO, "JAIK", 1.0, Rbb, "IJAB");
    CT(-1.0, t1b, "KB", OVOO, "IAJK", 1.0, Rbb, "IJAB");
    LADDER(ob * ob, vb, vb, I.VVVV, I.ld_VVVV, taubb, Rbb);
    return DMK_OK;
}

// one application of the amplitude equations to the vector `src`, the new amplitudes into `dst`
int uc_update(dmk_uccsd *h, const double *src, double *dst) {
    int rc;
    if ((rc = uc_rod(h, src))) return rc;
    const double *rhs[5] = {h->n1a, h->n1b, h->Raa, h->Rab, h->Rbb};
    for (int p = 0; p < 5; ++p)
        if ((rc = uc_div(h, p, rhs[p], dst))) return rc;
    return DMK_OK;
}

#undef LADDER
#undef TAU
#undef CT
#undef PM

int uc_init(dmk_uccsd *h) {
    int rc;
    const double *rhs[5] = {h->fova, h->fovb, h->Gaa, h->Gab, h->Gbb};
    for (int p = 0; p < 5; ++p)
        if ((rc = uc_div(h, p, rhs[p], h->T.x))) return rc;
    // E(MP2): the doubles alone, as PySCF's init_amps reports it
    if ((rc = cc_dot(h, h->P.cnt[2], h->Gaa, h->T.x + h->P.off[2], 0.25, 0, h->rec + 15))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[3], h->Gab, h->T.x + h->P.off[3], 1.0, 1, h->rec + 15))) return rc;
    if ((rc = cc_dot(h, h->P.cnt[4], h->Gbb, h->T.x + h->P.off[4], 0.25, 1, h->rec + 15))) return rc;
    h->have_amps = true;
    return DMK_OK;
}

}  // namespace

extern "C" {

int dmk_transpose_f64(dmk_ctx *ctx, int64_t rows, int64_t cols, const double *in, double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (rows < 1 || cols < 1 || rows > 0x7fffffffLL || cols > 0x7fffffffLL || !in || !out || in == out)
        return dmk_fail(ctx, DMK_ERR_INVALID, "transpose_f64: bad arguments (1 <= rows, cols < 2^31; two different arrays)");
    Engine E;
    E.ctx = ctx; E.extents((int)rows, (int)cols, 0, 0);
    return E.perm(1.0, in, "ia", 0.0, out, "ai");
}

int dmk_uccsd_plan(int nocc_a, int nvir_a, int nocc_b, int nvir_b, int diis_dim, int64_t *bytes_host) {
    if (!bytes_host || !extents_ok(nocc_a, nvir_a, nocc_b, nvir_b) || diis_dim < 0 || diis_dim > DIIS_MAX) return DMK_ERR_INVALID;
    dmk_uccsd h(nullptr, nocc_a, nvir_a, nocc_b, nvir_b, diis_dim);
    bytes_host[0] = (int64_t)h.carve(nullptr);
    bytes_host[1] = h.ws_bytes();
    return DMK_OK;
}

int dmk_uccsd_create(dmk_ctx *ctx, int nocc_a, int nvir_a, int nocc_b, int nvir_b, const dmk_uccsd_ints *ints, int diis_dim, dmk_uccsd **out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (!out || !ints || !extents_ok(nocc_a, nvir_a, nocc_b, nvir_b))
        return dmk_fail(ctx, DMK_ERR_INVALID, "uccsd_create: bad arguments (every extent in [1, 512]; the integrals and the result)");
    if (diis_dim < 0 || diis_dim > DIIS_MAX) return dmk_fail(ctx, DMK_ERR_INVALID, "uccsd_create: diis_dim %d outside [0, %d]", diis_dim, DIIS_MAX);
    const dmk_uccsd_ints &I = *ints;
    for (const double *p : {I.fock_a, I.fock_b, I.oooo, I.ovoo, I.ovov, I.oovv, I.ovvv, I.vvvv, I.OOOO, I.OVOO, I.OVOV, I.OOVV, I.OVVV, I.VVVV, I.ooOO,
                            I.ovOO, I.ovOV, I.ooVV, I.ovVV, I.vvVV, I.OVoo, I.OOvv, I.OVvv})
        if (!p) return dmk_fail(ctx, DMK_ERR_INVALID, "uccsd_create: a NULL Fock matrix or integral block");
    if (I.ld_vvvv < pair_of(nvir_a) || I.ld_VVVV < pair_of(nvir_b) || I.ld_vvVV < pair_of(nvir_b))
        return dmk_fail(ctx, DMK_ERR_INVALID, "uccsd_create: pitch of a packed block below npair of its columns");
    *out = nullptr;
    dmk_uccsd *h = new dmk_uccsd(ctx, nocc_a, nvir_a, nocc_b, nvir_b, diis_dim);
    h->I = I;
    return cc_create(h, "uccsd_create", [&]() -> int {
        {
            FamScope fs(ctx, DMK_FAM_MISC);
            const int na = nocc_a + nvir_a, nb = nocc_b + nvir_b;
            hipLaunchKernelGGL(cc_fock_split_kernel, dim3(grid_of((long long)na * na)), dim3(NT), 0, ctx->stream, nocc_a, nvir_a, I.fock_a, h->fooa,
                               h->fvva, h->fova, h->eoa, h->eva);
            hipLaunchKernelGGL(cc_fock_split_kernel, dim3(grid_of((long long)nb * nb)), dim3(NT), 0, ctx->stream, nocc_b, nvir_b, I.fock_b, h->foob,
                               h->fvvb, h->fovb, h->eob, h->evb);
            if (hipGetLastError() != hipSuccess) return dmk_fail(ctx, DMK_ERR_HIP, "uccsd_create: kernel launch failed");
        }
        // <ij||ab> = (ia|jb) - (ib|ja) in (i, j, a, b) order for the same-spin blocks, <iJ|aB> = (ia|JB) for the mixed one
        int rc;
        if ((rc = h->E.perm(1.0, I.ovov, "iajb", 0.0, h->Gaa, "ijab"))) return rc;
        if ((rc = h->E.perm(-1.0, I.ovov, "ibja", 1.0, h->Gaa, "ijab"))) return rc;
        if ((rc = h->E.perm(1.0, I.OVOV, "IAJB", 0.0, h->Gbb, "IJAB"))) return rc;
        if ((rc = h->E.perm(-1.0, I.OVOV, "IBJA", 1.0, h->Gbb, "IJAB"))) return rc;
        return h->E.perm(1.0, I.ovOV, "iaJB", 0.0, h->Gab, "iJaB");
    }, out);
}

int dmk_uccsd_free(dmk_uccsd *h) { return cc_free(h); }

int dmk_uccsd_init(dmk_uccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    return h->synced([h] { return uc_init(h); });
}

int dmk_uccsd_set(dmk_uccsd *h, const double *t1a, const double *t1b, const double *t2aa, const double *t2ab, const double *t2bb) {
    if (!h) return DMK_ERR_INVALID;
    const double *src[5] = {t1a, t1b, t2aa, t2ab, t2bb};
    for (const double *p : src)
        if (!p) return dmk_fail(h->ctx, DMK_ERR_INVALID, "uccsd_set: NULL amplitudes");
    return h->set(src, h->T.x, &h->have_amps);
}

int dmk_uccsd_energy(dmk_uccsd *h, double *e_dev) {
    if (!h) return DMK_ERR_INVALID;
    if (!e_dev || !h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "uccsd_energy: no amplitudes yet (init or set first), or a NULL result");
    return h->synced([=] { return uc_energy(h, h->T.x, e_dev); });
}

int dmk_uccsd_update(dmk_uccsd *h) {
    if (!h) return DMK_ERR_INVALID;
    if (!h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "uccsd_update: no amplitudes yet (init or set first)");
    return h->step(h->T, [h](const double *from, double *to) { return uc_update(h, from, to); });
}

int dmk_uccsd_run(dmk_uccsd *h, int max_iter, double tol_e, double tol_normt, double *result_host) {
    if (!h) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (!result_host || max_iter < 0) return dmk_fail(ctx, DMK_ERR_INVALID, "uccsd_run: bad arguments");
    int rc;
    if (!h->have_amps && (rc = uc_init(h))) return rc;
    // without a ring the steps are kept in n1a / n1b / tataa / tatab / tatbb, free between updates
    const Iterate s{&h->T, {h->n1a, h->n1b, h->tataa, h->tatab, h->tatbb}, true, "uccsd_run"};
    return cc_iterate(h, s, max_iter, tol_e, tol_normt, [h](const double *from, double *to) { return uc_update(h, from, to); },
                      [h](const double *amp, double *e_dev) { return uc_energy(h, amp, e_dev); }, result_host);
}

int dmk_uccsd_get(dmk_uccsd *h, int what, double *out) {
    if (!h) return DMK_ERR_INVALID;
    if (!out || what < DMK_UCCSD_T1A || what > DMK_UCCSD_EMP2) return dmk_fail(h->ctx, DMK_ERR_INVALID, "uccsd_get: bad arguments");
    if (!h->have_amps) return dmk_fail(h->ctx, DMK_ERR_STATE, "uccsd_get: no amplitudes yet (init or set first)");
    return h->get(h->T.x, what, out);          // DMK_UCCSD_T1A .. _T2BB = 0 .. 4: the parts, then DMK_UCCSD_EMP2
}

}  // extern "C"
