// What csrc/ccsd_t.hip (K22) reads of a dmk_rccsd handle, whose layout stays private to csrc/ccsd.hip (K21): the borrowed blocks, the
// pieces of the Fock matrix and the CURRENT amplitudes.  Nothing here is written through; the pointers are good until the next call
// that changes the handle's amplitudes.
#pragma once
#include "common.h"

struct RccsdView {
    dmk_ctx *ctx;
    int o, v;
    bool have_amps;
    const double *ovoo, *ovov, *ovvv;      // (ia|jk), (ia|jb), (ia|bc), row-major in the order of the letters
    const double *fov, *eo, *ev;           // f_ia and the Fock diagonal
    const double *t1, *t2;                 // (i, a) and (i, j, a, b)
};
int dmk_rccsd_view(dmk_rccsd *h, RccsdView *out);

// out (index order so) = alpha in (index order si) + beta out with the cc_perm_* kernels of csrc/ccsd.hip: letters i j k l have
// extent o, a b c d extent v, up to four of them
int dmk_cc_perm(dmk_ctx *ctx, int o, int v, double alpha, const double *in, const char *si, double beta, double *out, const char *so);
