// Shared pieces of the hot half-transform kernels (zhot.hip, zhot_tab.hip): the complex 16 x 16 x 4 tile step on the
// real f64 MFMA, the tril-pack accumulate epilogue and the queue part of the step-2 kernel arguments.
#pragma once
#include "common.h"

namespace {

constexpr int HNT = 256;

// Karatsuba "3M" complex product: T1 += Ar Br, T2 += Ai Bi, T3 += (Ar + Ai)(Br + Bi); Re = T1 - T2, Im = T3 - T1 - T2.
// 25 % fewer MFMAs than the four-product form for 1.5x the accumulator registers; with LDS-DMA there are no staging
// registers in these kernels, so up to 9 accumulator tiles (216 VGPRs) of a wave fit two waves per SIMD without spilling.
// Normwise backward stable; the parity tests hold it to the same 1e-8 / 1e-10 budgets (measured 2e-15).
struct cfrag { double2 v; double s; };      // operand fragment and re + im
struct cacc { d4_t p, q, t; };              // T1, T2, T3
__device__ __forceinline__ void cacc_zero(cacc &c) {
    c.p = d4_t{0.0, 0.0, 0.0, 0.0};
    c.q = d4_t{0.0, 0.0, 0.0, 0.0};
    c.t = d4_t{0.0, 0.0, 0.0, 0.0};
}
__device__ __forceinline__ double2 lds_frag(const double2 *p) { return *p; }
__device__ __forceinline__ cfrag cfrag_of(double2 v) {
    cfrag f;
    f.v = v;
    f.s = v.x + v.y;
    return f;
}
__device__ __forceinline__ void cmfma(cacc &c, const cfrag &a, const cfrag &b) {
    c.p = __builtin_amdgcn_mfma_f64_16x16x4f64(a.v.x, b.v.x, c.p, 0, 0, 0);
    c.q = __builtin_amdgcn_mfma_f64_16x16x4f64(a.v.y, b.v.y, c.q, 0, 0, 0);
    c.t = __builtin_amdgcn_mfma_f64_16x16x4f64(a.s, b.s, c.t, 0, 0, 0);
}
__device__ __forceinline__ double cacc_re(const cacc &c, int r) { return c.p[r] - c.q[r]; }
__device__ __forceinline__ double cacc_im(const cacc &c, int r) { return (c.t[r] - c.p[r]) - c.q[r]; }

// RE = true: only the REAL part of the product is wanted -- a momentum transfer kL that is its own time-reversal partner
// (weight 1) contributes Re(Lij)^T Re(Lij) only (eri_transform.py:453-455, 464-467: the imaginary part of its planes is never read),
// so step 2 runs Re S = Ur Cr - Ui Ci: two real MFMAs per complex block step instead of the three of 3M, no operand sums, no T3
// accumulator, one plane atomic per element.  RE = false is the code above, instruction for instruction.
template <bool RE> __device__ __forceinline__ cfrag cfrag_of_t(double2 v) {
    if constexpr (RE) { cfrag f; f.v = v; f.s = 0.0; return f; }
    else return cfrag_of(v);
}
template <bool RE> __device__ __forceinline__ void cmfma_t(cacc &c, const cfrag &a, const cfrag &b) {
    if constexpr (RE) {
        c.p = __builtin_amdgcn_mfma_f64_16x16x4f64(a.v.x, b.v.x, c.p, 0, 0, 0);
        c.q = __builtin_amdgcn_mfma_f64_16x16x4f64(a.v.y, b.v.y, c.q, 0, 0, 0);
    } else {
        cmfma(c, a, b);
    }
}

// planes[(ri * naux + L) * npair + row (row + 1) / 2 + col] += value for row >= col, row < nrows.
// Single writer per address per launch -> deterministic; fire-and-forget atomics: no load latency in the epilogue.
__device__ __forceinline__ void pack_acc(double *planes, long long naux, long long npair, int L, int row, int col,
                                         double vr, double vi, int nrows = 0x7fffffff) {
    if (row >= col && row < nrows) {
        const long long idx = (long long)row * (row + 1) / 2 + col;
        unsafeAtomicAdd(planes + (long long)L * npair + idx, vr);
        unsafeAtomicAdd(planes + (naux + (long long)L) * npair + idx, vi);
    }
}

template <bool RE> __device__ __forceinline__ void pack_acc_t(double *planes, long long naux, long long npair, int L, int row, int col,
                                                             const cacc &c, int r, int nrows = 0x7fffffff) {
    if constexpr (RE) {
        if (row >= col && row < nrows)
            unsafeAtomicAdd(planes + (long long)L * npair + (long long)row * (row + 1) / 2 + col, cacc_re(c, r));
    } else {
        pack_acc(planes, naux, npair, L, row, col, cacc_re(c, r), cacc_im(c, r), nrows);
    }
}

// Kernel-argument arrays must only be indexed with compile-time constants, and the argument struct must
// never be passed by reference: either makes hipcc copy the whole struct to scratch (private memory), whose
// loads need s_waitcnt vmcnt(0) -- draining the LDS-DMA ring -- and whose per-dispatch scratch set-up cost
// ~17 ms per launch when a step-2 kernel first did it.
#define H2_PICK_CJ(G, SLOT)                                                                        \
    ((SLOT) == 0 ? (G).Cj[0] : (SLOT) == 1 ? (G).Cj[1] : (SLOT) == 2 ? (G).Cj[2] : (SLOT) == 3 ? (G).Cj[3]      \
     : (SLOT) == 4 ? (G).Cj[4] : (SLOT) == 5 ? (G).Cj[5] : (SLOT) == 6 ? (G).Cj[6] : (SLOT) == 7 ? (G).Cj[7]    \
     : (SLOT) == 8 ? (G).Cj[8] : (SLOT) == 9 ? (G).Cj[9] : (SLOT) == 10 ? (G).Cj[10] : (SLOT) == 11 ? (G).Cj[11] \
     : (SLOT) == 12 ? (G).Cj[12] : (SLOT) == 13 ? (G).Cj[13] : (SLOT) == 14 ? (G).Cj[14] : (G).Cj[15])

// k_i of block SLOT from the packed halves of H2WArgs::ki2 (compile-time indices only, as above)
#define H2_PICK_K2(A, SLOT)                                                                        \
    ((((SLOT) >> 1) == 0 ? A[0] : ((SLOT) >> 1) == 1 ? A[1] : ((SLOT) >> 1) == 2 ? A[2] : ((SLOT) >> 1) == 3 ? A[3] \
      : ((SLOT) >> 1) == 4 ? A[4] : ((SLOT) >> 1) == 5 ? A[5] : ((SLOT) >> 1) == 6 ? A[6] : A[7])             \
         >> (16 * ((SLOT) & 1)) & 0xffffu)

// Host side, what the kernel arguments of both step-2 kernels (H2Args, H2TArgs) share: the queue of a Half2Launch -- operands,
// partner-term mask, strides, sizes and the K loop bound on a K tile of `bk` rows.  False where the launcher declines: a queue
// length, spin count or K bound the kernels do not cover, or an operand off the 16 bytes of an LDS-DMA piece.
template <class Args> bool fill_half2_queue(Args &a, const Half2Launch &q, int bk) {
    constexpr int MAXSLOT = (int)(sizeof(a.Cj) / sizeof(a.Cj[0]));
    const int kdim = q.kdim ? q.kdim : q.nao;
    if (kdim < q.nao || (kdim % bk) != 0 || q.nslot < 1 || q.nslot > MAXSLOT || q.nspin < 1 || q.nspin > 2) return false;
    if (reinterpret_cast<uintptr_t>(q.Ut) & 15) return false;
    a.Ut = reinterpret_cast<const double2 *>(q.Ut); a.symmask = 0;
    for (int i = 0; i < MAXSLOT; ++i) {
        a.Cj[i] = reinterpret_cast<const double2 *>(q.Cj[i < q.nslot ? i : 0]);
        if (i < q.nslot && q.sym[i]) a.symmask |= 1u << i;
        if (reinterpret_cast<uintptr_t>(a.Cj[i]) & 15) return false;
    }
    a.slot_stride = q.slot_stride; a.planes = q.planes; a.naux = q.plane_rows; a.npair = q.row_len;
    a.nL = q.nL; a.nao = q.nao; a.nslot = q.nslot; a.kdim = kdim; a.nspin = q.nspin;
    a.ut_spin_stride = q.ut_spin_stride; a.cj_spin_stride = q.cj_spin_stride; a.planes_spin_stride = q.planes_spin_stride;
    // every queued block carries the partner term: the diagonal blocks run one segment and are folded in the epilogue
    a.fold_diag = (a.symmask == (1u << q.nslot) - 1u) ? 1 : 0;
    return true;
}

}  // namespace
