// K6 hot kernels -- the density-fitted half transform at production tile sizes.
//
//   step 1  Ut[L][q][a] = sum_p Lpq[L][p][q] conj(C_i[p][a])                 (r_e2, first index)
//   step 2  S_L[a][b]   = sum_q Ut[L][q][a] C_j[q][b] (+ sum_q C_j[q][a] Ut[L][q][b])   (second index
//           + lib.hermi_sum of the time-reversal partner), a >= b, tril-packed and ACCUMULATED
//           into the Re / Im planes of Lij_s4
//   reference: basis_transform/eri_transform.py:368-378, 403-434
//
// Why a second implementation next to the generic zgemm.hip (numbers: MI355X, rocprof PMC and the
// ablation labs under tools/):
//   * the generic register-staged kernels kept the f64 matrix pipe only 56-62 % busy with 30-45 % of
//     the wave cycles parked in s_waitcnt / s_barrier, and cutting the MFMA count by 25 % (3M) changed
//     nothing: the half transform was latency-bound on its operand feed, not pipe-bound
//     (tools/mfma_f64_probe.hip: 77.5 TFLOP/s is reachable from registers);
//   * operands therefore arrive by LDS-DMA (global_load_lds_dwordx4) into a 3-4 stage ring, issued
//     two to three K-tiles ahead and retired by a counted s_waitcnt vmcnt(N) + ONE raw s_barrier per
//     K-tile; no staging registers, no scratch (round 4: the LDS-DMA pieces are addressed as scalar tile base + one loop-invariant
//     32-bit offset VGPR per piece, which removed half2_kernel's last 18 spilled VGPRs), so the counted waits are never drained
//     by the compiler;
//   * 256-thread workgroups, TWO per CU: a 512-thread workgroup sharing a larger tile halves the L2
//     bytes per flop but runs its two waves per SIMD in barrier lock-step and measured 10 % slower
//     than two independent workgroups that desynchronise by themselves (tools/gemm_lab*.hip);
//   * step 2 never computes a 16 x 16 block above the diagonal AND keeps every wave equally loaded:
//     per L four workgroups -- the two 64 x 128 halves of the off-diagonal square (8 blocks per wave)
//     and the two 128 x 128 diagonal triangles with block rows paired (w, 7 - w) so that each wave owns
//     exactly 9 of a triangle's 36 blocks; in a triangle both segments of the symmetrised product read
//     the SAME two LDS panels;
//   * step 2 runs straight through up to 16 queued AO blocks per launch: accumulators and the
//     tril-pack epilogue are shared, and the epilogue uses fire-and-forget f64 atomics (exactly one
//     writer per plane element per launch, so the sum stays deterministic).
// Complex arithmetic is 3M (Karatsuba: three real MFMAs per complex tile step, see cmfma below); with LDS-DMA
// there are no staging registers, so the 1.5x accumulator set still fits two waves per SIMD without spilling.
//
// Constraints (else the caller falls back to zgemm.hip): nao % 8 == 0, nemb == 256 for step 2,
// 16-B aligned operands.
#include "common.h"
#include <cstdlib>
#include <algorithm>
#include <type_traits>

#include "zhot_common.h"

namespace {

// =============================================================================================
// step 1: flattened M-blocks (batch L folded into M), tile 128 x 64, BK = 8, 3-stage ring (72 KiB)
// =============================================================================================
constexpr int H1_BM = 128, H1_BN = 64, H1_BK = 8, H1_D = 3;

// out[L][m][n] = sum_k A[L][k][m] * op(B[k][n]),  op = conj (CONJB; step 1: B = C_i -- the only form the library launches) or
// identity.  A is K-major: element (k, m) of batch L at L * (nao * mrows) + k * mrows + m  (step 1: Lpq, mrows = nao).
// The batch index is folded into M in 16-row blocks.
struct H1Args {
    const double2 *Lpq;    // A
    const double2 *Ci;     // B [nao][nemb]
    double2 *Ut;           // out [nL][mrows][nemb]
    int nL, nao, nemb, nblk;   // nao = K; nblk = ceil(mrows / 16)
    int mrows;
    // K loop bound: nao rounded up to the K tile.  B must hold kdim rows, ZERO beyond nao (the pipeline keeps a padded copy of
    // C_ao_emb); the A rows of the padding are the clamped row nao - 1 -- finite numbers against zeros, never read past a block
    int kdim;
    int tiles_m, tiles_n;
    unsigned nblocks;
    // both spin channels in one launch: the same A tile (AO block) against C_i of spin 0 / spin 1 into their own Ut;
    // the workgroups of one M tile are adjacent (n tile fastest, then spin), so they share the A tile in L2
    int nspin;
    long long b_spin_stride, out_spin_stride;
    // several queued AO blocks in one launch (one ramp-up / drain instead of one per block): block `slot` is the A
    // operand Lpq + slot * a_slot_stride, its B operand Ci + bk[slot] * b_k_stride, its output Ut + slot * out_slot_stride
    int nslot;
    unsigned per_slot;      // workgroups per block = tiles_m * tiles_n * nspin
    long long a_slot_stride, out_slot_stride, b_k_stride;
    int bk[16];
};

#define H1_PICK_BK(G, SLOT)                                                                        \
    ((SLOT) == 0 ? (G).bk[0] : (SLOT) == 1 ? (G).bk[1] : (SLOT) == 2 ? (G).bk[2] : (SLOT) == 3 ? (G).bk[3]      \
     : (SLOT) == 4 ? (G).bk[4] : (SLOT) == 5 ? (G).bk[5] : (SLOT) == 6 ? (G).bk[6] : (SLOT) == 7 ? (G).bk[7]    \
     : (SLOT) == 8 ? (G).bk[8] : (SLOT) == 9 ? (G).bk[9] : (SLOT) == 10 ? (G).bk[10] : (SLOT) == 11 ? (G).bk[11] \
     : (SLOT) == 12 ? (G).bk[12] : (SLOT) == 13 ? (G).bk[13] : (SLOT) == 14 ? (G).bk[14] : (G).bk[15])

// BM = 128 (wave tile 64 x 32, 8 accumulator tiles, two workgroups per CU) or BM = 64 (wave tile 32 x 32, 4 tiles, three
// workgroups per CU).  NARROW: the output tile is 48 instead of 64 columns wide -- the four waves are stacked along M
// (wave tile BM / 4 x 48: 6 accumulator tiles at BM = 128) -- for embedding dimensions that three 48-column tiles cover
// with less padding than 64-column ones (C4: nemb 136 -> 144 instead of 192 computed columns).  The B panel keeps its
// 64-column LDS rows (lanes 48-63 of a piece land in the padding), so the LDS-DMA issue pattern is the same for both.
// The M index is the FLAT row (L, q) -> L * mrows + q with no padding between batches: a 16-row block may straddle two L
// (every lane carries its own source address, and Ut[L][q][:] is one contiguous array of nL * mrows rows).
// LAB (tools/zhot_lab.hip only; the product instantiates LAB = 0, where every `if constexpr` below folds away): ablation bits that
// remove one ingredient of the K loop at a time so that its share of the time can be MEASURED on the real kernel -- 1: no Ut
// stores, 2: no LDS-DMA after the prologue (the ring keeps stale tiles), 4: no s_barrier.  Results of a LAB != 0 instantiation are
// meaningless by construction.
// KPAD: the K loop runs over g.kdim > g.nao (an AO dimension off the K tile); only then are the A rows clamped -- the instantiation
// for dimensions on the tile is the kernel of rounds 2 - 5, instruction for instruction (the clamp measured 2.4 % on it).
template <bool CONJB, int BM, int OCC, bool NARROW, int LAB = 0, bool KPAD = false>
__global__ __launch_bounds__(HNT, OCC) void half1_kernel(const H1Args g) {
    __shared__ __attribute__((aligned(16))) double2 lds[H1_D * H1_BK * (BM + H1_BN)];
#define ZH_BLOCK_ID blockIdx.x
#include "zhot_half1_body.inc"
#undef ZH_BLOCK_ID
}

// The same body as a device function: block `bid` of a step-1 grid of g.nblocks, on an LDS ring the caller owns (half12_kernel).
// half1_kernel includes the text instead of calling this: behind a call, even an inlined one, hipcc schedules the body differently,
// and the kernels of the separate launches are kept instruction for instruction.
template <bool CONJB, int BM, bool NARROW, int LAB, bool KPAD>
__device__ __forceinline__ void half1_body(const H1Args &g, const unsigned bid, double2 *const lds) {
#define ZH_BLOCK_ID bid
#include "zhot_half1_body.inc"
#undef ZH_BLOCK_ID
}

// =============================================================================================
// W (K6l): the partner term of step-2 type 1 from the other side
// =============================================================================================
// W[L][p][n] = sum_q Lpq[L][p][q] C_j[q][col0 + n], n < 64, of every queued block that carries the partner term: with it the partner
// segment of the type-1 workgroups is sum_p W[p][a] conj(C_i[p][b]) and no longer reads columns [0,128) of Ut, so a warm call
// transforms columns [128,256) only in step 1.  Same tile and ring as half1_kernel<true, 128, 2, false>.
struct HWArgs {
    const double2 *Lpq;    // A [nslot][nL][nao][nao], read K-contiguous: row (L, p) at (L nao + p) nao
    const double2 *C;      // B: C_j of slot s at C + bk[s] * c_k_stride (+ spin), [nao][nemb]
    double2 *W;            // out [spin][slot][nL nao][64]
    int nL, nao, nemb, col0;
    int nspin, nslot;
    unsigned per_slot, nblocks;   // workgroups per block = tiles_m * nspin
    unsigned symmask;      // bit s: block s carries the partner term (the others are skipped)
    long long a_slot_stride, w_slot_stride, w_spin_stride, c_spin_stride, c_k_stride;
    int bk[16];            // k_j of every slot
};

__device__ __forceinline__ void halfw_body(const HWArgs &g, const unsigned bid, double2 *const lds) {
#define ZH_BLOCK_ID bid
#include "zhot_halfw_body.inc"
#undef ZH_BLOCK_ID
}

// step 1 of a queued group and, behind its workgroups, the W tiles of the same group
__global__ __launch_bounds__(HNT, 2) void half1w_kernel(const H1Args g, const HWArgs gw) {
    __shared__ __attribute__((aligned(16))) double2 lds[H1_D * H1_BK * (H1_BM + H1_BN)];
    if (blockIdx.x < g.nblocks) half1_body<true, H1_BM, false, 0, false>(g, blockIdx.x, lds);
    else halfw_body(gw, blockIdx.x - g.nblocks, lds);
}

// =============================================================================================
// step 2 (nemb == 256): per L four workgroups
//   type 0 / 1 : rows [128,192) / [192,256) x cols [0,128) of the off-diagonal square (8 blocks / wave)
//   type 2 / 3 : diagonal triangle [0,128)^2 / [128,256)^2, block rows (w, 7-w) per wave (9 blocks / wave)
// strip order (K6m, half2s_kernel): type 3 gives way to
//   strip      : rows [192,256) x cols [128,256), type 1's geometry and W partner, b <= a written (8 blocks / wave)
//   corner     : diagonal triangle [128,192)^2, block rows (w, 3-w) on waves 0 and 1 (5 blocks each)
// =============================================================================================
constexpr int H2_N = 256, H2_BK = 4;
constexpr int H2_MAXSLOT = 16;
constexpr int H2S_STAGE = H2_BK * 384, H2S_D = 3;     // square: Ua[4][64] | Cb[4][128] | Ca[4][64] | Ub[4][128] (24 KiB)
constexpr int H2T_STAGE = H2_BK * 256, H2T_D = 4;     // triangle: U[4][128] | C[4][128]                        (16 KiB)
constexpr int H2_LDS = (H2S_STAGE * H2S_D > H2T_STAGE * H2T_D) ? H2S_STAGE * H2S_D : H2T_STAGE * H2T_D;

struct H2Args {
    const double2 *Ut;     // [nslot][nL][nao][256]: step-1 outputs of `nslot` consecutive AO blocks
    const double2 *Cj[H2_MAXSLOT];   // [nao][256] of each block
    unsigned symmask;      // bit s: add the time-reversal partner term of block s?
    long long slot_stride; // elements between the Ut of consecutive slots
    double *planes;        // [(ri * naux + L) * npair + pair]
    long long naux, npair;
    int nL, nao, nslot;
    int kdim;              // K loop bound: nao rounded up to the K tile; Cj holds kdim rows, zero beyond nao (Ut rows of the padding
                           // are whatever follows in the pipeline's own, initialised buffer: finite numbers against zeros)
    unsigned nblocks;
    // both spin channels in ONE launch (4 nL nspin workgroups): one ramp-up / drain per group of queued blocks instead
    // of one per spin (measured at C5: 2 x 8.19 ms -> 15.75 ms).  Cutting the last rounds of workgroups into shorter
    // ones (slot ranges accumulated through partial buffers) was tried on top and measured slower: the launch is
    // throughput-bound in steady state, the extra epilogues cost more than the shorter drain saves.
    int nspin;
    long long ut_spin_stride, cj_spin_stride, planes_spin_stride;   // elements between the spin channels
    // every queued block carries the time-reversal partner term: the 16 DIAGONAL 16 x 16 blocks then skip segment 2 and are
    // completed as P + P^T in the epilogue (S_rr = U_r^T C_r + C_r^T U_r, and the second product is the transpose of the
    // first): 256 instead of 272 block products per L, and triangle waves issue 16 per K step like the square ones
    int fold_diag;
    // the caller has already put the iteration-invariant part of the planes in place (types 0 and 2: every pair with a < 192 that
    // those two workgroups own, eri_engine.hip dmk_eri_cache): only types 1 and 3 run, two workgroups per (L, spin)
    int skip_invariant;
};

// K6l, the split instantiations (SPL in zhot_half2_body.inc): type 1 takes the A fragments of its partner segment from the W panel of
// the block and the B fragments from conj(C_i) columns [0,128) -- the same number of LDS-DMA pieces and MFMAs per K tile.
struct H2WArgs {
    const double2 *W;                 // [spin][slot][nL][nao][64], dense: block s of spin sp at ((sp nslot_max + s) nL nao) 64
    const double2 *C;                 // [spin][nk][nao][256]: C_i / C_j of block s at C + k(s) * nao * 256 (+ the spin stride of Cj)
    // k_i and k_j of the blocks, 16 bits each: the split kernels address BOTH operands through them and never read H2Args::Cj -- a
    // second pointer per block on top of Cj[16] does not fit the scalar registers of the fused kernel
    unsigned ki2[H2_MAXSLOT / 2], kj2[H2_MAXSLOT / 2];
    long long w_spin_stride;
};

// LAB: ablation bits of tools/zhot_lab.hip, as in half1_kernel (1: no plane atomics, 2: no LDS-DMA after the prologue, 4: no
// s_barrier); the product instantiates LAB = 0.
template <int LAB = 0, bool RE = false>
__global__ __launch_bounds__(HNT, 2) void half2_kernel(const H2Args g) {
    __shared__ __attribute__((aligned(16))) double2 lds[H2_LDS];
    constexpr bool SPL = false, STRIP = false;
    const H2WArgs gw{};
#define ZH_BLOCK_ID blockIdx.x
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}

template <bool RE>
__global__ __launch_bounds__(HNT, 2) void half2w_kernel(const H2Args g, const H2WArgs gw) {
    __shared__ __attribute__((aligned(16))) double2 lds[H2_LDS];
    constexpr int LAB = 0;
    constexpr bool SPL = true, STRIP = false;
#define ZH_BLOCK_ID blockIdx.x
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}

// K6m, the strip instantiations (STRIP in zhot_half2_body.inc): per (L, spin) the workgroups 0, 1, 2, corner, strip (dense) or 1 and
// the strip (warm) -- no workgroup reads columns [128,192) of Ut on a warm kL.  Same arguments as the split form.
template <bool RE>
__global__ __launch_bounds__(HNT, 2) void half2s_kernel(const H2Args g, const H2WArgs gw) {
    __shared__ __attribute__((aligned(16))) double2 lds[H2_LDS];
    constexpr int LAB = 0;
    constexpr bool SPL = true, STRIP = true;
#define ZH_BLOCK_ID blockIdx.x
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}

// (as half1_body: the device function of the same text, for half12_kernel)
template <int LAB, bool RE>
__device__ __forceinline__ void half2_body(const H2Args &g, const unsigned bid, double2 *const lds) {
    constexpr bool SPL = false, STRIP = false;
    const H2WArgs gw{};
#define ZH_BLOCK_ID bid
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}
template <bool RE>
__device__ __forceinline__ void half2w_body(const H2Args &g, const H2WArgs &gw, const unsigned bid, double2 *const lds) {
    constexpr int LAB = 0;
    constexpr bool SPL = true, STRIP = false;
#define ZH_BLOCK_ID bid
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}

template <bool RE>
__device__ __forceinline__ void half2s_body(const H2Args &g, const H2WArgs &gw, const unsigned bid, double2 *const lds) {
    constexpr int LAB = 0;
    constexpr bool SPL = true, STRIP = true;
#define ZH_BLOCK_ID bid
#include "zhot_half2_body.inc"
#undef ZH_BLOCK_ID
}

// =============================================================================================
// steps 2 and 1 in ONE launch: step 2 of a queued group and, behind it, step 1 of the NEXT group
// =============================================================================================
// A step-2 launch is a few thousand workgroups of equal length on 512 resident slots (256 CUs x 2): C5 warm 3200 -> 6.25 rounds,
// paid as 7 with 3/4 of the slots empty in the last one.  Step 1 of the next group (tens of thousands of short workgroups, the
// same 256 threads, 2 workgroups per CU and 73 728 B of LDS) does not depend on it once Ut has two halves, but an in-order stream
// never overlaps two launches.  Here the step-2 workgroups take the low block ids and the step-1 workgroups follow: as step-2
// workgroups retire, their slots go to step 1 at once.  Every workgroup does what it does in the separate launches -- the same
// body, the same arguments, its block id within its own grid (XCD remap over its own count) -- so results are bit-identical.
// One LDS array serves whichever body runs (two would halve the occupancy).  Step-1 side: the 128 x 64 tile only.
constexpr int H12_LDS = (H1_D * H1_BK * (H1_BM + H1_BN) > H2_LDS) ? H1_D * H1_BK * (H1_BM + H1_BN) : H2_LDS;
template <bool RE, bool KPAD>
__global__ __launch_bounds__(HNT, 2) void half12_kernel(const H2Args g2, const H1Args g1) {
    __shared__ __attribute__((aligned(16))) double2 lds[H12_LDS];
    if (blockIdx.x < g2.nblocks) half2_body<0, RE>(g2, blockIdx.x, lds);
    else half1_body<true, H1_BM, false, 0, KPAD>(g1, blockIdx.x - g2.nblocks, lds);
}

// The split form (K6l): [step 2 with the W partner | Ut tiles of the next group | W tiles of the next group]
template <bool RE>
__global__ __launch_bounds__(HNT, 2) void half12w_kernel(const H2Args g2, const H2WArgs gw2, const H1Args g1, const HWArgs gw1) {
    __shared__ __attribute__((aligned(16))) double2 lds[H12_LDS];
    if (blockIdx.x < g2.nblocks) half2w_body<RE>(g2, gw2, blockIdx.x, lds);
    else if (blockIdx.x - g2.nblocks < g1.nblocks) half1_body<true, H1_BM, false, 0, false>(g1, blockIdx.x - g2.nblocks, lds);
    else halfw_body(gw1, blockIdx.x - g2.nblocks - g1.nblocks, lds);
}

// The strip form (K6m): the same launch with the strip instantiation of step 2
template <bool RE>
__global__ __launch_bounds__(HNT, 2) void half12s_kernel(const H2Args g2, const H2WArgs gw2, const H1Args g1, const HWArgs gw1) {
    __shared__ __attribute__((aligned(16))) double2 lds[H12_LDS];
    if (blockIdx.x < g2.nblocks) half2s_body<RE>(g2, gw2, blockIdx.x, lds);
    else if (blockIdx.x - g2.nblocks < g1.nblocks) half1_body<true, H1_BM, false, 0, false>(g1, blockIdx.x - g2.nblocks, lds);
    else halfw_body(gw1, blockIdx.x - g2.nblocks - g1.nblocks, lds);
}

bool hot_enabled() {
    static const bool on = [] { const char *e = getenv("DMK_ERI_HOT"); return !(e && atoi(e) == 0); }();
    return on;
}

}  // namespace

// shapes the flattened kernel covers when the flattened row count is nL x nao (step 1)
int half1_hot_usable(int nL, int nao, int nemb) {
    // the per-lane part of an LDS-DMA source address is a 32-bit byte offset from the block's base (glds16s): an AO block must stay
    // below 4 GiB (C5: 512 MB); larger ones take the generic kernels
    // (nao need not be a multiple of the K tile: the K loop runs over hot_kdim(nao) with a zero-padded B operand)
    return hot_enabled() && nao >= 2 * H1_BK && nemb >= 32 && (long long)nL * nao >= 4 * H1_BM &&
           (long long)nL * nao * nao * 16 < (1LL << 32);
}

// Auxiliary rows one step-1 launch may cover: the per-lane part of an LDS-DMA source address is a 32-bit byte offset from the
// block's base, so a launch spans < 4 GiB of its AO block; blocks beyond that (naux nao^2 >= 2^28) are transformed in several
// launches over ranges of L (eri_engine.hip). DMK_ERI_HOT_LCHUNK caps it (tests: the cut on small shapes).
int half1_hot_max_rows(int nao) {
    long long rows = ((1LL << 32) - 1) / ((long long)nao * nao * 16);
    if (const char *e = getenv("DMK_ERI_HOT_LCHUNK")) { const int v = atoi(e); if (v > 0 && v < rows) rows = v; }
    return (int)std::min<long long>(rows, 0x7fffffff);
}

// K loop bound of the hot kernels for an AO dimension: the next multiple of the step-1 K tile (8; the step-2 tiles are 4)
int hot_kdim(int nao) { return (nao + H1_BK - 1) / H1_BK * H1_BK; }

namespace {

// Output tile of a step-1 launch for embedding dimension N: BM rows (128; DMK_ERI_H1_BM=64 asks for 64) by 64 columns (2 x 2 waves)
// or 48 (4 x 1 waves), whichever pads N less; DMK_ERI_H1_BN = 64 | 48 overrides
void half1_hot_tile(int N, int &bm, int &bn) {
    static const int bm_env = [] { const char *e = getenv("DMK_ERI_H1_BM"); return (e && atoi(e) == 64) ? 64 : 128; }();
    bm = bm_env;
    bn = (((N + 47) / 48) * 48 < ((N + 63) / 64) * 64) ? 48 : 64;
    if (const char *e = getenv("DMK_ERI_H1_BN")) { const int v = atoi(e); if (v == 48 || v == 64) bn = v; }
    if (bm != 128) bn = 64;
}

// What launch_half1_hot and launch_half12_hot share: the launch of `q` as the step-1 kernel sees it -- arguments, tile and the flop
// it issues -- or false where the hot kernel declines it.
bool half1_hot_plan(const Half1Launch &q, H1Args &a, int &bm, int &bn, double &flops) {
    const int nL = q.nL, nao = q.nao, N = q.nemb, nslot = q.nslot;
    const int kdim = q.kdim ? q.kdim : nao;             // B holds kdim rows, zero beyond nao
    if (q.nspin < 1 || q.nspin > 2 || nslot < 1 || nslot > 16 || kdim < nao || (kdim % H1_BK) != 0) return false;
    if (!half1_hot_usable(nL, nao, N)) return false;
    if ((reinterpret_cast<uintptr_t>(q.Lpq) | reinterpret_cast<uintptr_t>(q.C) | reinterpret_cast<uintptr_t>(q.Ut)) & 15) return false;
    half1_hot_tile(N, bm, bn);
    // a launch from column tile first_col_tile on: the operand and the output are entered at that column and the tile count shrinks;
    // the kernel keeps the row pitch N and sees tiles 0 .. of a narrower matrix (its column guards compare against N: never taken)
    const int c0 = q.first_col_tile * bn;
    if (q.first_col_tile < 0 || (q.first_col_tile > 0 && (N % bn != 0 || c0 >= N))) return false;
    a.Lpq = reinterpret_cast<const double2 *>(q.Lpq);
    a.Ci = reinterpret_cast<const double2 *>(q.C) + c0;
    a.Ut = reinterpret_cast<double2 *>(q.Ut) + c0;
    a.nL = nL; a.nao = nao; a.nemb = N; a.mrows = nao; a.kdim = kdim;
    a.nblk = (nao + 15) / 16;
    a.tiles_m = (int)(((long long)nL * nao + bm - 1) / bm);          // flat rows: no padding between the nL batches
    a.tiles_n = (N - c0 + bn - 1) / bn;
    a.nspin = q.nspin; a.b_spin_stride = q.ci_spin_stride; a.out_spin_stride = q.ut_spin_stride;
    a.nslot = nslot; a.a_slot_stride = q.a_slot_stride; a.out_slot_stride = q.ut_slot_stride;
    a.b_k_stride = q.ki ? (long long)kdim * N : 0;
    for (int i = 0; i < 16; ++i) a.bk[i] = (q.ki && i < nslot) ? q.ki[i] : 0;
    a.per_slot = (unsigned)(a.tiles_m * a.tiles_n * q.nspin);
    if ((unsigned long long)a.per_slot * (unsigned)nslot > 0x7fffffffull) return false;
    a.nblocks = a.per_slot * (unsigned)nslot;
    flops = 6.0 * (double)a.nblocks * bm * bn * (double)kdim;
    return true;
}

// The W launch that goes with a step-1 launch on the 128 x 64 tile, or false where it is declined (an AO dimension off the K tile,
// an operand off 16 bytes, a shape step 1 would decline).
bool halfw_hot_plan(const HalfWLaunch &q, HWArgs &a, double &flops) {
    if (q.nspin < 1 || q.nspin > 2 || q.nslot < 1 || q.nslot > 16 || (q.nao % H1_BK) != 0 || q.nemb != H2_N || !q.kj || !q.sym) return false;
    if (!half1_hot_usable(q.nL, q.nao, q.nemb)) return false;
    if ((reinterpret_cast<uintptr_t>(q.Lpq) | reinterpret_cast<uintptr_t>(q.C) | reinterpret_cast<uintptr_t>(q.W)) & 15) return false;
    a.Lpq = reinterpret_cast<const double2 *>(q.Lpq);
    a.C = reinterpret_cast<const double2 *>(q.C);
    a.W = reinterpret_cast<double2 *>(q.W);
    a.nL = q.nL; a.nao = q.nao; a.nemb = q.nemb; a.col0 = H2_N - H1_BN;
    a.nspin = q.nspin; a.nslot = q.nslot;
    const long long tiles_m = ((long long)q.nL * q.nao + H1_BM - 1) / H1_BM;
    if (tiles_m * q.nspin * q.nslot > 0x7fffffffLL) return false;
    a.per_slot = (unsigned)(tiles_m * q.nspin);
    a.nblocks = a.per_slot * (unsigned)q.nslot;
    a.symmask = 0;
    for (int i = 0; i < 16; ++i) {
        a.bk[i] = i < q.nslot ? q.kj[i] : 0;
        if (i < q.nslot && q.sym[i]) a.symmask |= 1u << i;
    }
    a.a_slot_stride = q.a_slot_stride; a.w_slot_stride = q.w_slot_stride; a.w_spin_stride = q.w_spin_stride;
    a.c_spin_stride = q.c_spin_stride; a.c_k_stride = (long long)q.nao * q.nemb;
    flops = 6.0 * (double)a.per_slot * __builtin_popcount(a.symmask) * H1_BM * H1_BN * (double)q.nao;
    return true;
}

// The split part of a step-2 launch (q.W set): false where the split kernels decline it.
bool half2w_hot_plan(const Half2Launch &q, const H2Args &a, H2WArgs &w) {
    if (!q.C || !q.ki || a.kdim != a.nao || ((reinterpret_cast<uintptr_t>(q.W) | reinterpret_cast<uintptr_t>(q.C)) & 15)) return false;
    w.W = reinterpret_cast<const double2 *>(q.W);
    w.C = reinterpret_cast<const double2 *>(q.C);
    if (q.w_slot_stride != (long long)q.nL * q.nao * 64) return false;      // the body steps from block to block by this
    for (int i = 0; i < H2_MAXSLOT / 2; ++i) w.ki2[i] = w.kj2[i] = 0;
    for (int i = 0; i < q.nslot; ++i) {
        if (q.ki[i] < 0 || q.ki[i] > 0xffff || q.kj[i] < 0 || q.kj[i] > 0xffff) return false;
        if (a.Cj[i] != w.C + (long long)q.kj[i] * q.nao * H2_N) return false;      // the same operand as the pointer form
        w.ki2[i >> 1] |= (unsigned)q.ki[i] << (16 * (i & 1));
        w.kj2[i >> 1] |= (unsigned)q.kj[i] << (16 * (i & 1));
    }
    w.w_spin_stride = q.w_spin_stride;
    return true;
}

// The same for step 2 on the nemb = 256 kernel: 1 with `a` and `flops` set, 0 where the kernel declines, < 0 for a launch that
// carries fields of the table kernel.
int half2_hot_plan(dmk_ctx *ctx, const Half2Launch &q, H2Args &a, double &flops) {
    if (q.first_row_block != 0 || q.nsub != 1 || q.planes_sub || q.sub_stride != 0)
        return dmk_fail(ctx, DMK_ERR_INVALID, "half2_hot: first_row_block, nsub, planes_sub and sub_stride belong to the table kernel");
    if (!half2_hot_usable(q.nao, q.nemb)) return 0;
    if (!fill_half2_queue(a, q, H2_BK)) return 0;
    a.skip_invariant = q.skip_invariant ? 1 : 0;
    if (q.strip && !q.W) return dmk_fail(ctx, DMK_ERR_INVALID, "half2_hot: the strip order needs the W operand of the split partner term");
    if ((long long)(q.skip_invariant ? 2 : q.strip ? 5 : 4) * q.nL * q.nspin > 0x7fffffffLL) return 0;
    a.nblocks = (unsigned)((q.skip_invariant ? 2 : q.strip ? 5 : 4) * q.nL * q.nspin);
    // 136 of the 256 16 x 16 blocks per L and spin; a block with the time-reversal partner term runs a second segment
    // (without the 16 diagonal blocks when the whole group is symmetrised: they are folded in the epilogue)
    // skip_invariant: types 1 and 3 only -- 32 + 36 = 68 blocks, the partner term without the 8 diagonal blocks of type 3 when folded
    const double nsym = (double)__builtin_popcount(a.symmask);
    // strip order (K6m): warm, type 1 and the strip -- 32 + 32 blocks, each with its partner product; dense, types 0, 1, 2, the
    // corner (10 blocks, 4 of them diagonal) and the strip -- 32 + 32 + 36 + 10 + 32 = 142, the partner term without the 8 + 4 folded
    // diagonal blocks
    const double blocks = q.strip ? (q.skip_invariant ? 64.0 * q.nslot + 64.0 * nsym : 142.0 * q.nslot + (a.fold_diag ? 130.0 : 142.0) * nsym)
                          : q.skip_invariant ? 68.0 * q.nslot + (a.fold_diag ? 60.0 : 68.0) * nsym
                                           : 136.0 * q.nslot + (a.fold_diag ? 120.0 : 136.0) * nsym;
    flops = (q.re_only ? 4.0 : 6.0) * blocks * 256.0 * (double)a.kdim * (double)q.nL * (double)q.nspin;
    return 1;
}

}  // namespace

// Returns 1 if the hot path handled the launch, 0 if the caller must use the generic kernel, < 0 on error.
int launch_half1_hot(dmk_ctx *ctx, const Half1Launch &q, const HalfWLaunch *w) {
    H1Args a;
    int bm, bn;
    double flops;
    if (!half1_hot_plan(q, a, bm, bn, flops)) return 0;
    const bool kp = a.kdim != a.nao;
    if (w) {                              // with the W tiles of the same blocks behind the step-1 workgroups
        HWArgs aw;
        double fw;
        if (kp || bm != H1_BM || bn != H1_BN || !halfw_hot_plan(*w, aw, fw) || (unsigned long long)a.nblocks + aw.nblocks > 0x7fffffffull) return 0;
        FamScope fs(ctx, DMK_FAM_ZGEMM_HALF1);
        fs.mfma_flops(flops + fw);
        hipLaunchKernelGGL(half1w_kernel, dim3(a.nblocks + aw.nblocks), dim3(HNT), 0, ctx->stream, a, aw);
        DMK_CHECK_LAUNCH(ctx);
        return 1;
    }
    FamScope fs(ctx, DMK_FAM_ZGEMM_HALF1);
    fs.mfma_flops(flops);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a); };
    if (bm == 128 && bn == 48) kp ? go(half1_kernel<true, 128, 2, true, 0, true>) : go(half1_kernel<true, 128, 2, true>);
    else if (bm == 128) kp ? go(half1_kernel<true, 128, 2, false, 0, true>) : go(half1_kernel<true, 128, 2, false>);
    else kp ? go(half1_kernel<true, 64, 3, false, 0, true>) : go(half1_kernel<true, 64, 3, false>);
    DMK_CHECK_LAUNCH(ctx);
    return 1;
}

int launch_half2_hot(dmk_ctx *ctx, const Half2Launch &q) {
    H2Args a;
    double flops;
    const int rc = half2_hot_plan(ctx, q, a, flops);
    if (rc != 1) return rc;
    if (q.W) {
        H2WArgs w;
        if (!half2w_hot_plan(q, a, w)) return 0;
        FamScope fs(ctx, DMK_FAM_ZGEMM_HALF2);
        fs.mfma_flops(flops);
        if (q.strip) {
            if (q.re_only) hipLaunchKernelGGL(half2s_kernel<true>, dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a, w);
            else hipLaunchKernelGGL(half2s_kernel<false>, dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a, w);
        }
        else if (q.re_only) hipLaunchKernelGGL(half2w_kernel<true>, dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a, w);
        else hipLaunchKernelGGL(half2w_kernel<false>, dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a, w);
        DMK_CHECK_LAUNCH(ctx);
        return 1;
    }
    FamScope fs(ctx, DMK_FAM_ZGEMM_HALF2);
    fs.mfma_flops(flops);
    if (q.re_only) hipLaunchKernelGGL((half2_kernel<0, true>), dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a);
    else hipLaunchKernelGGL((half2_kernel<0, false>), dim3(a.nblocks), dim3(HNT), 0, ctx->stream, a);
    DMK_CHECK_LAUNCH(ctx);
    return 1;
}

// Would a group of this shape go through the fused launch at all?  (dmk_eri_begin: whether Ut gets its second half.)  The tile rule
// is the one half1_hot_plan applies; launch_half12_hot still decides every launch.
int half12_hot_usable(int nL, int nao, int nemb) {
    if (!half1_hot_usable(nL, nao, nemb) || !half2_hot_usable(nao, nemb)) return 0;
    int bm, bn;
    half1_hot_tile(nemb, bm, bn);
    return bm == H1_BM && bn == H1_BN;
}

// Step 2 of one queued group and step 1 of the next one in ONE launch (half12_kernel).  1: launched; 0: declined -- one of the two
// separate launchers would decline, or step 1 would not run the 128 x 64 tile -- and nothing was launched; < 0: error.
int launch_half12_hot(dmk_ctx *ctx, const Half2Launch &q2, const Half1Launch &q1, const HalfWLaunch *w1) {
    H2Args a2;
    H1Args a1;
    int bm, bn;
    double f1, f2;
    const int rc = half2_hot_plan(ctx, q2, a2, f2);
    if (rc != 1) return rc;
    if (!half1_hot_plan(q1, a1, bm, bn, f1) || bm != H1_BM || bn != H1_BN) return 0;
    const bool kp = a1.kdim != a1.nao;
    if ((q2.W != nullptr) != (w1 != nullptr)) return 0;          // one order for the whole transform
    if (w1) {
        H2WArgs w2;
        HWArgs aw;
        double fw;
        if (kp || !half2w_hot_plan(q2, a2, w2) || !halfw_hot_plan(*w1, aw, fw)) return 0;
        const unsigned long long nbw = (unsigned long long)a2.nblocks + a1.nblocks + aw.nblocks;
        if (nbw > 0x7fffffffull) return 0;
        FamScope fs(ctx, DMK_FAM_ZGEMM_HALF2);
        fs.share_with(DMK_FAM_ZGEMM_HALF1, f2, f1 + fw);
        if (q2.strip) {
            if (q2.re_only) hipLaunchKernelGGL(half12s_kernel<true>, dim3((unsigned)nbw), dim3(HNT), 0, ctx->stream, a2, w2, a1, aw);
            else hipLaunchKernelGGL(half12s_kernel<false>, dim3((unsigned)nbw), dim3(HNT), 0, ctx->stream, a2, w2, a1, aw);
        }
        else if (q2.re_only) hipLaunchKernelGGL(half12w_kernel<true>, dim3((unsigned)nbw), dim3(HNT), 0, ctx->stream, a2, w2, a1, aw);
        else hipLaunchKernelGGL(half12w_kernel<false>, dim3((unsigned)nbw), dim3(HNT), 0, ctx->stream, a2, w2, a1, aw);
        DMK_CHECK_LAUNCH(ctx);
        return 1;
    }
    const unsigned long long nb = (unsigned long long)a2.nblocks + a1.nblocks;
    if (nb > 0x7fffffffull) return 0;
    // One event interval for both families: it is split between them in proportion to the flop each side
    // issues, so both show the combined rate of the launch -- a true fraction of the peak -- and their sum is the launch's time;
    // each family counts one launch and the flop its separate launch would have reported.
    FamScope fs(ctx, DMK_FAM_ZGEMM_HALF2);
    fs.share_with(DMK_FAM_ZGEMM_HALF1, f2, f1);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(HNT), 0, ctx->stream, a2, a1); };
    if (q2.re_only) kp ? go(half12_kernel<true, true>) : go(half12_kernel<true, false>);
    else kp ? go(half12_kernel<false, true>) : go(half12_kernel<false, false>);
    DMK_CHECK_LAUNCH(ctx);
    return 1;
}

int half2_hot_usable(int nao, int nemb) { return hot_enabled() && nemb == H2_N && nao >= 3 * H2_BK; }
int half2_hot_maxslot() { return H2_MAXSLOT; }
