// The ERI pipeline handle (dmk_eri) and the few internal functions that eri_engine.hip (begin / finish, block queue, kL,
// contractions) and eri_cache.hip (dmk_eri_cache: the invariant planes and the invariant block of the result) share.
#pragma once
#include "common.h"
#include "kmesh.h"
#include "devres.h"
#include <cstdlib>
#include <algorithm>

struct dmk_eri {
    dmk_ctx *ctx;
    Mesh mesh;
    int nao, naux, nemb, spin, tr;
    int64_t npair;
    const double2 *C;     // spin x nk x nao x nemb
    // AO dimensions off the K tile of the hot kernels (8): they loop over kdim = hot_kdim(nao) against Ch, the pipeline's own copy
    // of C with kdim rows per k point, zero beyond nao (Ch == C and kdim == nao when nao is on the tile)
    int kdim = 0;
    const double2 *Ch = nullptr;
    DevMem Cpad;
    double *eri;
    // PLANE GEOMETRY: a Re or Im plane has `pr` rows (naux rounded up to the K tile of the contraction kernel, 8) of `pl` doubles
    // (npair rounded up to even).  The padding rows and the padding column are never written by the half transform and stay zero
    // from the memset at the start of a kL, so the contraction always runs on the LDS-DMA kernel with its symmetric launch --
    // up to round 5 an auxiliary basis off the tile (naux 411) or an odd pair count (nemb 250) fell to the register-staged kernel
    // without the symmetric saving.  pr == naux and pl == npair for shapes on the tile: the layout of rounds 1 - 5.
    int64_t pr = 0, pl = 0;
    DevMem planes;              // spin x (2 pr) x pl (bytes(): its capacity -- it may come from the context's cache, like Ut)
    DevMem planes_view;         // dmk_eri_planes with a padded geometry: compact (spin, 2, naux, npair) copy
    DevMem Ut;                  // lchunk x nao x nemb
    int lchunk;
    int hot_rows = 0;     // auxiliary rows per hot step-1 launch (half1_hot_max_rows): blocks of 4 GiB and more go in ranges of L
    int use_3m = 1;       // Karatsuba complex product in the generic half transform (DMK_ERI_3M=0 restores 4M)
    // hot path: step-1 outputs of up to `group` consecutive AO blocks are queued and transformed by ONE
    // step-2 launch whose accumulators (and tril-pack epilogue) are shared by all of them
    int group = 1;
    DevMem imag;              // flags & 2 (no time reversal): Im of the contraction, spin_pair x npair^2, for dmk_eri_imag_norm
    bool hot256 = false;      // step 2 by the nemb = 256 kernel (zhot.hip) instead of the table-driven one (zhot_tab.hip)
    // THE BLOCK QUEUE.  `pending` blocks are queued for the next step-2 launch, k points and partner flag of each in ki / kj / sym.
    // block ring (dmk_eri_block_ring / dmk_eri_push_ring_slot): `group` AO-block buffers owned by the pipeline; blocks
    // written there are queued WITHOUT running step 1, and the flush runs ONE step-1 launch over all of them
    // PRODUCER STREAM of the ring (dmk_eri_ring_slot): the ring is double buffered and device-side producers of group g + 1
    // (a generator kernel, a decompressor) run on `gen_stream` while the compute stream transforms group g.  Ordering by events:
    // ev_free[half] = step 1 of the group that last used that half has run (recorded on the compute stream; the producer stream
    // waits on it before the first fill of the half), ev_gen[half] = the fills of the pending group (recorded on the producer
    // stream after every fill; step 1 of that group waits on it).
    struct Queue {
        int pending = 0;
        int kj[16], sym[16], ki[16];
        DevMem ring;
        int ring_pending = 0;       // queued ring slots whose step 1 has not run yet (they are the first `ring_pending` slots)
        const double2 *resident_src = nullptr;   // dmk_eri_push_resident: the queued group is read in place from here, not from the ring
        DevStream gen_stream;
        DevEvent ev_gen[2], ev_free[2];
        int ring_halves = 1;        // 2 when the ring is double buffered
        int fill_half = 0;          // half of the pending group
        int next_half = 0;          // half the next group of a ring_slot producer will fill
        bool gen_pending = false;   // the pending group was (partly) filled on the producer stream
        int slot_reserved = -1;     // ring slot handed out by dmk_eri_ring_slot and not pushed yet (-1: none)
        // one more block in the next free slot; `from_ring`: its step 1 has not run (a ring slot or a resident block)
        void push(int ki_, int kj_, int sym_, bool from_ring) {
            ki[pending] = ki_; kj[pending] = kj_; sym[pending] = sym_ ? 1 : 0;
            pending += 1; ring_pending += from_ring ? 1 : 0;
        }
        // step 1 of the ring slots / resident blocks has been enqueued
        void step1_done() {
            resident_src = nullptr; ring_pending = 0; gen_pending = false;
            fill_half = 0;          // a producer on the compute stream (no dmk_eri_ring_slot) always uses half 0
        }
    } queue;
    int cur_kL = -1;
    double flops_half = 0.0, flops_contract = 0.0;
    // plane STACK (dmk_eri_stack): nslots > 1 defers the contraction -- the planes of up to nslots kL stay resident, weight-2 kL
    // fill slots from the front, weight-1 kL (only their Re halves are contracted) from the back, and one K-stacked GEMM per
    // weight class and spin block contracts them all (dmk_eri_contract, or automatically when the stack is full / at finish)
    int nslots = 1, n_w2 = 0, n_w1 = 0, cur_slot = 0, cur_weight = 1;
    // A kL that is its own time-reversal partner (weight 1) only ever contributes the REAL part of its planes (eri_transform.py:453-455,
    // 464-467), so step 2 of its blocks computes Re S alone -- two real products instead of the three of 3M (zhot_common.h RE).
    // Known when the kL is begun with its weight (dmk_eri_begin_kL_weighted); dmk_eri_begin_kL keeps the full product.
    bool re_only = false;
    // host feed (dmk_eri_push_block_host): two device staging blocks filled on a copy stream while the compute stream
    // transforms the other one; created on first use
    HostFeed feed;
    DevMem tstage;                   // conjugate-transposed copy of a block uploaded for the swapped pair
    // sub-group plane copies of the table-driven step 2 (zhot_tab.hip H2TArgs): run p >= 1 of a launch accumulates into copy
    // p - 1 ([spin][2 naux][npair] each); they are zeroed when a kL begins and added to its planes, in order, when it ends
    DevMem sub_planes;
    int nsub_max = 1, sub_used = 1;
    // Freivalds probe (dmk_eri_probe, eri_probe.hip): yref[b] += w X_a^T (X_b x) for every kL that is contracted
    const double *probe_x = nullptr;
    double *probe_y = nullptr;
    bool probe_pending = false;      // planes entered the stack since the probe last ran over it
    // iteration-invariant planes (dmk_eri_attach_cache / _cols): inv_warm -- the region of the current kL came from the cache and
    // step 2 runs the two-type grid (nemb = 256 kernel) or the table without the region's block rows (table kernel); inv_save -- a
    // cold kL begun with a key, whose region goes into a new entry when it ends.  inv_A: 0 with the region of the nemb = 256 kernel,
    // else the table path's region -- the pairs b <= a < inv_A (a multiple of 16), the prefix of every plane row.
    dmk_eri_cache *cache = nullptr;
    bool inv_warm = false, inv_save = false;
    int inv_A = 0;
    // invariant block of the result (dmk_eri_attach_cache_block): blk_S > 0 -- armed, the corner of blk_S x blk_S tiles of every spin
    // block is a function of columns [0, blk_ne) of C alone.  slot_keys: what the planes resident in each stack slot were begun
    // with (keyed: by dmk_eri_begin_kL_cached with the cache attached) -- the block's key is made of them.
    int blk_S = 0, blk_ne = 0;
    struct SlotKey { int kL; uint64_t key; int weight, re_only; bool keyed; };
    std::vector<SlotKey> slot_keys;
    uint64_t cur_key = 0;
    bool cur_keyed = false;
    // FUSED LAUNCHES (zhot.hip half12_kernel): inside a kL, step 2 of a group whose step 1 runs at its flush (ring
    // slots, resident blocks) is not launched at once but kept in `deferred` and goes out in ONE launch with step 1 of the next
    // group; eri_drain launches it alone where there is no next group.  Ut then has two halves, ut_half_elems apart, each with
    // the rows of the K padding behind it, and consecutive deferred groups alternate between them: step 1 of group g + 1 never
    // writes what step 2 of group g reads.  Everything step 2 of a group needs is held by value.
    struct Step2Group {
        Half2Launch q;              // (Cj and sym stay unset here: desc() points them at the arrays below)
        const void *cj[16]; int sym[16], kj[16], ki[16];
        const double2 *ut = nullptr;
        int n = 0, slot = 0;
        bool inv_warm = false, live = false;
        Half2Launch desc() const { Half2Launch r = q; r.Cj = cj; r.sym = sym; if (r.W) { r.ki = ki; r.kj = kj; } return r; }
    };
    bool fuse = false;            // DMK_ERI_FUSE (default on), the nemb = 256 kernel, one range of L per block, memory for both halves
    int ut_half = 0;              // the half the group being queued is transformed into
    size_t ut_half_elems = 0;
    Step2Group deferred;
    int64_t fused_launches = 0;
    // SPLIT STEP 1 (dmk_eri_begin flags bit 3): the partner term of the type-1 workgroups of step 2 is computed from
    // W[L][p][n] = sum_q Lpq[L][p][q] C_j[q][192 + n] and conj(C_i) -- for EVERY kL of the transform, warm or dense, so that the two
    // stay bit-identical -- and a warm kL runs step 1 over columns [128,256) only.  W sits behind the halves of Ut in the same
    // workspace, one half per half of Ut, [spin][group][naux nao][64] each.
    bool split1 = false;
    // STRIP STEP 1 (flags bit 4; implies split1, granted with it): step 2 covers the triangle [128,256)^2 with a strip
    // (rows [192,256) x cols [128,256), the W partner) and a corner ([128,192)^2) in place of type 3, the cached region grows by the
    // corner to the pairs b <= a < 192, and a warm kL runs step 1 over columns [192,256) only (tile 3 of four) plus W.
    bool strip1 = false;
    double2 *Wbuf = nullptr;
    size_t w_half_elems = 0;
    dmk_eri(dmk_ctx *c, const int m[3]) : ctx(c), mesh(m) {}

    double2 *ut_cur() const { return Ut.get<double2>() + (size_t)ut_half * ut_half_elems; }
    double2 *w_cur() const { return Wbuf + (size_t)ut_half * w_half_elems; }
    size_t w_slot_elems() const { return (size_t)naux * nao * 64; }                             // W of one queued block and spin

    double *slot_planes(int slot, int spin_idx) const {
        return planes.get<double>() + ((size_t)spin_idx * nslots + slot) * 2 * (size_t)pr * pl;
    }
    size_t slot_elems() const { return (size_t)naux * nao * nemb; }                              // Ut of one queued block and spin
    long long planes_spin_stride() const { return (long long)nslots * 2LL * pr * pl; }           // spin 0 -> spin 1 of the same slot
    long long c_spin_stride() const { return (long long)mesh.nk * kdim * nemb; }                 // spin 0 -> spin 1 of Ch
    int spin_blocks() const { return spin == 2 ? 3 : 1; }
    // algorithmic flops of both half-transform steps of one AO block
    double block_flops() const {
        return (double)spin * (8.0 * naux * (double)nao * nao * nemb + 8.0 * naux * (double)nao * nemb * nemb);
    }
    // The resident slots of one weight class: weight-2 kL are adjacent from the front and their Re and Im planes form one
    // contiguous K range; weight-1 kL sit at the back and only their Re halves enter: K segments of pr rows, one slot apart.
    struct WeightClass { int first, n, seg_rows; double weight; };
    WeightClass weight_class(int w) const {
        return w == 2 ? WeightClass{0, n_w2, (int)(2 * pr), 2.0} : WeightClass{nslots - n_w1, n_w1, (int)pr, 1.0};
    }
};

// eri_engine.hip, used by the cache
int eri_begin_kL_impl(dmk_eri *h, int kL, int weight);
DgemmTn planes_gemm(const dmk_eri *h, int slot, int spin_a, int spin_b, int K, double alpha, double *C, int stacked_rows = 0);
// eri_cache.hip, the hooks of the engine: the region of a cold keyed kL when it ends, and the invariant block of the result before
// and after a whole stacked contraction
int inv_save_entry(dmk_eri *h);
int blk_decide(dmk_eri *h, int kchunk_w2, int kchunk_w1, int *skip, bool *save, uint64_t *key);
int blk_finish(dmk_eri *h, bool warm, bool save, uint64_t key);
