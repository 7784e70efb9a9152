// The iteration-invariant part of the ERI pipeline (dmk_eri_cache): the invariant step-2 planes, the invariant block of the result
// and their three small kernels.  The pipeline itself is eri_engine.hip; eri_engine.h is what the two share.  The cache owns its
// device buffers (devres.h): forgetting an entry frees it, after the stream has been synchronised where it may still be in use.
#include "eri_engine.h"

// =============================================================================================
// iteration-invariant step-2 planes
// =============================================================================================
// The nemb = 256 step-2 kernel (zhot.hip) gives the pairs (a, b) with a < 192 that its workgroup types 0 and 2 own to workgroups of
// their own: the prefix [0, 8256) of the packed pair index (triangle [0,128)^2) and, for a in [128,192), the 128 entries from
// a (a + 1) / 2 (rows [128,192) x cols [0,128)).  They are a function of columns [0,192) of C_ao_emb, the DF blocks and the visiting
// plan alone; a cache entry holds that region of one kL's finished planes, INV_ROW doubles per auxiliary row and plane.
//
// The table-driven kernel (zhot_tab.hip) owns blocks by data: with A = 16 floor(ninv / 16) for `ninv` invariant leading columns, the
// 16 x 16 blocks of block rows below A / 16 hold exactly the pairs b <= a < A -- the prefix [0, A (A + 1) / 2) of every plane row, a
// function of columns [0, A) alone.  A warm kL copies the prefix back and launches the table without those block rows.
//
// In the strip order (K6m) the corner [128,192)^2 has a workgroup type of its own too, and the region is every pair b <= a < 192: the
// contiguous prefix [0, INV_STRIP_ROW) of every plane row, copied like the table path's.
constexpr int INV_COLS = 192, INV_PREFIX = 8256, INV_ROW = INV_PREFIX + 64 * 128, INV_STRIP_ROW = 192 * 193 / 2;

struct dmk_eri_cache {
    dmk_ctx *ctx;
    size_t budget = 0, held = 0;
    // what the entries were built from: the shape, the region (tab_A: 0 = that of the nemb = 256 kernel, else A of the table path)
    // and columns [0, ncols) of C_ao_emb ([spin nk nao][ncols] c128; ncols = INV_COLS or A)
    bool have_cols = false;
    int shape[8] = {0, 0, 0, 0, 0, 0, 0, 0};    // mesh, nao, naux, nemb, spin, order of step 2 (0 old, 1 split step 1, 2 strip)
    int tab_A = 0, ncols = 0;
    DevMem cols;
    size_t cols_rows = 0;
    DevMem flag;                                 // device: mismatch flag of the column compare (one int)
    struct Entry { int kL; uint64_t key; int re_only; DevMem buf; };
    std::vector<Entry> entries;
    long long hits = 0, misses = 0, drops = 0;
    // The invariant block of the result (one entry): the corner [0, blk_S 128)^2 of every spin block, [blocks][blk_S 128][blk_S 128],
    // built from columns [0, blk_ne) of C_ao_emb -- [0, ncols) are the stored `cols`, [blk_lo, blk_ne) (blk_lo = ncols when the
    // block was set up) are kept in blk_cols ([rows][blk_ne - blk_lo]).  blk_bytes() counts against the budget while blk_buf is held.
    int blk_ne = 0, blk_lo = 0, blk_S = 0;
    DevMem blk_cols, blk_buf;
    size_t blk_bytes() const { return blk_buf.bytes(); }
    bool blk_valid = false;
    uint64_t blk_key = 0;
    long long blk_hits = 0, blk_misses = 0;
    explicit dmk_eri_cache(dmk_ctx *c) : ctx(c) {}
};

namespace {
// flag = 1 if any of the 128-bit patterns of columns [0, ncols) of C ([rows][nemb]) differs from cols ([rows][ncols]); n = rows x ncols
// (col0: the first compared column)
__global__ void inv_cols_compare_kernel(long long n, int nemb, int ncols, int col0, const ulonglong2 *__restrict__ Cm,
                                        const ulonglong2 *__restrict__ cols, int *__restrict__ flag) {
    bool diff = false;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        const long long row = t / ncols;
        const int col = (int)(t - row * ncols);
        const ulonglong2 x = Cm[row * nemb + col0 + col], y = cols[t];
        diff = diff || x.x != y.x || x.y != y.y;
    }
    if (diff) *flag = 1;
}

// The invariant region of the planes of one kL <-> a cache entry.  grid (chunks of the region row, auxiliary row L, spin x plane);
// entry: [spin][plane][naux][row], planes: (ri * pr + L) * pl + a (a + 1) / 2 + b per spin.  A region row is the prefix [0, prefix)
// of the plane row and then, for a = 128, 129, ..., 128 entries from a (a + 1) / 2 (the nemb = 256 kernel: prefix INV_PREFIX of
// INV_ROW; the table path: the prefix alone, row == prefix).  Consecutive threads move consecutive doubles on both sides.
template <bool TO_PLANES>
__global__ void inv_region_copy_kernel(double *__restrict__ planes, double *__restrict__ entry, long long planes_spin_stride,
                                       long long pr, long long pl, int naux, int nplanes, int row, int prefix) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= row) return;
    const int L = blockIdx.y, s = blockIdx.z / nplanes, ri = blockIdx.z - s * nplanes;
    long long pair = e;
    if (e >= prefix) {
        const int a = 128 + ((e - prefix) >> 7), b = (e - prefix) & 127;
        pair = (long long)a * (a + 1) / 2 + b;
    }
    double *p = planes + (long long)s * planes_spin_stride + ((long long)ri * pr + L) * pl + pair;
    double *q = entry + (((long long)s * nplanes + ri) * naux + L) * row + e;
    if (TO_PLANES) *p = *q; else *q = *p;
}

// The corner [0, n)^2 (n a multiple of 128) of `blocks` spin blocks of the ERI (row pitch np, blocks blk_stride doubles apart) <-> the
// block entry [blocks][n][n].  One workgroup per 1024-column chunk of one row (cpr chunks per row): consecutive threads move
// consecutive doubles, plain loads and stores.  MODE 0: corner -> entry, 1: entry -> corner, 2: flag = 1 if any bit of the corner is set.
constexpr int BLK_CHUNK = 1024;
template <int MODE>
__global__ void blk_corner_kernel(double *__restrict__ eri, double *__restrict__ entry, long long n, long long np, long long blk_stride,
                                  int cpr, int *__restrict__ flag) {
    const long long id = blockIdx.x;
    const int cx = (int)(id % cpr);
    const long long rr = id / cpr, r = rr % n, b = rr / n;
    double *p = eri + b * blk_stride + r * np;
    double *q = entry + (b * n + r) * n;
    bool set = false;
#pragma unroll
    for (int i = 0; i < BLK_CHUNK / 256; ++i) {
        const long long c = (long long)cx * BLK_CHUNK + i * 256 + threadIdx.x;
        if (c >= n) continue;
        if (MODE == 0) q[c] = p[c];
        else if (MODE == 1) p[c] = q[c];
        else set = set || __double_as_longlong(p[c]) != 0;
    }
    if (MODE == 2 && set) *flag = 1;
}

// doubles per auxiliary row and plane of a cache entry of this pipeline's region
int inv_row_len(const dmk_eri *h) { return h->inv_A ? h->inv_A * (h->inv_A + 1) / 2 : h->strip1 ? INV_STRIP_ROW : INV_ROW; }

// One verdict of a device-side check: the cache's flag is zeroed, `launch` enqueues a kernel that sets it, and the flag is read
// back (the one synchronisation of the check).
template <class Launch> int device_flag(dmk_ctx *ctx, dmk_eri_cache *c, int *flag, Launch &&launch) {
    DMK_HIP(ctx, hipMemsetAsync(c->flag.get<void>(), 0, sizeof(int), ctx->stream));
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        launch();
        DMK_CHECK_LAUNCH(ctx);
    }
    *flag = 1;
    DMK_HIP(ctx, hipMemcpyAsync(flag, c->flag.get<void>(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DMK_OK;
}

// Are columns [col0, col0 + ncols) of the pipeline's C_ao_emb `stored` ([rows of the cache][ncols]) bit for bit?  The bit patterns
// of every (spin, k, AO row) are reduced to one flag on the device and read back once.
int cols_same(dmk_eri *h, dmk_eri_cache *c, const double2 *stored, int col0, int ncols, bool *same) {
    const long long n = (long long)c->cols_rows * ncols;
    int diff = 1;
    int rc = device_flag(h->ctx, c, &diff, [&] {
        const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 4096);
        hipLaunchKernelGGL(inv_cols_compare_kernel, dim3(grid), dim3(256), 0, h->ctx->stream, n, h->nemb, ncols, col0,
                           reinterpret_cast<const ulonglong2 *>(h->C), reinterpret_cast<const ulonglong2 *>(stored), c->flag.get<int>());
    });
    *same = diff == 0;
    return rc;
}
}  // namespace

static int inv_region_copy(dmk_eri *h, double *entry, bool to_planes) {
    dmk_ctx *ctx = h->ctx;
    const int nplanes = h->re_only ? 1 : 2;
    const int row = inv_row_len(h), prefix = (h->inv_A || h->strip1) ? row : INV_PREFIX;
    const dim3 grid((row + 255) / 256, (unsigned)h->naux, (unsigned)(h->spin * nplanes));
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(to_planes ? inv_region_copy_kernel<true> : inv_region_copy_kernel<false>, grid, dim3(256), 0, ctx->stream,
                       h->slot_planes(h->cur_slot, 0), entry, h->planes_spin_stride(), (long long)h->pr, (long long)h->pl, h->naux, nplanes,
                       row, prefix);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// end of a cold kL begun with a key: its finished region becomes a cache entry when the budget holds it (else the kL stays dense)
int inv_save_entry(dmk_eri *h) {
    dmk_eri_cache *c = h->cache;
    h->inv_save = false;
    if (!c) return DMK_OK;
    const size_t bytes = (size_t)h->spin * (h->re_only ? 1 : 2) * h->naux * inv_row_len(h) * sizeof(double);
    if (c->held + c->blk_bytes() + bytes > c->budget) return DMK_OK;
    DevMem buf;
    if (buf.alloc(h->ctx, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return DMK_OK;
    }
    if (int rc = inv_region_copy(h, buf.get<double>(), false)) return rc;
    c->entries.push_back({h->cur_kL, h->cur_key, h->re_only ? 1 : 0, std::move(buf)});
    c->held += bytes;
    return DMK_OK;
}

// forget the invariant block of the result and the columns kept for it
static void blk_drop(dmk_eri_cache *c) {
    if (c->blk_buf || c->blk_cols) (void)hipStreamSynchronize(c->ctx->stream);
    c->blk_buf.reset();
    c->blk_cols.reset();
    c->blk_valid = false;
    c->blk_ne = c->blk_lo = c->blk_S = 0;
}

// forget every entry (and, with `cols`, the columns they were built from and the block of the result, which rests on them too)
static void inv_cache_clear(dmk_eri_cache *c, bool cols) {
    if (cols) blk_drop(c);
    if (!c->entries.empty() || (cols && c->cols)) (void)hipStreamSynchronize(c->ctx->stream);
    c->drops += (long long)c->entries.size();
    c->entries.clear();
    c->held = 0;
    if (cols) {
        c->cols.reset();
        c->cols_rows = 0;
        c->have_cols = false;
    }
}

int dmk_eri_cache_create(dmk_ctx *ctx, int64_t budget_bytes, dmk_eri_cache **out) {
    if (!ctx || !out) return DMK_ERR_INVALID;
    *out = nullptr;
    size_t free_b = 0, total_b = 0;
    DMK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    dmk_eri_cache *c = new dmk_eri_cache(ctx);
    c->budget = std::min<size_t>(budget_bytes > 0 ? (size_t)budget_bytes : 0, free_b / 4);
    if (c->flag.alloc(ctx, sizeof(int)) != hipSuccess) {
        delete c;
        return dmk_fail(ctx, DMK_ERR_NOMEM, "eri_cache_create: allocation failed");
    }
    *out = c;
    return DMK_OK;
}

int dmk_eri_cache_drop(dmk_eri_cache *cache) {
    if (!cache) return DMK_ERR_INVALID;
    inv_cache_clear(cache, true);
    return DMK_OK;
}

int dmk_eri_cache_destroy(dmk_eri_cache *cache) {
    if (!cache) return DMK_OK;
    inv_cache_clear(cache, true);
    delete cache;
    return DMK_OK;
}

int dmk_eri_cache_stats(const dmk_eri_cache *cache, int64_t stats[5]) {
    if (!cache || !stats) return DMK_ERR_INVALID;
    stats[0] = cache->hits; stats[1] = cache->misses; stats[2] = (int64_t)cache->entries.size();
    stats[3] = (int64_t)cache->held; stats[4] = cache->drops;
    return DMK_OK;
}

// What both attach entry points share once the path and its region are known: tab_A = 0 and ncols = INV_COLS (nemb = 256 kernel) or
// tab_A = ncols = A (table kernel).  The stored columns are compared bitwise on the device; any difference in the shape, the region
// or a single bit drops every entry.
static int inv_attach(dmk_eri *h, dmk_eri_cache *cache, int tab_A, int ncols, int *attached) {
    dmk_ctx *ctx = h->ctx;
    const int shape[8] = {h->mesh.n[0], h->mesh.n[1], h->mesh.n[2], h->nao, h->naux, h->nemb, h->spin, h->strip1 ? 2 : h->split1 ? 1 : 0};
    const size_t rows = (size_t)h->spin * h->mesh.nk * h->nao;
    bool same = cache->have_cols && cache->cols_rows == rows && cache->tab_A == tab_A && cache->ncols == ncols;
    for (int i = 0; i < 8 && same; ++i) same = cache->shape[i] == shape[i];
    if (same) {
        if (int rc = cols_same(h, cache, cache->cols.get<double2>(), 0, ncols, &same)) return rc;
    }
    if (!same) {
        inv_cache_clear(cache, true);
        if (cache->cols.alloc(ctx, rows * ncols * sizeof(double2)) != hipSuccess) {
            (void)hipGetLastError();
            return DMK_OK;                          // no room for the columns: the pipeline stays dense
        }
        DMK_HIP(ctx, hipMemcpy2DAsync(cache->cols.get<void>(), (size_t)ncols * sizeof(double2), h->C, (size_t)h->nemb * sizeof(double2),
                                      (size_t)ncols * sizeof(double2), rows, hipMemcpyDeviceToDevice, ctx->stream));
        for (int i = 0; i < 8; ++i) cache->shape[i] = shape[i];
        cache->tab_A = tab_A;
        cache->ncols = ncols;
        cache->cols_rows = rows;
        cache->have_cols = true;
    }
    h->cache = cache;
    h->inv_A = tab_A;
    if (attached) *attached = 1;
    return DMK_OK;
}

int dmk_eri_attach_cache(dmk_eri *h, dmk_eri_cache *cache, int *attached) {
    if (!h || !cache) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (attached) *attached = 0;
    if (cache->ctx != ctx) return dmk_fail(ctx, DMK_ERR_INVALID, "eri_attach_cache: the cache belongs to another context");
    if (h->cur_kL >= 0) return dmk_fail(ctx, DMK_ERR_STATE, "eri_attach_cache: a kL is in progress");
    // only the grouped nemb = 256 path has the workgroup types the region is made of; the partner term and Re-only planes need time reversal
    if (!h->hot256 || h->group <= 1 || !h->tr || h->imag || h->sub_planes || h->nemb != 256) return DMK_OK;
    return inv_attach(h, cache, 0, INV_COLS, attached);
}

int dmk_eri_attach_cache_cols(dmk_eri *h, dmk_eri_cache *cache, int ninv, int *attached, int *cols_used) {
    if (!h || !cache) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (attached) *attached = 0;
    if (cols_used) *cols_used = 0;
    if (cache->ctx != ctx) return dmk_fail(ctx, DMK_ERR_INVALID, "eri_attach_cache_cols: the cache belongs to another context");
    if (h->cur_kL >= 0) return dmk_fail(ctx, DMK_ERR_STATE, "eri_attach_cache_cols: a kL is in progress");
    int att = 0, rc;
    if (h->hot256) {
        // the region of the nemb = 256 kernel is fixed: all of its INV_COLS columns must be invariant
        if (ninv < INV_COLS) return DMK_OK;
        rc = dmk_eri_attach_cache(h, cache, &att);
        if (rc == DMK_OK && att && cols_used) *cols_used = INV_COLS;
    } else {
        // the grouped table path; the partner term and Re-only planes need time reversal, sub-group copies hold parts of the planes
        if (h->group <= 1 || !h->tr || h->imag || h->sub_planes || !half2_tab_usable(h->nao, h->nemb)) return DMK_OK;
        const int A = 16 * (std::min(ninv, h->nemb) / 16);
        if (A < 16) return DMK_OK;
        rc = inv_attach(h, cache, A, A, &att);
        if (rc == DMK_OK && att && cols_used) *cols_used = A;
    }
    if (attached) *attached = att;
    return rc;
}

// =============================================================================================
// the invariant block of the result
// =============================================================================================

int dmk_eri_cache_block_stats(const dmk_eri_cache *cache, int64_t stats[4]) {
    if (!cache || !stats) return DMK_ERR_INVALID;
    stats[0] = cache->blk_hits; stats[1] = cache->blk_misses;
    stats[2] = cache->blk_valid ? (int64_t)cache->blk_bytes() : 0; stats[3] = cache->blk_valid ? cache->blk_S : 0;
    return DMK_OK;
}

// Would every launch of the stacked contraction run on the kernel that can leave tiles out?  Both weight classes (a class differs
// in its segment length) and both spin operands (a launch of a later K chunk starts whole slots further on: the same alignment).
static bool blk_can_skip(const dmk_eri *h) {
    for (int w = 2; w >= 1; --w) {
        const dmk_eri::WeightClass wc = h->weight_class(w);
        for (int s = 0; s < h->spin; ++s)
            if (!dgemm_tn_can_skip(planes_gemm(h, 0, s, s, wc.seg_rows, wc.weight, h->eri, wc.seg_rows))) return false;
    }
    return true;
}

static unsigned blk_grid(const dmk_eri *h, long long n, int *cpr) {
    *cpr = (int)((n + BLK_CHUNK - 1) / BLK_CHUNK);
    return (unsigned)((long long)h->spin_blocks() * n * *cpr);
}

int dmk_eri_attach_cache_block(dmk_eri *h, dmk_eri_cache *cache, int ninv, int *tiles) {
    if (!h || !cache) return DMK_ERR_INVALID;
    dmk_ctx *ctx = h->ctx;
    if (tiles) *tiles = 0;
    h->blk_S = h->blk_ne = 0;
    if (cache->ctx != ctx) return dmk_fail(ctx, DMK_ERR_INVALID, "eri_attach_cache_block: the cache belongs to another context");
    if (h->cur_kL >= 0) return dmk_fail(ctx, DMK_ERR_STATE, "eri_attach_cache_block: a kL is in progress");
    if (h->cache != cache || !cache->have_cols) return DMK_OK;              // the planes of this pipeline are not keyed by this cache
    if (!h->eri || !h->tr || h->imag) return DMK_OK;
    const int n_e = std::min(ninv, h->nemb);
    if (n_e < 1) return DMK_OK;
    const long long P = (long long)n_e * (n_e + 1) / 2;
    const int S = (int)(P / 128);
    if (S < 1) return DMK_OK;
    const long long n = (long long)S * 128;
    if ((long long)h->spin_blocks() * n * ((n + BLK_CHUNK - 1) / BLK_CHUNK) > 0x7fffffffLL) return DMK_OK;    // grid of the corner kernels
    if (!blk_can_skip(h)) return DMK_OK;
    // columns [0, ncols) were compared when the planes attached (a difference there dropped the block too); the rest of [0, n_e) here
    const int lo = std::min(cache->ncols, n_e), extra = n_e - lo;
    const size_t rows = cache->cols_rows;
    bool same = cache->blk_ne == n_e && cache->blk_lo == lo && (extra == 0 || cache->blk_cols);
    if (same && extra > 0) {
        if (int rc = cols_same(h, cache, cache->blk_cols.get<double2>(), lo, extra, &same)) return rc;
    }
    if (!same) {
        blk_drop(cache);
        if (extra > 0) {
            if (cache->blk_cols.alloc(ctx, rows * extra * sizeof(double2)) != hipSuccess) {
                (void)hipGetLastError();
                return DMK_OK;                      // no room for the columns: the contraction stays dense
            }
            DMK_HIP(ctx, hipMemcpy2DAsync(cache->blk_cols.get<void>(), (size_t)extra * sizeof(double2), h->C + lo, (size_t)h->nemb * sizeof(double2),
                                          (size_t)extra * sizeof(double2), rows, hipMemcpyDeviceToDevice, ctx->stream));
        }
        cache->blk_ne = n_e;
        cache->blk_lo = lo;
    }
    h->blk_S = S;
    h->blk_ne = n_e;
    if (tiles) *tiles = S;
    return DMK_OK;
}

static inline uint64_t blk_mix(uint64_t hsh, uint64_t v) {       // FNV-1a over the eight bytes of v
    for (int i = 0; i < 8; ++i) {
        hsh ^= (v >> (8 * i)) & 0xffu;
        hsh *= 0x100000001b3ULL;
    }
    return hsh;
}

// Before a whole stacked contraction of an armed pipeline: *skip = S (warm: every launch leaves the corner out, blk_finish copies
// the entry back), or *save (cold: dense, blk_finish keeps the corner), or neither (dense, nothing kept).  The corner of the result
// is the kept one only when the same planes are summed in the same order on top of zeros: every resident kL must carry a key, the
// key of the block covers them in contraction order with the slots-per-launch rule, and the corner of the ERI is checked on the
// device to be zero bit for bit -- which also turns away a caller that did not zero the buffer, the later rounds of a stack
// smaller than the kL list and another engine that has added to the same ERI.
int blk_decide(dmk_eri *h, int kchunk_w2, int kchunk_w1, int *skip, bool *save, uint64_t *key) {
    dmk_ctx *ctx = h->ctx;
    dmk_eri_cache *c = h->cache;
    *skip = 0;
    *save = false;
    const int S = h->blk_S;
    const long long n = (long long)S * 128;
    if (h->n_w2 + h->n_w1 == 0) return DMK_OK;
    uint64_t k = 0xcbf29ce484222325ULL;
    const int64_t head[] = {h->mesh.n[0], h->mesh.n[1], h->mesh.n[2], h->nao, h->naux, h->nemb, h->spin, h->pr, h->pl, h->blk_ne, S,
                            kchunk_w2, kchunk_w1, h->n_w2, h->n_w1};
    if (h->split1) k = blk_mix(k, 0x73706c6974ULL);          // the other partner order of type 1: never the same entry
    if (h->strip1) k = blk_mix(k, 0x7374726970ULL);          // nor the strip order
    for (int64_t v : head) k = blk_mix(k, (uint64_t)v);
    for (int w = 2; w >= 1; --w) {
        const dmk_eri::WeightClass wc = h->weight_class(w);
        for (int i = 0; i < wc.n; ++i) {
            const int slot = wc.first + i;
            if (slot >= (int)h->slot_keys.size() || !h->slot_keys[slot].keyed) {       // planes without a key: not eligible
                c->blk_misses += 1;
                return DMK_OK;
            }
            const dmk_eri::SlotKey &sk = h->slot_keys[slot];
            k = blk_mix(blk_mix(blk_mix(blk_mix(k, (uint64_t)sk.kL), sk.key), (uint64_t)sk.weight), (uint64_t)sk.re_only);
        }
    }
    *key = k;
    if (!blk_can_skip(h)) {
        c->blk_misses += 1;
        return DMK_OK;
    }
    int cpr;
    const unsigned grid = blk_grid(h, n, &cpr);
    int nonzero = 1;
    int rc = device_flag(ctx, c, &nonzero, [&] {
        hipLaunchKernelGGL(blk_corner_kernel<2>, dim3(grid), dim3(256), 0, ctx->stream, h->eri, (double *)nullptr, n, (long long)h->npair,
                           (long long)h->npair * h->npair, cpr, c->flag.get<int>());
    });
    if (rc) return rc;
    if (nonzero) {
        c->blk_misses += 1;
        return DMK_OK;
    }
    if (c->blk_valid && c->blk_buf && c->blk_key == k && c->blk_S == S && c->blk_ne == h->blk_ne) {
        c->blk_hits += 1;
        *skip = S;
        return DMK_OK;
    }
    c->blk_misses += 1;
    const size_t bytes = (size_t)h->spin_blocks() * (size_t)n * (size_t)n * sizeof(double);
    *save = c->held + bytes <= c->budget;           // (the entry it replaces goes first)
    return DMK_OK;
}

// After the launches of that contraction: the kept corner goes back into the ERI (warm) or the finished corner becomes the entry
// (save; it replaces an older one; no memory: nothing is kept).
int blk_finish(dmk_eri *h, bool warm, bool save, uint64_t key) {
    dmk_ctx *ctx = h->ctx;
    dmk_eri_cache *c = h->cache;
    const long long n = (long long)h->blk_S * 128;
    int cpr;
    const unsigned grid = blk_grid(h, n, &cpr);
    if (warm) {
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(blk_corner_kernel<1>, dim3(grid), dim3(256), 0, ctx->stream, h->eri, c->blk_buf.get<double>(), n, (long long)h->npair,
                           (long long)h->npair * h->npair, cpr, (int *)nullptr);
        DMK_CHECK_LAUNCH(ctx);
        return DMK_OK;
    }
    if (!save) return DMK_OK;
    const size_t bytes = (size_t)h->spin_blocks() * (size_t)n * (size_t)n * sizeof(double);
    c->blk_valid = false;
    if (c->blk_buf && c->blk_bytes() != bytes) {
        (void)hipStreamSynchronize(ctx->stream);
        c->blk_buf.reset();
    }
    if (!c->blk_buf && c->blk_buf.alloc(ctx, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return DMK_OK;
    }
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(blk_corner_kernel<0>, dim3(grid), dim3(256), 0, ctx->stream, h->eri, c->blk_buf.get<double>(), n, (long long)h->npair,
                           (long long)h->npair * h->npair, cpr, (int *)nullptr);
        DMK_CHECK_LAUNCH(ctx);
    }
    c->blk_key = key;
    c->blk_S = h->blk_S;
    c->blk_valid = true;
    return DMK_OK;
}

int dmk_eri_begin_kL_cached(dmk_eri *h, int kL, int weight, uint64_t key64) {
    if (!h) return DMK_ERR_INVALID;
    int rc = eri_begin_kL_impl(h, kL, weight);
    if (rc || !h->cache) return rc;
    dmk_eri_cache *c = h->cache;
    h->cur_key = key64;
    h->cur_keyed = true;
    for (const auto &e : c->entries)
        if (e.kL == kL && e.key == key64 && e.re_only == (h->re_only ? 1 : 0)) {
            rc = inv_region_copy(h, e.buf.get<double>(), true);
            if (rc) return rc;
            h->inv_warm = true;
            c->hits += 1;
            return DMK_OK;
        }
    c->misses += 1;
    h->inv_save = true;
    return DMK_OK;
}

