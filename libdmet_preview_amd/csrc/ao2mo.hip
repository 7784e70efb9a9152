// K19 -- four-index transform of one 4-fold packed ERI block (dmk_ao2mo_s4): the MO integrals every post-HF solver starts from.
//
//     out[(i,j)][(k,l)] = sum_pqrs c1[p][i] c2[q][j] eri[pair(p,q)][pair(r,s)] c3[r][k] c4[s][l]
//
// Two half transforms, both "H[row] = Xa^T M_row Xb for a stack of packed symmetric matrices M_row", served by ONE kernel template:
//
//   ao2mo_gemm_kernel<1, 0>  the packed rows stacked along M:  T[(row, r)][x] = sum_s M_row[r][s] X[s][x].  The A-operand loader
//                            expands the triangle on the fly, (r, s) -> row * ld + pair(max, min); the X tile staged in LDS serves
//                            every row of the stack.  X is the narrower coefficient matrix.
//   ao2mo_gemm_kernel<0, *>  per row, the other index:  H_row[y][x] = sum_r Y[r][y] T_row[r][x]  (batch = rows), stored dense or
//                            packed (hi >= lo, pair order).  <0, 1> swaps the MFMA operands so that the lanes of a store run along
//                            y, for the case that y is the contiguous index of the destination.
//
// 64 x 64 workgroup tile, K tile 16, four waves of 2 x 2 v_mfma_f64_16x16x4_f64 accumulators; both operand tiles k-major in LDS with
// a row pitch of 81 doubles (162 dwords): 34 mod 64 for the reads -- the lanes l and l + 16 of a ds_read_b64, one k row apart, land
// in opposite bank halves but for two banks -- and 2 mod 32 for the stores of the gathered tile, whose lanes run along k (a pitch
// of 80 put the 16 k of a store on one bank pair; 118.4 -> 115.9 ms for the full transform at n = 256).  Two LDS stages, the next
// tile's global loads in flight during the MFMAs, one barrier per K tile.
//
// The ket half writes H (npair x columns); an explicit tiled transpose turns it into packed ROWS for the bra half, whose result is
// transposed into `out`.  The call works in slabs of the index k so that H fits the workspace; each slab yields complete output
// columns.  Every sum has a fixed order (no atomics) and the order of an element does not depend on the slabbing.
#include "devres.h"
#include <algorithm>

namespace {

constexpr int NT = 256, BM = 64, BN = 64, BK = 16, LDT = 81;
constexpr int64_t T_BYTES_MAX = (int64_t)256 << 20;       // the step-1 intermediate of a row chunk
constexpr int ROWS_MAX = 16384;

struct Ao2moGemm {
    int M, N, K, batch;
    const double *A; long long lda; int n;      // GATHER: packed rows (pitch lda) of symmetric n x n matrices, M = rows * n, K = n
                                                // else   : A[k * lda + m], shared by the batch
    const double *B; long long ldb, sB;         // B[k * ldb + x] (+ b * sB)
    double *C; long long sCb, sCm, sCn;         // dense store: C[b * sCb + m * sCm + x * sCn]
    int pack; long long hi_off, pbase;          // packed store: hi = hi_off + x, lo = m, kept when lo <= hi at b * sCb + pair(hi, lo) - pbase
};

template <int GATHER, int TD>
__global__ __launch_bounds__(NT) void ao2mo_gemm_kernel(Ao2moGemm g) {
    __shared__ double As[2][BK][LDT], Bs[2][BK][LDT];
    const int tilesN = (g.N + BN - 1) / BN, tilesM = (g.M + BM - 1) / BM;
    long long bid = blockIdx.x;
    const int tn = (int)(bid % tilesN); bid /= tilesN;
    const int tm = (int)(bid % tilesM);
    const long long b = bid / tilesM;
    const int m0 = tm * BM, n0 = tn * BN;
    if (g.pack && (long long)m0 > g.hi_off + n0 + BN - 1) return;        // every lo of the tile lies above every hi (uniform exit)
    const double *Bp = g.B + b * g.sB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;

    // operand loaders: four elements per thread and tile
    const int c64 = tid & 63, k4 = tid >> 6;          // column-fastest map (B; A when dense): k = k4 + 4 j
    const int kg = tid & 15, mg = tid >> 4;           // k-fastest map (gathered A): m = mg + 16 j
    long long rowoff[4]; int rr[4];                   // gathered A: start of the packed row and the index r of the four rows
    if (GATHER) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + mg + 16 * j;
            rr[j] = m < g.M ? m % g.n : -1;
            rowoff[j] = m < g.M ? (long long)(m / g.n) * g.lda : 0;
        }
    }
    double ra[4], rb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + k4 + 4 * j;
            rb[j] = (k < g.K && n0 + c64 < g.N) ? Bp[(long long)k * g.ldb + n0 + c64] : 0.0;
            if (GATHER) {
                const int s = k0 + kg, r = rr[j];
                const int hi = r > s ? r : s, lo = r > s ? s : r;
                ra[j] = (r >= 0 && s < g.K) ? g.A[rowoff[j] + (long long)hi * (hi + 1) / 2 + lo] : 0.0;
            } else {
                ra[j] = (k < g.K && m0 + c64 < g.M) ? g.A[(long long)k * g.lda + m0 + c64] : 0.0;
            }
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Bs[buf][k4 + 4 * j][c64] = rb[j];
            if (GATHER) As[buf][kg][mg + 16 * j] = ra[j];
            else As[buf][k4 + 4 * j][c64] = ra[j];
        }
    };

    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4_t{0.0, 0.0, 0.0, 0.0};
    const int nk = (g.K + BK - 1) / BK;
    load(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) load((t + 1) * BK);
#pragma unroll
        for (int kk = 0; kk < BK / 4; ++kk) {
            double a[2], bb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = As[buf][4 * kk + q][wm + 16 * i + x];
                bb[i] = Bs[buf][4 * kk + q][wn + 16 * i + x];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = TD ? __builtin_amdgcn_mfma_f64_16x16x4f64(bb[j], a[i], acc[i][j], 0, 0, 0)
                                   : __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
        }
        if (t + 1 < nk) stage(buf ^ 1);      // the other stage was last read before the previous barrier
        __syncthreads();
    }
    // D layout: row = (lane >> 4) + 4 r, column = lane & 15; with TD the tile is the transpose (rows run along x, columns along m)
    double *Cb = g.C + b * g.sCb;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + (TD ? x : q + 4 * r);
                const int xx = n0 + wn + 16 * j + (TD ? q + 4 * r : x);
                if (m >= g.M || xx >= g.N) continue;
                if (g.pack) {
                    const long long hi = g.hi_off + xx;
                    if (m <= hi) Cb[hi * (hi + 1) / 2 + m - g.pbase] = acc[i][j][r];
                } else {
                    Cb[(long long)m * g.sCm + (long long)xx * g.sCn] = acc[i][j][r];
                }
            }
}

// out[c * ldo + r] = in[r * ldi + c], r < rows, c < cols: 32 x 32 tiles through LDS, both sides in 256-byte runs
__global__ __launch_bounds__(NT) void ao2mo_transpose_kernel(long long rows, long long cols, const double *__restrict__ in, long long ldi,
                                                             double *__restrict__ out, long long ldo) {
    __shared__ double tile[32][33];
    const long long tc = (cols + 31) / 32;
    const long long r0 = ((long long)blockIdx.x / tc) * 32, c0 = ((long long)blockIdx.x % tc) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const long long r = r0 + ty + 8 * p, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 8 * p][tx] = in[r * ldi + c];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const long long c = c0 + ty + 8 * p, r = r0 + tx;
        if (r < rows && c < cols) out[c * ldo + r] = tile[tx][ty + 8 * p];
    }
}

long long pair_of(long long k) { return k * (k + 1) / 2; }

template <int GATHER, int TD>
int gemm_launch(dmk_ctx *ctx, const Ao2moGemm &g) {
    if (g.M <= 0 || g.N <= 0 || g.batch <= 0) return DMK_OK;
    const long long blocks = (long long)((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN) * g.batch;
    if (blocks > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: a launch of %lld workgroups", blocks);
    const int tilesM = (g.M + BM - 1) / BM, tilesN = (g.N + BN - 1) / BN;
    long long live = (long long)tilesM * tilesN;          // tiles that reach the K loop: a packed store leaves at once where every lo > hi
    if (g.pack) {
        live = 0;
        for (int tn = 0; tn < tilesN; ++tn)
            live += std::min<long long>(tilesM, (g.hi_off + (long long)tn * BN + BN - 1) / BM + 1);
    }
    FamScope fs(ctx, DMK_FAM_DGEMM);
    fs.mfma_flops(2.0 * BM * BN * (double)((g.K + BK - 1) / BK * BK) * (double)live * g.batch);
    hipLaunchKernelGGL((ao2mo_gemm_kernel<GATHER, TD>), dim3((unsigned)blocks), dim3(NT), 0, ctx->stream, g);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

int transpose_launch(dmk_ctx *ctx, long long rows, long long cols, const double *in, long long ldi, double *out, long long ldo) {
    if (rows <= 0 || cols <= 0) return DMK_OK;
    const long long blocks = ((rows + 31) / 32) * ((cols + 31) / 32);
    if (blocks > 0x7fffffffLL) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: a transpose of %lld tiles", blocks);
    FamScope fs(ctx, DMK_FAM_MISC);
    hipLaunchKernelGGL(ao2mo_transpose_kernel, dim3((unsigned)blocks), dim3(NT), 0, ctx->stream, rows, cols, in, ldi, out, ldo);
    DMK_CHECK_LAUNCH(ctx);
    return DMK_OK;
}

// One half transform of `rows` packed rows (pitch ld): dst[row][(f, s)] = sum_ab Cf[a][f] M_row[a][b] Cs[b][s], f in [f0, f0 + fw) of the
// first matrix, every s < ns of the second; dense with the pair (f - f0, s) at (f - f0) * ns + s, or packed (s <= f) at
// pair(f, s) - pair(f0, 0).  `first_leads`: the first matrix is contracted in step 1 (the choice must not depend on f0, fw).
int half_transform(dmk_ctx *ctx, int n, long long rows, const double *src, long long ld, const double *Cf, long long ldf, int f0, int fw,
                   const double *Cs, long long lds_, int ns, bool first_leads, bool pack, double *dst, long long ldd, double *T,
                   long long t_doubles) {
    const int nx = first_leads ? fw : ns;
    const int chunk = (int)std::max<long long>(1, std::min<long long>(ROWS_MAX, t_doubles / ((long long)n * nx)));
    for (long long r0 = 0; r0 < rows; r0 += chunk) {
        const int nr = (int)std::min<long long>(chunk, rows - r0);
        Ao2moGemm a{};
        a.M = nr * n; a.N = nx; a.K = n; a.batch = 1;
        a.A = src + r0 * ld; a.lda = ld; a.n = n;
        a.B = first_leads ? Cf + f0 : Cs; a.ldb = first_leads ? ldf : lds_; a.sB = 0;
        a.C = T; a.sCb = 0; a.sCm = nx; a.sCn = 1;
        int rc = gemm_launch<1, 0>(ctx, a);
        if (rc) return rc;
        Ao2moGemm d{};
        d.K = n; d.batch = nr; d.n = n;
        d.B = T; d.ldb = nx; d.sB = (long long)n * nx;
        d.C = dst + r0 * ldd; d.sCb = ldd;
        if (first_leads) {           // m = s, x = f - f0: the destination runs along m
            d.M = ns; d.N = fw; d.A = Cs; d.lda = lds_;
            d.sCm = 1; d.sCn = ns;
            d.pack = pack ? 1 : 0; d.hi_off = f0; d.pbase = pair_of(f0);
            rc = gemm_launch<0, 1>(ctx, d);
        } else {                     // m = f - f0, x = s
            d.M = fw; d.N = ns; d.A = Cf + f0; d.lda = ldf;
            d.sCm = ns; d.sCn = 1;
            rc = gemm_launch<0, 0>(ctx, d);
        }
        if (rc) return rc;
    }
    return DMK_OK;
}

struct Plan {
    long long npair, nij, nkl;
    bool pack_bra, pack_ket, ket_first_leads, bra_first_leads;
    long long t_doubles, col_cap;       // step-1 intermediate; most columns of a slab
    int64_t bytes;                      // workspace of the largest slab
    int nslab;
    std::vector<int> k_edges;           // slab s covers k in [k_edges[s], k_edges[s + 1])
};

long long slab_cols(const Plan &p, int n4, int k0, int k1) {
    return p.pack_ket ? pair_of(k1) - pair_of(k0) : (long long)(k1 - k0) * n4;
}

// 0 or the bytes that the smallest possible plan needs (then nothing of `p` is valid)
int64_t make_plan(int n, int n1, int n2, int n3, int n4, int flags, int64_t ws_bytes, Plan &p) {
    p.npair = pair_of(n);
    p.pack_bra = flags & DMK_AO2MO_PACK_BRA; p.pack_ket = flags & DMK_AO2MO_PACK_KET;
    p.nij = p.pack_bra ? pair_of(n1) : (long long)n1 * n2;
    p.nkl = p.pack_ket ? pair_of(n3) : (long long)n3 * n4;
    p.ket_first_leads = !(n4 < n3);     // the narrower matrix leads; on a tie the one whose index is slabbed (no repeated step 1)
    p.bra_first_leads = !(n2 < n1);
    const int64_t budget = ws_bytes > 0 ? ws_bytes : DMK_AO2MO_WS_DEFAULT;
    const long long t_min = (long long)n * std::max(std::max(n1, n2), std::max(n3, n4));      // one row
    const long long per_col = (std::max(p.npair, p.nij) + p.npair) * 8;
    const long long widest = p.pack_ket ? n3 : n4;                                            // columns of the slab k = n3 - 1 alone
    const int64_t least = (int64_t)dmk_align256((size_t)t_min * 8) + 512 + widest * per_col;
    if (budget < least) return least;
    p.t_doubles = std::max<long long>(t_min, std::min<int64_t>(T_BYTES_MAX, budget / 4) / 8);
    const long long t_need = std::min<long long>(p.t_doubles, std::max(p.npair, p.nkl) * t_min);   // never more than every row at once
    p.t_doubles = std::max(t_min, t_need);
    p.col_cap = (budget - (int64_t)dmk_align256((size_t)p.t_doubles * 8) - 512) / per_col;
    if (p.col_cap < widest) {           // the intermediate gives way to the slab
        p.t_doubles = t_min;
        p.col_cap = (budget - (int64_t)dmk_align256((size_t)p.t_doubles * 8) - 512) / per_col;
    }
    p.k_edges.assign(1, 0);
    long long most = 0;
    for (int k0 = 0; k0 < n3;) {
        int k1 = k0 + 1;
        while (k1 < n3 && slab_cols(p, n4, k0, k1 + 1) <= p.col_cap) ++k1;
        most = std::max(most, slab_cols(p, n4, k0, k1));
        p.k_edges.push_back(k1);
        k0 = k1;
    }
    p.nslab = (int)p.k_edges.size() - 1;
    p.col_cap = most;
    p.bytes = (int64_t)dmk_align256((size_t)p.t_doubles * 8) + (int64_t)dmk_align256((size_t)(std::max(p.npair, p.nij) * most) * 8) +
              (int64_t)dmk_align256((size_t)(p.npair * most) * 8);
    return 0;
}

bool widths_ok(int n, int n1, int n2, int n3, int n4) {
    return n >= 1 && n <= 512 && n1 >= 1 && n1 <= n && n2 >= 1 && n2 <= n && n3 >= 1 && n3 <= n && n4 >= 1 && n4 <= n;
}

}  // namespace

extern "C" {

int dmk_ao2mo_plan(int n, int n1, int n2, int n3, int n4, int flags, int64_t ws_bytes, int64_t *plan_host) {
    if (!plan_host || !widths_ok(n, n1, n2, n3, n4) || ws_bytes < 0 || (flags & ~(DMK_AO2MO_PACK_BRA | DMK_AO2MO_PACK_KET)) ||
        ((flags & DMK_AO2MO_PACK_BRA) && n1 != n2) || ((flags & DMK_AO2MO_PACK_KET) && n3 != n4))
        return DMK_ERR_INVALID;
    Plan p;
    const int64_t least = make_plan(n, n1, n2, n3, n4, flags, ws_bytes, p);
    if (least) { plan_host[0] = 0; plan_host[1] = least; plan_host[2] = 0; return DMK_ERR_INVALID; }
    plan_host[0] = p.nslab; plan_host[1] = p.bytes; plan_host[2] = p.nij * p.nkl;
    return DMK_OK;
}

int dmk_ao2mo_s4(dmk_ctx *ctx, int n, const double *eri, int64_t ld, const double *c1, int64_t ldc1, int n1, const double *c2, int64_t ldc2,
                 int n2, const double *c3, int64_t ldc3, int n3, const double *c4, int64_t ldc4, int n4, int flags, int64_t ws_bytes,
                 double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (!eri || !c1 || !c2 || !c3 || !c4 || !out) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: a NULL pointer");
    if (n < 1 || n > 512) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: supports 1 <= n <= 512 (got %d)", n);
    if (ld < pair_of(n)) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: row pitch %lld below npair = %lld", (long long)ld, pair_of(n));
    if (!widths_ok(n, n1, n2, n3, n4) || ldc1 < n1 || ldc2 < n2 || ldc3 < n3 || ldc4 < n4)
        return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: coefficient widths (%d, %d, %d, %d) must lie in [1, %d] and within their "
                        "leading dimensions", n1, n2, n3, n4, n);
    if (ws_bytes < 0 || (flags & ~(DMK_AO2MO_PACK_BRA | DMK_AO2MO_PACK_KET)))
        return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: bad flags or workspace size");
    if ((flags & DMK_AO2MO_PACK_BRA) && (c1 != c2 || ldc1 != ldc2 || n1 != n2))
        return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: PACK_BRA needs c1 and c2 to be one matrix");
    if ((flags & DMK_AO2MO_PACK_KET) && (c3 != c4 || ldc3 != ldc4 || n3 != n4))
        return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: PACK_KET needs c3 and c4 to be one matrix");
    Plan p;
    const int64_t least = make_plan(n, n1, n2, n3, n4, flags, ws_bytes, p);
    if (least) return dmk_fail(ctx, DMK_ERR_INVALID, "ao2mo_s4: the workspace must hold %lld bytes (one k of a slab)", (long long)least);
    DevMem ws;
    if (ws.alloc(ctx, (size_t)p.bytes) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "ao2mo_s4: no device memory for a workspace of %lld bytes", (long long)p.bytes);
    }
    StreamDrain drain{ctx->stream};          // declared after the owners of device memory: the stream is drained before they let go
    char *base = ws.get<char>();
    double *T = reinterpret_cast<double *>(base);
    double *bufA = reinterpret_cast<double *>(base + dmk_align256((size_t)p.t_doubles * 8));
    double *bufB = reinterpret_cast<double *>(reinterpret_cast<char *>(bufA) + dmk_align256((size_t)(std::max(p.npair, p.nij) * p.col_cap) * 8));
    long long col0 = 0;
    for (int s = 0; s < p.nslab; ++s) {
        const int k0 = p.k_edges[s], k1 = p.k_edges[s + 1];
        const long long ncs = slab_cols(p, n4, k0, k1);
        // ket half: H (npair x ncs) in bufA, its transpose (ncs packed rows of pitch npair) in bufB
        int rc = half_transform(ctx, n, p.npair, eri, ld, c3, ldc3, k0, k1 - k0, c4, ldc4, n4, p.ket_first_leads, p.pack_ket, bufA, ncs, T,
                                p.t_doubles);
        if (!rc) rc = transpose_launch(ctx, p.npair, ncs, bufA, ncs, bufB, p.npair);
        // bra half: (ncs x nij) in bufA, transposed into the slab's columns of out
        if (!rc) rc = half_transform(ctx, n, ncs, bufB, p.npair, c1, ldc1, 0, n1, c2, ldc2, n2, p.bra_first_leads, p.pack_bra, bufA, p.nij, T,
                                     p.t_doubles);
        if (!rc) rc = transpose_launch(ctx, ncs, p.nij, bufA, p.nij, out + col0, p.nkl);
        if (rc) return rc;
        col0 += ncs;
    }
    return DMK_OK;
}

}  // extern "C"
