// K17: what a DMET iteration does behind the impurity solver.
//
//   dmk_dmet_h2_scaled   copy of an embedding ERI scaled by the number of impurity indices of every element
//                        (routine/slater.py:1734-1778 get_H2_scaled, fused with the ao2mo.restore around it)
//   dmk_rho_glob         democratic global density stripe of one fragment (routine/slater_helper.py:183-270 get_rho_glob_R)
//
// The scaling is HBM streaming: every element is read once and written once, the weight comes from one class byte per packed
// pair (c = m_i + m_j, m the impurity indicator) that stays in cache.  No atomics, no LDS; every element offset is 64-bit.
#include "devres.h"
#include <algorithm>

namespace {

constexpr int NT = 256;

// cls[pair(k,l)] = m_k + m_l and, for the gathers, kl[pair(k,l)] = k << 16 | l   (k >= l)
__global__ __launch_bounds__(NT) void pair_class_kernel(int n, const unsigned char *__restrict__ mask, unsigned char *__restrict__ cls,
                                                        unsigned *__restrict__ kl) {
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= n * n) return;
    const int k = t / n, l = t % n;
    if (l > k) return;
    const int q = k * (k + 1) / 2 + l;
    cls[q] = (unsigned char)(mask[k] + mask[l]);
    if (kl) kl[q] = ((unsigned)k << 16) | (unsigned)l;
}

// The rule of the 4-fold form (slater.py:1745-1761): class sum 4 untouched, 0 ASSIGNED +0.0, otherwise one multiply.
// The 1-fold form (slater.py:1762-1775) multiplies every element, by 0.0 and by 1.0 too.
template <bool ASSIGN_ZERO>
__device__ __forceinline__ double scaled(double v, int csum) {
    if (ASSIGN_ZERO) {
        if (csum == 4) return v;
        if (csum == 0) return 0.0;
    }
    return v * (0.25 * (double)csum);
}

struct ScaleArgs {
    int n;                   // orbitals
    int nrow, ncol;          // of the OUTPUT: npair x npair (4-fold) or n^2 x n^2 (1-fold)
    const double *in;
    double *out;
    long long ld_in, ld_out;
    const unsigned char *mask, *cls;
    const unsigned *kl;
};

__device__ __forceinline__ long long tri(long long a, long long b) { return a >= b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

// One workgroup per output row at a time (the row class is uniform), VEC columns per thread and step.
//   IN == OUT: same layout, element for element (in place allowed)
//   IN 4 | 8 -> OUT 1: out[(i,j)][(k,l)] = in(pair(i,j), pair(k,l))
//   IN 1 | 8 -> OUT 4: out[p][q] = in((i,j), (k,l))  with (i,j), (k,l) unpacked through the kl table
template <int IN, int OUT, int VEC>
__global__ __launch_bounds__(NT) void h2_scale_kernel(ScaleArgs a) {
    constexpr bool ASSIGN_ZERO = !(IN == 1 && OUT == 1);
    const int n = a.n;
    const int step = NT * VEC;
    const int dk = step / n, dl = step % n;           // (k, l) of a 1-fold column advance without a division per element
    for (int r = blockIdx.x; r < a.nrow; r += gridDim.x) {
        int crow, ri = 0, rj = 0;
        long long rp = 0;                             // packed pair of the row
        if (OUT == 4) {
            crow = a.cls[r];
            rp = r;
            if (IN == 1) { const unsigned u = a.kl[r]; ri = (int)(u >> 16); rj = (int)(u & 0xffffu); }
        } else {
            ri = r / n; rj = r % n;
            crow = a.mask[ri] + a.mask[rj];
            rp = tri(ri, rj);
        }
        const double *in_row = a.in;
        if (IN == 4) in_row += rp * a.ld_in;
        else if (IN == 1) in_row += ((long long)ri * n + rj) * a.ld_in;
        double *out_row = a.out + (long long)r * a.ld_out;

        int c = threadIdx.x * VEC;
        int k = 0, l = 0;
        if (OUT == 1) { k = c / n; l = c % n; }
        for (; c < a.ncol; c += step) {
            double v[VEC] = {};
            int cs[VEC];
            if (IN == OUT) {
                if (VEC == 2 && c + 1 < a.ncol) {
                    const double2 t = *reinterpret_cast<const double2 *>(in_row + c);
                    v[0] = t.x; v[VEC - 1] = t.y;
                } else {
                    v[0] = in_row[c];
                    if (VEC == 2) v[VEC - 1] = 0.0;
                }
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int ce = c + e;
                if (ce >= a.ncol) { cs[e] = 4; continue; }
                long long q;                          // packed pair of the column
                int ck = k, cl = l + e;
                if (OUT == 1) {
                    if (cl >= n) { cl -= n; ++ck; }
                    q = tri(ck, cl);
                    cs[e] = crow + (IN == 1 ? a.mask[ck] + a.mask[cl] : a.cls[q]);
                } else {
                    q = ce;
                    cs[e] = crow + a.cls[q];
                }
                if (IN != OUT) {
                    if (IN == 4) v[e] = in_row[q];
                    else if (IN == 8) { const long long hi = rp > q ? rp : q, lo = rp > q ? q : rp; v[e] = a.in[hi * (hi + 1) / 2 + lo]; }
                    else { const unsigned u = a.kl[q]; v[e] = in_row[(long long)(u >> 16) * n + (u & 0xffffu)]; }
                }
            }
            if (VEC == 2 && c + 1 < a.ncol) {
                double2 t;
                t.x = scaled<ASSIGN_ZERO>(v[0], cs[0]);
                t.y = scaled<ASSIGN_ZERO>(v[VEC - 1], cs[VEC - 1]);
                *reinterpret_cast<double2 *>(out_row + c) = t;
            } else {
                out_row[c] = scaled<ASSIGN_ZERO>(v[0], cs[0]);
            }
            if (OUT == 1) {
                k += dk; l += dl;
                if (l >= n) { l -= n; ++k; }
            }
        }
    }
}

// 4-fold -> scaled 1-fold for even n on 16-byte aligned output rows (the C5 path of get_H_dmet(compact=False)).  The generic kernel
// above reads the half l > k of every (k, l) plane with a stride of about l doubles between neighbouring lanes and runs at a quarter
// of the copy rate.  Here a wave owns a tile of 4 k x 32 l: it WRITES 4 segments of 256 contiguous bytes (lane = (k, l pair)); above
// the diagonal it READS with k fastest (lane = (l, k pair): 32-byte pieces of the packed row, each 128-byte line used by four
// consecutive k tiles of the same wave) and the lanes exchange their values through the cross-lane network (__shfl: no LDS is
// allocated).  Tiles below the diagonal read as they write; tiles on it or on the edge go element by element.
__global__ __launch_bounds__(NT) void h2_scale_4to1_kernel(ScaleArgs a) {
    const int n = a.n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkt = (n + 3) / 4, nlt = (n + 31) / 32;
    const int wa = lane >> 4, wb = lane & 15;           // write role: k = k0 + wa, l = l0 + 2 wb, l + 1
    const int rl = lane >> 1, rk = lane & 1;            // read role above the diagonal: l = l0 + rl, k = k0 + 2 rk, k + 1
    const int s0 = 4 * wb + (wa >> 1), s1 = s0 + 2;     // read-role lanes that hold (k, l) and (k, l + 1) of this write-role lane
    for (int r = blockIdx.x; r < a.nrow; r += gridDim.x) {
        const int ri = r / n, rj = r % n;
        const int crow = a.mask[ri] + a.mask[rj];
        const double *in_row = a.in + tri(ri, rj) * a.ld_in;
        double *out_row = a.out + (long long)r * a.ld_out;
        for (int lt = wave; lt < nlt; lt += NT / 64) {
            const int l0 = lt * 32, l = l0 + 2 * wb;
            const bool l_full = l0 + 32 <= n;
            int kt = 0;
            while (kt < nkt) {
                const int k0 = kt * 4;
                // four k tiles at once where all of them lie on one side of the diagonal: their loads are issued together (16.4 ->
                // 13.2 ms at n = 256, profiles/dmet_ham_notes.txt)
                if (l_full && k0 + 16 <= n && (l0 >= k0 + 16 || l0 + 31 <= k0)) {
                    double g0[4], g1[4];
                    if (l0 >= k0 + 16) {
                        const long long q = (long long)(l0 + rl) * (l0 + rl + 1) / 2 + k0 + 2 * rk;
                        double v0[4], v1[4];
#pragma unroll
                        for (int t = 0; t < 4; ++t) { v0[t] = in_row[q + 4 * t]; v1[t] = in_row[q + 4 * t + 1]; }
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const double x00 = __shfl(v0[t], s0), x01 = __shfl(v1[t], s0), x10 = __shfl(v0[t], s1), x11 = __shfl(v1[t], s1);
                            g0[t] = (wa & 1) ? x01 : x00;
                            g1[t] = (wa & 1) ? x11 : x10;
                        }
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const long long kk = k0 + 4 * t + wa, q = kk * (kk + 1) / 2 + l;
                            g0[t] = in_row[q];
                            g1[t] = in_row[q + 1];
                        }
                    }
                    const int cl0 = crow + a.mask[l], cl1 = crow + a.mask[l + 1];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int kk = k0 + 4 * t + wa, mk = a.mask[kk];
                        double2 t2;
                        t2.x = scaled<true>(g0[t], cl0 + mk);
                        t2.y = scaled<true>(g1[t], cl1 + mk);
                        *reinterpret_cast<double2 *>(out_row + (long long)kk * n + l) = t2;
                    }
                    kt += 4;
                    continue;
                }
                kt += 1;
                const int k = k0 + wa;
                const bool full = l_full && k0 + 4 <= n;        // (wave uniform, as are the two tests below)
                double e0, e1;
                if (full && l0 >= k0 + 4) {                     // every l > k
                    const long long q = (long long)(l0 + rl) * (l0 + rl + 1) / 2 + k0 + 2 * rk;
                    const double v0 = in_row[q], v1 = in_row[q + 1];
                    const double x00 = __shfl(v0, s0), x01 = __shfl(v1, s0), x10 = __shfl(v0, s1), x11 = __shfl(v1, s1);
                    e0 = (wa & 1) ? x01 : x00;
                    e1 = (wa & 1) ? x11 : x10;
                } else if (full && l0 + 31 <= k0) {             // every l <= k
                    const long long q = (long long)k * (k + 1) / 2 + l;
                    e0 = in_row[q];
                    e1 = in_row[q + 1];
                } else {
                    if (k >= n || l >= n) continue;             // (n and l are even: l + 1 < n)
                    e0 = in_row[tri(k, l)];
                    e1 = in_row[tri(k, l + 1)];
                }
                const int ck = crow + a.mask[k];
                double2 t;
                t.x = scaled<true>(e0, ck + a.mask[l]);
                t.y = scaled<true>(e1, ck + a.mask[l + 1]);
                *reinterpret_cast<double2 *>(out_row + (long long)k * n + l) = t;
            }
        }
    }
}

template <int IN, int OUT>
void launch_scale(dmk_ctx *ctx, const ScaleArgs &a, bool vec) {
    const int grid = std::min(a.nrow, 16384);
    if (vec) hipLaunchKernelGGL((h2_scale_kernel<IN, OUT, 2>), dim3(grid), dim3(NT), 0, ctx->stream, a);
    else hipLaunchKernelGGL((h2_scale_kernel<IN, OUT, 1>), dim3(grid), dim3(NT), 0, ctx->stream, a);
}

// bytes an ERI of `sym` with pitch ld spans from its first element
long long span_bytes(int n, int sym, long long ld) {
    const long long npair = (long long)n * (n + 1) / 2, nn = (long long)n * n;
    if (sym == 8) return npair * (npair + 1) / 2 * 8;
    const long long rows = sym == 4 ? npair : nn;
    return ((rows - 1) * ld + rows) * 8;
}

// rho[s][I][i][j] = 1/2 ( m_j G[s][I][i][j] + m_i G[s][-I][j][i] ),  -I = lattice.subtract(0, I); a masked term is left out
// (never multiplied by zero), as the reference assigns its env-env block.
__global__ __launch_bounds__(NT) void rho_combine_kernel(int n0, int n1, int n2, int nlo, const unsigned char *__restrict__ mask,
                                                         const double *__restrict__ G, double *__restrict__ out) {
    const int ncells = n0 * n1 * n2;
    const int I = blockIdx.y % ncells, s = blockIdx.y / ncells;
    const int a2 = I % n2, a1 = (I / n2) % n1, a0 = I / (n2 * n1);
    const int Im = (((n0 - a0) % n0) * n1 + (n1 - a1) % n1) * n2 + (n2 - a2) % n2;
    const long long blk = (long long)nlo * nlo;
    const double *g = G + ((long long)s * ncells + I) * blk;
    const double *gm = G + ((long long)s * ncells + Im) * blk;
    double *o = out + ((long long)s * ncells + I) * blk;
    for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < blk; t += (long long)gridDim.x * NT) {
        const int i = (int)(t / nlo), j = (int)(t % nlo);
        double v = 0.0;
        if (mask[j]) v = g[t];
        if (mask[i]) v += gm[(long long)j * nlo + i];
        o[t] = 0.5 * v;
    }
}

// impurity index list -> indicator bytes; false if an index is outside [0, n) or repeated
bool make_mask(int n, const int32_t *idx, int nimp, std::vector<unsigned char> &m) {
    m.assign(n, 0);
    for (int t = 0; t < nimp; ++t) {
        if (idx[t] < 0 || idx[t] >= n || m[idx[t]]) return false;
        m[idx[t]] = 1;
    }
    return true;
}

}  // namespace

extern "C" {

int dmk_dmet_h2_scaled(dmk_ctx *ctx, int n, const int32_t *imp_idx_host, int nimp, int in_symmetry, const double *in, int64_t ld_in,
                       int out_symmetry, double *out, int64_t ld_out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (n <= 0 || n > 32767 || nimp < 0 || nimp > n || (nimp > 0 && !imp_idx_host) || !in || !out)
        return dmk_fail(ctx, DMK_ERR_INVALID, "dmet_h2_scaled: bad arguments");
    if ((in_symmetry != 1 && in_symmetry != 4 && in_symmetry != 8) || (out_symmetry != 1 && out_symmetry != 4) ||
        (in_symmetry == 8 && out_symmetry == 1))
        return dmk_fail(ctx, DMK_ERR_INVALID, "dmet_h2_scaled: symmetry %d -> %d is not one of 1->1, 1->4, 4->4, 4->1, 8->4",
                        in_symmetry, out_symmetry);
    const long long npair = (long long)n * (n + 1) / 2, nn = (long long)n * n;
    if ((in_symmetry != 8 && ld_in < (in_symmetry == 4 ? npair : nn)) || ld_out < (out_symmetry == 4 ? npair : nn))
        return dmk_fail(ctx, DMK_ERR_INVALID, "dmet_h2_scaled: pitch shorter than a row");
    std::vector<unsigned char> mask;
    if (!make_mask(n, imp_idx_host, nimp, mask))
        return dmk_fail(ctx, DMK_ERR_INVALID, "dmet_h2_scaled: impurity indices must lie in [0, %d) without repeats", n);
    const bool same = (const void *)in == (const void *)out && in_symmetry == out_symmetry && ld_in == ld_out;
    if (!same) {
        const char *a0 = reinterpret_cast<const char *>(in), *b0 = reinterpret_cast<const char *>(out);
        const char *a1 = a0 + span_bytes(n, in_symmetry, ld_in), *b1 = b0 + span_bytes(n, out_symmetry, ld_out);
        if (a0 < b1 && b0 < a1)
            return dmk_fail(ctx, DMK_ERR_INVALID, "dmet_h2_scaled: input and output overlap (only in == out with one layout may)");
    }

    // mask (n bytes), class table (npair bytes), pair -> (k, l) table of the 1-fold gather
    const bool need_kl = in_symmetry == 1 && out_symmetry == 4;
    const size_t off_cls = ((size_t)n + 255) & ~(size_t)255, off_kl = off_cls + (((size_t)npair + 255) & ~(size_t)255);
    DevMem tab;
    if (tab.alloc(ctx, off_kl + (need_kl ? (size_t)npair * 4 : 0)) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "dmet_h2_scaled: no memory for the class table");
    }
    unsigned char *d_mask = tab.get<unsigned char>();
    unsigned char *d_cls = d_mask + off_cls;
    unsigned *d_kl = need_kl ? reinterpret_cast<unsigned *>(d_mask + off_kl) : nullptr;
    DMK_HIP(ctx, hipMemcpyAsync(d_mask, mask.data(), (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    {
        FamScope fs(ctx, DMK_FAM_MISC);
        hipLaunchKernelGGL(pair_class_kernel, dim3((unsigned)((nn + NT - 1) / NT)), dim3(NT), 0, ctx->stream, n, d_mask, d_cls, d_kl);
        DMK_CHECK_LAUNCH(ctx);
        ScaleArgs a;
        a.n = n;
        a.nrow = a.ncol = (int)(out_symmetry == 4 ? npair : nn);
        a.in = in; a.out = out; a.ld_in = ld_in; a.ld_out = ld_out;
        a.mask = d_mask; a.cls = d_cls; a.kl = d_kl;
        // 16-byte stores (and loads of the element-for-element forms) need even pitches on 16-byte aligned bases
        bool vec = ((uintptr_t)out % 16 == 0) && ld_out % 2 == 0;
        if (in_symmetry == out_symmetry) vec = vec && ((uintptr_t)in % 16 == 0) && ld_in % 2 == 0;
        if (in_symmetry == 4 && out_symmetry == 4) launch_scale<4, 4>(ctx, a, vec);
        else if (in_symmetry == 1 && out_symmetry == 1) launch_scale<1, 1>(ctx, a, vec);
        else if (in_symmetry == 4 && out_symmetry == 1 && vec && n % 2 == 0)
            hipLaunchKernelGGL(h2_scale_4to1_kernel, dim3(std::min(a.nrow, 16384)), dim3(NT), 0, ctx->stream, a);
        else if (in_symmetry == 4 && out_symmetry == 1) launch_scale<4, 1>(ctx, a, vec);
        else if (in_symmetry == 1 && out_symmetry == 4) launch_scale<1, 4>(ctx, a, vec);
        else launch_scale<8, 4>(ctx, a, vec);
        DMK_CHECK_LAUNCH(ctx);
    }
    DMK_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the tables (and `mask`) are released on return
    return DMK_OK;
}

int dmk_rho_glob(dmk_ctx *ctx, const int mesh[3], int nlo, int neo, int spin, const double *basis, const double *rho_emb,
                 const int32_t *imp_idx_host, int nimp, double *out) {
    if (!ctx) return DMK_ERR_INVALID;
    if (!mesh || mesh[0] <= 0 || mesh[1] <= 0 || mesh[2] <= 0 || (long long)mesh[0] * mesh[1] * mesh[2] >= (1LL << 15) || nlo <= 0 ||
        neo <= 0 || spin < 1 || spin > 2 || !basis || !rho_emb || !out || nimp < 0 || (nimp > 0 && !imp_idx_host))
        return dmk_fail(ctx, DMK_ERR_INVALID, "rho_glob: bad arguments");
    const int ncells = mesh[0] * mesh[1] * mesh[2];
    std::vector<unsigned char> mask;
    if (!make_mask(nlo, imp_idx_host, nimp, mask))
        return dmk_fail(ctx, DMK_ERR_INVALID, "rho_glob: impurity indices must lie in the first cell, [0, %d), without repeats", nlo);
    const long long M = (long long)ncells * nlo;
    if (M > 2097120) return dmk_fail(ctx, DMK_ERR_INVALID, "rho_glob: ncells * nlo too large for one product");
    // W[s] = rho[s] B[s][0]^T (neo x nlo), G[s] = B[s] W[s] (ncells nlo x nlo), mask bytes
    const size_t b_w = (((size_t)spin * neo * nlo * 8) + 255) & ~(size_t)255, b_g = (((size_t)spin * M * nlo * 8) + 255) & ~(size_t)255;
    DevMem ws;
    if (ws.alloc(ctx, b_w + b_g + (size_t)nlo) != hipSuccess) {
        (void)hipGetLastError();
        return dmk_fail(ctx, DMK_ERR_NOMEM, "rho_glob: no memory for the product (%zu bytes)", b_w + b_g);
    }
    double *W = ws.get<double>();
    double *G = reinterpret_cast<double *>(ws.get<char>() + b_w);
    unsigned char *d_mask = ws.get<unsigned char>() + b_w + b_g;
    DMK_HIP(ctx, hipMemcpyAsync(d_mask, mask.data(), (size_t)nlo, hipMemcpyHostToDevice, ctx->stream));
    int rc = dmk_dgemm_batched(ctx, 0, 1, neo, nlo, neo, spin, 1.0, rho_emb, neo, (int64_t)neo * neo, basis, neo, (int64_t)M * neo, 0.0, W,
                               nlo, (int64_t)neo * nlo);
    if (rc == DMK_OK)
        rc = dmk_dgemm_batched(ctx, 0, 0, (int)M, nlo, neo, spin, 1.0, basis, neo, (int64_t)M * neo, W, nlo, (int64_t)neo * nlo, 0.0, G,
                               nlo, (int64_t)M * nlo);
    if (rc == DMK_OK) {
        FamScope fs(ctx, DMK_FAM_MISC);
        const unsigned gx = (unsigned)std::min<long long>(((long long)nlo * nlo + NT - 1) / NT, 64);
        hipLaunchKernelGGL(rho_combine_kernel, dim3(gx, (unsigned)(spin * ncells)), dim3(NT), 0, ctx->stream, mesh[0], mesh[1], mesh[2],
                           nlo, d_mask, G, out);
        DMK_CHECK_LAUNCH(ctx);
    }
    const hipError_t e = hipStreamSynchronize(ctx->stream);      // the workspace is released on return
    if (rc != DMK_OK) return rc;
    if (e != hipSuccess) return dmk_fail(ctx, DMK_ERR_HIP, "rho_glob: %s", hipGetErrorString(e));
    return DMK_OK;
}

}  // extern "C"
