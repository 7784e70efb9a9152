// Body of the W kernel (zhot.hip, DESIGN.md K6l), included as text like zhot_half1_body.inc.  In scope at the include: `g` (HWArgs);
// `lds`, the ring of H1_D stages of H1_BK * (H1_BM + H1_BN) complex in LDS; ZH_BLOCK_ID, the workgroup's block id within the W grid
// (before the XCD remap over g.nblocks).
//
//   W[L][p][n] = sum_q Lpq[L][p][q] C_j[q][col0 + n],  n < 64        M = the flat row (L, p), K = q
//
// The tile, the wave layout, the B panel and the MFMA stream are those of the step-1 kernel (128 x 64, 2 x 2 waves, BK = 8, six
// LDS-DMA pieces per wave and K tile).  The A operand is K-CONTIGUOUS here (row m of the flat array at m * nao): a piece is eight
// rows by one K tile, lane l fetches (row l & 7, k = l >> 3) -- eight 128-B row segments -- and lands as an [k][8 rows] tile of 64
// complex.  A 16-row fragment read then sees two runs of eight consecutive complex, 1 KiB apart; with k along the lane groups every
// 16-lane group of a 16-B LDS read covers the sixteen 16-B slots of a bank row once: conflict-free without padding.
    constexpr int BM = H1_BM, STAGE = H1_BK * (BM + H1_BN);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int frag_k = lane >> 4, frag_x = lane & 15;

    const unsigned lid_all = xcd_remap(ZH_BLOCK_ID, g.nblocks);
    const int slot = (int)(lid_all / g.per_slot);
    if (!((g.symmask >> slot) & 1u)) return;             // a block without the partner term has no use for W (the whole workgroup leaves)
    const unsigned lid = lid_all - (unsigned)slot * g.per_slot;
    const int tile_m = (int)(lid / (unsigned)g.nspin);
    const int sp = (int)(lid - (unsigned)tile_m * (unsigned)g.nspin);
    const long long nao = g.nao, nemb = g.nemb;
    const long long rows_total = (long long)g.nL * nao;
    const double2 *const Asl = g.Lpq + (long long)slot * g.a_slot_stride;
    const double2 *const Bsp = g.C + (long long)sp * g.c_spin_stride + (long long)H1_PICK_BK(g, slot) * g.c_k_stride;
    double2 *const Osp = g.W + (long long)sp * g.w_spin_stride + (long long)slot * g.w_slot_stride;

    // ---- LDS-DMA sources: wave w streams the A pieces of rows [32 w, 32 w + 32) and the B rows 2w, 2w+1 of the K tile ----
    unsigned voffA[4], voffB;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        long long r = (long long)tile_m * BM + 8 * (4 * wave + h) + (lane & 7);
        if (r >= rows_total) r = rows_total - 1;         // clamped lanes only ever feed masked outputs
        voffA[h] = (unsigned)((r * nao + (lane >> 3)) * 16);
    }
    voffB = (unsigned)((g.col0 + lane) * 16);
    auto issue = [&](int t) {
        double2 *st = lds + (t % H1_D) * STAGE;
        const int k0 = wave * 2;
        const double2 *a = Asl + (long long)t * H1_BK;                                                        // wave-uniform
        const double2 *b0 = Bsp + ((long long)t * H1_BK + k0) * nemb, *b1 = b0 + nemb;
        glds16s_x6(voffA[0], voffA[1], voffA[2], voffA[3], voffB, voffB, a, a, a, a, b0, b1, lds_addr_of(st + (4 * wave) * 64),
                   lds_addr_of(st + (4 * wave + 1) * 64), lds_addr_of(st + (4 * wave + 2) * 64), lds_addr_of(st + (4 * wave + 3) * 64),
                   lds_addr_of(st + H1_BK * BM + k0 * H1_BN), lds_addr_of(st + H1_BK * BM + (k0 + 1) * H1_BN));
    };

    cacc acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) cacc_zero(acc[i][j]);

    const int T = g.nao / H1_BK;
    issue(0);
    if (T > 1) issue(1);
    for (int t = 0; t < T; ++t) {
        if (t + 1 < T) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");      // tile t landed; tile t+1 may be in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (t + 2 < T) issue(t + 2);
        // element (k, m) of the A panel: piece m / 8 (64 complex each), then [k][m % 8]
        const double2 *Ab = lds + (t % H1_D) * STAGE + wm * 512 + (frag_x >> 3) * 64 + frag_k * 8 + (frag_x & 7);
        const double2 *Bb = lds + (t % H1_D) * STAGE + H1_BK * BM + wn * 32 + frag_x;
#pragma unroll
        for (int kk = 0; kk < H1_BK / 4; ++kk) {
            cfrag a[4], b[2];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = cfrag_of(lds_frag(&Ab[kk * 32 + i * 128]));
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = cfrag_of(lds_frag(&Bb[(kk * 4 + frag_k) * H1_BN + j * 16]));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) cmfma(acc[i][j], a[i], b[j]);
        }
    }

    // ---- epilogue: W[L][p][n] = row (L * nao + p) of one contiguous (nL * nao) x 64 array ----------------------------------
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long rr = (long long)tile_m * BM + (wm * 4 + i) * 16 + frag_k + 4 * r;
            if (rr >= rows_total) continue;
            double2 *row = Osp + rr * H1_BN;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                row[wn * 32 + j * 16 + frag_x] = make_double2(cacc_re(acc[i][j], r), cacc_im(acc[i][j], r));
        }
    }
