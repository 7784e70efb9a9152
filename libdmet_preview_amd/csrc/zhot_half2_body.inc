// Body of the nemb = 256 step-2 kernel (zhot.hip), included as text where a kernel runs it: half2_kernel and half2_body, the device
// function behind half12_kernel.  In scope at the include: the template parameters LAB, RE; `g` (H2Args); `lds`, H2_LDS complex in
// LDS; ZH_BLOCK_ID, the workgroup's block id within the step-2 grid (before the XCD remap over g.nblocks); SPL and `gw` (H2WArgs):
// the split partner term of type 1 (DESIGN.md K6l) -- with SPL false every `if constexpr (SPL)` folds away and `gw` is never read;
// STRIP (K6m, implies SPL): the triangle [128,256)^2 is covered by a strip (type 4: rows [192,256) x cols [128,256), type 1's geometry
// moved 128 columns to the right, W partner) and a corner (type 5: the triangle [128,192)^2, four block rows) instead of type 3.
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar LDS-DMA addressing
    const int frag_k = lane >> 4, frag_x = lane & 15;
    const unsigned lid = xcd_remap(ZH_BLOCK_ID, g.nblocks);
    // (blockIdx and kernel arguments only: wave-uniform either way)
    int Lall_, type_;
    if constexpr (STRIP) {
        // warm: types 1 and 4 per (L, spin); dense: 0, 1, 2, the corner and the strip
        if (g.skip_invariant) { Lall_ = (int)(lid >> 1); type_ = (lid & 1) ? 4 : 1; }
        else { Lall_ = (int)(lid / 5u); const int t5 = (int)lid - 5 * Lall_; type_ = t5 < 3 ? t5 : t5 == 3 ? 5 : 4; }
    } else {
        Lall_ = g.skip_invariant ? (int)(lid >> 1) : (int)(lid >> 2);
        type_ = g.skip_invariant ? 1 + 2 * (int)(lid & 1) : (int)(lid & 3);
    }
    const int Lall = Lall_, type = type_;
    const int sp = Lall >= g.nL ? 1 : 0;     // nspin <= 2
    const int L = Lall - sp * g.nL;
    const long long nemb = H2_N;
    const int Tb = g.kdim / H2_BK;           // K-tiles per AO block
    const int T = Tb * g.nslot;              // the ring runs straight through all queued blocks
    const double2 *Ubase = g.Ut + (long long)sp * g.ut_spin_stride + (long long)L * g.nao * nemb;
    double *const g_planes = g.planes + (long long)sp * g.planes_spin_stride;
    const long long cj_off = (long long)sp * g.cj_spin_stride;
    const long long g_naux = g.naux, g_npair = g.npair, g_slot_stride = g.slot_stride;
    const unsigned g_symmask = g.symmask;
    const bool fold = g.fold_diag != 0;
    // C_j of queued block SLOT: the pointer of the launch, or (SPL) through the packed k_j
#define ZH_CJ(SLOT) (SPL ? gw.C + cj_off + (long long)H2_PICK_K2(gw.kj2, SLOT) * (g.nao * nemb) : H2_PICK_CJ(g, SLOT) + cj_off)

    if (STRIP ? (type == 2 || type == 5) : type >= 2) {
        // ---------------- diagonal triangle [d0, d0+128)^2 ----------------------------------------
        // (STRIP, type 5: the same panels at d0 = 128, of which only block rows 0-3 -- the corner [128,192)^2 -- are computed)
        const int d0 = STRIP ? (type == 5 ? 128 : 0) : (type - 2) * 128;
        // stage = 16 pieces of 64 complex: piece p < 8 -> U row p/2, half p%2 ; p >= 8 -> C likewise; 4 pieces per wave
        unsigned voff[4];                      // byte offset of this lane's 16 B inside a K-tile of the operand
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int piece = wave + 4 * h;
            voff[h] = (unsigned)((((piece & 7) >> 1) * (int)nemb + d0 + (piece & 1) * 64 + lane) * 16);
        }
        // running issue state (wave-uniform, SGPRs): no division and no kernel-argument load per K-tile
        int is_t = 0, is_slot = 0, is_stage = 0;
        const double2 *is_ub = Ubase, *is_cb = ZH_CJ(0);
        // (spreading the four pieces of a tile over the MFMA stream of a K step, instead of a burst after the barrier,
        // measured 2.5 % slower: the inline-asm DMA statements pin the compiler's MFMA / ds_read schedule)
        auto issue_advance = [&]() {
            is_stage = is_stage + 1 == H2T_D ? 0 : is_stage + 1;
            if (++is_t == Tb) {
                is_t = 0;
                ++is_slot;
                is_ub = Ubase + (long long)is_slot * g_slot_stride;
                is_cb = ZH_CJ(is_slot);
            } else {
                is_ub += H2_BK * nemb;
                is_cb += H2_BK * nemb;
            }
        };
        auto issue = [&]() {
            double2 *st = lds + is_stage * H2T_STAGE;
            // scalar tile bases + loop-invariant per-lane byte offsets: no vector ALU work per piece (common.h glds16s_x4)
            glds16s_x4(voff[0], voff[1], voff[2], voff[3], is_ub, is_ub, is_cb, is_cb, lds_addr_of(st + wave * 64),
                       lds_addr_of(st + (wave + 4) * 64), lds_addr_of(st + (wave + 8) * 64), lds_addr_of(st + (wave + 12) * 64));
            issue_advance();
        };
        auto run = [&](auto tag, auto tag2) {
            constexpr int R1 = decltype(tag)::value;
            constexpr int R2 = decltype(tag2)::value;
            cacc acc1[R1 + 1], acc2[R2 + 1];
#pragma unroll
            for (int c = 0; c <= R1; ++c) cacc_zero(acc1[c]);
#pragma unroll
            for (int c = 0; c <= R2; ++c) cacc_zero(acc2[c]);
            issue();
            if (T > 1) issue();
            if (T > 2) issue();
            int c_t = 0, c_stage = 0;
            unsigned c_sym = g_symmask & 1u, c_mask = g_symmask;
            for (int t = 0; t < T; ++t) {
                const int later = T - 1 - t;
                if (later >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else if (later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if constexpr (!(LAB & 4)) __builtin_amdgcn_s_barrier();
                if constexpr (LAB & 2) { if (t + 3 < T && g.nslot < 0) issue(); }
                else { if (t + 3 < T) issue(); }
                const double2 *U = lds + c_stage * H2T_STAGE + frag_k * 128 + frag_x;
                c_stage = c_stage + 1 == H2T_D ? 0 : c_stage + 1;
                const double2 *C = U + H2_BK * 128;
                {   // segment 1: S[a][b] += U[q][a] C[q][b]   (one B fragment live at a time)
                    const cfrag a1 = cfrag_of_t<RE>(lds_frag(&U[R1 * 16])), a2 = cfrag_of_t<RE>(lds_frag(&U[R2 * 16]));
#pragma unroll
                    for (int c = 0; c <= R2; ++c) {
                        const cfrag b = cfrag_of_t<RE>(lds_frag(&C[c * 16]));
                        if (c <= R1) cmfma_t<RE>(acc1[c <= R1 ? c : 0], a1, b);
                        cmfma_t<RE>(acc2[c], a2, b);
                    }
                }
                if (c_sym) {   // segment 2: S[a][b] += C[q][a] U[q][b]   (same two panels)
                    const cfrag a1 = cfrag_of_t<RE>(lds_frag(&C[R1 * 16])), a2 = cfrag_of_t<RE>(lds_frag(&C[R2 * 16]));
#pragma unroll
                    for (int c = 0; c <= R2; ++c) {
                        const cfrag b = cfrag_of_t<RE>(lds_frag(&U[c * 16]));
                        if (c < R1 || (c == R1 && !fold)) cmfma_t<RE>(acc1[c <= R1 ? c : 0], a1, b);
                        if (c < R2 || !fold) cmfma_t<RE>(acc2[c], a2, b);
                    }
                }
                if (++c_t == Tb) {
                    c_t = 0;
                    c_mask >>= 1;
                    c_sym = c_mask & 1u;
                }
            }
            if (fold) {
                // diagonal blocks hold P = U_r^T C_r only: add P^T through a wave-private LDS tile (the ring is idle now)
                __syncthreads();
                double *tr = reinterpret_cast<double *>(lds) + wave * (2 * 16 * 17);
                auto fold_block = [&](cacc &acc) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tr[(frag_k + 4 * r) * 17 + frag_x] = cacc_re(acc, r);
                        if constexpr (!RE) tr[272 + (frag_k + 4 * r) * 17 + frag_x] = cacc_im(acc, r);
                    }
                    double tre[4], tim[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {                      // the LDS pipe keeps a wave's own accesses in order
                        tre[r] = tr[frag_x * 17 + frag_k + 4 * r];
                        tim[r] = RE ? 0.0 : tr[272 + frag_x * 17 + frag_k + 4 * r];
                    }
                    // fold into the T1 / T2 / T3 representation: Re += tre, Im += tim  (T1 += tre, T3 += tre + tim)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        acc.p[r] += tre[r];
                        if constexpr (!RE) acc.t[r] += tre[r] + tim[r];
                    }
                };
                fold_block(acc1[R1]);
                fold_block(acc2[R2]);
            }
            if constexpr (LAB & 1) { if (g.nslot >= 0) return; }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row1 = d0 + R1 * 16 + frag_k + 4 * r, row2 = d0 + R2 * 16 + frag_k + 4 * r;
#pragma unroll
                for (int c = 0; c <= R1; ++c)
                    pack_acc_t<RE>(g_planes, g_naux, g_npair, L, row1, d0 + c * 16 + frag_x, acc1[c], r);
#pragma unroll
                for (int c = 0; c <= R2; ++c)
                    pack_acc_t<RE>(g_planes, g_naux, g_npair, L, row2, d0 + c * 16 + frag_x, acc2[c], r);
            }
        };
        if constexpr (STRIP) {
            if (type == 5) {
                // the corner: block rows paired (w, 3 - w), 5 of its 10 blocks each on waves 0 and 1 -- every accumulator sees the
                // products type 3 of the other orders gives it, in the same sequence; waves 2 and 3 feed the ring and keep the barriers
                if (wave == 0) run(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
                else if (wave == 1) run(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
                else {
                    issue();
                    if (T > 1) issue();
                    if (T > 2) issue();
                    for (int t = 0; t < T; ++t) {
                        const int later = T - 1 - t;
                        if (later >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                        else if (later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                        __builtin_amdgcn_s_barrier();
                        if (t + 3 < T) issue();
                    }
                    if (fold) __syncthreads();
                }
                return;
            }
        }
        switch (wave) {
            case 0: run(std::integral_constant<int, 0>{}, std::integral_constant<int, 7>{}); break;
            case 1: run(std::integral_constant<int, 1>{}, std::integral_constant<int, 6>{}); break;
            case 2: run(std::integral_constant<int, 2>{}, std::integral_constant<int, 5>{}); break;
            default: run(std::integral_constant<int, 3>{}, std::integral_constant<int, 4>{}); break;
        }
        return;
    }

    // ---------------- off-diagonal half square: rows [r0, r0+64) x cols [0,128) -------------------------
    const int r0 = STRIP ? (type == 0 ? 128 : 192) : 128 + 64 * type;
    const int cb0 = (STRIP && type == 4) ? 128 : 0;       // first column of the Cb and Ub (C_i) pieces and of the output
    const int wm = wave >> 1, wn = wave & 1;            // wave tile 32 x 64
    // SPL, type 1: the partner segment is S[a][b] += sum_p W[p][a] conj(C_i[p][b]) -- the Ca pieces are rows of the W panel (64
    // columns), the Ub pieces rows of C_i (columns [0,128), conjugated at the fragment read); type 0 keeps Ca / Ub.
    // The pieces of a block WITHOUT the partner term are streamed all the same (the ring does not branch per block): its W panel was
    // never written (halfw_body skips it) and holds whatever the buffer held -- deliberate, the loads stay inside the allocation and
    // c_sym gates every MFMA that would read them.  Likewise columns [0,128) of Ut are stale on a warm kL: only type 0 reads them.
    bool wpart = false;
    if constexpr (SPL) wpart = STRIP ? type != 0 : type == 1;
    const double csign = wpart ? -1.0 : 1.0;
    // stage = 24 pieces of 64 complex: 0-3 Ua rows, 4-11 Cb (row*2+half), 12-15 Ca rows, 16-23 Ub (row*2+half)
    unsigned voff[6];
#pragma unroll
    for (int h = 0; h < 6; ++h) {
        const int piece = wave + 4 * h;
        int row, col;
        if (piece < 4) { row = piece; col = r0; }
        else if (piece < 12) { row = (piece - 4) >> 1; col = cb0 + ((piece - 4) & 1) * 64; }
        else if (piece < 16) { row = piece - 12; col = r0; }
        else { row = (piece - 16) >> 1; col = cb0 + ((piece - 16) & 1) * 64; }
        voff[h] = (unsigned)((row * (int)nemb + col + lane) * 16);
        if constexpr (SPL) { if (wpart && piece >= 12 && piece < 16) voff[h] = (unsigned)((row * 64 + lane) * 16); }
    }
    int is_t = 0, is_slot = 0, is_stage = 0;
    const double2 *is_ub = Ubase, *is_cb = ZH_CJ(0);
    const double2 *is_wb = nullptr, *is_ci = nullptr;
    if constexpr (SPL) {
        is_wb = gw.W + (long long)sp * gw.w_spin_stride + (long long)L * g.nao * 64;
        is_ci = gw.C + cj_off + (long long)H2_PICK_K2(gw.ki2, 0) * (g.nao * nemb);
    }
    auto issue = [&]() {
        double2 *st = lds + is_stage * H2S_STAGE;
        // pieces wave + 4 h: h = 0 Ua, 1-2 Cb, 3 Ca, 4-5 Ub -- which operand a piece belongs to does not depend on the wave, so the
        // bases are the two scalar tile pointers and the per-lane part is a loop-invariant byte offset (common.h glds16s_x6)
        if constexpr (SPL) {
            const double2 *const s3 = wpart ? is_wb : is_cb, *const s45 = wpart ? is_ci : is_ub;       // wave-uniform
            glds16s_x6(voff[0], voff[1], voff[2], voff[3], voff[4], voff[5], is_ub, is_cb, is_cb, s3, s45, s45, lds_addr_of(st + wave * 64),
                       lds_addr_of(st + (wave + 4) * 64), lds_addr_of(st + (wave + 8) * 64), lds_addr_of(st + (wave + 12) * 64),
                       lds_addr_of(st + (wave + 16) * 64), lds_addr_of(st + (wave + 20) * 64));
        } else {
        glds16s_x6(voff[0], voff[1], voff[2], voff[3], voff[4], voff[5], is_ub, is_cb, is_cb, is_cb, is_ub, is_ub, lds_addr_of(st + wave * 64),
                   lds_addr_of(st + (wave + 4) * 64), lds_addr_of(st + (wave + 8) * 64), lds_addr_of(st + (wave + 12) * 64),
                   lds_addr_of(st + (wave + 16) * 64), lds_addr_of(st + (wave + 20) * 64));
        }
        is_stage = is_stage + 1 == H2S_D ? 0 : is_stage + 1;
        if (++is_t == Tb) {
            is_t = 0;
            ++is_slot;
            is_ub = Ubase + (long long)is_slot * g_slot_stride;
            is_cb = ZH_CJ(is_slot);
            if constexpr (SPL) {
                is_wb += H2_BK * 64 + (long long)(g.nL - 1) * g.nao * 64;       // the same L of the next block (dense layout)
                is_ci = gw.C + cj_off + (long long)H2_PICK_K2(gw.ki2, is_slot) * (g.nao * nemb);
            }
        } else {
            is_ub += H2_BK * nemb;
            is_cb += H2_BK * nemb;
            if constexpr (SPL) {
                is_wb += H2_BK * 64;
                is_ci += H2_BK * nemb;
            }
        }
    };
    cacc acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cacc_zero(acc[i][j]);
    issue();
    if (T > 1) issue();
    int c_t = 0, c_stage = 0;
    unsigned c_sym = g_symmask & 1u, c_mask = g_symmask;
    for (int t = 0; t < T; ++t) {
        if (t + 1 < T) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (!(LAB & 4)) __builtin_amdgcn_s_barrier();
        if constexpr (LAB & 2) { if (t + 2 < T && g.nslot < 0) issue(); }
        else { if (t + 2 < T) issue(); }
        const double2 *Ua = lds + c_stage * H2S_STAGE + frag_k * 64 + wm * 32 + frag_x;
        const double2 *Cb = lds + c_stage * H2S_STAGE + 256 + frag_k * 128 + wn * 64 + frag_x;
        c_stage = c_stage + 1 == H2S_D ? 0 : c_stage + 1;
        const double2 *Ca = Ua + 768;
        const double2 *Ub = Cb + 768;
        {
            cfrag a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = cfrag_of_t<RE>(lds_frag(&Ua[i * 16]));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = cfrag_of_t<RE>(lds_frag(&Cb[j * 16]));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cmfma_t<RE>(acc[i][j], a[i], b[j]);
        }
        if (c_sym) {
            cfrag a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = cfrag_of_t<RE>(lds_frag(&Ca[i * 16]));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (SPL) {
                    double2 v = lds_frag(&Ub[j * 16]);
                    v.y *= csign;                       // conj(C_i) on the W path; type 0 multiplies by one
                    b[j] = cfrag_of_t<RE>(v);
                } else {
                    b[j] = cfrag_of_t<RE>(lds_frag(&Ub[j * 16]));
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) cmfma_t<RE>(acc[i][j], a[i], b[j]);
        }
        if (++c_t == Tb) {
            c_t = 0;
            c_mask >>= 1;
            c_sym = c_mask & 1u;
        }
    }
    if constexpr (LAB & 1) { if (g.nslot >= 0) return; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + wm * 32 + i * 16 + frag_k + 4 * r;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                pack_acc_t<RE>(g_planes, g_naux, g_npair, L, row, cb0 + wn * 64 + j * 16 + frag_x, acc[i][j], r);      // (strip: b <= a only)
        }
#undef ZH_CJ
