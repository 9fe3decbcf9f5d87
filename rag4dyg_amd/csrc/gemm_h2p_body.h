// The body of gemm_h2p_kernel and gemm_h2p_rowmap_kernel (gemm_h2p.hip), included as TEXT inside both (no include guard): as a
// function it changes the register allocation of the kernels that exist (tools/isa_equal.py).  The including kernel provides
// BM, BN, EPI, OUT_LINES, WGM, WGN, ROWMAP (compile-time), Al, Bp, Cg, biasg, residg, the shape `g` and the row-block map `rm`
// (read with ROWMAP only: the kernels without it get no new code).
    constexpr int NW = WGM * WGN;
    constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 32, TN = WN / 32;
    constexpr int STAGE = (BM + BN) * 8;                              // uint4 units: a row = 8 slots of 16 bytes (hi 0..3, lo' 4..7, XOR-ed)
    constexpr int NBUF = 3;
    constexpr int NGA = BM / 8 / NW, NGB = BN / 8 / NW;               // 8-row groups per wavefront and k-tile: 2 of A, 4 (2) of W with 8 wavefronts
    constexpr int NDMA = NGA + NGB;
    // a lane owns two neighbouring columns: the 128 x 256 tile of gemm_h2p_kernel, every output but the h2 words.  (The h2-word c_attn
    // was built on the pair mapping too -- 8-byte word stores, the K slot by ONE exchange stage -- and measured no faster per launch,
    // 312 against 311 us; the row-block map on it did not reproduce the full launch's bits, cause not found: DESIGN_LOG 12.30.  Both
    // keep one column per lane)
    constexpr bool PAIRS = TN == 2 && !ROWMAP && EPI != EPI_H2WORDS;
    static_assert(BM == 128 && (BN == 256 || BN == 128) && TM >= 1 && TN >= 1 && (NGA == 2 || NGA == 4) && (NGB == 2 || NGB == 4 || NGB == 8), "tile");
    __shared__ u32x4 lds[NBUF * STAGE];

    static_assert(!ROWMAP || (EPI == EPI_H2WORDS && !OUT_LINES), "row-block map: the h2-word c_attn only");
    int m0, n0;
    if constexpr (ROWMAP) {
        // how many blocks are listed is known on the device only: the first tiles_m * tiles_n workgroups of the worst-case grid walk
        // them in the grouped order of a grid of THAT size, so every XCD keeps an equal share (cut off at the listed row panels
        // instead, the XCDs that own the later panels idle: measured, no faster than the full launch); the rest return before a copy is issued
        const int tiles_m = rm.hdr[0] >> 2, tiles_n = (g.N + BN - 1) / BN, nreal = tiles_m * tiles_n;
        if ((int)blockIdx.x >= nreal) return;                         // (wave-uniform)
        grouped_tile<BM, BN>(tiles_m, tiles_n, (int)blockIdx.x, nreal, m0, n0);
    } else {
        grouped_tile<BM, BN>(g.M, g.N, m0, n0);                      // XCD-aware grouped tile order
    }
    const int nkt = g.K / 32;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid / WGN, wn = wid % WGN;
    const int li = lane & 31, lh = lane >> 5;

    // DMA lane offsets (bytes from the operand's base; the k-tile is added to the scalar base): group j = rows 8j .. 8j+7 of the tile
    unsigned va[NGA], vb[NGB];
    const int lrow = lane >> 3, lslot = lane & 7;
#pragma unroll
    for (int i = 0; i < NGA; ++i) {
        const int r = (wid * NGA + i) * 8 + lrow;                     // row of the A tile
        int arow;
        if constexpr (ROWMAP) {
            const int gr = rm.list[(m0 + r) >> 5] * 32 + (r & 31);
            arow = gr >= rm.m_tab ? rm.m_tab - 1 : (gr >= rm.m_real && gr < ((rm.m_real + 31) & ~31) ? rm.m_real - 1 : gr);
        } else {
            arow = min(m0 + r, g.M - 1);
        }
        va[i] = (unsigned)arow * (unsigned)(g.K * 4) + 16u * (unsigned)(lslot ^ ((r >> 1) & 7)) + 3072u - 1024u * (i & 3);
    }
#pragma unroll
    for (int i = 0; i < NGB; ++i) {
        const int r = (wid * NGB + i) * 8 + lrow;                     // row of the W tile's LDS image
        // PAIRS: image row 64a + 32j + l holds W row 64a + 2l + j, so that lane l of accumulator tiles j = 0 / 1 holds the
        // NEIGHBOURING columns 2l, 2l + 1.  Only the source moves: the image, the swizzle and every sum stay what they were
        const int rs = PAIRS ? (r & ~63) + 2 * (r & 31) + ((r >> 5) & 1) : r;
        vb[i] = (unsigned)min(n0 + rs, g.N - 1) * (unsigned)(g.K * 4) + 16u * (unsigned)(lslot ^ ((r >> 1) & 7)) + 3072u - 1024u * (i & 3);
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)lds);
    const unsigned wid_s = __builtin_amdgcn_readfirstlane((unsigned)wid);     // wave-uniform: the DMA destinations live in SGPRs (M0)
    const unsigned dst_a = lds0 + (wid_s * NGA) * 1024u, dst_b = lds0 + ((unsigned)(BM / 8) + wid_s * NGB) * 1024u;
    const char* abase = reinterpret_cast<const char*>(Al) - 3072;     // (the lane offsets carry + 3 KB - i KB: never negative, whatever the shape)
    const char* bbase = reinterpret_cast<const char*>(Bp) - 3072;
#define H2P_ISSUE(KT, STG)                                                                         \
    {                                                                                              \
        const unsigned so_ = (unsigned)(STG) * (unsigned)(STAGE * 16);                             \
        if constexpr (NGA == 4) h2p_dma4(abase + (size_t)(KT) * 128, va[0], va[1], va[2], va[3], dst_a + so_); \
        else h2p_dma2(abase + (size_t)(KT) * 128, va[0], va[1], dst_a + so_);                      \
        if constexpr (NGB == 8) {                                                                  \
            h2p_dma4(bbase + (size_t)(KT) * 128, vb[0], vb[1], vb[2], vb[3], dst_b + so_);          \
            h2p_dma4(bbase + (size_t)(KT) * 128, vb[4], vb[5], vb[6], vb[7], dst_b + so_ + 4096u);  /* same global base: only M0 moves */ \
        } else if constexpr (NGB == 4) h2p_dma4(bbase + (size_t)(KT) * 128, vb[0], vb[1], vb[2], vb[3], dst_b + so_); \
        else h2p_dma2(bbase + (size_t)(KT) * 128, vb[0], vb[1], dst_b + so_);                       \
    }

    // fragment addresses: lane (row li of its 32-row tile, half lh), k-step s, plane p -> slot (4p + 2s + lh) ^ ((li >> 1) & 7)
    const int fsw = (li >> 1) & 7;
    int f_off[2][2];                                                 // [k-step][plane]
#pragma unroll
    for (int s_ = 0; s_ < 2; ++s_)
#pragma unroll
        for (int p = 0; p < 2; ++p) f_off[s_][p] = li * 8 + ((4 * p + 2 * s_ + lh) ^ fsw);
    const int fa_base = wm * WM * 8, fb_base = BM * 8 + wn * WN * 8;

    f32x16 acc0[TM][TN], acc1[TM][TN];                  // hi.hi  /  the two cross terms (factor 2^11)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[i][j][r] = 0.f; acc1[i][j][r] = 0.f; }

#define H2P_MFMA(ACC, A_, B_, I_, J_) \
    ACC[I_][J_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A_), __builtin_bit_cast(f16x8, B_), ACC[I_][J_], 0, 0, 0);
    u32x4 fa[2][TM][2], fb[2][TN][2];                   // two fragment sets: the reads of k-step s+1 travel under the MFMAs of k-step s
#define H2P_FRAGS(SET, STG, S)                                                                     \
    {                                                                                              \
        const u32x4* st_ = lds + (STG) * STAGE;                                                   \
        /* in the order the MFMAs want them: lo(A) . hi(B) first */                                \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[SET][i][1] = st_[fa_base + i * 256 + f_off[S][1]]; \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[SET][j][0] = st_[fb_base + j * 256 + f_off[S][0]]; \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) fa[SET][i][0] = st_[fa_base + i * 256 + f_off[S][0]]; \
        _Pragma("unroll") for (int j = 0; j < TN; ++j) fb[SET][j][1] = st_[fb_base + j * 256 + f_off[S][1]]; \
    }
    /* gemm_h2.hip's order: consecutive MFMAs go to different accumulators; the two writes of one acc1 tile are TM TN instructions apart */
#define H2P_MFMAS(SET)                                                                             \
    {                                                                                              \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) H2P_MFMA(acc1, fa[SET][i][1], fb[SET][j][0], i, j) \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) H2P_MFMA(acc0, fa[SET][i][0], fb[SET][j][0], i, j) \
        _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j) H2P_MFMA(acc1, fa[SET][i][0], fb[SET][j][1], i, j) \
    }

    // prologue: k-tiles 0 and 1 on their way, k-tile 0 landed for everybody, k-step 0 of it in fragment set 0
    H2P_ISSUE(0, 0)
    if (nkt > 1) { H2P_ISSUE(1, 1) h2p_wait_vm<NDMA>(); } else { h2p_wait_vm<0>(); }
    __syncthreads();
    H2P_FRAGS(0, 0, 0)

    constexpr int NMF = 3 * TM * TN, NFR = 2 * (TM + TN);
    static_assert(NMF >= NFR, "interleave");
    // iteration kt (stage CUR = kt % 3 landed and visible, fragment set 0 = its k-step 0):
    //   the DMA of k-tile kt + 2 into stage (kt + 2) % 3 -- last read in iteration kt - 1, in front of that iteration's barrier;
    //   k-step 0's MFMAs with the reads of k-step 1 (set 1) between them;
    //   wait for the wave's own copies of k-tile kt + 1 (all but the NDMA just issued), barrier: k-tile kt + 1 is in LDS for everybody
    //   and nobody reads stage CUR's k-step 1 any more ... (the fragments are in registers: lgkmcnt(0) in front of the barrier);
    //   k-step 1's MFMAs with the reads of k-step 0 of stage NXT between them.
#define H2P_ITER(CUR, NXT, WR)                                                                     \
    {                                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        const bool more_ = kt + 2 < nkt;                                                           \
        if (more_) H2P_ISSUE(kt + 2, WR)                                                           \
        H2P_FRAGS(1, CUR, 1)                                                                       \
        H2P_MFMAS(0)                                                                               \
        _Pragma("unroll") for (int m_ = 0; m_ < NMF; ++m_) {                                       \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
            if (m_ < NFR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                       \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        if (more_) h2p_wait_vm<NDMA>(); else h2p_wait_vm<0>();                                     \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");                            \
        H2P_FRAGS(0, NXT, 0)                                                                       \
        H2P_MFMAS(1)                                                                               \
        _Pragma("unroll") for (int m_ = 0; m_ < NMF; ++m_) {                                       \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
            if (m_ < NFR) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                       \
        }                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                         \
    }
    // (in the last iteration stage NXT holds nothing new: its k-step-0 reads fetch stale bytes nobody multiplies)
    int kt = 0;
    for (; kt + 2 < nkt; kt += 3) {                                   // compile-time stages
        H2P_ITER(0, 1, 2)
        { ++kt; H2P_ITER(1, 2, 0) }
        { ++kt; H2P_ITER(2, 0, 1) }
        kt -= 2;
    }
    if (kt < nkt) {                                                   // kt is a multiple of 3 here: one or two k-tiles left
        H2P_ITER(0, 1, 2)
        if (kt + 1 < nkt) { ++kt; H2P_ITER(1, 2, 0) }
    }
#undef H2P_ITER
#undef H2P_FRAGS
#undef H2P_MFMAS
#undef H2P_MFMA
#undef H2P_ISSUE

    // epilogue on value = (acc0 + 2^-11 acc1) * unscale.  Beside its f16x2-line output this file keeps its OWN copy of the row-major
    // epilogue (the arithmetic of gemm_epilogue_rowmajor.h as gemm_h2.hip uses it; helpers from gemm_common.h): it gathers the 16 words of
    // an accumulator tile ahead of their stores, so that the K third of the h2-word output can go to the key-blocked image 16 bytes at
    // a time.  Through the shared text the six row-major kernels without h2 words get another instruction order, and with a
    // gathered-stores switch in that text the 128 x 256 residual kernel still gets another SGPR assignment (DESIGN_LOG 12.15): unshared.
    constexpr float UNS = H2_A_UNSCALE;
    float* __restrict__ C = Cg;
    const bool interior = ROWMAP || ((m0 + BM <= g.M) & (n0 + BN <= g.N));       // wave-uniform (ROWMAP: whole blocks, N % BN == 0)
    if constexpr (OUT_LINES) {
        // The result as f16x2 lines [M][N/32][2][32] (the A operand of the next GEMM; value / 4 split as split2_pair<true>).  A lane
        // holds ONE column of a 32-column block (= one line) for 16 rows; the two fp16 of a packed word are NEIGHBOURING columns:
        // lanes 2c and 2c+1 swap one value per pair of rows (one DPP move), the even lane then packs row r, the odd lane row r+1 --
        // columns (2c, 2c+1) of its row -- and stores one hi word and one lo' word: as many 4-byte stores as the fp32 epilogue.
        static_assert(EPI == EPI_GELU, "line output: the c_fc epilogue only");
        unsigned char* __restrict__ L = reinterpret_cast<unsigned char*>(Cg);
        const long long row_bytes = (long long)g.N * 4;              // N/32 lines of 128 bytes
        if constexpr (PAIRS) {
            // PAIRS: the lane holds columns (2 li, 2 li + 1) of the wave's 64 in tiles j = 0 / 1 -- one packed word of a line for each of
            // its 32 rows, no exchange.  The value arithmetic and the GELU stay packed over ROW pairs of one tile (adjacent
            // registers), and so do the two scalings of the split; only v_cvt_pk and the two mix instructions take their sources
            // from both tiles (split2_vq).  Stores through a descriptor: lane offset once, the row on the scalar unit
            const int colp = n0 + wn * WN + 2 * li;
            const bool col_ok = colp < g.N;                           // (N % 32 == 0: both columns or none)
            const float bias0 = (biasg && col_ok) ? biasg[colp] : 0.f, bias1 = (biasg && col_ok) ? biasg[colp + 1] : 0.f;
            const int rows_in = min(BM, g.M - m0), cols_in = min(BN, g.N - n0);
            const __amdgpu_buffer_rsrc_t l_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                L + (long long)m0 * row_bytes + (long long)n0 * 4, 0, ((rows_in - 1) * g.N + cols_in) * 4, 0x00020000);
            const int lane_l = (wm * WM + 4 * lh) * (g.N * 4) + (wn * (WN / 32) + (li >> 4)) * 128 + (li & 15) * 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r2 = 0; r2 < 16; r2 += 2) {
                    f32x2 va2 = {__builtin_fmaf(acc1[i][0][r2], H2_LO_UNSCALE, acc0[i][0][r2]) * UNS + bias0,
                                 __builtin_fmaf(acc1[i][0][r2 + 1], H2_LO_UNSCALE, acc0[i][0][r2 + 1]) * UNS + bias0};
                    f32x2 vb2 = {__builtin_fmaf(acc1[i][1][r2], H2_LO_UNSCALE, acc0[i][1][r2]) * UNS + bias1,
                                 __builtin_fmaf(acc1[i][1][r2 + 1], H2_LO_UNSCALE, acc0[i][1][r2 + 1]) * UNS + bias1};
                    va2 = gelu_new2(va2);
                    vb2 = gelu_new2(vb2);
                    const f32x2 sa = va2 * H2_A_PRESCALE, sb = vb2 * H2_A_PRESCALE;
                    const f32x2 qa = va2 * (H2_A_PRESCALE * H2_LO_SCALE), qb = vb2 * (H2_A_PRESCALE * H2_LO_SCALE);
                    unsigned h[2], l[2];
                    split2_vq(sa.x, sb.x, qa.x, qb.x, h[0], l[0]);   // row r2
                    split2_vq(sa.y, sb.y, qa.y, qb.y, h[1], l[1]);   // row r2 + 1
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        const int rr = i * 32 + ((r2 + t) & 3) + 8 * ((r2 + t) >> 2);      // row of the wave tile, less 4 lh
                        if (interior || (m0 + wm * WM + rr + 4 * lh < g.M && col_ok)) {
                            __builtin_amdgcn_raw_buffer_store_b32(h[t], l_rsrc, lane_l, rr * (g.N * 4), 0);
                            __builtin_amdgcn_raw_buffer_store_b32(l[t], l_rsrc, lane_l + 64, rr * (g.N * 4), 0);     // the lo' half of the line
                        }
                    }
                }
            }
            return;
        }
        const bool odd = li & 1;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int colb = n0 + wn * WN + j * 32;                   // first column of the block: line colb / 32
            const bool col_ok = colb + li < g.N;                      // (N % 32 == 0: a block is in or out as a whole)
            const float bias = (biasg && col_ok) ? biasg[colb + li] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r2 = 0; r2 < 16; r2 += 2) {
                    f32x2 v2 = {__builtin_fmaf(acc1[i][j][r2], H2_LO_UNSCALE, acc0[i][j][r2]) * UNS + bias,
                                __builtin_fmaf(acc1[i][j][r2 + 1], H2_LO_UNSCALE, acc0[i][j][r2 + 1]) * UNS + bias};
                    v2 = gelu_new2(v2);
                    const float vx = v2.x, vy = v2.y;                 // rows r2 and r2 + 1 of this lane's column
                    const float send = odd ? vx : vy;
                    const float recv = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, send), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
                    const float c0 = odd ? recv : vx, c1 = odd ? vy : recv;      // columns (2c, 2c+1) of row r2 (even lane) / r2 + 1 (odd lane)
                    unsigned h, l;
                    split2_pair<true>(c0, c1, h, l);
                    const int r = r2 + (odd ? 1 : 0);
                    const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (interior || (row < g.M && col_ok)) {
                        unsigned* dst = reinterpret_cast<unsigned*>(L + (long long)row * row_bytes + (long long)(colb >> 5) * 128 + (li >> 1) * 4);
                        dst[0] = h;
                        dst[16] = l;                                  // + 64 bytes: the lo' half of the line
                    }
                }
            }
        }
        return;
    } else {
        if constexpr (PAIRS) {
            // PAIRS: the lane holds columns (2 li, 2 li + 1) of the wave's 64 in tiles j = 0 / 1 for each of its 32 rows: 8-byte stores
            // and residual loads, half as many instructions, each still whole lines (residual launch 266 -> 262 us in the bench
            // step).  An odd row stride takes the element-wise path below (the 8-byte accesses need dword alignment only, which
            // every shape has; with even strides they are 8-byte aligned wherever the base pointers are)
            if (interior && ((g.ldc | (EPI == EPI_RESIDUAL ? g.ldr : 0)) & 1) == 0) {
                const int cb = n0 + wn * WN;
                const int lane_c = ((wm * WM + 4 * lh) * g.ldc + wn * WN + 2 * li) * 4;
                const int lane_r = ((wm * WM + 4 * lh) * g.ldr + wn * WN + 2 * li) * 4;
                const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    C + (long long)m0 * g.ldc + n0, 0, ((BM - 1) * g.ldc + BN) * 4, 0x00020000);
                const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(EPI == EPI_RESIDUAL ? residg + (long long)m0 * g.ldr + n0 : Cg), 0,
                    EPI == EPI_RESIDUAL ? ((BM - 1) * g.ldr + BN) * 4 : 0, 0x00020000);
                const float bias0 = biasg ? biasg[cb + 2 * li] : 0.f, bias1 = biasg ? biasg[cb + 2 * li + 1] : 0.f;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    u32x2 res[16];
                    if (EPI == EPI_RESIDUAL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            res[r] = __builtin_amdgcn_raw_buffer_load_b64(r_rsrc, lane_r, ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldr) * 4, 0);
                    }
                    unsigned o[2][16];
#pragma unroll
                    for (int r2 = 0; r2 < 16; r2 += 2) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float bias = j ? bias1 : bias0;
                            f32x2 v2 = {__builtin_fmaf(acc1[i][j][r2], H2_LO_UNSCALE, acc0[i][j][r2]) * UNS + bias,
                                         __builtin_fmaf(acc1[i][j][r2 + 1], H2_LO_UNSCALE, acc0[i][j][r2 + 1]) * UNS + bias};
                            if (EPI == EPI_GELU) v2 = gelu_new2(v2);
                            else if (EPI == EPI_RESIDUAL) {
                                v2.x += __builtin_bit_cast(float, j ? res[r2].y : res[r2].x);
                                v2.y += __builtin_bit_cast(float, j ? res[r2 + 1].y : res[r2 + 1].x);
                            }
                            const float vx = v2.x, vy = v2.y;     // (copies first: __builtin_bit_cast on an ext-vector ELEMENT reads element 0)
                            o[j][r2] = __builtin_bit_cast(unsigned int, vx); o[j][r2 + 1] = __builtin_bit_cast(unsigned int, vy);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const u32x2 w = {o[0][r], o[1][r]};
                        __builtin_amdgcn_raw_buffer_store_b64(w, c_rsrc, lane_c, ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldc) * 4, 0);
                    }
                }
                return;
            }
        } else if (interior) {
            // ROWMAP: the (wm, i) MFMA tile is ONE listed block: its rows start at that block's first global row (a scalar offset),
            // the resource spans every row
            const int lane_c = (((ROWMAP ? 0 : wm * WM) + 4 * lh) * g.ldc + wn * WN + li) * 4;
            const int lane_r = ((wm * WM + 4 * lh) * g.ldr + wn * WN + li) * 4;
            const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                C + (long long)(ROWMAP ? 0 : m0) * g.ldc + n0, 0, (((ROWMAP ? g.M : BM) - 1) * g.ldc + BN) * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(EPI == EPI_RESIDUAL ? residg + (long long)m0 * g.ldr + n0 : Cg), 0,
                EPI == EPI_RESIDUAL ? ((BM - 1) * g.ldr + BN) * 4 : 0, 0x00020000);
            // EPI_H2WORDS with a key-blocked K image: a 32-column block of the K third is (one head, four steps u0 .. u0+3); the MFMA
            // tile's 32 rows ARE one key block (m0, WM and the tile are multiples of 32): element (row, col) -> chunk (block, head, u),
            // slot [half = (e >> 2) & 1][row & 31][e & 3], e = the column within the head
            const int kd = g.N / 3;
            const __amdgpu_buffer_rsrc_t kb_rsrc = __builtin_amdgcn_make_buffer_rsrc(
                (EPI == EPI_H2WORDS && g.kb_hd) ? g.kblk : reinterpret_cast<unsigned*>(Cg), 0,
                (EPI == EPI_H2WORDS && g.kb_hd) ? ((g.M + 31) / 32) * (kd * 128) : 0, 0x00020000);
            const int lane_kb = (li >> 3) * 1024 + ((li >> 2) & 1) * 512 + ((li & 3) + 4 * lh) * 16;       // chunk (step), half, row slot of the lane after the quad transpose
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float bias = biasg ? biasg[n0 + wn * WN + j * 32 + li] : 0.f;
                const int colb = n0 + wn * WN + j * 32;
                const bool to_kb = EPI == EPI_H2WORDS && g.kb_hd && colb >= kd && colb < 2 * kd;        // wave-uniform
                const int kb_chunk = to_kb ? ((colb - kd) / g.kb_hd) * (g.kb_hd / 8) + ((colb - kd) % g.kb_hd) / 8 : 0;   // head * NSTEP + u0
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int blk = ROWMAP ? __builtin_amdgcn_readfirstlane(rm.list[(m0 + wm * WM + i * 32) >> 5]) : ((m0 + wm * WM + i * 32) >> 5);
                    const int kb_soff = (blk * (kd / 8) + kb_chunk) * 1024;     // bytes: block * (H * NSTEP) chunks of 1 KB
                    const int row_c = ROWMAP ? blk * 32 : i * 32;
                    float res[16];
                    if (EPI == EPI_RESIDUAL) {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            res[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                r_rsrc, lane_r, ((i * 32 + (r & 3) + 8 * (r >> 2)) * g.ldr + j * 32) * 4, 0));
                    }
                    unsigned o[16];
#pragma unroll
                    for (int r2 = 0; r2 < 16; r2 += 2) {
                        f32x2 v2 = {__builtin_fmaf(acc1[i][j][r2], H2_LO_UNSCALE, acc0[i][j][r2]) * UNS + bias,
                                     __builtin_fmaf(acc1[i][j][r2 + 1], H2_LO_UNSCALE, acc0[i][j][r2 + 1]) * UNS + bias};
                        if (EPI == EPI_GELU) v2 = gelu_new2(v2);
                        else if (EPI == EPI_RESIDUAL) { v2.x += res[r2]; v2.y += res[r2 + 1]; }
                        const float vx = v2.x, vy = v2.y;     // (copies first: __builtin_bit_cast on an ext-vector ELEMENT reads element 0)
                        o[r2] = __builtin_bit_cast(unsigned int, vx); o[r2 + 1] = __builtin_bit_cast(unsigned int, vy);
                        if (EPI == EPI_H2WORDS) h2_words<true>(v2.x, v2.y, o[r2], o[r2 + 1]);     // C is the uint32 word image of the result (attention_h2.hip)
                    }
                    if (EPI == EPI_H2WORDS && to_kb) {
                        // registers 4a .. 4a+3 of the four lanes of a quad = rows 8a + (0..3) + 4 lh x the four words of one 16-byte
                        // slot: a 4 x 4 transpose inside the quad (two DPP exchange stages) gives every lane ONE row's slot, and the
                        // wavefront's store covers eight whole 128-byte lines (8 consecutive rows of 8 (step, half) chunks) -- as 4-byte
                        // stores to 16 scattered pieces per instruction the c_attn launch was 80 us longer.  (The same transpose for the
                        // ROW-MAJOR stores of every epilogue -- 16 bytes per lane, four times fewer store instructions -- was measured too:
                        // c_attn 295 -> 307 us, residual 258 -> 261: the VALU work costs more than the stores save.  Not kept.)
                        const bool o1 = li & 1, o2 = li & 2;
#pragma unroll
                        for (int a4 = 0; a4 < 16; a4 += 4) {
                            unsigned x0 = o[a4], x1 = o[a4 + 1], x2 = o[a4 + 2], x3 = o[a4 + 3];
                            {   // stage 1: lanes t ^ 1, registers r ^ 1
                                const unsigned s01 = o1 ? x0 : x1, s23 = o1 ? x2 : x3;
                                const unsigned r01 = (unsigned)__builtin_amdgcn_mov_dpp((int)s01, 0xB1, 0xF, 0xF, true);     // quad_perm [1,0,3,2]
                                const unsigned r23 = (unsigned)__builtin_amdgcn_mov_dpp((int)s23, 0xB1, 0xF, 0xF, true);
                                if (o1) { x0 = r01; x2 = r23; } else { x1 = r01; x3 = r23; }
                            }
                            {   // stage 2: lanes t ^ 2, registers r ^ 2
                                const unsigned s02 = o2 ? x0 : x2, s13 = o2 ? x1 : x3;
                                const unsigned r02 = (unsigned)__builtin_amdgcn_mov_dpp((int)s02, 0x4E, 0xF, 0xF, true);     // quad_perm [2,3,0,1]
                                const unsigned r13 = (unsigned)__builtin_amdgcn_mov_dpp((int)s13, 0x4E, 0xF, 0xF, true);
                                if (o2) { x0 = r02; x1 = r13; } else { x2 = r02; x3 = r13; }
                            }
                            const u32x4 slot = {x0, x1, x2, x3};
                            __builtin_amdgcn_raw_buffer_store_b128(slot, kb_rsrc, lane_kb, kb_soff + 2 * a4 * 16, 0);      // rows 8 (a4 / 4) ..
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            __builtin_amdgcn_raw_buffer_store_b32(o[r], c_rsrc, lane_c, ((row_c + (r & 3) + 8 * (r >> 2)) * g.ldc + j * 32) * 4, 0);
                    }
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {                                   // edge tiles: clamped reads, guarded stores
            const int col = n0 + wn * WN + (PAIRS ? 2 * li + j : j * 32 + li);
            const bool col_ok = col < g.N;
            const int colc = min(col, g.N - 1);
            const float bias = biasg ? biasg[colc] : 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    float v = __builtin_fmaf(acc1[i][j][r], H2_LO_UNSCALE, acc0[i][j][r]) * UNS + bias;
                    if (EPI == EPI_GELU) v = gelu_new1(v);
                    else if (EPI == EPI_RESIDUAL) v += residg[(long long)min(row, g.M - 1) * g.ldr + colc];
                    else if (EPI == EPI_H2WORDS) { unsigned w0, w1; h2_words<true>(v, 0.f, w0, w1); v = __builtin_bit_cast(float, w0); }
                    if (EPI == EPI_H2WORDS && g.kb_hd && col >= g.N / 3 && col < 2 * (g.N / 3)) {      // the K third: key-blocked image
                        const int kd = g.N / 3, e = (col - kd) % g.kb_hd, chunk = ((col - kd) / g.kb_hd) * (g.kb_hd / 8) + (e >> 3);
                        if (row < g.M)
                            g.kblk[((long long)(row >> 5) * (kd / 8) + chunk) * 256 + (((e >> 2) & 1) * 32 + (row & 31)) * 4 + (e & 3)] =
                                __builtin_bit_cast(unsigned, v);
                        continue;
                    }
                    if (row < g.M && col_ok) C[(long long)row * g.ldc + col] = v;
                }
            }
        }
    }
