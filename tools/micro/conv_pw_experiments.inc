// Point-wise GEMM kernels that were built, parity-tested, measured on MI355X and NOT adopted (round 4; DESIGN.md Appendix A
// rows 17-24, 31-33; evidence under profiles/r04_gemm_*, r04_streamk_*): the Stream-K form of the persistent kernel and the
// generalised persistent kernel (eight tile shapes x three pipeline depths x a tile scheduler), with their launchers and
// the run-time tuning entry point.  NOT part of libfgn_hip.so: csrc/conv_igemm.hip includes this file only under
// -DFGN_EXPERIMENTS (tools/micro/build_experiments.sh -> tools/micro/libfgn_hip_exp.so, tools/micro/gemm_clock), in two
// parts: 1 = kernels and tuning state (before the dispatcher's planning helpers), 2 = launchers and dispatcher hooks.
// The C-ABI of the experimental build is the product's plus fgn_conv2d_tune: the workspaces these kernels need (tile
// scheduler counters, Stream-K tickets and slabs) are private to this file - one zero-initialised allocation per device,
// carved up per launch in a ring (launches of ONE stream at a time: these are single-stream timing tools).
#if FGN_EXP_PART == 1
constexpr int FGN_TILE_SCHED_WORDS = 8 * 16;         // conv_pw_persist2_kernel's counters
constexpr int FGN_STREAMK_MAX_GRID = 1280;           // tickets of conv_pw_streamk_kernel: one per remaining tile < grid
constexpr int FGN_SCHED_WORDS = FGN_TILE_SCHED_WORDS + FGN_STREAMK_MAX_GRID;
// (diagnostic builds only: the same without the M0 write - the data lands where the previous load's did)
__device__ __forceinline__ void lds_dma16_s_nom0(const i32x4& rs, unsigned voff, unsigned soff) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2 offen lds" : : "v"(voff), "s"(rs), "s"(soff) : "memory");
}
// 16-byte store that writes through the XCD's L2 to device-coherent memory (sc1 = agent scope): how a workgroup publishes
// a split-K partial tile that a workgroup on another XCD will read (the L2s of the eight XCDs are not coherent with each
// other for plain stores; a release fence instead would write back the whole L2).
__device__ __forceinline__ void store_wt16(float* ptr, const f32x4& v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(ptr), "v"(v) : "memory");
}
// 16-byte load at agent scope (sc1): reads what store_wt16 of a workgroup on another XCD published, without the
// acquire fence's invalidation of this XCD's L2 (which holds the operands every other workgroup is streaming).  The
// caller waits with wait_loads() before it uses the value.
__device__ __forceinline__ f32x4 load_agent16(const float* ptr) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}
__device__ __forceinline__ void wait_loads(f32x4& a, f32x4& b, f32x4& c, f32x4& d) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}

// ------------------------------------------------------------------------------------------------
// Stream-K form of the persistent point-wise kernel (round 4): the work of a launch is tiles x K-tiles, and what
// conv_pw_persist_kernel and the one-tile-per-workgroup kernel lose is the LAST round of whole tiles - 7.31 rounds take
// 7.75 tile times on the AG-RPN GEMM, 408 tiles on 1024 resident slots leave 104 CUs with one workgroup and 152 with two.
// Here the tiles beyond the last full round of the grid (all tiles, when there are fewer than workgroups) are shared out by
// K-TILE: the workgroups of an XCD split the K-tiles of that XCD's remaining tiles into equal contiguous ranges of
// U <= KT K-tiles (a range touches at most two tiles).  A workgroup first runs its range, then its whole tiles
// (tile = blockIdx, + grid, ...) exactly as conv_pw_persist_kernel does.
//   * A range that covers a tile from K-tile 0 to KT - 1 ends in the normal epilogue.
//   * Any other range is a PIECE: the raw 64x64 partial sums go to the workgroup's private slab (ws + (2 * blockIdx +
//     seg) * 4096 floats, seg = 0 if the workgroup's range starts inside this tile, 1 if it started in the tile before)
//     with write-through stores, then one ticket per tile (tickets[remaining tile], zero before the launch and again
//     after it).  The workgroup that draws the last ticket of a tile sums the pieces IN K ORDER (its own from LDS, the
//     others from their slabs: a fixed order whoever comes last - deterministic results), applies the epilogue and
//     stores.  Nobody waits for anybody: no workgroup depends on another one being resident.
// Remaining tiles keep the XCD-contiguous numbering of the whole-tile walk: tile = dp_tiles + 8 * rl + xcd is the rl-th
// remaining tile of XCD xcd's run, and only that XCD's workgroups (blockIdx & 7 == xcd) work on it, so its operands stay
// in one L2.  Per output element the K order is that of the other kernels; the grouping of the partial sums differs
// (pieces are summed after the fact), so results agree with conv_pw_persist_kernel to rounding, not bitwise.
// LDS: the two stages + one flag word.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 4) void conv_pw_streamk_kernel(const ConvParams p, const int total_tiles,
                                                                 const int dp_tiles, const int U, const int dbg) {
    constexpr int BM = 64, BN = 64, WN = 32, WM = 32;
    constexpr int A_LD = 2, B_LD = 2;
    constexpr int STAGE = (BM + BN) * BK;          // floats
    constexpr int PITCH = BN;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int M = (p.n_img_dev ? min(p.n_img, *p.n_img_dev) : p.n_img) * p.Ho * p.Wo;
    int grp_valid = p.grp_valid;
    if (p.grp_rows && p.grp_count_dev) grp_valid = min(grp_valid, min(p.grp_items, *p.grp_count_dev) * p.grp_rows_per_item);

    const int col4 = t & 7, row0 = t >> 3;
    const int src_c4 = col4 ^ ((row0 >> 1) & 7);
    const i32x4 x_rs = make_rsrc(p.x, p.x_bytes);
    const i32x4 w_rs = make_rsrc(p.w, p.w_bytes);
    const int KT = p.K / BK;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<size_t>(smem));
    const unsigned wave_row_bytes = __builtin_amdgcn_readfirstlane(wv) * 8 * 128;
    constexpr unsigned OOB = 0x7ffffff0u;

    const int nq = total_tiles >> 3, nr = total_tiles & 7;
    auto coords = [&](int tile, int& m0, int& n0) -> bool {
        const int xcd = tile & 7, idx = tile >> 3;
        const int bid = (xcd < nr ? xcd * (nq + 1) : nr * (nq + 1) + (xcd - nr) * nq) + idx;
        int tile_m = bid / p.n_tiles_n;
        int tile_n = bid - tile_m * p.n_tiles_n;
        if (p.band_nt > 0) {
            const int per_grp = p.band_mt * p.n_tiles_n;
            const int grp = bid / per_grp;
            int r = bid - grp * per_grp;
            const int per_band = p.band_mt * p.band_nt;
            const int band = r / per_band;
            r -= band * per_band;
            const int mi = r / p.band_nt;
            tile_m = grp * p.band_mt + mi;
            tile_n = band * p.band_nt + (r - mi * p.band_nt);
        }
        m0 = tile_m * BM;
        n0 = tile_n * BN;
        if (m0 >= M) return false;
        if (p.grp_rows && m0 - (m0 / p.grp_rows) * p.grp_rows >= grp_valid) return false;
        return true;
    };

    // this workgroup's share of the remaining tiles' K-tiles: units [u, u_end) of its XCD's run, unit = rl * KT + kt
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    const int rem_x = nq + (xcd < nr ? 1 : 0) - (dp_tiles >> 3);
    const int units_x = rem_x * KT;
    int u = min(li * U, units_x);
    const int u_end = min(u + U, units_x);
    int dp_cur = blockIdx.x;
    struct Item { int m0, n0, k0, k1, rl; };            // rl < 0: a whole tile of the fixed walk
    auto next_item = [&](Item& it) -> bool {
        while (u < u_end) {
            const int rl = u / KT, k0 = u - rl * KT, k1 = min(KT, k0 + (u_end - u));
            u += k1 - k0;
            if (coords(dp_tiles + rl * 8 + xcd, it.m0, it.n0)) {
                it.k0 = k0; it.k1 = k1; it.rl = rl;
                return true;
            }
        }
        for (; dp_cur < dp_tiles; dp_cur += gridDim.x)
            if (coords(dp_cur, it.m0, it.n0)) {
                it.k0 = 0; it.k1 = KT; it.rl = -1;
                dp_cur += gridDim.x;
                return true;
            }
        return false;
    };

    unsigned a_voff[A_LD], b_voff[B_LD];
    auto set_offsets = [&](int m0, int n0) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = m0 + row0 + 32 * i;
            a_voff[i] = m < M ? (unsigned)((m * p.Cin + src_c4 * 4) * 4) : OOB;
        }
        int b0 = ((n0 + row0) * p.K + src_c4 * 4) * 4;
        if (p.grp_rows) b0 += (m0 / p.grp_rows) * p.grp_w_stride * 4;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) b_voff[i] = (unsigned)(b0 + i * 32 * p.K * 4);
    };
    auto issue_tile = [&](int kt, int stage) {
        const unsigned sa = lds_base + stage * (STAGE * 4) + wave_row_bytes;
        const unsigned ko = (unsigned)(kt * BK * 4);
#pragma unroll
        for (int i = 0; i < A_LD; ++i) lds_dma16_s(x_rs, sa + i * 32 * 128, a_voff[i], ko);
        const unsigned sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) lds_dma16_s(w_rs, sb + i * 32 * 128, b_voff[i], ko);
    };

    const int frag_row = lane & 31;
    const float* const rd_a = smem + (wm * WM + frag_row) * BK;
    const float* const rd_b = smem + BM * BK + (wn * WN + frag_row) * BK;
    float* const cbase = smem + STAGE;              // stage 1
    volatile int* const s_last = reinterpret_cast<volatile int*>(smem + 2 * STAGE);
    const int r16 = lane & 15, g16 = lane >> 4;
    constexpr int C4 = BN / 4, RPP = 256 / C4;       // 16 float4 per row, 16 rows per pass
    const int c4 = t % C4, rr = t / C4;

    Item it;
    if (!next_item(it)) return;
    CLOCK_STAMP_BEGIN();
    set_offsets(it.m0, it.n0);
    issue_tile(it.k0, 0);

    while (true) {
        f32x4 acc4[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        int cur = 0;
        for (int kt = it.k0; kt < it.k1; ++kt) {
            if (kt + 1 < it.k1) issue_tile(kt + 1, cur ^ 1);
            asm volatile("" ::: "memory");
            const float* As = rd_a + cur * STAGE;
            const float* Bs = rd_b + cur * STAGE;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                float4 af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int row = r16 + 16 * i;
                    const int pc = ((kk * 4 + g16) ^ ((row >> 1) & 7)) * 4;
                    af[i] = *reinterpret_cast<const float4*>(As + (row - frag_row) * BK + pc);
                    bf[i] = *reinterpret_cast<const float4*>(Bs + (row - frag_row) * BK + pc);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bf[j].x, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bf[j].y, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bf[j].z, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bf[j].w, acc4[i][j], 0, 0, 0);
                    }
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            cur ^= 1;
        }
        // both stages are free: the first K-tile of the next item goes to stage 0 while this one drains through stage 1
        Item nx;
        const bool more = next_item(nx);
        if (more) {
            set_offsets(nx.m0, nx.n0);
            issue_tile(nx.k0, 0);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float* cw = cbase + (wm * WM + 16 * i + 4 * g16) * PITCH + wn * WN + 16 * j + r16;
#pragma unroll
                for (int r = 0; r < 4; ++r) cw[r * PITCH] = acc4[i][j][r];
            }
        __syncthreads();
        const int n = it.n0 + c4 * 4;
        // rl0 / rl1: first and last workgroup (index within the XCD) with K-tiles of this remaining tile
        const bool piece = it.rl >= 0 && (it.k0 != 0 || it.k1 != KT);
        bool reduce = false;
        int i0 = 0, i1 = 0;
        if (piece && dbg == 1) {
            // timing experiment (tuning knob 5): pieces are dropped - WRONG results, the cost of the exchange by difference
        } else if (piece) {
            float* slab = p.ws + ((size_t)blockIdx.x * 2 + ((li * U) / KT == it.rl ? 0 : 1)) * (BM * BN);
#pragma unroll
            for (int k = 0; k < BM / RPP; ++k) {
                const int row = rr + RPP * k;
                const float4 v = *reinterpret_cast<const float4*>(cbase + row * PITCH + c4 * 4);
                store_wt16(slab + row * BN + c4 * 4, f32x4{v.x, v.y, v.z, v.w});
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this thread's slab stores are acknowledged
            __syncthreads();                                        // ... and every thread's
            i0 = (it.rl * KT) / U;
            i1 = (it.rl * KT + KT - 1) / U;
            if (t == 0) {
                int32_t* tk = p.tickets + (it.rl * 8 + xcd);
                const int got = atomicAdd(tk, 1);
                *s_last = got == i1 - i0;
                if (got == i1 - i0) *tk = 0;                        // ready for the next launch
            }
            __syncthreads();
            reduce = *s_last != 0;
        }
        if ((!piece || reduce) && n < p.Cout) {
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + n);
            if (p.shift) sh = *reinterpret_cast<const float4*>(p.shift + n);
            float4 res[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = it.m0 + rr + RPP * k;
                res[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.residual && m < M) res[k] = *reinterpret_cast<const float4*>(p.residual + (size_t)m * p.Cout + n);
            }
            f32x4 sum[4];
            if (reduce) {
                // pieces in K order, whoever came last: the own one from LDS, the others from their slabs (agent-scope loads)
                for (int i = i0; i <= i1; ++i) {
                    f32x4 b[4];
                    if (i == li) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) b[k] = *reinterpret_cast<const f32x4*>(cbase + (rr + RPP * k) * PITCH + c4 * 4);
                    } else {
                        const float* src = p.ws + ((size_t)(i * 8 + xcd) * 2 + ((i * U) / KT == it.rl ? 0 : 1)) * (BM * BN) + c4 * 4;
#pragma unroll
                        for (int k = 0; k < 4; ++k) b[k] = load_agent16(src + (rr + RPP * k) * BN);
                        wait_loads(b[0], b[1], b[2], b[3]);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (i == i0) sum[k] = b[k];
                        else sum[k] += b[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int row = rr + RPP * k;
                const int m = it.m0 + row;
                if (m >= M) continue;
                float4 v;
                if (reduce)
                    v = make_float4(sum[k][0], sum[k][1], sum[k][2], sum[k][3]);
                else
                    v = *reinterpret_cast<const float4*>(cbase + row * PITCH + c4 * 4);
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                v.x += res[k].x; v.y += res[k].y; v.z += res[k].z; v.w += res[k].w;
                if (p.relu) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                *reinterpret_cast<float4*>(p.y + (size_t)m * p.Cout + n) = v;
            }
        }
        if (!more) break;
        it = nx;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CLOCK_STAMP_END(blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Persistent point-wise kernel, second form (round 4): any workgroup tile BM x BN out of wave tiles WM x WN
// (NW = (BM/WM)*(BN/WN) waves), v_mfma_f32_16x16x4_f32 only, and NO LDS round trip in the epilogue.
//   * The MFMA is issued with its operands SWAPPED (B fragment as "A", A fragment as "B"): the 16x16 result tile is then
//     C^T, i.e. lane (c = lane & 15, g = lane >> 4) holds C[m = c][n = 4g .. 4g+3] in its four accumulator registers -
//     four CONSECUTIVE output channels of one row.  The epilogue is one 16-byte global store (and one 16-byte residual
//     load, one 16-byte scale / shift load) per 16x16 tile straight from the accumulators: no C tile in LDS, no
//     epilogue barriers, and the LDS the C tile took is free for a larger operand tile.  (Same products in the same k
//     order as the unswapped form: bit-identical sums.)
//   * Larger tiles: a 64x64 wave tile reads half the LDS bytes per MFMA of the 32x32 one and a 128x128 workgroup tile
//     takes half the L2 -> LDS bytes per MFMA of the 64x64 one - the two largest levers on the clock the chip holds in
//     an MFMA-dense loop (cdna_hip_programming.md 5.4 rule 28) - and runs one barrier per 4096 MFMA cycles of a wave
//     instead of one per 1024.
//   * Fragments of the next 16-deep step are read while the current step's MFMAs issue (two register sets).
//   * Grouped GEMM with any BM: a row tile never straddles two groups (tiles are numbered per group, the last one of a
//     group is cut at the group's valid rows), so t_pad stays a multiple of 64.
// Tile order: XCD-contiguous runs of logical tiles; inside a group band-major ([band][row tile][channel tile of the
// band]) so that a band's weights stay in the XCD's L2 while the group's rows stream past.
// ------------------------------------------------------------------------------------------------
struct Persist2Geom {
    int mt;          // row tiles per group (grouped GEMM) or of the whole launch
    int band_nt;     // channel tiles per band (divides n_tiles_n; n_tiles_n = no banding)
    int n_groups;    // 1 for a plain convolution
};

template <int BM, int BN, int WM, int WN, int NST, int MINW>
__global__ __launch_bounds__((BM / WM) * (BN / WN) * 64, MINW) void conv_pw_persist2_kernel(const ConvParams p,
                                                                                          const Persist2Geom gm,
                                                                                          const int total_tiles) {
    constexpr int NWM = BM / WM, NWN = BN / WN, NW = NWM * NWN;
    constexpr int RPP = NW * 8;                        // tile rows one DMA pass of the workgroup covers
    constexpr int A_LD = BM / RPP, B_LD = BN / RPP;
    constexpr int TI = WM / 16, TJ = WN / 16;
    constexpr int STAGE = (BM + BN) * BK;              // floats
    constexpr int LOADS = A_LD + B_LD;                 // LDS-DMA wave-instructions per K-tile and wave
    static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the DMA pass");
    static_assert(NST >= 2 && NST <= 4 && (NST - 2) * LOADS <= 63, "stages");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wm = wv / NWN, wn = wv - wm * NWN;
    const int M = (p.n_img_dev ? min(p.n_img, *p.n_img_dev) : p.n_img) * p.Ho * p.Wo;
    int grp_valid = p.grp_valid;
    if (p.grp_rows && p.grp_count_dev) grp_valid = min(grp_valid, min(p.grp_items, *p.grp_count_dev) * p.grp_rows_per_item);
    grp_valid = min(grp_valid, p.grp_rows);

    const int col4 = t & 7, row0 = t >> 3;
    const int src_c4 = col4 ^ ((row0 >> 1) & 7);
    const i32x4 x_rs = make_rsrc(p.x, p.x_bytes);
    const i32x4 w_rs = make_rsrc(p.w, p.w_bytes);
    const int KT = p.K / BK;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<size_t>(smem));
    const unsigned wave_row_bytes = __builtin_amdgcn_readfirstlane(wv) * 8 * 128;
    constexpr unsigned OOB = 0x7ffffff0u;

    // Tiles are cut into 8 contiguous shares (one per value of blockIdx & 7: workgroups b and b + 8 sit on one XCD, so a
    // share's operands stay in that XCD's L2); `idx` counts inside this workgroup's share.
    const int nq = total_tiles >> 3, nr = total_tiles & 7;
    const int xk = blockIdx.x & 7, nwg_x = gridDim.x >> 3;
    const int size_x = nq + (xk < nr ? 1 : 0);
    const int start_x = xk < nr ? xk * (nq + 1) : nr * (nq + 1) + (xk - nr) * nq;
    const int per_grp = gm.mt * p.n_tiles_n, per_band = gm.mt * gm.band_nt;
    // tile of the share -> (first row, row limit, first channel, weight offset of the group); false: nothing to compute
    auto coords = [&](int idx, int& m0, int& mend, int& n0, int& wofs) -> bool {
        const int bid = start_x + idx;
        const int grp = bid / per_grp;
        int r = bid - grp * per_grp;
        const int band = r / per_band;
        r -= band * per_band;
        const int mi = r / gm.band_nt;
        n0 = (band * gm.band_nt + (r - mi * gm.band_nt)) * BN;
        if (p.grp_rows) {
            m0 = grp * p.grp_rows + mi * BM;
            mend = min(M, grp * p.grp_rows + grp_valid);
            wofs = grp * p.grp_w_stride;
        } else {
            m0 = mi * BM;
            mend = M;
            wofs = 0;
        }
        return m0 < mend;
    };
    // ---- tile scheduler.  The first tile of a workgroup is idx = blockIdx >> 3 (no atomic in front of the first DMA);
    // every further one is nwg_x + (old value of the share's counter).  Every workgroup ends on exactly one pull past
    // the end of its share, so a share sees max(size_x - nwg_x, 0) + nwg_x pulls in all and the workgroup that draws
    // the last of them returns the counter to zero for the next launch (kernel boundaries order it).  One lane pulls;
    // the value reaches the other waves through one LDS word behind a workgroup barrier.
    int* const s_next = reinterpret_cast<int*>(smem + NST * STAGE);
    int32_t* const counter = p.sched ? p.sched + xk * 16 : nullptr;
    const int pulls_x = max(size_x - nwg_x, 0) + nwg_x;
    int pulled = 0;                                    // lane 0 of the workgroup: the value its pending pull returned
    auto pull_issue = [&]() {
        if (t == 0) pulled = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto pull_publish = [&]() {                        // lane 0: hand the pulled index to the workgroup (LDS word)
        if (t == 0) {
            if (pulled == pulls_x - 1) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_next[0] = nwg_x + pulled;
        }
    };
    // blocking form (start of a workgroup whose own first tile is empty, or a pulled tile without valid rows - a launch
    // cut short by a device-side count): pull until a tile with work or the end of the share
    auto pull_blocking = [&](int& m0, int& mend, int& n0, int& wofs) -> int {
        int idx;
        do {
            pull_issue();
            pull_publish();
            __syncthreads();
            idx = __builtin_amdgcn_readfirstlane(s_next[0]);
            __syncthreads();
        } while (idx < size_x && !coords(idx, m0, mend, n0, wofs));
        return idx;
    };

    unsigned a_voff[A_LD], b_voff[B_LD];
    auto set_offsets = [&](int m0, int mend, int n0, int wofs) {
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = m0 + row0 + RPP * i;
            a_voff[i] = m < mend ? (unsigned)((m * p.Cin + src_c4 * 4) * 4) : OOB;
        }
        const int b0 = (wofs + (n0 + row0) * p.K + src_c4 * 4) * 4;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) b_voff[i] = (unsigned)(b0 + i * RPP * p.K * 4);
    };
    auto issue_tile = [&](int kt, int stage) {
        const unsigned sa = lds_base + stage * (STAGE * 4) + wave_row_bytes;
        const unsigned ko = (unsigned)(kt * BK * 4);
#pragma unroll
        for (int i = 0; i < A_LD; ++i) lds_dma16_s(x_rs, sa + i * RPP * 128, a_voff[i], ko);
        const unsigned sb = sa + BM * 128;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) lds_dma16_s(w_rs, sb + i * RPP * 128, b_voff[i], ko);
    };

    const int r16 = lane & 15, g16 = lane >> 4;
    // fragment read: row (base + 16 i + r16), 16-byte chunk (4 kk + g16) ^ swizzle(row); the swizzle of row r is
    // (r >> 1) & 7 and the bases are multiples of 16, so it depends on r16 alone
    const int fswz = (r16 >> 1) & 7;
    const float* const rd_a = smem + (wm * WM + r16) * BK;
    const float* const rd_b = smem + BM * BK + (wn * WN + r16) * BK;

    int m0 = 0, mend = 0, n0 = 0, wofs = 0;
    int idx = blockIdx.x >> 3;
    if (counter) {
        if (!(idx < size_x && coords(idx, m0, mend, n0, wofs))) idx = pull_blocking(m0, mend, n0, wofs);
    } else {
        while (idx < size_x && !coords(idx, m0, mend, n0, wofs)) idx += nwg_x;
    }
    if (idx >= size_x) return;
    CLOCK_STAMP_BEGIN();
    set_offsets(m0, mend, n0, wofs);
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
        if (s < KT) issue_tile(s, s);

    while (true) {
        f32x4 acc[TI][TJ];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // NST LDS stages: K-tiles kt + 1 .. kt + NST - 2 are in flight while tile kt is multiplied and tile kt + NST - 1
        // is issued.  One barrier per K-tile, at its top: behind it tile kt has landed for every wave (own DMAs by the
        // counted vmcnt - completion is in issue order, so "at most (NST - 2) * LOADS outstanding" means tile kt is in;
        // stores of the previous epilogue and the scheduler's atomic only make that wait longer, never shorter) and
        // every wave has finished reading the stage of tile kt - 1, which tile kt + NST - 1 overwrites.  With one or
        // two workgroups on a CU (launches of few tiles, and the last round of every launch) a K-tile is ~1100
        // MFMA cycles against a DMA latency of 2000-3000: two stages leave the pipe idle two thirds of the time
        // (measured r04: a lone workgroup needs ~3300 cycles per K-tile), the deeper ring covers it.
        int cur = 0;
        for (int kt = 0; kt < KT; ++kt) {
            if (NST > 2 && kt + NST - 2 < KT) {
                if (NST == 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LOADS) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LOADS) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            if (kt == 0 && counter) pull_issue();        // the next tile's index arrives under this tile's K loop
            if (kt + NST - 1 < KT) {
                int st = cur + NST - 1;
                if (st >= NST) st -= NST;
                issue_tile(kt + NST - 1, st);
            }
            if (kt == KT - 1 && counter) pull_publish(); // ... and is handed to the workgroup behind the barrier after the loop
            asm volatile("" ::: "memory");
            const float* As = rd_a + cur * STAGE;
            const float* Bs = rd_b + cur * STAGE;
            f32x4 af[2][TI], bf[2][TJ];
            const int pc0 = ((0 * 4 + g16) ^ fswz) * 4, pc1 = ((1 * 4 + g16) ^ fswz) * 4;
#pragma unroll
            for (int i = 0; i < TI; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(As + 16 * i * BK + pc0);
#pragma unroll
            for (int j = 0; j < TJ; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(Bs + 16 * j * BK + pc0);
#pragma unroll
            for (int i = 0; i < TI; ++i) af[1][i] = *reinterpret_cast<const f32x4*>(As + 16 * i * BK + pc1);
#pragma unroll
            for (int j = 0; j < TJ; ++j) bf[1][j] = *reinterpret_cast<const f32x4*>(Bs + 16 * j * BK + pc1);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                // k-slot e of the 16-deep step over ALL accumulators before slot e + 1: an accumulator sees its next
                // MFMA TI*TJ issues later (dependent latency 40 cycles, issue 32); operands swapped: the accumulator
                // holds C^T (see the header of this kernel)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TI; ++i)
#pragma unroll
                        for (int j = 0; j < TJ; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[kk][j][e], af[kk][i][e], acc[i][j], 0, 0, 0);
            }
            cur = cur + 1 == NST ? 0 : cur + 1;
        }
        // every wave is done with the last stage (and lane 0's hand-off word is visible) before the next tile's first
        // K-tiles are issued: they fly while this tile's accumulators are stored
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int em0 = m0, emend = mend, en0 = n0;
        int nm0 = 0, nmend = 0, nn0 = 0, nwofs = 0;
        int next;
        if (counter) {
            next = __builtin_amdgcn_readfirstlane(s_next[0]);
            if (next < size_x && !coords(next, nm0, nmend, nn0, nwofs)) next = pull_blocking(nm0, nmend, nn0, nwofs);
        } else {
            next = idx + nwg_x;
            while (next < size_x && !coords(next, nm0, nmend, nn0, nwofs)) next += nwg_x;
        }
        if (next < size_x) {
            set_offsets(nm0, nmend, nn0, nwofs);
#pragma unroll
            for (int s = 0; s < NST - 1; ++s)
                if (s < KT) issue_tile(s, s);
        }
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
            const int n = en0 + wn * WN + 16 * j + 4 * g16;
            if (n >= p.Cout) continue;                                   // Cout % 4 == 0 (checked by the launcher)
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + n);
            if (p.shift) sh = *reinterpret_cast<const float4*>(p.shift + n);
            // all residual rows of this channel block first (TI independent 16-byte loads in flight), then the arithmetic
            float4 res[TI];
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int m = em0 + wm * WM + 16 * i + r16;
                res[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.residual && m < emend) res[i] = *reinterpret_cast<const float4*>(p.residual + (size_t)m * p.Cout + n);
            }
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const int m = em0 + wm * WM + 16 * i + r16;
                if (m >= emend) continue;
                float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                v.x += res[i].x; v.y += res[i].y; v.z += res[i].z; v.w += res[i].w;
                if (p.relu) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                *reinterpret_cast<float4*>(p.y + (size_t)m * p.Cout + n) = v;
            }
        }
        if (next >= size_x) break;
        idx = next; m0 = nm0; mend = nmend; n0 = nn0; wofs = nwofs;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CLOCK_STAMP_END(blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Round 5 (VERDICT r4 item 3): conv_pw_persist_kernel with a PRODUCER wave.  Five waves per workgroup: waves 0..3 are the
// consumers (ds_read_b128 fragments + MFMA, the epilogue) and issue no LDS-DMA at all; wave 4 issues the 16
// `buffer_load ... lds` of every K-tile (8 A-row groups + 8 B-row groups of 8 rows x 128 B), waits for them and joins the
// same one barrier per K-tile.  Round 4's decomposition put the in-loop DMA issue at 4 points of the kernel's rate; this
// form takes the issue out of the MFMA waves without removing the data movement.  Bit-identical results.  Measured
// (profiles/r05_producer_wave.txt): back to back on the large GEMMs +1.9 % (AG-RPN 468.3 -> 459.4 us = 0.856 of the
// MFMA peak, 300-RoI 176.1 -> 172.9, relation Q 231.5 -> 227.2, the shape without a partial round 0.884 -> 0.895); in
// the PIPELINED step -2.7 % (three interleaved pairs on one box, 100 steps: 202.6-203.1 -> 196.7-198.6 img/s): 20
// instead of 16 resident waves per CU leave the other episode's kernels less room.  Not adopted.  Knob 6 = 1 / FGN_PW_WS=1.
// (Every unsplit 64x64 point-wise launch on this kernel, one tile per workgroup where a launch has fewer tiles than
// workgroups, lost another 2 %: 190.4 -> 186.7 img/s.)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(320, 5) void conv_pw_persist_ws_kernel(const ConvParams p, const int total_tiles) {
    constexpr int BM = 64, BN = 64, WN = 32, WM = 32;
    constexpr int STAGE = (BM + BN) * BK;          // floats
    constexpr int PITCH = BN;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool producer = __builtin_amdgcn_readfirstlane(wv) == 4;
    const int wm = (wv >> 1) & 1, wn = wv & 1;
    const int M = (p.n_img_dev ? min(p.n_img, *p.n_img_dev) : p.n_img) * p.Ho * p.Wo;
    int grp_valid = p.grp_valid;
    if (p.grp_rows && p.grp_count_dev) grp_valid = min(grp_valid, min(p.grp_items, *p.grp_count_dev) * p.grp_rows_per_item);
    const int KT = p.K / BK;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<size_t>(smem));
    constexpr unsigned OOB = 0x7ffffff0u;

    const int nq = total_tiles >> 3, nr = total_tiles & 7;
    auto coords = [&](int tile, int& m0, int& n0) -> bool {
        const int xcd = tile & 7, idx = tile >> 3;
        const int bid = (xcd < nr ? xcd * (nq + 1) : nr * (nq + 1) + (xcd - nr) * nq) + idx;
        int tile_m = bid / p.n_tiles_n;
        int tile_n = bid - tile_m * p.n_tiles_n;
        if (p.band_nt > 0) {
            const int per_grp = p.band_mt * p.n_tiles_n;
            const int grp = bid / per_grp;
            int r = bid - grp * per_grp;
            const int per_band = p.band_mt * p.band_nt;
            const int band = r / per_band;
            r -= band * per_band;
            const int mi = r / p.band_nt;
            tile_m = grp * p.band_mt + mi;
            tile_n = band * p.band_nt + (r - mi * p.band_nt);
        }
        m0 = tile_m * BM;
        n0 = tile_n * BN;
        if (m0 >= M) return false;
        if (p.grp_rows && m0 - (m0 / p.grp_rows) * p.grp_rows >= grp_valid) return false;
        return true;
    };
    auto next_active = [&](int tile, int& m0, int& n0) -> int {
        for (; tile < total_tiles; tile += gridDim.x)
            if (coords(tile, m0, n0)) return tile;
        return -1;
    };

    auto leave = [&]() {};
    int m0, n0;
    int tile = next_active(blockIdx.x, m0, n0);
    if (tile < 0) { leave(); return; }              // workgroup-uniform: nobody waits at a barrier
    CLOCK_STAMP_BEGIN();

    if (producer) {
        // ---- wave 4: the LDS-DMA of every K-tile.  Lane l covers row 8 i + (l >> 3), 16-byte chunk l & 7 of instruction i
        const i32x4 x_rs = make_rsrc(p.x, p.x_bytes);
        const i32x4 w_rs = make_rsrc(p.w, p.w_bytes);
        const int r8 = lane >> 3, c8 = lane & 7;
        unsigned a_voff[8], b_voff[8];
        auto set_offsets = [&](int tm0, int tn0) {
            int b0 = tn0 * p.K * 4;
            if (p.grp_rows) b0 += (tm0 / p.grp_rows) * p.grp_w_stride * 4;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = 8 * i + r8;
                const int src_c4 = c8 ^ ((row >> 1) & 7);
                const int m = tm0 + row;
                a_voff[i] = m < M ? (unsigned)((m * p.Cin + src_c4 * 4) * 4) : OOB;
                b_voff[i] = (unsigned)(b0 + (row * p.K + src_c4 * 4) * 4);
            }
        };
        auto issue_tile = [&](int kt, int stage) {
            const unsigned sa = lds_base + stage * (STAGE * 4);
            const unsigned ko = (unsigned)(kt * BK * 4);
#pragma unroll
            for (int i = 0; i < 8; ++i) lds_dma16_s(x_rs, sa + i * 1024, a_voff[i], ko);
#pragma unroll
            for (int i = 0; i < 8; ++i) lds_dma16_s(w_rs, sa + BM * 128 + i * 1024, b_voff[i], ko);
        };
        set_offsets(m0, n0);
        issue_tile(0, 0);
        while (true) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                      // (top of the tile)
            int cur = 0;
            for (int kt = 0; kt < KT; ++kt) {
                if (kt + 1 < KT) issue_tile(kt + 1, cur ^ 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();                  // (the loop's barrier)
                cur ^= 1;
            }
            int nm0 = 0, nn0 = 0;
            const int next = next_active(tile + gridDim.x, nm0, nn0);
            if (next >= 0) {
                set_offsets(nm0, nn0);
                issue_tile(0, 0);                              // stage 0 is free; the epilogue drains through stage 1
            }
            __builtin_amdgcn_s_barrier();                      // (the epilogue's barrier)
            if (next < 0) break;
            tile = next;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ---- waves 0..3: fragments + MFMA + epilogue (conv_pw_persist_ws_kernel without its DMA)
    const int r16 = lane & 15, g16 = lane >> 4;
    const float* const rd_a = smem + (wm * WM + r16) * BK;
    const float* const rd_b = smem + BM * BK + (wn * WN + r16) * BK;
    float* const cbase = smem + STAGE;
    while (true) {
        f32x4 acc4[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        int cur = 0;
        for (int kt = 0; kt < KT; ++kt) {
            const float* As = rd_a + cur * STAGE;
            const float* Bs = rd_b + cur * STAGE;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                float4 af[2], bf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int row = r16 + 16 * i;
                    const int pc = ((kk * 4 + g16) ^ ((row >> 1) & 7)) * 4;
                    af[i] = *reinterpret_cast<const float4*>(As + 16 * i * BK + pc);
                    bf[i] = *reinterpret_cast<const float4*>(Bs + 16 * i * BK + pc);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].x, bf[j].x, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].y, bf[j].y, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].z, bf[j].z, acc4[i][j], 0, 0, 0);
                        acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i].w, bf[j].w, acc4[i][j], 0, 0, 0);
                    }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            cur ^= 1;
        }
        const int em0 = m0, en0 = n0;
        int nm0 = 0, nn0 = 0;
        const int next = next_active(tile + gridDim.x, nm0, nn0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float* cw = cbase + (wm * WM + 16 * i + 4 * g16) * PITCH + wn * WN + 16 * j + r16;
#pragma unroll
                for (int r = 0; r < 4; ++r) cw[r * PITCH] = acc4[i][j][r];
            }
        __syncthreads();                                       // (one s_barrier: the producer's third barrier of the tile)
        {
            constexpr int C4 = BN / 4, RPP = 256 / C4;
            const int c4 = t % C4, rr = t / C4;
            const int n = en0 + c4 * 4;
            if (n < p.Cout) {
                float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + n);
                if (p.shift) sh = *reinterpret_cast<const float4*>(p.shift + n);
                float4 res[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = em0 + rr + RPP * k;
                    res[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (p.residual && m < M) res[k] = *reinterpret_cast<const float4*>(p.residual + (size_t)m * p.Cout + n);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int row = rr + RPP * k;
                    const int m = em0 + row;
                    if (m >= M) continue;
                    float4 v = *reinterpret_cast<const float4*>(cbase + row * PITCH + c4 * 4);
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                    v.x += res[k].x; v.y += res[k].y; v.z += res[k].z; v.w += res[k].w;
                    if (p.relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                    *reinterpret_cast<float4*>(p.y + (size_t)m * p.Cout + n) = v;
                }
            }
        }
        if (next < 0) break;
        tile = next; m0 = nm0; n0 = nn0;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    leave();
    CLOCK_STAMP_END(blockIdx.x);
}

static int g_ws_mode = getenv("FGN_PW_WS") ? atoi(getenv("FGN_PW_WS")) : 0;      // 1: the producer-wave kernel for every persistent launch (single-operand launches)

static int g_sk_mode = getenv("FGN_STREAMK") ? atoi(getenv("FGN_STREAMK")) : 0;
static int g_sk_fill_pct = getenv("FGN_STREAMK_FILL") ? atoi(getenv("FGN_STREAMK_FILL")) : 85;
static int g_sk_debug = 0;
static int g_sk_min_tiles = getenv("FGN_STREAMK_MIN_TILES") ? atoi(getenv("FGN_STREAMK_MIN_TILES")) : 320;
#endif   // part 1

#if FGN_EXP_PART == 2
// Stream-K plan (conv_pw_streamk_kernel) for a point-wise launch of `tiles` 64x64 output tiles with KT K-tiles each.
// g_sk_mode 0: never; 1: launches with more tiles than resident workgroups whose last round is at most g_sk_fill_pct
// per cent full; 2: also launches of g_sk_min_tiles .. grid tiles (today's one-tile-per-workgroup launches); 3: every
// eligible launch.  Tuning knobs 2..4 of fgn_conv2d_tune.
static size_t streamk_ws_bytes() { return (size_t)persist_blocks() * 2 * 64 * 64 * sizeof(float); }
static bool plan_streamk(long long tiles, int KT, int* dp_tiles, int* U) {
    const int G = persist_blocks();
    if (g_sk_mode <= 0 || G <= 0 || G > FGN_STREAMK_MAX_GRID || KT < 4 || tiles <= 0 || tiles >= (1ll << 30)) return false;
    const int dp = (int)(tiles / G) * G;
    const int rem = (int)(tiles - dp);
    if (rem == 0) return false;
    if (g_sk_mode < 3) {
        if (rem * 100ll > (long long)g_sk_fill_pct * G) return false;       // a nearly full round gains nothing
        if (dp == 0 && (g_sk_mode < 2 || tiles < g_sk_min_tiles)) return false;
    }
    const int nq = (int)(tiles >> 3), nr = (int)(tiles & 7);
    const int rem_max = nq + (nr ? 1 : 0) - dp / 8;                         // remaining tiles of the longest XCD run
    const int per = cdiv(rem_max * KT, G / 8);
    *U = std::max(per, std::min(KT, 4));                                    // <= KT: rem_max <= G / 8
    *dp_tiles = dp;
    return true;
}

// tuning knobs (fgn_conv2d_tune): forced tile code (-1 = heuristic) and workgroups per CU (0 = the tile's default)
static int g_pw2_force = getenv("FGN_PW2") ? atoi(getenv("FGN_PW2")) : -1;      // -1: the heuristic below
static int g_pw2_wgs = getenv("FGN_PW2_WGS") ? atoi(getenv("FGN_PW2_WGS")) : 0;   // 0: the tile's own workgroups per CU
// ---- conv_pw_persist2_kernel: launch -------------------------------------------------------------------------
// tile codes: 1 = 128x128 (4 waves of 64x64), 2 = 64x128 (32x64), 3 = 128x64 (64x32), 4 = 64x64 (32x32),
// 5 = 128x128 with 8 waves of 32x64, 6 = 64x64 with 8 waves of 32x16, 7 = 64x128 with 8 waves of 32x32, 8 = 32x64 (16x32)
template <int BM, int BN, int WM, int WN, int NST, int WG_MAX>
static int launch_persist2_t(const ConvParams& p0, int M_max, hipStream_t stream) {
    constexpr int NT = (BM / WM) * (BN / WN) * 64;
    constexpr size_t LDS = (size_t)NST * (BM + BN) * BK * sizeof(float) + 16;      // + the scheduler's hand-off word
    // workgroups per CU: what LDS and the 2048-thread limit admit, at most the tile's own bound
    constexpr int BY_LDS = (int)(160 * 1024 / LDS), BY_THREADS = 2048 / NT;
    constexpr int WG_PER_CU = BY_LDS < BY_THREADS ? (BY_LDS < WG_MAX ? BY_LDS : WG_MAX) : (BY_THREADS < WG_MAX ? BY_THREADS : WG_MAX);
    constexpr int MINW = WG_PER_CU * NT / 256;           // __launch_bounds__: waves per SIMD the grid needs
    static_assert(WG_PER_CU >= 1, "tile does not fit");
    ConvParams p = p0;
    p.n_tiles_n = cdiv(p.Cout, BN);
    Persist2Geom gm;
    gm.n_groups = p.grp_rows ? M_max / p.grp_rows : 1;
    gm.mt = p.grp_rows ? cdiv(p.grp_rows, BM) : cdiv(M_max, BM);
    constexpr long long budget = 2048 * 1024;
    const long long per_nt = (long long)BN * p.K * 4;
    gm.band_nt = p.n_tiles_n;
    if (budget > 0 && per_nt * p.n_tiles_n > budget) {
        int nb = (int)std::max<long long>(1, budget / per_nt);
        while (nb > 1 && p.n_tiles_n % nb) --nb;
        gm.band_nt = nb;
    }
    const long long total = (long long)gm.n_groups * gm.mt * p.n_tiles_n;
    if (total <= 0 || total >= (1ll << 30)) return FGN_ERR_SHAPE;
    const int per_cu = g_pw2_wgs > 0 ? std::min(g_pw2_wgs, WG_PER_CU) : WG_PER_CU;
    const int cap = 256 * per_cu;
    const int grid = (int)std::min<long long>((total + 7) / 8 * 8, cap);
    static unsigned long long ok = 0ull;
    hipError_t attr = fgn_allow_full_lds(reinterpret_cast<const void*>(conv_pw_persist2_kernel<BM, BN, WM, WN, NST, MINW>), &ok);
    if (attr != hipSuccess) return (int)attr;
    FGN_LAUNCH_TIMED((conv_pw_persist2_kernel<BM, BN, WM, WN, NST, MINW>), dim3(grid), dim3(NT), LDS, stream, p, gm, (int)total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

template <int BM, int BN, int WM, int WN, int WG_MAX>
static int launch_persist2_st(int nst, const ConvParams& p, int M_max, hipStream_t stream) {
    switch (nst) {
        case 3: return launch_persist2_t<BM, BN, WM, WN, 3, WG_MAX>(p, M_max, stream);
        case 4: return launch_persist2_t<BM, BN, WM, WN, 4, WG_MAX>(p, M_max, stream);
        default: return launch_persist2_t<BM, BN, WM, WN, 2, WG_MAX>(p, M_max, stream);
    }
}

// code = tile + 10 * (LDS stages, 0 = 2)
static int launch_persist2(int code, const ConvParams& p, int M_max, hipStream_t stream) {
    const int nst = code / 10 ? code / 10 : 2;
    switch (code % 10) {
        case 1: return launch_persist2_t<128, 128, 64, 64, 2, 2>(p, M_max, stream);
        case 2: return launch_persist2_st<64, 128, 32, 64, 3>(nst, p, M_max, stream);
        case 3: return launch_persist2_t<128, 64, 64, 32, 2, 3>(p, M_max, stream);
        case 4: return launch_persist2_st<64, 64, 32, 32, 4>(nst, p, M_max, stream);
        case 5: return launch_persist2_t<128, 128, 32, 64, 2, 2>(p, M_max, stream);
        case 6: return launch_persist2_st<64, 64, 32, 16, 4>(nst, p, M_max, stream);       // 8 waves on a 64x64 tile
        case 7: return launch_persist2_st<64, 128, 32, 32, 3>(nst, p, M_max, stream);      // 8 waves on a 64x128 tile
        case 8: return launch_persist2_st<32, 64, 16, 32, 5>(nst, p, M_max, stream);       // 4 waves on a 32x64 tile
        default: return FGN_ERR_ARG;
    }
}

// Which point-wise launches take conv_pw_persist2_kernel, and with which tile (0: none).  FGN_PW2 forces a code for
// every eligible launch (tools/gemm_time.py A/B); eligible = 1x1 / stride 1 on the LDS-DMA path, no split-K, no fused
// input scale, Cout % 4 == 0.

static int pick_persist2(long long M, int Cout, int K, bool grouped, int grp_rows = 0, bool has_residual = false) {
    if (g_pw2_force >= 0) return g_pw2_force;
    if (has_residual) return 0;
    // Measured on MI355X against the round-3 kernels, interleaved in one process (tools/gemm_variants.py;
    // profiles/r04_gemm_variants_*.txt, four boxes):
    //  * the large grouped Winograd GEMMs (AG-RPN 36 x 819 x 1024 x 1024, shared head on 300 RoIs 36 x 1200 x 512 x 512)
    //    on 64x128 tiles, three workgroups per CU: 466-472 us against 476-485, 178-182 against 182-187 (the row
    //    count of a launch over 768 slots leaves a shorter last round, and half the L2 -> LDS bytes per MFMA of the
    //    64x64 tile); the smaller grouped GEMMs are equal or slower -> round-3 kernel;
    //  * plain 1x1 convolutions of 500..1000 64x64-tile equivalents and K >= 512 (first shared-head conv on the
    //    feature map 4200 x 1024 > 512, on 100 RoIs 4900 x 1024 > 512, layer2 conv1 26016 x 512 > 128) on 32x64 tiles:
    //    49-51 us against 55-56, 50-51 against 55-57, 38-39 against 40-42 - twice the workgroups of a grid that fills
    //    two to four slots per CU unevenly;
    //  * everything else (residual epilogues: the 16-byte stores from the accumulators touch 16 rows x 64 B per
    //    instruction, the LDS round trip 4 rows x 256 B; small K; full grids of 64x64 tiles): round-3 kernels.
    // In the pipelined step (two caller streams, three episodes in flight) the other episode's kernels fill a GEMM's
    // last round, and none of this shows: same-box A/B of bench.py with these choices on / off, r04: B = 1 188.6-190.9
    // vs 190.1-190.8 img/s, B = 4 212.3-212.5 vs 209.2-211.0, B = 8 213.2 vs 215.5.  The choices stay behind
    // FGN_PW2_AUTO=1 (and the per-launch knob); the default keeps every launch on the round-3 kernels.
    static const bool automatic = getenv("FGN_PW2_AUTO") && atoi(getenv("FGN_PW2_AUTO")) != 0;
    if (!automatic) return 0;
    const long long tiles64 = ((M + 63) / 64) * ((Cout + 63) / 64);
    if (grouped) return (grp_rows >= 800 && Cout >= 512 && K >= 512) ? 2 : 0;
    if (K >= 512 && tiles64 >= 500 && tiles64 <= 1000) return 8;
    return 0;
}

// Tuning knobs at run time (tools/: interleaved A/B of kernel variants inside ONE process, cdna_hip_programming.md 5.4
// rule 24).  knob 0: tile code of conv_pw_persist2_kernel for every eligible point-wise launch (-1 = heuristic,
// 0 = never); knob 1: its workgroups per CU (0 = the tile's default).  Returns the previous value.
extern "C" int fgn_conv2d_tune(int knob, int value) {
    int* k = knob == 0 ? &g_pw2_force : knob == 1 ? &g_pw2_wgs : knob == 2 ? &g_sk_mode : knob == 3 ? &g_sk_fill_pct :
             knob == 4 ? &g_sk_min_tiles : knob == 5 ? &g_sk_debug : knob == 6 ? &g_ws_mode : nullptr;
    if (!k) return FGN_ERR_ARG;
    const int prev = *k;
    *k = value;
    return prev;
}

// ---- private workspaces (see the header of this file)
struct ExpWorkspace { int32_t* words; float* slabs; int next; };
static ExpWorkspace* exp_workspace() {
    static ExpWorkspace ws[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev >= 64) return nullptr;
    ExpWorkspace& w = ws[dev];
    if (!w.words) {
        constexpr int RING = 64;
        if (hipMalloc(&w.words, (size_t)RING * FGN_SCHED_WORDS * sizeof(int32_t)) != hipSuccess) return nullptr;
        if (hipMemset(w.words, 0, (size_t)RING * FGN_SCHED_WORDS * sizeof(int32_t)) != hipSuccess) return nullptr;
        if (hipMalloc(&w.slabs, streamk_ws_bytes()) != hipSuccess) return nullptr;
    }
    return &w;
}
static int32_t* exp_sched_words() {
    ExpWorkspace* w = exp_workspace();
    if (!w) return nullptr;
    w->next = (w->next + 1) % 64;
    return w->words + (size_t)w->next * FGN_SCHED_WORDS;
}

// conv_pw_persist_ws_kernel in place of conv_pw_persist_kernel (knob 6 = 1 / FGN_PW_WS=1): true when it took the launch
static bool fgn_exp_launch_persist_ws(const ConvParams& p, int total_tiles, hipStream_t stream, int* rc) {
    if (g_ws_mode != 1 || p.x2) return false;
    static unsigned long long ok = 0ull;
    hipError_t attr = fgn_allow_full_lds(reinterpret_cast<const void*>(conv_pw_persist_ws_kernel), &ok);
    if (attr != hipSuccess) { *rc = (int)attr; return true; }
    const size_t plds = (size_t)2 * (64 + 64) * BK * sizeof(float);
    FGN_LAUNCH_TIMED(conv_pw_persist_ws_kernel, dim3(persist_blocks()), dim3(320), plds, stream, p, total_tiles);
    hipError_t e = hipGetLastError();
    *rc = e == hipSuccess ? FGN_OK : (int)e;
    return true;
}

static int fgn_exp_launch_streamk(const ConvParams& p, int total_tiles, hipStream_t stream) {
    static unsigned long long sk_ok = 0ull;
    hipError_t attr = fgn_allow_full_lds(reinterpret_cast<const void*>(conv_pw_streamk_kernel), &sk_ok);
    if (attr != hipSuccess) return (int)attr;
    const size_t sklds = (size_t)2 * (64 + 64) * BK * sizeof(float) + 16;
    FGN_LAUNCH_TIMED(conv_pw_streamk_kernel, dim3(persist_blocks()), dim3(256), sklds, stream, p, total_tiles, p.sk_dp, p.sk_U,
                     g_sk_debug);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// kernel id of a point-wise launch (plan mode 1 / 4) that takes one of the experimental kernels (0: none):
// conv_pw_persist2_kernel = tile code * 10 + 5 (the grouped Winograd GEMM asks with tile_hint 4), Stream-K = tile * 10 + 6
static int fgn_exp_kernel_id(const ConvPlan& pl, int Cout, int tile_hint, int has_residual) {
    const bool pw = pl.mode == 1 || pl.mode == 4;
    if (pw && (Cout & 3) == 0 && (tile_hint == 4 || (tile_hint == 0 && pl.splits == 1))) {
        // (asked per group: M / 36 rows; F(2x2) launches have 16 groups and never reach the row threshold)
        const int code = pick_persist2(pl.M, Cout, pl.K, tile_hint == 4, tile_hint == 4 ? (int)(pl.M / 36) : 0, has_residual != 0);
        if (code) return (code % 10) * 10 + 5;
    }
    if (pw && pl.tile == 4 && (Cout & 3) == 0 && tile_hint == 0 && pl.splits == 1) {
        int dp = 0, U = 0;
        if (plan_streamk(((pl.M + 63) / 64) * cdiv(Cout, 64), pl.K / BK, &dp, &U)) return pl.tile * 10 + 6;
    }
    return 0;
}

// Dispatcher hook for an eligible point-wise launch (1x1 / stride 1 on the LDS-DMA path, no split-K, no fused input scale,
// Cout % 4 == 0): launches conv_pw_persist2_kernel and returns true (*rc = its status), or arms `p` for Stream-K (the
// dispatcher's own launch_cfg then takes conv_pw_streamk_kernel) and returns false, or leaves `p` alone.
static bool fgn_exp_pointwise(ConvParams& p, long long M, int tile, bool grouped, int grp_rows, hipStream_t stream, int* rc) {
    const int code = pick_persist2(M, p.Cout, p.K, grouped, grp_rows, p.residual != nullptr);
    if (code) {
        p.sched = exp_sched_words();
        *rc = launch_persist2(code, p, (int)M, stream);
        return true;
    }
    int dp = 0, U = 0;
    if (tile == 4 && plan_streamk(((M + 63) / 64) * cdiv(p.Cout, 64), p.K / BK, &dp, &U)) {
        ExpWorkspace* w = exp_workspace();
        int32_t* words = exp_sched_words();
        if (w && words) {
            p.ws = w->slabs; p.tickets = words + FGN_TILE_SCHED_WORDS; p.sk_U = U; p.sk_dp = dp;
        }
    }
    return false;
}
#endif   // part 2
