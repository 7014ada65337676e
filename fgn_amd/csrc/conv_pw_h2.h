// conv_pw_h2_kernel - the point-wise / grouped GEMM of conv_pw_x3_kernel with THREE f16 MFMA products per f32 product
// instead of six bf16 ones.  Included by conv_igemm.hip after conv_pw_x3.h (ConvParams, make_rsrc, lds_dma16_s, BK).
//
// Why.  conv_pw_x3_kernel is power-bound: what it costs is the number of MFMA products per f32 product.  An f32 value
// scaled by a power of two into the f16 range is h + l + e with h = f16(x), l = f16(x - h) (both round-to-nearest, the
// subtraction exact) and |e| <= 2^-23 |x|: l keeps 11 of the at most 13 bits h leaves, so the two planes hold x to one ulp
// of the f32 value at worst, a quarter of it on average.  Products of two f16 values are exact in f32 (22 significant
// bits), so a * b = ha hb + ha lb + la hb + (la lb <= 2^-22 |a b|, left out): each product within 2^-21 |a b| at worst and
// ~2^-24 |a b| rms - the order of the rounding an f32 FMA chain makes at every step: three v_mfma_f32_16x16x32_f16 per f32
// MFMA's worth of K,
// accumulated in f32 by the matrix pipe.  Against fp64 the result is as close as the f32 kernels' (the accumulation's own
// rounding dominates all three arithmetics: tests/test_hip_conv.py::test_h2_*, tools/x3_probe.py).
//
// Range.  f16 has 5 exponent bits, so the operands are scaled by powers of two (exact) and the scales taken out again:
//  * the weights per output column at pack time (ops.pack_h2: column maximum into [2^14, 2^15); the inverse scales, [group]
//    [npad] floats, lie behind the image and multiply the C tile in the epilogue);
//  * the activations by a scale the kernel finds itself, per WAVE and OUTPUT TILE: the first K-tile of the tile whose
//    32 RB x 32 fragment holds a non-zero element sets S so that the fragment's largest |x| lands in [2^13, 2^14); every
//    later K-tile is looked at once (max |x| of the raw fragment against 65504 / S: `v_max3_f32` with |.| modifiers, 0.25 vector instruction per element),
//    and one that would leave the f16 range - an element 4x .. 8x above what S was chosen for - picks a new S from its
//    own maximum and multiplies the accumulators by the ratio (a power of two: exact); the maxima are those of the
//    FINITE elements (a row holding Inf / NaN comes out non-finite and leaves the other rows' scale alone: they keep the
//    bits they have with that element replaced by zero).  S comes out of the accumulators
//    when they go to the C tile.  An element within 2^15 of the maximum S was chosen for keeps both planes at full
//    precision; a smaller one loses low bits of its l plane (f16 subnormals): an absolute error below 2^-38 of that
//    maximum per element.  The splits are scale-invariant otherwise: row tiles / stage counts differ only through such
//    elements (tests: within 1e-7 of the range of each other).  No producer has to supply a maximum: the form that
//    took one from device memory (written by the Winograd input transform with atomics) ran the GEMM 5-10 % faster and
//    the transform 3x slower (profiles/r05_ab_h2_100steps.jsonl, r05_h2_probe_record_vs_own_scale.jsonl; DESIGN appendix A).
//
// Structure: conv_pw_x3_kernel's (16x16x32 form): BM = 32 RB WMW rows x 128 columns, WMW x 2 waves, wave tile 32 RB x 64,
// a ring of NST LDS stages of (BM * 128 + 16384) bytes running across output tiles (the C tile goes through the stage the
// last K-tile was read from: every wave takes its own accumulators through a 16-row region of its own, behind one
// workgroup barrier per output tile - "the epilogue" in the kernel; two K-groups: one wave row at a time, the second
// group's sum added in place: 32 RB rows x 512 bytes fit the stage for either row tile), the f32 activations split in
// registers after the ds_read (2 vector instructions per element: v_fma_mixlo / mixhi_f16), the weight image
// [group][K-tile][plane][npad][32] f16 with the k order and chunk swizzle of ops.pack_x3's 16x16x32 form.  64 rows: 48 KB
// of LDS, three workgroups per CU; 128 rows: 64 KB, two; 64 rows on two K-groups (KG = 2, below): 96 KB, one.
#pragma once

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));

struct H2Frag { f16x8_t hi, lo; };

// four f32, scaled by the power of two s (wave-uniform) -> hi = f16(x s), lo = f16(x s - hi) as two packed pairs each.
// v_fma_mixlo / mixhi_f16 take f32 and f16 sources in one fma and round the f32 result to f16 once: x s is exact (a power
// of two), x s - hi is exact in f32, so each plane is one instruction per element (the compiler's own sequence for the
// same C expressions is three).  The pairs are interleaved so that no instruction reads a register in the slot right
// behind a half-register write to it (gfx940+ dst-forwarding rule; the hazard recognizer does not look inside an asm block).
__device__ __forceinline__ void h2_split4(const float x0, const float x1, const float x2, const float x3, const float s,
                                          unsigned& h01, unsigned& h23, unsigned& l01, unsigned& l23) {
    asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\t"
        "v_fma_mixlo_f16 %1, %6, %8, 0\n\t"
        "v_fma_mixhi_f16 %0, %5, %8, 0\n\t"
        "v_fma_mixhi_f16 %1, %7, %8, 0\n\t"
        "v_fma_mixlo_f16 %2, %4, %8, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %3, %6, %8, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %2, %5, %8, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %3, %7, %8, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"        // an MFMA may read the planes next: VALU write -> MFMA read needs two wait states (not inserted for asm)
        : "=&v"(h01), "=&v"(h23), "=&v"(l01), "=&v"(l23)
        : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "s"(s));
}

// h2_split4 in its four steps of two instructions, for issue one step at a time in the gaps between MFMAs (an MFMA holds
// vector issue for half of its cycles): STEP 0 / 1 the low / high halves of the h pairs, 2 / 3 those of the l pairs.  The
// same instructions in the same order, so the half-register rule above holds whatever lies between two steps; the caller
// keeps two wait states between step 3 and the first MFMA that reads the planes.
__device__ __forceinline__ void h2_split4_step(const int step, const float x0, const float x1, const float x2, const float x3,
                                               const float s, unsigned& h01, unsigned& h23, unsigned& l01, unsigned& l23) {
    // (`step` is a constant once the caller's loops are unrolled: one of the four statements remains)
    if (step == 0)
        asm("v_fma_mixlo_f16 %0, %2, %4, 0\n\t"
            "v_fma_mixlo_f16 %1, %3, %4, 0"
            : "=&v"(h01), "=&v"(h23) : "v"(x0), "v"(x2), "s"(s));
    else if (step == 1)
        asm("v_fma_mixhi_f16 %0, %2, %4, 0\n\t"
            "v_fma_mixhi_f16 %1, %3, %4, 0"
            : "+v"(h01), "+v"(h23) : "v"(x1), "v"(x3), "s"(s));
    else if (step == 2)
        asm("v_fma_mixlo_f16 %0, %2, %4, -%5 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixlo_f16 %1, %3, %4, -%6 op_sel:[0,0,0] op_sel_hi:[0,0,1]"
            : "=&v"(l01), "=&v"(l23) : "v"(x0), "v"(x2), "s"(s), "v"(h01), "v"(h23));
    else
        asm("v_fma_mixhi_f16 %0, %2, %4, -%5 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
            "v_fma_mixhi_f16 %1, %3, %4, -%6 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
            : "+v"(l01), "+v"(l23) : "v"(x1), "v"(x3), "s"(s), "v"(h01), "v"(h23));
}

// eight f32 -> two planes of eight f16
__device__ __forceinline__ H2Frag h2_split(const float4& a, const float4& b, const float s) {
    unsigned h[4], l[4];
    h2_split4(a.x, a.y, a.z, a.w, s, h[0], h[1], l[0], l[1]);
    h2_split4(b.x, b.y, b.z, b.w, s, h[2], h[3], l[2], l[3]);
    H2Frag f;
    f.hi = __builtin_bit_cast(f16x8_t, make_uint4(h[0], h[1], h[2], h[3]));
    f.lo = __builtin_bit_cast(f16x8_t, make_uint4(l[0], l[1], l[2], l[3]));
    return f;
}

// max |x| over sixteen f32 values: eight v_max3_f32 with |.| source modifiers (the compiler's own sequence for the same
// fmaxf / fabsf tree is three times as long: it does not fold the inner maximum)
__device__ __forceinline__ float h2_absmax16(const float4& a, const float4& b, const float4& c, const float4& d) {
    float m;
    asm("v_max3_f32 %0, |%1|, |%2|, 0\n\t"
        "v_max3_f32 %0, |%3|, |%4|, %0\n\t"
        "v_max3_f32 %0, |%5|, |%6|, %0\n\t"
        "v_max3_f32 %0, |%7|, |%8|, %0\n\t"
        "v_max3_f32 %0, |%9|, |%10|, %0\n\t"
        "v_max3_f32 %0, |%11|, |%12|, %0\n\t"
        "v_max3_f32 %0, |%13|, |%14|, %0\n\t"
        "v_max3_f32 %0, |%15|, |%16|, %0"
        : "=&v"(m)
        : "v"(a.x), "v"(a.y), "v"(a.z), "v"(a.w), "v"(b.x), "v"(b.y), "v"(b.z), "v"(b.w),
          "v"(c.x), "v"(c.y), "v"(c.z), "v"(c.w), "v"(d.x), "v"(d.y), "v"(d.z), "v"(d.w));
    return m;
}

constexpr int H2_BN = 128;                       // columns the weight image is padded to

// Second tensor / spatial structure of an IM2COL launch (conv_pw_h2_kernel<..., true>): a KH x KW / stride / pad convolution
// (KW 1 or 3, Cin / 32 a power of two) as an implicit GEMM over the rows of ONE or TWO NHWC tensors with the same weights
// (the query map and the support maps of a backbone layer): rows [0, M0) are the output pixels of tensor 0 (ConvParams:
// n_img, H, W, Ho, Wo; input at x + x_off0 bytes, output y), rows [M0, M0 + M1) those of tensor 1 (input at x + x_off1,
// output y1).  Both inputs lie inside the one buffer descriptor [x, x + x_bytes).
struct H2Im2col {
    float* y1;
    unsigned x_off0, x_off1;
    int M0, M1;
    int H1, W1, Ho1, Wo1;
    int cin_shift;            // log2(Cin / 32)
};

// K-groups (KG = 2): for a grid of at most one output tile per CU, where a workgroup is alone on its CU and
// each SIMD holds ONE wave that walks the K-tiles as a serial chain (wait, barrier, DMA issue, LDS reads, split, MFMA), a
// second set of WMW x WNW waves works on the SAME output tile.  A K-step is KG consecutive K-tiles: group kg = wave / (WMW
// WNW) requests K-tile step * KG + kg into a ring of NST stages of its own (behind group 0's), reads only that ring and
// keeps its own accumulators and its own per-wave activation scale; a wave waits only for its own DMAs, and all waves meet
// at the one workgroup barrier per step.  The chain is KT / KG steps long and each SIMD holds two waves that are out of
// step in their phases.  In the epilogue group 0 writes its scaled accumulators to the C tile and group 1 adds its own
// behind a barrier (a fixed order: the result is deterministic); all the threads store.  KG * NST stages of LDS.
// phase clocks of one wave (tools/x3_probe.py --phases; -DH2_PHASES: the diagnostic build of tools/micro/build_x3_phases.sh
// only, nothing in the product library executes a stamp): cycles in [wait + barrier | request issue | LDS reads landed |
// watch + split of fragment 0 | MFMAs (with the split under them) | everything outside the K-tiles], written by wave 0 of
// workgroups 0 and 1 to p.ws.  The build waits for every LDS read before the third mark, which the product does not.
#ifdef H2_PHASES
#define H2_T(i) do { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ph_[i] += now_ - last_; last_ = now_; } while (0)
#else
#define H2_T(i) do { } while (0)
#endif
struct H2Yes { static constexpr bool value = true; };
struct H2No { static constexpr bool value = false; };
// The body of both kernels below.  Two operands: the K-tiles from p.kt1 on come from a second one (p.x2, p.x2_rows: conv3 +
// shortcut of a stage's first block as one K loop, three launches of an episode).  DUAL says at compile time whether
// there is one: H2_ONE - the instance holds no second descriptor, no second set of row offsets and no select of descriptor
// and offsets per K-tile (that select cost the one-operand launches 1.4 %: DESIGN 8, item 1) -, H2_TWO, or H2_EITHER: the
// look at p.x2 at run time that every instance had before.  Only the one-operand two-K-group instance without the
// implicit-GEMM loader keeps H2_EITHER: as H2_ONE each of the five 6504 x 1024 -> 256 launches of an episode measured 2 us
// (8 %) slower in isolation, in both runs (profiles/launch_fixed_cost_ab.json, DESIGN appendix A row 63) - the instance
// that lost to the branch-free cursor too (OLD_CURSOR below).
constexpr int H2_ONE = 0, H2_TWO = 1, H2_EITHER = 2;
template <int WMW, int WNW, int RB, int NST, bool IM2COL, int KG, int DUAL>
__device__ __forceinline__ void conv_pw_h2_body(const ConvParams p, const H2Im2col q2, const int total_tiles) {
    static_assert(!(DUAL != H2_ONE && IM2COL), "the implicit-GEMM loader reads one operand");
    // NW / NTHR_G: waves / threads of ONE K-group (the roles wm, wn and the DMA rows are those of the wave inside its group)
    constexpr int BM = 32 * RB * WMW, BN = 64 * WNW, NW = WMW * WNW, NTHR_G = 64 * NW, NTHR = NTHR_G * KG;
    static_assert(KG == 1 || KG == 2, "one or two K-groups");
    constexpr int A_LD = BM / 8 / NW;                       // activation wave-instructions per wave per K-tile (8 rows each)
    constexpr int A_STAGE = BM * 128;                       // bytes
    constexpr int B_STAGE = 2 * BN * 64;                    // bytes of one K-tile of the weight image for BN columns
    constexpr int STAGE = A_STAGE + B_STAGE;                // bytes
    constexpr int BQ = BN / 16;                             // weight wave-instructions per plane per K-tile (16 rows each)
    constexpr int B_LD = 2 * BQ / NW;                       // weight wave-instructions per wave per K-tile
    static_assert(A_LD * 8 * NW == BM && B_LD * NW == 2 * BQ, "tile / wave split");
    constexpr int PER = A_LD + B_LD;                        // LDS-DMA wave-instructions per wave per K-tile
    constexpr int ROWS_PER_PASS = NTHR_G / 8;               // A rows one pass of a K-group's DMAs covers
    // The two-K-group instance without the implicit-GEMM loader keeps the K loop and the issue cursor it had before the
    // branch-free cursor below: with that cursor every 6504 x 1024 -> 256 launch of an episode measured 0.7 - 1 us slower in
    // isolation (23.1 - 24.9 -> 23.8 - 25.6 us, whichever of its parts was taken out again)
    constexpr bool OLD_CURSOR = KG == 2 && !IM2COL;
    // The wave-private epilogue (below, "the epilogue") of the one-K-group instances; two K-groups add their sums in the C
    // tile in a fixed order and keep the pass per wave row.  (-DH2_EPILOGUE_PASSES: that form on every instance, for the
    // phase clocks of tools/micro/build_x3_phases.sh to measure both with the same stamps.)
#ifdef H2_EPILOGUE_PASSES
    constexpr bool WPE = false;
#else
    constexpr bool WPE = KG == 1;
#endif
#ifdef H2_PHASES
    constexpr bool PEEL = true;                             // (the phase clocks tell a tile's first K-tile by its call site)
#else
    constexpr bool PEEL = WPE;
#endif
    constexpr int C_LD = 68;                                // floats of a staged C row: 64 + 4, so that the four row groups
                                                            // of a 16x16 block write to different banks
    static_assert(!WPE || NW * 16 * C_LD * 4 <= STAGE, "a 16-row block per wave fits the free stage");
    static_assert(NST == 2, "a ring of two stages: one K-tile in flight ahead of the one being multiplied");   // (three: measured 5-12 % slower, DESIGN appendix A row 53)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_h2[];

    const int t = threadIdx.x, lane = t & 63;
    const int kg = KG == 1 ? 0 : __builtin_amdgcn_readfirstlane((t >> 6) / NW);      // the wave's K-group
    const int wv = KG == 1 ? t >> 6 : (t >> 6) % NW;                // the wave inside its group
    const int tg = KG == 1 ? t : t % NTHR_G;                        // the thread inside its group
    const int wm = wv / WNW, wn = wv % WNW;
    const int M = IM2COL ? q2.M0 + q2.M1 : (p.n_img_dev ? min(p.n_img, *p.n_img_dev) : p.n_img) * p.Ho * p.Wo;
    int grp_valid = p.grp_valid;
    if (p.grp_rows && p.grp_count_dev) grp_valid = min(grp_valid, min(p.grp_items, *p.grp_count_dev) * p.grp_rows_per_item);

    float a_s = 1.f, a_inv = 1.f;                   // the wave's activation scale and its inverse (powers of two)

    const int col4 = tg & 7, row0 = tg >> 3;
    const int src_c4 = col4 ^ ((row0 >> 1) & 7);
    const i32x4 x_rs = make_rsrc(p.x, p.x_bytes);
    const i32x4 w_rs = make_rsrc(p.w3, p.w3_bytes);
    [[maybe_unused]] const bool dual = DUAL == H2_EITHER ? p.x2 != nullptr : DUAL == H2_TWO;
    [[maybe_unused]] const i32x4 x2_rs = DUAL != H2_ONE ? make_rsrc(dual ? p.x2 : p.x, dual ? p.x2_bytes : p.x_bytes) : x_rs;
    const int KT = p.K / BK / KG;                // K-steps: the K-tiles of one group; >= 2, K / BK a multiple of KG (launcher)
    const unsigned kt_bytes = (unsigned)(2 * p.npad3 * 64);          // one K-tile of the image, both planes, all rows
    const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)reinterpret_cast<size_t>(smem_h2) + kg * (NST * STAGE));   // the group's ring
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
    auto next_active = [&](int tile, int& m0, int& n0) -> int {
        for (; tile < total_tiles; tile += gridDim.x)
            if (coords(tile, m0, n0)) return tile;
        return -1;
    };

    // IM2COL: a[i] = byte offset of filter tap (0, 0) of the row's receptive field (may lie before the tensor: wraps),
    // a2[i] = bit (ky KW + kx) set when the tap is inside the image (and the row < M) | bit 31 when the row is of tensor 1;
    // two operands: a2[i] = the row's byte offset in the second one; H2_ONE outside IM2COL: no a2
    constexpr int A2_LD = (IM2COL || DUAL != H2_ONE) ? A_LD : 1;
    struct Offs { unsigned a[A_LD], a2[A2_LD], b[B_LD]; };
    unsigned b_lds[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) {
        const int q = wv + NW * i;                     // wave-instruction q of 2 BQ: plane q / BQ, rows 16 * (q % BQ) ..
        b_lds[i] = __builtin_amdgcn_readfirstlane((unsigned)(A_STAGE + (q / BQ) * (BN * 64) + (q % BQ) * 1024));
    }
    auto offsets = [&](int m0, int n0) -> Offs {
        Offs o;
        o.a2[0] = 0u;
        // rows past M, and the rows of a group past its valid ones (the unwritten tail of a Winograd V), are fetched out of
        // bounds - zeros: a wave's rows share one scale, so whatever lies in memory there must not reach the fragment
        const int g_end = p.grp_rows ? (m0 / p.grp_rows) * p.grp_rows + grp_valid : M;
#pragma unroll
        for (int i = 0; i < A_LD; ++i) {
            const int m = m0 + row0 + ROWS_PER_PASS * i;
            if constexpr (IM2COL) {
                o.a[i] = 0u; o.a2[i] = 0u;
                if (m < M) {
                    const bool t1 = m >= q2.M0;
                    const int mm = t1 ? m - q2.M0 : m;
                    const int H = t1 ? q2.H1 : p.H, W = t1 ? q2.W1 : p.W, Wo = t1 ? q2.Wo1 : p.Wo;
                    const int HoWo = (t1 ? q2.Ho1 : p.Ho) * Wo;
                    const int img = mm / HoWo;
                    const int rem = mm - img * HoWo;
                    const int oy = rem / Wo;
                    const int ox = rem - oy * Wo;
                    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
                    o.a[i] = (t1 ? q2.x_off1 : q2.x_off0) + (unsigned)((((img * H + iy0) * W + ix0) * p.Cin + src_c4 * 4) * 4);
                    unsigned tm = t1 ? 0x80000000u : 0u;
                    int tp = 0;
                    for (int ky = 0; ky < p.KH; ++ky) {
                        const bool y_ok = (unsigned)(iy0 + ky) < (unsigned)H;
                        for (int kx = 0; kx < p.KW; ++kx, ++tp)
                            if (y_ok && (unsigned)(ix0 + kx) < (unsigned)W) tm |= 1u << tp;
                    }
                    o.a2[i] = tm;
                }
                continue;
            }
            const bool in = m < M && m < g_end;
            o.a[i] = in ? (unsigned)((m * p.Cin + src_c4 * 4) * 4) : OOB;
            if constexpr (DUAL != H2_ONE) {
                o.a2[i] = OOB;
                if (dual && in) o.a2[i] = (unsigned)(((p.x2_rows ? p.x2_rows[m] : m) * p.cin2 + src_c4 * 4) * 4);
            }
        }
        unsigned g0 = 0;
        if (p.grp_rows) g0 = (unsigned)(m0 / p.grp_rows) * (unsigned)(KT * KG) * kt_bytes;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) {
            const int q = wv + NW * i;
            const int plane = q / BQ, row = (q % BQ) * 16 + (lane >> 2);
            o.b[i] = g0 + (unsigned)(((plane * p.npad3 + n0 + row) * 4 + (lane & 3)) * 16);
        }
        return o;
    };
    // Issue cursor: the K-step the next request is for, as the byte offsets it takes (all wave-uniform).  seek() places
    // it once per output tile; advance() moves it one K-step on by adds of loop-invariant values - no multiply, no division
    // and no branch per K-tile.  IM2COL: the K-tiles of a filter row are contiguous in an NHWC row (Cin * 4 = 128 bytes
    // x the slices of a tap), so the tap offset grows by 128 per K-tile and by the rest of the image row at a row's end.
    const unsigned ko_step = (unsigned)(KG * BK * 4), kb_step = (unsigned)KG * kt_bytes;
    [[maybe_unused]] const unsigned ko1 = (DUAL != H2_ONE && dual) ? (unsigned)(p.kt1 * BK * 4) : 0xffffffffu;      // the second operand's first K-tile, in bytes of a row (one operand: never reached)
    unsigned c_ko = 0u, c_kb = 0u;                   // the K-tile's bytes in an activation row / in the weight image
    int c_tap = 0, c_cs = 0, c_kx = 0;               // IM2COL: filter tap, channel slice of it, column of the tap
    unsigned c_off0 = 0u, c_off1 = 0u;               //         the tap's byte offset in tensor 0 / 1
    const int im_ct = 1 << q2.cin_shift;
    const unsigned im_skip0 = (unsigned)((p.W - p.KW) * p.Cin * 4), im_skip1 = (unsigned)((q2.W1 - p.KW) * p.Cin * 4);
    auto seek = [&](int step) {
        const int kt = step * KG + kg;           // the absolute K-tile
        c_ko = (unsigned)(kt * BK * 4);
        c_kb = (unsigned)kt * kt_bytes;
        if constexpr (IM2COL) {
            c_tap = kt >> q2.cin_shift;
            c_cs = kt - (c_tap << q2.cin_shift);
            const int ky = p.KW == 3 ? (c_tap * 43) >> 7 : c_tap;         // tap / 3 for tap <= 8; KW == 1: one column
            c_kx = c_tap - ky * p.KW;
            c_off0 = (unsigned)(((ky * p.W + c_kx) * p.Cin + c_cs * BK) * 4);
            c_off1 = (unsigned)(((ky * q2.W1 + c_kx) * p.Cin + c_cs * BK) * 4);
        }
    };
    auto advance = [&]() {
        c_ko += ko_step;
        c_kb += kb_step;
        if constexpr (IM2COL) {
#pragma unroll
            for (int g = 0; g < KG; ++g) {
                const bool tw = ++c_cs == im_ct;             // the tap's last slice is behind
                c_cs = tw ? 0 : c_cs;
                c_tap += tw;
                c_kx += tw;
                const bool rw = c_kx == p.KW;                // ... and the filter row's last tap
                c_kx = rw ? 0 : c_kx;
                c_off0 += 128u + (rw ? im_skip0 : 0u);
                c_off1 += 128u + (rw ? im_skip1 : 0u);
            }
        }
    };
    // LDS-DMA wave-instruction `idx` of the PER a wave issues per K-tile (A_LD activation ones, then B_LD weight ones) for
    // the cursor's K-tile of the output tile `o`, into the stage at byte `wr` of the group's ring
    auto piece = [&](const Offs& o, const unsigned wr, const int idx) {
        const unsigned st = lds_base + wr;
        if (idx >= A_LD) {
            const int i = idx - A_LD;
            lds_dma16_s(w_rs, st + b_lds[i], o.b[i], c_kb);
            return;
        }
        const int i = idx;
        const unsigned dst = st + wave_row_bytes + i * ROWS_PER_PASS * 128;
        if constexpr (IM2COL) {
            const bool ok = (o.a2[i] >> c_tap) & 1u;
            const unsigned voff = ok ? o.a[i] + ((o.a2[i] >> 31) ? c_off1 : c_off0) : OOB;     // out-of-image taps: zeros
            lds_dma16_s(x_rs, dst, voff, 0u);
        } else if constexpr (DUAL != H2_ONE) {
            // the K-tiles from p.kt1 on come from the second operand: a select of descriptor and offsets, not a branch
            const bool second = c_ko >= ko1;
            i32x4 rs;
            rs[0] = second ? x2_rs[0] : x_rs[0]; rs[1] = second ? x2_rs[1] : x_rs[1];
            rs[2] = second ? x2_rs[2] : x_rs[2]; rs[3] = x_rs[3];
            // (the K offset is selected next to the row offset, in a vector register: back into a scalar one by hand)
            lds_dma16_s(rs, dst, second ? o.a2[i] : o.a[i], __builtin_amdgcn_readfirstlane(second ? c_ko - ko1 : c_ko));
        } else {
            lds_dma16_s(x_rs, dst, o.a[i], c_ko);
        }
    };

    // (OLD_CURSOR) K-step `step` of the output tile `o` into the stage at byte `wr` of the group's ring, the offsets computed
    // from the step
    auto issue_step = [&](const Offs& o, const int step, const unsigned wr) {
        const int kt = step * KG + kg;           // the absolute K-tile
        const unsigned st = lds_base + wr;
        const unsigned sa = st + wave_row_bytes;
        const unsigned ko = (unsigned)(kt * BK * 4);
        bool second = false;
        if constexpr (DUAL != H2_ONE) second = dual && kt >= p.kt1;
        if (second) {
            const unsigned ko2 = (unsigned)((kt - p.kt1) * BK * 4);
#pragma unroll
            for (int i = 0; i < A_LD; ++i) lds_dma16_s(x2_rs, sa + i * ROWS_PER_PASS * 128, o.a2[DUAL != H2_ONE ? i : 0], ko2);
        } else {
#pragma unroll
            for (int i = 0; i < A_LD; ++i) lds_dma16_s(x_rs, sa + i * ROWS_PER_PASS * 128, o.a[i], ko);
        }
        const unsigned kb = (unsigned)kt * kt_bytes;
#pragma unroll
        for (int i = 0; i < B_LD; ++i) lds_dma16_s(w_rs, st + b_lds[i], o.b[i], kb);
    };

    // 16x16x32: lane (r = lane & 15, g = lane >> 4) holds 8 operand positions of row / column r of its block; the k order
    // (lane group g: the f32 chunks g and g + 4 of an activation row) and the chunk swizzles are conv_pw_x3_kernel's
    const int r16 = lane & 15, g4 = lane >> 4;
    const int a16_row = wm * 32 * RB + r16;       // (+ 16 i for row block i: (row >> 1) & 7 is the same)
    const unsigned a16_sw = (unsigned)((a16_row >> 1) & 7);
    const unsigned a16_rd0 = (unsigned)(a16_row * 128) + ((((unsigned)g4) ^ a16_sw) << 4);
    const unsigned a16_rd1 = (unsigned)(a16_row * 128) + ((((unsigned)(g4 + 4)) ^ a16_sw) << 4);
    const int n16 = wn * 64 + r16;                // (+ 16 j for column block j: (n >> 2) & 3 is the same)
    const unsigned tau16 = (0x1230u >> (4 * ((n16 >> 2) & 3))) & 3u;           // {0, 3, 2, 1}
    const unsigned b16_rd = (unsigned)(A_STAGE + n16 * 64) + ((((unsigned)g4) ^ tau16) << 4);

    if (p.stamp && t == 0 && blockIdx.x == 0) atomicExch(p.stamp, __builtin_amdgcn_s_memrealtime());
    auto leave = [&]() {
        if (!p.stamp || t != 0) return;
        const unsigned shard = blockIdx.x & 7u;
        const unsigned long long in_shard = (gridDim.x - shard + 7u) / 8u;
        unsigned long long* const sc = p.stamp + 8 * (1 + shard);
        if (atomicAdd(sc, 1ull) != in_shard - 1) return;
        atomicExch(sc, 0ull);
        const unsigned long long shards = gridDim.x < 8u ? gridDim.x : 8u;
        if (atomicAdd(p.stamp + 2, 1ull) != shards - 1) return;
        const unsigned long long d = __builtin_amdgcn_s_memrealtime() - atomicExch(p.stamp, 0ull);
        atomicExch(p.stamp + 2, 0ull);
        atomicAdd(p.stamp + 1, d);
        atomicAdd(p.stamp + 3, 1ull);
        atomicMin(p.stamp + 4, d);
        atomicMax(p.stamp + 5, d);
    };

    int m0, n0, nm0 = 0, nn0 = 0;
    int tile = next_active(blockIdx.x, m0, n0);
    if (tile < 0) { leave(); return; }
    Offs cur = offsets(m0, n0);
    int ntile = next_active(tile + gridDim.x, nm0, nn0);
    auto following = [&]() -> Offs { return ntile >= 0 ? offsets(nm0, nn0) : cur; };
    Offs nxt = following();
    // One K-step is in flight ahead of the one being multiplied: iteration kt of an output tile requests K-step kt + 1 of
    // it, the last one K-step 0 of the next output tile (when there is one) - into the stage the iteration before read
    // (OLD_CURSOR) the next K-step to be requested is step ic_kt of the current (ic_next = false) or the next output tile
    int ic_kt = 0;
    bool ic_next = false;
    auto issue_one = [&](const unsigned wr) {
        if (!ic_next) {
            issue_step(cur, ic_kt, wr);
            if (++ic_kt == KT) { ic_next = true; ic_kt = 0; }
        } else {
            if (ntile < 0 || ic_kt >= KT) return;
            issue_step(nxt, ic_kt, wr);
            ++ic_kt;
        }
    };
    if constexpr (OLD_CURSOR) {
        issue_one(0u);
    } else {
        seek(0);
#pragma unroll
        for (int i = 0; i < PER; ++i) piece(cur, 0u, i);
        advance();
    }
    // (WPE) the first K-tile of an output tile finds its pieces waited for: here for the workgroup's first tile - its first
    // K-tile would wait at once anyway - and in the epilogue of the tile before for every other (k_tile, `first`)
    if constexpr (WPE) x3_wait_vm<0>();
    unsigned rd = 0u;                               // byte offset in the ring of the stage being multiplied: 0 or STAGE
#ifdef H2_PHASES
    bool walked = false;                            // the workgroup has an output tile behind it
    // [7 .. 12]: the time outside the K-tiles by its parts, summed over the output tiles ([13] counts them): [8] last MFMA ->
    // past the first epilogue barrier, [9] C-tile LDS writes and their barriers / waits, [10] the wait for the residual
    // rows (and whatever else is in flight), [11] LDS reads, arithmetic and store issue, [12] the tile walk (next_active,
    // offsets, accumulator clear; before the workgroup's first tile: nothing); [5] keeps what lies between the MFMA mark
    // of a K-tile and the top of the next one; [7] of [0]: the vmcnt wait at the top of the first K-tile of a tile that is
    // not the workgroup's first
    unsigned long long ph_[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_ = __builtin_amdgcn_s_memtime();
    const unsigned long long begin_ = last_;
#endif

    while (true) {
        f32x4 acc[2 * RB][4];
#pragma unroll
        for (int i = 0; i < 2 * RB; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        bool have_s = false;                        // no scale chosen yet for this output tile
        float a_lim = 0.f;                          // |x| above this leaves the f16 range under the current scale (no scale yet:
                                                    // any non-zero element; an all-zero fragment - padded rows - passes as it is)
        a_s = 1.f; a_inv = 1.f;
        // (WPE) the residual values of the rows and the column quad this thread stores in the epilogue: rows g4 + 4 k of
        // the wave's 16-row block i, columns 4 r16 .. + 3 of the wave's 64.  Zeros without a residual and past M / Cout.
        // Block 0 is requested ahead of the epilogue's barrier, block i + 1 ahead of block i's stores.  (Requested behind the
        // last K-tile's requests, to land under its MFMAs, they are live beside the K-tile's fragments: all 2 RB blocks
        // cost 44 - 48 registers, block 0 alone 28 - 34, and the implicit-GEMM instances of the 64-row and 128 x 64 tiles
        // pass the 168 registers that three workgroups per CU leave a wave: DESIGN appendix A.)
        float4 res_e[4];
        auto residual_rows = [&](const int i) {
            const int n = n0 + wn * 64 + r16 * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = m0 + wm * (32 * RB) + 16 * i + g4 + 4 * k;
                res_e[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.residual && m < M && n < p.Cout) res_e[k] = *reinterpret_cast<const float4*>(p.residual + (size_t)m * p.Cout + n);
            }
        };
        // One K-tile, a straight line but for the overflow watch: wait, barrier, the requests for the cursor's
        // K-tile of the output tile `o` into the other stage (it was last read in the iteration before, and every wave has
        // passed this one's barrier), LDS reads, watch, split and MFMAs.  `last`: the last K-tile of an output tile
        auto k_tile = [&](auto&& requests, auto first) {
            // the K-tile has landed: everything in flight is waited for.  `first` (WPE: the first K-tile of an output
            // tile): every wave has waited for its pieces of this K-tile already - in the epilogue of the tile before,
            // ahead of its first store - so only that epilogue's stores are in flight: they are left to the next K-tile's
            // wait, one K-tile of work later, and the barrier alone says that all the pieces have landed.  (The stores
            // share the counter with the loads: waited for here, their acknowledgements stood in front of this K-tile.)
            if constexpr (decltype(first)::value) H2_T(12); else H2_T(5);     // since the epilogue's last store: the tile walk | since the last MFMA
            if constexpr (!(WPE && decltype(first)::value)) x3_wait_vm<0>();
#ifdef H2_PHASES
            if (decltype(first)::value && walked) H2_T(7);
#endif
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();            // ... for every wave; and every wave is done with the stage before
            asm volatile("" ::: "memory");           // (no LDS read moves above the barrier)
            H2_T(0);
            const unsigned wr = rd ^ (unsigned)STAGE;
            // the requests for the cursor's K-tile of `o` (the last K-tile of the last output tile: none)
            requests(wr);
            asm volatile("" ::: "memory");
            H2_T(1);
            const unsigned char* const S = smem_h2 + (KG == 1 ? 0 : kg * (NST * STAGE)) + rd;
            float4 alo[2 * RB], ahi[2 * RB];
            f16x8_t bq[4][2];
#pragma unroll
            for (int i = 0; i < 2 * RB; ++i) {
                alo[i] = *reinterpret_cast<const float4*>(S + a16_rd0 + i * (16 * 128));
                ahi[i] = *reinterpret_cast<const float4*>(S + a16_rd1 + i * (16 * 128));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    bq[j][q] = *reinterpret_cast<const f16x8_t*>(S + b16_rd + j * (16 * 64) + q * (BN * 64));
            __builtin_amdgcn_sched_barrier(0);       // every read of the K-tile in flight before the first split
#ifdef H2_PHASES
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            H2_T(2);
#endif
            // a new scale from the maximum of this K-tile's fragment (wave-uniform); the accumulators follow it.  Only finite
            // elements count: a row holding Inf / NaN comes out non-finite whatever the scale, and must not take the scale of
            // the wave's other rows with it (Inf would leave them at the old scale - or at 1 - however large or small they are)
            auto adapt = [&]() {
                auto fin = [](const float v) { const float a = fabsf(v); return a < __builtin_inff() ? a : 0.f; };   // NaN: 0
                float m = 0.f;
#pragma unroll
                for (int i = 0; i < 2 * RB; ++i) {
                    m = fmaxf(m, fmaxf(fmaxf(fin(alo[i].x), fin(alo[i].y)), fmaxf(fin(alo[i].z), fin(alo[i].w))));
                    m = fmaxf(m, fmaxf(fmaxf(fin(ahi[i].x), fin(ahi[i].y)), fmaxf(fin(ahi[i].z), fin(ahi[i].w))));
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
                const unsigned mb = __builtin_amdgcn_readfirstlane(__float_as_uint(m));
                const int e = (int)((mb >> 23) & 0xffu);
                if (e < 27) return;                         // all zero (or tiny, or nothing finite): keep the scale
                // the finite elements fit the scale the wave has (only a non-finite one sent it here): keep it.  (A finite
                // fragment comes here only with an element above a_lim: this never returns for one, its bits are unchanged.)
                if (have_s && __uint_as_float(mb) <= a_lim) return;
                const float ns = __uint_as_float((unsigned)(267 - e) << 23);         // 2^(13 - (e - 127))
                const float ratio = ns * a_inv;                                      // new / old, a power of two
                if (have_s) {
#pragma unroll
                    for (int i = 0; i < 2 * RB; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] *= ratio;
                }
                a_s = ns;
                a_inv = __uint_as_float((unsigned)(e - 13) << 23);
                a_lim = 65504.f * a_inv;
                have_s = true;
            };
            {                                        // one look at the raw fragment per K-tile, then straight-line code
                float big = h2_absmax16(alo[0], ahi[0], alo[1], ahi[1]);
                if constexpr (RB == 2) big = fmaxf(big, h2_absmax16(alo[2], ahi[2], alo[3], ahi[3]));
                // (a_lim = 0 until a scale is chosen: the first K-tile with a non-zero element chooses it)
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(big <= a_lim)) != 0ull, 0)) adapt();
            }
            if constexpr (RB == 2 || OLD_CURSOR) {
                // every row fragment split, then multiplied, one after the other (the split of the next fragment in the gaps
                // of this one's MFMAs, as below, measured 2 - 4 % slower on the 128-row instance: DESIGN appendix A row 58)
#pragma unroll
                for (int i = 0; i < 2 * RB; ++i) {
                    const H2Frag a = h2_split(alo[i], ahi[i], a_s);
#ifdef H2_PHASES
                    if (i == 0) { asm volatile("s_nop 0" ::"v"(a.hi), "v"(a.lo)); H2_T(3); }
#endif
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 c = acc[i][j];
                        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, bq[j][0], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, bq[j][1], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, bq[j][0], c, 0, 0, 0);
                        acc[i][j] = c;
                    }
                }
            } else {
                // row fragment 0 is split ahead of the MFMAs, fragment 1 in the gaps of fragment 0's: one step (two
                // instructions) behind each of its first eight MFMAs, pinned there by a scheduling barrier per MFMA
                unsigned fh[2][4], fl[2][4];         // the planes of the fragment being multiplied / being split
                h2_split4(alo[0].x, alo[0].y, alo[0].z, alo[0].w, a_s, fh[0][0], fh[0][1], fl[0][0], fl[0][1]);
                h2_split4(ahi[0].x, ahi[0].y, ahi[0].z, ahi[0].w, a_s, fh[0][2], fh[0][3], fl[0][2], fl[0][3]);
#ifdef H2_PHASES
                asm volatile("s_nop 0" ::"v"(fh[0][0]), "v"(fl[0][3]));
                H2_T(3);
#endif
#pragma unroll
                for (int i = 0; i < 2 * RB; ++i) {
                    const int u = i & 1, v = u ^ 1;
                    const f16x8_t a_hi = __builtin_bit_cast(f16x8_t, make_uint4(fh[u][0], fh[u][1], fh[u][2], fh[u][3]));
                    const f16x8_t a_lo = __builtin_bit_cast(f16x8_t, make_uint4(fl[u][0], fl[u][1], fl[u][2], fl[u][3]));
                    const int n = i + 1 < 2 * RB ? i + 1 : i;        // (the last fragment: nothing left to split)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 c = acc[i][j];
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            c = __builtin_amdgcn_mfma_f32_16x16x32_f16(m == 0 ? a_lo : a_hi, bq[j][m == 1 ? 1 : 0], c, 0, 0, 0);
                            if (m < 2 && i + 1 < 2 * RB) {
                                const int sn = 2 * j + m, half = sn >> 2;      // step sn of the eight of a fragment: 4 per half
                                const float4& x = half == 0 ? alo[n] : ahi[n];
                                h2_split4_step(sn & 3, x.x, x.y, x.z, x.w, a_s, fh[v][2 * half], fh[v][2 * half + 1],
                                               fl[v][2 * half], fl[v][2 * half + 1]);
                            }
                            __builtin_amdgcn_sched_barrier(0);       // (nothing moves out of its gap)
                        }
                        acc[i][j] = c;
                    }
                }
            }
#ifdef H2_PHASES
            asm volatile("s_nop 0" ::"v"(acc[0][0][0]), "v"(acc[2 * RB - 1][3][3]));
            H2_T(4);
            ++ph_[6];
#endif
            if constexpr (!OLD_CURSOR) advance();
            rd = wr;
        };
        auto request = [&](const Offs& o, const unsigned wr) {
#pragma unroll
            for (int k = 0; k < PER; ++k) piece(o, wr, k);
        };
        if constexpr (OLD_CURSOR) {
            for (int kt = 0; kt < KT; ++kt) k_tile([&](const unsigned wr) { issue_one(wr); }, H2No{});
        } else {
            // (WPE: the first K-tile is a call of its own - it does not wait; two K-groups keep the one loop they had)
            if constexpr (PEEL) k_tile([&](const unsigned wr) { request(cur, wr); }, H2Yes{});
            for (int kt = PEEL ? 1 : 0; kt < KT - 1; ++kt) k_tile([&](const unsigned wr) { request(cur, wr); }, H2No{});
            seek(0);
            k_tile([&](const unsigned wr) { if (ntile >= 0) request(nxt, wr); }, H2No{});
        }
        // the stage of the last K-tile (the other one than `rd` now; group 0's ring) takes the C tile once every wave
        // has read it
        float* const cbase = reinterpret_cast<float*>(smem_h2 + (rd ^ (unsigned)STAGE));
        const int em0 = m0, en0 = n0;
        const float* const winv = p.w_inv + (p.grp_rows ? (size_t)(em0 / p.grp_rows) * p.npad3 : 0);
        if constexpr (WPE) {
            // The wave-private epilogue.  ONE workgroup barrier: every wave has read the last K-tile's stage before any
            // wave writes to it.  Then each wave is on its own: it takes its accumulators through a region of that stage
            // no other wave touches (16 rows x C_LD floats), one 16-row block at a time - 16 ds_write_b32 per lane in the
            // 16x16 C/D layout (col = lane & 15, row = 4 * (lane >> 4) + reg), its own lgkmcnt wait, and the block back as
            // float4: lane (r16, g4) reads columns 4 r16 .. + 3 of rows g4 + 4 k, so a wave instruction stores 4 rows x
            // 256 bytes.  LDS operations of one wave execute in order: the next block's writes need no wait for these reads.
            // The barrier at the top of the next output tile's first K-tile keeps the stage from being refilled before
            // every wave is through.  The arithmetic per element and its order are those of the pass form below.
            residual_rows(0);                        // ahead of the barrier: in flight while the waves gather
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            H2_T(8);
            float* const cw0 = cbase + wv * (16 * C_LD);
            const int n = en0 + wn * 64 + r16 * 4;
            const bool n_in = n < p.Cout;
            float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f), iv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n_in) {
                if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + n);
                if (p.shift) sh = *reinterpret_cast<const float4*>(p.shift + n);
                iv = *reinterpret_cast<const float4*>(winv + n);                  // the column scales out again (exact)
            }
#pragma unroll
            for (int i = 0; i < 2 * RB; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) cw0[(4 * g4 + r) * C_LD + 16 * j + r16] = acc[i][j][r] * a_inv;      // the wave's scale out again
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                H2_T(9);
                if (i == 0) {
                    // Everything this wave has in flight - its pieces of the next output tile's first K-tile, the residual
                    // rows, the vectors above: all requested a K-tile ago or needed now - BEFORE its first store, so that
                    // the next tile's first K-tile need not wait for the stores (k_tile, `first`).  Not a counted wait:
                    // the threads of a ragged tile issue fewer stores.
                    x3_wait_vm<0>();
                    H2_T(10);
                }
                float4 res[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) res[k] = res_e[k];
                if (i + 1 < 2 * RB) residual_rows(i + 1);       // (m0, n0 are still this tile's)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int row = g4 + 4 * k;
                    const int m = em0 + wm * (32 * RB) + 16 * i + row;
                    if (m >= M || !n_in) continue;
                    float4 v = *reinterpret_cast<const float4*>(cw0 + row * C_LD + r16 * 4);
                    v.x *= iv.x; v.y *= iv.y; v.z *= iv.z; v.w *= iv.w;
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                    v.x += res[k].x; v.y += res[k].y; v.z += res[k].z; v.w += res[k].w;
                    if (p.relu) {
                        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                    }
                    float* const yrow = (IM2COL && m >= q2.M0) ? q2.y1 + (size_t)(m - q2.M0) * p.Cout : p.y + (size_t)m * p.Cout;
                    *reinterpret_cast<float4*>(yrow + n) = v;
                }
                asm volatile("" ::: "memory");
                H2_T(11);
            }
        }
        // (two K-groups) one pass per wave row: PR = 32 RB rows x 128 floats (16 / 32 KB: fits the stage for either row tile)
        constexpr int PR = 32 * RB;
#pragma unroll
        for (int pass = 0; pass < (WPE ? 0 : WMW); ++pass) {
            __syncthreads();
#ifdef H2_PHASES
            if (pass == 0) H2_T(8);
#endif
            if (wm == pass && kg == 0) {             // 16x16 C/D layout: col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
                for (int i = 0; i < 2 * RB; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float* cw = cbase + (16 * i + 4 * g4) * BN + wn * 64 + 16 * j + r16;
#pragma unroll
                        for (int r = 0; r < 4; ++r) cw[r * BN] = acc[i][j][r] * a_inv;      // the wave's scale out again
                    }
            }
            __syncthreads();
            if constexpr (KG == 2) {                 // the second group's sum on top, always in this order
                if (wm == pass && kg == 1) {
#pragma unroll
                    for (int i = 0; i < 2 * RB; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float* cw = cbase + (16 * i + 4 * g4) * BN + wn * 64 + 16 * j + r16;
#pragma unroll
                            for (int r = 0; r < 4; ++r) cw[r * BN] += acc[i][j][r] * a_inv;
                        }
                }
                __syncthreads();
            }
            H2_T(9);
            constexpr int C4 = BN / 4, RPP = NTHR / C4, NPASS = PR / RPP, SW = NPASS < 4 ? NPASS : 4;
            static_assert(NPASS % SW == 0, "row sweeps in groups of SW");
            const int c4 = t % C4, rr = t / C4;
            const int n = en0 + c4 * 4;
            if (n < p.Cout) {
                float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
                if (p.scale) sc = *reinterpret_cast<const float4*>(p.scale + n);
                if (p.shift) sh = *reinterpret_cast<const float4*>(p.shift + n);
                const float4 iv = *reinterpret_cast<const float4*>(winv + n);     // the column scales out again (exact)
#pragma unroll
                for (int k0 = 0; k0 < NPASS; k0 += SW) {
                    float4 res[SW];
#pragma unroll
                    for (int k = 0; k < SW; ++k) {
                        const int m = em0 + PR * pass + rr + RPP * (k0 + k);
                        res[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (p.residual && m < M) res[k] = *reinterpret_cast<const float4*>(p.residual + (size_t)m * p.Cout + n);
                    }
#ifdef H2_PHASES
                    x3_wait_vm<0>();                 // (the product waits where the compiler puts it: before the first use)
                    H2_T(10);
#endif
#pragma unroll
                    for (int k = 0; k < SW; ++k) {
                        const int row = rr + RPP * (k0 + k);
                        const int m = em0 + PR * pass + row;
                        if (m >= M) continue;
                        float4 v = *reinterpret_cast<const float4*>(cbase + row * BN + c4 * 4);
                        v.x *= iv.x; v.y *= iv.y; v.z *= iv.z; v.w *= iv.w;
                        v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                        v.x += res[k].x; v.y += res[k].y; v.z += res[k].z; v.w += res[k].w;
                        if (p.relu) {
                            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                        }
                        float* const yrow = (IM2COL && m >= q2.M0) ? q2.y1 + (size_t)(m - q2.M0) * p.Cout : p.y + (size_t)m * p.Cout;
                        *reinterpret_cast<float4*>(yrow + n) = v;
                    }
#ifdef H2_PHASES
                    asm volatile("" ::: "memory");
                    H2_T(11);
#endif
                }
            }
        }
#ifdef H2_PHASES
        ++ph_[13];
        walked = true;
#endif
        if (ntile < 0) break;
        // the next output tile becomes the current one (its first K-step is requested already: the cursor stands at its second)
        tile = ntile; m0 = nm0; n0 = nn0;
        cur = nxt;
        if constexpr (OLD_CURSOR) {
            ic_next = ic_kt >= KT;                   // (KT == 1: the whole new current tile is requested already)
            if (ic_next) ic_kt = 0;
        }
        ntile = next_active(tile + gridDim.x, nm0, nn0);
        nxt = following();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef H2_PHASES
    if (p.ws && lane == 0 && wv == 0 && kg == 0 && blockIdx.x < 2) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(p.ws) + 8 * blockIdx.x;
        for (int i = 0; i < 7; ++i) o[i] = ph_[i];
        o[7] = __builtin_amdgcn_s_memtime() - begin_;
        for (int i = 7; i < 14; ++i) o[16 + i - 7] = ph_[i];          // the epilogue's parts: behind the two workgroups' [0 .. 7]
    }
#endif
    leave();
}

// The one-operand instance: every launch but conv3 + shortcut.
template <int WMW, int WNW, int RB, int NST, bool IM2COL, int KG = 1>
__global__ __launch_bounds__(64 * WMW * WNW * KG, KG == 1 ? 2 : 1) void conv_pw_h2_kernel(const ConvParams p, const H2Im2col q2, const int total_tiles) {
    conv_pw_h2_body<WMW, WNW, RB, NST, IM2COL, KG, (KG == 2 && !IM2COL) ? H2_EITHER : H2_ONE>(p, q2, total_tiles);
}
// The two-operand instance (launches with p.x2; never the implicit-GEMM loader).
template <int WMW, int WNW, int RB, int NST, int KG = 1>
__global__ __launch_bounds__(64 * WMW * WNW * KG, KG == 1 ? 2 : 1) void conv_pw_h2_kernel_dual(const ConvParams p, const H2Im2col q2, const int total_tiles) {
    conv_pw_h2_body<WMW, WNW, RB, NST, false, KG, H2_TWO>(p, q2, total_tiles);
}
