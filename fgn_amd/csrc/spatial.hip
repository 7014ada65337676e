// HBM-bound spatial kernels of the FGN path: input layout conversion, stem max-pool,
// RoIAlign (both flavours the reference uses) and the support-set reductions.
// All tensors are NHWC fp32; every lane moves 16 B and a wave covers contiguous
// channels, so global accesses are fully coalesced.
#include "common.h"
#include "roi_geom.h"

// ----------------------------------------------------------------------------------
// NCHW [B,3,H,W] -> NHWC4 [B,H,W,4] (4th channel zero) so the 7x7 stem conv can stage
// one filter tap per 16-byte load.  (input side of fgn.py:212,215)
// ----------------------------------------------------------------------------------
__global__ void nchw3_to_nhwc4_kernel(const float* __restrict__ x, float4* __restrict__ y, int HW,
                                      long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / HW;
        const int p = (int)(i - b * HW);
        const float* s = x + b * 3 * HW + p;
        y[i] = make_float4(s[0], s[HW], s[2 * (size_t)HW], 0.f);
    }
}

extern "C" int fgn_nchw3_to_nhwc4_f32(const float* x, float* y, int n_img, int H, int W,
                                      hipStream_t stream) {
    if (!x || !y) return FGN_ERR_ARG;
    const long long total = (long long)n_img * H * W;
    if (total == 0) return FGN_OK;
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(nchw3_to_nhwc4_kernel, dim3(grid), dim3(256), 0, stream, x,
                       reinterpret_cast<float4*>(y), H * W, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// uint8 channels-last [n,H,W,3] -> NHWC4 [n,H,W,4] fp32, normalised: the same tensor nchw3_to_nhwc4_kernel makes of the
// host-normalised NCHW image (ToTensor + Normalize of the reference's data loader, mnistiseg_ds.py:69-70, moved behind
// the upload).  y = {lut[0][r], lut[1][g], lut[2][b], +0}: the per-channel table holds the host's own
// ((v / scale - mean) / std) for the 256 byte values, so the result does not depend on how the device rounds a division.
// The batch is one flat pixel array; a lane takes 4 consecutive pixels: one 12-byte load (dword-aligned: three dwords)
// and four 16-byte stores, 3 B read and 16 B written per pixel.  Pixels [4 * groups, total) - the last total % 4, or all
// of them when x is not dword-aligned (groups = 0: a sliced view) - go one per lane.
// The table sits in LDS (3 KB per workgroup); the lookups are ds_read_b32 at data-dependent addresses, so lanes of a
// half-wave do meet on a bank.  Accepted: an image's bytes repeat (background) and identical addresses broadcast, and
// the kernel waits on HBM stores, 64 B per lane and group, not on the LDS.
// ----------------------------------------------------------------------------------
constexpr int U8_BLOCK = 256;
constexpr int U8_GRID_CAP = 256 * 8;      // workgroups; more 4-pixel groups than U8_GRID_CAP * U8_BLOCK take further passes
__global__ __launch_bounds__(U8_BLOCK) void u8hwc3_to_nhwc4_kernel(const uint8_t* __restrict__ x,
                                                                   const float* __restrict__ lut,
                                                                   float4* __restrict__ y, long long groups,
                                                                   long long total) {
    __shared__ float t[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += U8_BLOCK) t[i] = lut[i];
    __syncthreads();
    const long long first = blockIdx.x * (long long)U8_BLOCK + threadIdx.x, step = (long long)gridDim.x * U8_BLOCK;
    const uint3* x12 = reinterpret_cast<const uint3*>(x);
    for (long long g = first; g < groups; g += step) {
        const uint3 w = x12[g];           // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        float4* o = y + 4 * g;
        o[0] = make_float4(t[w.x & 255u], t[256 + ((w.x >> 8) & 255u)], t[512 + ((w.x >> 16) & 255u)], 0.f);
        o[1] = make_float4(t[w.x >> 24], t[256 + (w.y & 255u)], t[512 + ((w.y >> 8) & 255u)], 0.f);
        o[2] = make_float4(t[(w.y >> 16) & 255u], t[256 + (w.y >> 24)], t[512 + (w.z & 255u)], 0.f);
        o[3] = make_float4(t[(w.z >> 8) & 255u], t[256 + ((w.z >> 16) & 255u)], t[512 + (w.z >> 24)], 0.f);
    }
    for (long long p = 4 * groups + first; p < total; p += step) {
        const uint8_t* s = x + 3 * p;
        y[p] = make_float4(t[s[0]], t[256 + s[1]], t[512 + s[2]], 0.f);
    }
}

extern "C" int fgn_u8hwc3_to_nhwc4_f32(const unsigned char* x, const float* lut, float* y, int n_img, int H, int W,
                                       hipStream_t stream) {
    if (!x || !lut || !y) return FGN_ERR_ARG;
    if (n_img < 0 || H < 0 || W < 0) return FGN_ERR_SHAPE;
    const long long total = (long long)n_img * H * W;
    if (total == 0) return FGN_OK;
    const long long groups = (reinterpret_cast<uintptr_t>(x) & 3u) ? 0 : total / 4;
    const long long items = std::max(groups, total - 4 * groups);
    const int grid = (int)std::min<long long>((items + U8_BLOCK - 1) / U8_BLOCK, U8_GRID_CAP);
    hipLaunchKernelGGL(u8hwc3_to_nhwc4_kernel, dim3(grid), dim3(U8_BLOCK), 0, stream, x, lut,
                       reinterpret_cast<float4*>(y), groups, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// Query resize behind the upload (BaseFewShotISEG.get_query, base_fst.py:876-887: cv2.resize of the decoded image and
// of every ground-truth mask to the network size).  The arithmetic is the integer rule of fgn_amd/fewshot_ds.py
// (resize_taps / resize_image_u8 / resize_masks) - a restatement of cv2's bilinear design (half-pixel
// centres, clamped edges, 11-bit weights, round half up), not cv2's bytes - and both kernels agree with those host
// functions bit for bit: everything is int32, every dimension is at most RESIZE_MAX_DIM.
//   tap of destination sample j on an axis of n_src -> n_dst samples:
//     num = (2j+1) * n_src - n_dst, den = 2 * n_dst, i0 = floor(num / den), rem = num - i0 * den,
//     w1 = (rem * 4096 + den) / (2 * den), w1 = 0 where i0 < 0, i1 = min(i0 + 1, n_src - 1), i0 clamped, w0 = 2048 - w1
// num > -den, so the floor division is one unsigned division of num + den; w1 costs a second one (divisor 2 * den).
// ----------------------------------------------------------------------------------
constexpr int RESIZE_MAX_DIM = 16384;
constexpr int RESIZE_BLOCK = 256;
constexpr int RESIZE_WAVES = RESIZE_BLOCK / 64;
constexpr int RESIZE_GRID_CAP = 256 * 8;      // workgroups; waves loop over further units
constexpr int RESIZE_HALF = 1 << 21;          // half of the weight sum 2048 * 2048

struct ResizeTap { int i0, i1, w0, w1; };
__device__ __forceinline__ ResizeTap resize_tap(int j, int n_src, int n_dst) {
    const unsigned den = 2u * (unsigned)n_dst;
    const unsigned nump = (2u * (unsigned)j + 1u) * (unsigned)n_src + (unsigned)n_dst;     // num + den, in [1, 2^30)
    const unsigned q = nump / den;                                                         // i0 + 1
    const unsigned rem = nump - q * den;
    ResizeTap t;
    t.w1 = q == 0u ? 0 : (int)((rem * 4096u + den) / (2u * den));
    t.w0 = 2048 - t.w1;
    t.i1 = min((int)q, n_src - 1);
    t.i0 = min(max((int)q - 1, 0), n_src - 1);
    return t;
}

// ----------------------------------------------------------------------------------
// Query augmentation behind the upload (BaseFewShotISEG.augment_with_imgaug, base_fst.py:735-770, on the geometric half
// of natural_fst.py:18-35 and its ChannelShuffle), composed with the resize above into ONE bilinear gather from the
// source image.  The arithmetic is the integer rule of fgn_amd/fewshot_ds.py (query_augment_record / augment_image_u8 /
// augment_masks) and both kernels agree with those host functions bit for bit.
//   record of an image, 16 int32: h w kind flip border perm c00 c01 c10 c11 c02(lo,hi) c12(lo,hi) - -
//   kind 0: the taps of resize_tap, of column W-1-ox under flip.
//   kind 1: U = c00*ox + c01*oy + c02, V = c10*ox + c11*oy + c12 in int64, units of 2^-20 source samples;
//           i0 = U >> 20, f = U & (2^20-1), w1 = (f + 256) >> 9, w0 = 2048 - w1; taps i0, i0+1 (and j0, j0+1);
//           a tap outside the image reads its symmetric extension (border 1: r = k mod 2n, r < n ? r : 2n-1-r) or 0.
//   |c00|,|c01|,|c10|,|c11| <= 2^26 and |c02|,|c12| <= 2^40, so |U| < 2^42 and i0 fits int32.
// As fewshot_ds._augment_acc calls _resize_acc for kind 0, the resize kernels are the gathers below without a record:
// kind 0, no flip, channel order 0, all of it known to the compiler.
// ----------------------------------------------------------------------------------
constexpr int AUG_REC_INTS = 16;
constexpr int AUG_FRAC_BITS = 20;
constexpr int AUG_LIN_MAX = 1 << 26;
constexpr long long AUG_OFF_MAX = 1ll << 40;

struct AugRec {
    int h, w, kind, flip, border, perm, c00, c01, c10, c11;
    long long c02, c12;
    bool ok;                                  // every field inside its set: the only records a kernel reads pixels for
};
// REC: rc is a record; without it rc is {h, w} alone, read as the neutral record of that size (the plain resize).
template <bool REC>
__device__ __forceinline__ AugRec aug_record(const int* __restrict__ rc) {
    AugRec r = {};
    r.h = rc[0]; r.w = rc[1];
    if constexpr (REC) {
        r.kind = rc[2]; r.flip = rc[3]; r.border = rc[4]; r.perm = rc[5];
        r.c00 = rc[6]; r.c01 = rc[7]; r.c10 = rc[8]; r.c11 = rc[9];
        r.c02 = (long long)(((unsigned long long)(unsigned)rc[11] << 32) | (unsigned)rc[10]);
        r.c12 = (long long)(((unsigned long long)(unsigned)rc[13] << 32) | (unsigned)rc[12]);
    }
    const auto lin = [](int v) { return v >= -AUG_LIN_MAX && v <= AUG_LIN_MAX; };
    const auto off = [](long long v) { return v >= -AUG_OFF_MAX && v <= AUG_OFF_MAX; };
    r.ok = r.h >= 1 && r.h <= RESIZE_MAX_DIM && r.w >= 1 && r.w <= RESIZE_MAX_DIM && (r.kind == 0 || r.kind == 1) &&
           (r.flip == 0 || r.flip == 1) && (r.border == 0 || r.border == 1) && r.perm >= 0 && r.perm <= 5 &&
           lin(r.c00) && lin(r.c01) && lin(r.c10) && lin(r.c11) && off(r.c02) && off(r.c12);
    return r;
}

// Taps of one axis of n samples at coordinate U (kind 1): indices into the axis, or -1 for "reads 0".
__device__ __forceinline__ ResizeTap aug_tap(long long U, int n, bool symmetric) {
    const int k = (int)(U >> AUG_FRAC_BITS);
    const int f = (int)(U & ((1ll << AUG_FRAC_BITS) - 1));
    ResizeTap t;
    t.w1 = (f + 256) >> 9;
    t.w0 = 2048 - t.w1;
    if ((unsigned)k < (unsigned)(n - 1)) {                  // both taps inside (the common case)
        t.i0 = k;
        t.i1 = k + 1;
    } else if (symmetric) {
        const int p = 2 * n;
        int r = k % p;
        r = r < 0 ? r + p : r;
        const int r1 = r + 1 == p ? 0 : r + 1;
        t.i0 = r < n ? r : p - 1 - r;
        t.i1 = r1 < n ? r1 : p - 1 - r1;
    } else {
        t.i0 = (unsigned)k < (unsigned)n ? k : -1;
        t.i1 = (unsigned)(k + 1) < (unsigned)n ? k + 1 : -1;
    }
    return t;
}

__device__ __forceinline__ int aug_pick(const int v[3], int p) { return p == 0 ? v[0] : (p == 1 ? v[1] : v[2]); }

// The four taps (ty.i0 | ty.i1) x (tx.i0 | tx.i1) of an image of rows of w pixels of NCH bytes, blended with wy * wx
// (which sum to 2^22): acc[k] += byte k of the tap * weight - or, with BITS, the weight where the byte is nonzero (masks).
// GUARD: a tap index may be -1, "reads 0" (kind 1); without it every index is inside the image (kind 0).  The offsets are
// 32-bit on a wave-uniform base: (i * w + j) * NCH < 3 * 16384^2.
template <int NCH, bool BITS, bool GUARD>
__device__ __forceinline__ void blend4(const uint8_t* __restrict__ img, int w, const ResizeTap& ty, const ResizeTap& tx,
                                       int acc[NCH]) {
    const int iy[2] = {ty.i0, ty.i1}, wy[2] = {ty.w0, ty.w1};
    const int ix[2] = {tx.i0, tx.i1}, wx[2] = {tx.w0, tx.w1};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        if (GUARD && iy[a] < 0) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (GUARD && ix[c] < 0) continue;
            const uint8_t* p = img + (unsigned)((iy[a] * w + ix[c]) * NCH);
            const int wgt = wy[a] * wx[c];
#pragma unroll
            for (int k = 0; k < NCH; ++k) acc[k] += BITS ? (p[k] ? wgt : 0) : (int)p[k] * wgt;
        }
    }
}

// The unit of work of the row kernels (these gathers and support_from_source_kernel): one wave on 64 consecutive lane
// items of ONE output row.  Item (image, mask or instance), row, the row's y taps or row terms and a record are
// wave-uniform (scalar registers, one scalar division pair per unit for resize_tap), the x taps are per lane; for kind 1
// a lane adds one 32x32->64 multiply per axis to the row terms c01*oy + c02, c11*oy + c12.
struct WaveUnits { int lane, first, step; };              // the units first, first + step, ... of this lane's wave
__device__ __forceinline__ WaveUnits wave_units() {
    WaveUnits q;
    q.lane = threadIdx.x & 63;
    q.first = blockIdx.x * RESIZE_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    q.step = gridDim.x * RESIZE_WAVES;
    return q;
}
struct RowUnit { int r, item, row, chunk; };              // r = item * rows + row
__device__ __forceinline__ RowUnit row_unit(int u, int chunks, int rows) {
    RowUnit q;
    q.r = u / chunks;
    q.chunk = u - q.r * chunks;
    q.item = q.r / rows;
    q.row = q.r - q.item * rows;
    return q;
}

// The normalisation table into LDS (3 KB), as in u8hwc3_to_nhwc4_kernel.
__device__ __forceinline__ void lut_to_lds(float* __restrict__ t, const float* __restrict__ lut) {
    for (int i = threadIdx.x; i < 3 * 256; i += RESIZE_BLOCK) t[i] = lut[i];
    __syncthreads();
}

// Launch geometry of the row kernels: `rows` output rows of `items` lane items, `chunk` of them to a wave's unit, at most
// `grid_cap` workgroups.  Unit indices are int32, the stride of wave_units (grid_cap workgroups of RESIZE_WAVES)
// included: more units than that is FGN_ERR_SHAPE.
struct RowGrid { int chunks, units, grid; };
static int row_grid(long long rows, int items, int chunk, int grid_cap, RowGrid* g) {
    g->chunks = cdiv(items, chunk);
    const long long units = rows * g->chunks;
    if (units > INT32_MAX - RESIZE_WAVES * grid_cap) return FGN_ERR_SHAPE;
    g->units = (int)units;
    g->grid = (int)std::min<long long>((units + RESIZE_WAVES - 1) / RESIZE_WAVES, grid_cap);
    return FGN_OK;
}

// Source images [h_b, w_b, 3] uint8 at src + b * stride (any byte alignment), described by the DEVICE array desc - the
// records recs[b] (REC), or src_hw[b] = {h_b, w_b} - so that no launch argument depends on a source size or on the
// augmentation: one captured launch serves them all.  -> y [n,H,W,4] fp32 = u8hwc3_to_nhwc4_kernel of augment_image_u8's
// image (resize_image_u8's without a record): channel c of the output is table c of byte order[c] of the blended pixel,
// {lut[0][r], lut[1][g], lut[2][b], +0} for order 0.  A lane makes one output pixel: 4 taps x 3 bytes - for kind 0 from
// two source rows (neighbouring lanes share cache lines; the source is a few MB and stays in L2), for kind 1 along a
// slanted line through the source (at 10 degrees a wave's 64 pixels span about 11 source rows, the gathers are served by
// L2) - three table lookups in LDS, one 16-byte store: 1 KB per wave, coalesced; like u8hwc3_to_nhwc4_kernel it waits on
// those stores.  Every index of kind 0 is clamped into [0,h) x [0,w).  A record out of range, a size outside
// 1..RESIZE_MAX_DIM or an image that does not fit its slot is written as zeros and none of its bytes are read.
// Without a record, kind, flip, channel order and "every tap is inside" are compile-time: no int64 coordinates, no tap
// guards, no selects.
template <bool REC>
__device__ __forceinline__ void image_gather(const uint8_t* __restrict__ src, long long stride,
                                             const int* __restrict__ desc, const float* __restrict__ lut,
                                             float4* __restrict__ y, int H, int W, int chunks, int units) {
    __shared__ float t[3 * 256];
    lut_to_lds(t, lut);
    const WaveUnits wu = wave_units();
    for (int u = wu.first; u < units; u += wu.step) {
        const RowUnit q = row_unit(u, chunks, H);           // item: the image
        const AugRec g = aug_record<REC>(desc + (size_t)q.item * (REC ? AUG_REC_INTS : 2));
        const int ox = q.chunk * 64 + wu.lane, oy = q.row;
        if (ox >= W) continue;
        float4* o = y + (size_t)q.r * W + ox;
        if (!g.ok || (long long)g.h * g.w * 3 > stride) {
            *o = make_float4(0.f, 0.f, 0.f, 0.f);
            continue;
        }
        ResizeTap ty, tx;
        if (!REC || g.kind == 0) {
            ty = resize_tap(oy, g.h, H);
            tx = resize_tap(REC && g.flip ? W - 1 - ox : ox, g.w, W);
        } else {
            const long long ru = (long long)g.c01 * oy + g.c02, rv = (long long)g.c11 * oy + g.c12;     // wave-uniform
            tx = aug_tap(ru + (long long)g.c00 * ox, g.w, g.border == 1);
            ty = aug_tap(rv + (long long)g.c10 * ox, g.h, g.border == 1);
        }
        int acc[3] = {0, 0, 0};
        blend4<3, false, REC>(src + (long long)q.item * stride, g.w, ty, tx, acc);
        int v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (acc[k] + RESIZE_HALF) >> 22;
        if constexpr (REC) {
            // itertools.permutations(range(3))[perm] = (p0, p1, p2), two bits each
            const int p0 = (0xA50 >> (2 * g.perm)) & 3, p1 = (0x489 >> (2 * g.perm)) & 3, p2 = (0x126 >> (2 * g.perm)) & 3;
            *o = make_float4(t[aug_pick(v, p0)], t[256 + aug_pick(v, p1)], t[512 + aug_pick(v, p2)], 0.f);
        } else {
            *o = make_float4(t[v[0]], t[256 + v[1]], t[512 + v[2]], 0.f);
        }
    }
}

__global__ __launch_bounds__(RESIZE_BLOCK) void resize_u8hwc3_to_nhwc4_kernel(const uint8_t* __restrict__ src,
                                                                              long long stride,
                                                                              const int* __restrict__ src_hw,
                                                                              const float* __restrict__ lut,
                                                                              float4* __restrict__ y, int H, int W,
                                                                              int chunks, int units) {
    image_gather<false>(src, stride, src_hw, lut, y, H, W, chunks, units);
}

__global__ __launch_bounds__(RESIZE_BLOCK) void augment_u8hwc3_to_nhwc4_kernel(const uint8_t* __restrict__ src,
                                                                               long long stride,
                                                                               const int* __restrict__ recs,
                                                                               const float* __restrict__ lut,
                                                                               float4* __restrict__ y, int H, int W,
                                                                               int chunks, int units) {
    image_gather<true>(src, stride, recs, lut, y, H, W, chunks, units);
}

template <class Kernel>
static int image_gather_launch(Kernel kernel, const unsigned char* src, long long src_stride_bytes, const int* desc,
                               const float* lut, float* y, int n_img, int H, int W, hipStream_t stream) {
    if (!src || !desc || !lut || !y) return FGN_ERR_ARG;
    if (n_img < 0 || H < 0 || W < 0 || H > RESIZE_MAX_DIM || W > RESIZE_MAX_DIM || src_stride_bytes < 0)
        return FGN_ERR_SHAPE;
    if ((long long)n_img * H * W == 0) return FGN_OK;
    RowGrid g;
    if (row_grid((long long)n_img * H, W, 64, RESIZE_GRID_CAP, &g) != FGN_OK) return FGN_ERR_SHAPE;
    hipLaunchKernelGGL(kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, src, src_stride_bytes, desc, lut,
                       reinterpret_cast<float4*>(y), H, W, g.chunks, g.units);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_resize_u8hwc3_to_nhwc4_f32(const unsigned char* src, long long src_stride_bytes, const int* src_hw,
                                              const float* lut, float* y, int n_img, int H, int W,
                                              hipStream_t stream) {
    return image_gather_launch(resize_u8hwc3_to_nhwc4_kernel, src, src_stride_bytes, src_hw, lut, y, n_img, H, W, stream);
}

extern "C" int fgn_augment_u8hwc3_to_nhwc4_f32(const unsigned char* src, long long src_stride_bytes, const int* recs,
                                               const float* lut, float* y, int n_img, int H, int W,
                                               hipStream_t stream) {
    return image_gather_launch(augment_u8hwc3_to_nhwc4_kernel, src, src_stride_bytes, recs, lut, y, n_img, H, W, stream);
}

// Masks [G,h,w] (bool or bytes: nonzero = set) of ONE image -> [G,H,W] 0/1 bytes by the same taps on 0/1 values, set
// where acc >= 2^21 (half counts as set): cv2.resize(m.astype(uint8)).astype(bool) of base_fst.py:885, with a record rec
// (REC; device, 16 int32) by the taps of the record, where a tap outside the image is 0 whatever the record's border.  A
// lane makes the four pixels of one ALIGNED dword of the output row (the first group of a row starts up to 3 bytes before
// the row, so that dst + 4 * k is dword-aligned whatever W and the row are) and stores it whole; a group that the row's
// ends cut goes bytewise.  Dimensions are launch arguments: the ground-truth work of an episode is eager (G differs per
// image).  A record out of range, or one for another source size than (h, w), gives empty masks and nothing is read.
constexpr int MASK_LANE_BYTES = 4;
constexpr int MASK_GRID_CAP = 4 * RESIZE_GRID_CAP;        // (a mask unit writes 256 B, a quarter of an image unit's 1 KB)

// The pixels x_lo .. x_lo + 3 of a row as the bytes of a dword (those outside [0, W) stay 0); taps(ox, ty, tx) gives
// the taps of column ox, blend4's GUARD says whether they can be absent.
template <bool GUARD, class Taps>
__device__ __forceinline__ unsigned mask_word(const uint8_t* __restrict__ base, int w, int W, int x_lo, Taps taps) {
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < MASK_LANE_BYTES; ++k) {
        const int ox = x_lo + k;
        if (ox < 0 || ox >= W) continue;
        ResizeTap ty, tx;
        taps(ox, ty, tx);
        int acc = 0;
        blend4<1, true, GUARD>(base, w, ty, tx, &acc);
        word |= (acc >= RESIZE_HALF ? 1u : 0u) << (8 * k);
    }
    return word;
}

template <bool REC>
__device__ __forceinline__ void mask_gather(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                            const int* __restrict__ rec, int h, int w, int H, int W, int chunks,
                                            int units) {
    AugRec g = {};
    if constexpr (REC) g = aug_record<true>(rec);
    const bool ok = !REC || (g.ok && g.h == h && g.w == w);
    const WaveUnits wu = wave_units();
    for (int u = wu.first; u < units; u += wu.step) {
        const RowUnit q = row_unit(u, chunks, H);           // item: the mask
        const int oy = q.row;
        uint8_t* row = dst + (size_t)q.r * W;
        const int lead = (int)(reinterpret_cast<uintptr_t>(row) & 3u);      // bytes of the row's first dword before it
        const int x_lo = (q.chunk * 64 + wu.lane) * MASK_LANE_BYTES - lead;
        if (x_lo >= W) continue;
        unsigned word = 0;
        const uint8_t* base = src + (size_t)q.item * h * w;             // (wave-uniform; the taps' offsets are 32-bit)
        if (!REC || (ok && g.kind == 0)) {
            const ResizeTap ry = resize_tap(oy, h, H);
            word = mask_word<false>(base, w, W, x_lo, [&](int ox, ResizeTap& ty, ResizeTap& tx) {
                ty = ry;
                tx = resize_tap(REC && g.flip ? W - 1 - ox : ox, w, W);
            });
        } else if (ok) {
            const long long ru = (long long)g.c01 * oy + g.c02, rv = (long long)g.c11 * oy + g.c12;     // wave-uniform
            word = mask_word<true>(base, w, W, x_lo, [&](int ox, ResizeTap& ty, ResizeTap& tx) {
                tx = aug_tap(ru + (long long)g.c00 * ox, w, false);
                ty = aug_tap(rv + (long long)g.c10 * ox, h, false);
            });
        }
        if (x_lo >= 0 && x_lo + MASK_LANE_BYTES <= W) {
            *reinterpret_cast<unsigned*>(row + x_lo) = word;
        } else {
#pragma unroll
            for (int k = 0; k < MASK_LANE_BYTES; ++k)
                if (x_lo + k >= 0 && x_lo + k < W) row[x_lo + k] = (uint8_t)((word >> (8 * k)) & 1u);
        }
    }
}

__global__ __launch_bounds__(RESIZE_BLOCK) void resize_mask_u8_kernel(const uint8_t* __restrict__ src,
                                                                      uint8_t* __restrict__ dst, int h, int w, int H,
                                                                      int W, int chunks, int units) {
    mask_gather<false>(src, dst, nullptr, h, w, H, W, chunks, units);
}

__global__ __launch_bounds__(RESIZE_BLOCK) void augment_mask_u8_kernel(const uint8_t* __restrict__ src,
                                                                       uint8_t* __restrict__ dst,
                                                                       const int* __restrict__ rec, int h, int w,
                                                                       int H, int W, int chunks, int units) {
    mask_gather<true>(src, dst, rec, h, w, H, W, chunks, units);
}

template <class Launch>
static int mask_gather_launch(bool pointers, int G, int h, int w, int H, int W, Launch launch) {
    if (!pointers) return FGN_ERR_ARG;
    if (G < 0 || h < 0 || w < 0 || H < 0 || W < 0 || h > RESIZE_MAX_DIM || w > RESIZE_MAX_DIM || H > RESIZE_MAX_DIM ||
        W > RESIZE_MAX_DIM)
        return FGN_ERR_SHAPE;
    if ((long long)G * H * W == 0) return FGN_OK;
    if (h == 0 || w == 0) return FGN_ERR_SHAPE;               // (pixels to make and none to make them of)
    RowGrid g;
    if (row_grid((long long)G * H, W + MASK_LANE_BYTES - 1, 64 * MASK_LANE_BYTES, MASK_GRID_CAP, &g) != FGN_OK)
        return FGN_ERR_SHAPE;
    launch(g);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_resize_mask_u8(const unsigned char* src, unsigned char* dst, int G, int h, int w, int H, int W,
                                  hipStream_t stream) {
    return mask_gather_launch(src && dst, G, h, w, H, W, [&](const RowGrid& g) {
        hipLaunchKernelGGL(resize_mask_u8_kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, src, dst, h, w, H, W,
                           g.chunks, g.units);
    });
}

extern "C" int fgn_augment_mask_u8(const unsigned char* src, unsigned char* dst, const int* rec, int G, int h, int w,
                                   int H, int W, hipStream_t stream) {
    return mask_gather_launch(src && dst && rec, G, h, w, H, W, [&](const RowGrid& g) {
        hipLaunchKernelGGL(augment_mask_u8_kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, src, dst, rec, h, w, H,
                           W, g.chunks, g.units);
    });
}

// ----------------------------------------------------------------------------------
// Photometric query augmentation on the source bytes, ahead of the resize / augment gathers above (the other six
// operators of augs_seq, natural_fst.py:18-35: AdditiveGaussianNoise, ImpulseNoise, GaussianBlur, AddToHue,
// AddToSaturation, AddToBrightness).  One out-of-place pass src -> dst in the slot layout of the kernels it feeds.  The
// arithmetic is the integer rule of fgn_amd/fewshot_ds.py (query_photometric_record / photometric_image_u8; DESIGN.md
// 4.4.6) and the kernel agrees with photometric_image_u8 bit for bit: every table that depends on a float (blur weights,
// noise thresholds) is made on the host and travels in the record, the device evaluates no transcendental.
//   record of an image, 64 int32: h w op seed a0 a1 rx ry | payload from 8
//   op 0 copy.
//   op 1 noise:   u = word 0 of Philox4x32-10 at counter (pixel, 0, 0, op), key (seed, 0); thresholds L[0..11] at 8;
//                 k = #{L[j] <= u} - 12 + #{~u < L[j]}; the three bytes of the pixel become clip(byte + k, 0, 255).
//   op 2 impulse: byte c is replaced where word c < a1 * 2^32 + a0, by 255 where bit c of word 3 is set, else by 0.
//   op 3 blur:    radii rx, ry in 1..16, weights w[0..rx] at 8 and w[0..ry] at 25 (offset |k|; w[0] + 2 sum w[1..] =
//                 2048); byte = (sum of byte * wy * wx + 2^21) >> 22, reflect-101 border (r = k mod (2n-2), r < n ? r :
//                 2n-2-r; 0 for n = 1).
//   op 4 / 5 / 6 hue / saturation / brightness: photo_hsv below (a0: the amount in the operator's fixed point).
// The grid is (tiles, images) and depends on the slot stride alone; record and operator are workgroup-uniform, a
// workgroup branches once on the operator and then loops over its tiles of the image.
// ----------------------------------------------------------------------------------
constexpr int PHOTO_REC_INTS = 64;
constexpr int PHOTO_PAYLOAD = 8;
constexpr int PHOTO_NOISE_K = 12;
constexpr int PHOTO_R_MAX = 16;
constexpr int PHOTO_BLOCK = 256;
constexpr int PHOTO_RUN = 4;                          // pixels per lane of a point operator: 12 bytes, three dwords
constexpr int PHOTO_TILE = 32;                        // blur: a workgroup makes 32 x 32 output pixels at a time
constexpr int PHOTO_IN = PHOTO_TILE + 2 * PHOTO_R_MAX;        // its input tile with the largest halo: 64 x 64 pixels
constexpr int PHOTO_GRID_CAP = 2048;                  // workgroups per image; further tiles take further passes
constexpr int PHOTO_ONE = 1 << 16;                    // hue and ramp in units of 2^-16; value and chroma in 2^-7 levels
constexpr int PHOTO_SIX = 6 << 16;

__device__ __forceinline__ bool photo_axis_ok(const int* __restrict__ wt, int r) {
    if (r < 1 || r > PHOTO_R_MAX) return false;
    int sum = 0;
    bool ok = true;
    for (int k = 0; k <= r; ++k) {
        const int v = wt[k];
        ok = ok && v >= 0 && v <= 2048;
        sum += (k ? 2 : 1) * (ok ? v : 0);
    }
    return ok && sum == 2048;
}

// Every field inside its set and the image inside its slot: the only records a workgroup reads pixels for.
__device__ __forceinline__ bool photo_record_ok(const int* __restrict__ rc, long long stride) {
    const int h = rc[0], w = rc[1], op = rc[2], a0 = rc[4], a1 = rc[5];
    if (h < 1 || h > RESIZE_MAX_DIM || w < 1 || w > RESIZE_MAX_DIM || op < 0 || op > 6) return false;
    if ((long long)h * w * 3 > stride) return false;
    switch (op) {
        case 2: return a1 == 0 || (a1 == 1 && a0 == 0);
        case 3: return photo_axis_ok(rc + PHOTO_PAYLOAD, rc[6]) && photo_axis_ok(rc + PHOTO_PAYLOAD + PHOTO_R_MAX + 1, rc[7]);
        case 4: return a0 >= 0 && a0 < PHOTO_SIX;
        case 5: return a0 >= -(1 << 23) && a0 <= (1 << 23);
        case 6: return a0 >= -(255 << 7) && a0 <= (255 << 7);
        default: return true;
    }
}

__device__ __forceinline__ void photo_philox(unsigned c0, unsigned c3, unsigned k0, unsigned out[4]) {
    unsigned c1 = 0u, c2 = 0u, k1 = 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Hue (OP 4), saturation (5), brightness (6) of one pixel.  V = max, d = V - min; the hue H in units of 2^-16 sextants
// from one rounded unsigned division by d; value V7 and chroma C7 in units of 2^-7 grey levels; channel n of (5, 3, 1)
// for (R, G, B) = (V7 * 2^16 - C7 * f + 2^22) >> 23, f = clip(min(k, 4 - k), 0, 1) of k = (n + H) mod 6.  All int32:
// V7 * 2^16 + 2^22 <= 255 * 2^23 + 2^22 < 2^31, V * |a0| <= 255 * 2^23.
template <int OP>
__device__ __forceinline__ void photo_hsv(int a0, int px[3]) {
    const int r = px[0], g = px[1], b = px[2];
    const int V = max(max(r, g), b), d = V - min(min(r, g), b);
    const bool is_r = V == r, is_g = !is_r && V == g;
    const int num = is_r ? g - b : (is_g ? b - r : r - g);
    const int q = d ? (int)((2u * (unsigned)abs(num) * (unsigned)PHOTO_ONE + (unsigned)d) / (2u * (unsigned)d)) : 0;
    int H = (is_r ? 0 : (is_g ? 2 : 4)) * PHOTO_ONE + (num >= 0 ? q : -q);
    H = d == 0 ? 0 : (H < 0 ? H + PHOTO_SIX : H);
    int V7 = V << 7, C7 = d << 7;
    if constexpr (OP == 4) {
        H += a0;
        H = H >= PHOTO_SIX ? H - PHOTO_SIX : H;
    } else if constexpr (OP == 5) {
        const int t = (int)(((unsigned)V * (unsigned)abs(a0) + (1u << 15)) >> 16);
        C7 = min(max(C7 + (a0 >= 0 ? t : -t), 0), V7);
    } else {
        V7 = min(max(V7 + a0, 0), 255 << 7);
        C7 = V ? (int)((2u * (unsigned)V7 * (unsigned)d + (unsigned)V) / (2u * (unsigned)V)) : 0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int k = (5 - 2 * c) * PHOTO_ONE + H;
        k = k >= PHOTO_SIX ? k - PHOTO_SIX : k;
        const int f = min(max(min(k, 4 * PHOTO_ONE - k), 0), PHOTO_ONE);
        px[c] = (V7 * PHOTO_ONE - C7 * f + (1 << 22)) >> 23;
    }
}

template <int OP>
__device__ __forceinline__ void photo_pixel(const int* __restrict__ rc, int p, int px[3]) {
    if constexpr (OP == 1) {
        unsigned wd[4];
        photo_philox((unsigned)p, 1u, (unsigned)rc[3], wd);
        const unsigned u = wd[0];
        int k = -PHOTO_NOISE_K;
#pragma unroll
        for (int j = 0; j < PHOTO_NOISE_K; ++j) {
            const unsigned L = (unsigned)rc[PHOTO_PAYLOAD + j];
            k += (L <= u ? 1 : 0) + (~u < L ? 1 : 0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = min(max(px[c] + k, 0), 255);
    } else if constexpr (OP == 2) {
        unsigned wd[4];
        photo_philox((unsigned)p, 2u, (unsigned)rc[3], wd);
        const unsigned lo = (unsigned)rc[4];
        const bool all = rc[5] != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (all || wd[c] < lo) px[c] = ((wd[3] >> c) & 1u) ? 255 : 0;
    } else if constexpr (OP >= 4) {
        photo_hsv<OP>(rc[4], px);
    }
}

// A point operator on tiles of PHOTO_BLOCK * PHOTO_RUN pixels of the flat pixel array: a lane takes PHOTO_RUN
// consecutive pixels, as three dwords each way where both slots are dword-aligned and the run is whole, bytewise
// otherwise (odd slots, the image's last pixels).  ``f(p, px)`` rewrites the three values of pixel p in registers.
template <class F>
__device__ __forceinline__ void photo_point(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int npix, F f) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0;
    const int tiles = (npix + PHOTO_BLOCK * PHOTO_RUN - 1) / (PHOTO_BLOCK * PHOTO_RUN);
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int p0 = (t * PHOTO_BLOCK + (int)threadIdx.x) * PHOTO_RUN;
        if (p0 >= npix) continue;
        const int n = min(PHOTO_RUN, npix - p0);
        const bool wide = aligned && n == PHOTO_RUN;
        int v[3 * PHOTO_RUN];
        if (wide) {
            const uint3 d = *reinterpret_cast<const uint3*>(in + 3 * (size_t)p0);
            const unsigned wd[3] = {d.x, d.y, d.z};
#pragma unroll
            for (int i = 0; i < 3 * PHOTO_RUN; ++i) v[i] = (int)((wd[i >> 2] >> (8 * (i & 3))) & 255u);
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PHOTO_RUN; ++i) v[i] = i < 3 * n ? (int)in[3 * (size_t)p0 + i] : 0;
        }
#pragma unroll
        for (int j = 0; j < PHOTO_RUN; ++j)
            if (j < n) f(p0 + j, v + 3 * j);
        if (wide) {
            unsigned wd[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 3 * PHOTO_RUN; ++i) wd[i >> 2] |= (unsigned)v[i] << (8 * (i & 3));
            *reinterpret_cast<uint3*>(out + 3 * (size_t)p0) = make_uint3(wd[0], wd[1], wd[2]);
        } else {
#pragma unroll
            for (int i = 0; i < 3 * PHOTO_RUN; ++i)
                if (i < 3 * n) out[3 * (size_t)p0 + i] = (uint8_t)v[i];
        }
    }
}

__device__ __forceinline__ int photo_reflect101(int k, int n) {
    if ((unsigned)k < (unsigned)n) return k;
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    int r = k % p;
    r = r < 0 ? r + p : r;
    return r < n ? r : p - r;
}

// The whole slot of a refused image as zeros, by all workgroups of the image.
__device__ __forceinline__ void photo_zero_slot(uint8_t* __restrict__ out, long long stride) {
    for (long long o = ((long long)blockIdx.x * PHOTO_BLOCK + (int)threadIdx.x) * 16; o < stride;
         o += (long long)gridDim.x * PHOTO_BLOCK * 16)
        for (int k = 0; k < 16; ++k)
            if (o + k < stride) out[o + k] = 0;
}

// The blur of record rc over the image, a 32 x 32 tile per workgroup at a time: the tile's input with a halo of the
// record's radii goes to LDS as bytes (reflected indices, so every read is inside the image), a horizontal pass leaves
// int32 sums (<= 255 * 2^11) of its 32 + 2 ry rows in LDS, a vertical pass makes the bytes.  No rounding between the
// passes: the separable form is the 2D rule bit for bit.  36 KB of LDS.  ``f(p, px)`` rewrites a staged pixel in
// registers on its way to LDS, p = sy * w + sx being the SOURCE pixel's own flat index, halo and reflected pixels
// included: the tile then holds what an intermediate image after f would have held.  UNROLL: staged pixels in flight.
template <int UNROLL, class F>
__device__ __forceinline__ void photo_blur(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                           const int* __restrict__ rc, int h, int w, F f) {
    __shared__ uint8_t tin[PHOTO_IN][PHOTO_IN * 3];
    __shared__ int hsum[PHOTO_IN][PHOTO_TILE * 3];
    __shared__ int wgt[2][PHOTO_R_MAX + 1];
    const int tid = threadIdx.x;
    const int rx = rc[6], ry = rc[7];
    if (tid <= rx) wgt[0][tid] = rc[PHOTO_PAYLOAD + tid];
    if (tid <= ry) wgt[1][tid] = rc[PHOTO_PAYLOAD + PHOTO_R_MAX + 1 + tid];
    const int tiles_x = (w + PHOTO_TILE - 1) / PHOTO_TILE, tiles = tiles_x * ((h + PHOTO_TILE - 1) / PHOTO_TILE);
    const int iw = PHOTO_TILE + 2 * rx, ih = PHOTO_TILE + 2 * ry;
    constexpr int ROW = PHOTO_TILE * 3;                     // ints of a row of hsum, bytes of a tile's row of pixels
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty = t / tiles_x;
        const int y0 = ty * PHOTO_TILE, x0 = (t - ty * tiles_x) * PHOTO_TILE;
        __syncthreads();                                    // (the weights; the last tile's reads of tin and hsum)
#pragma unroll UNROLL
        for (int i = tid; i < ih * iw; i += PHOTO_BLOCK) {             // (unrolled: several pixels' loads in flight)
            const int ly = i / iw, lx = i - ly * iw;
            const int sy = photo_reflect101(y0 - ry + ly, h), sx = photo_reflect101(x0 - rx + lx, w);
            const int q = sy * w + sx;
            const uint8_t* p = in + (unsigned)(q * 3);                          // (< 3 * 16384^2: a 32-bit offset)
            int px[3] = {(int)p[0], (int)p[1], (int)p[2]};
            f(q, px);
            tin[ly][3 * lx] = (uint8_t)px[0];
            tin[ly][3 * lx + 1] = (uint8_t)px[1];
            tin[ly][3 * lx + 2] = (uint8_t)px[2];
        }
        __syncthreads();
        for (int i = tid; i < ih * ROW; i += PHOTO_BLOCK) {
            const int ly = i / ROW, x3 = i - ly * ROW;      // x3 = 3 * column + channel
            const uint8_t* c = &tin[ly][x3 + 3 * rx];
            int acc = (int)c[0] * wgt[0][0];
            for (int k = 1; k <= rx; ++k) acc += ((int)c[-3 * k] + (int)c[3 * k]) * wgt[0][k];
            hsum[ly][x3] = acc;
        }
        __syncthreads();
        for (int i = tid; i < PHOTO_TILE * ROW; i += PHOTO_BLOCK) {
            const int oy = i / ROW, x3 = i - oy * ROW;
            const int y = y0 + oy, x = x0 + x3 / 3;
            if (y >= h || x >= w) continue;
            int acc = hsum[oy + ry][x3] * wgt[1][0];
            for (int k = 1; k <= ry; ++k) acc += (hsum[oy + ry - k][x3] + hsum[oy + ry + k][x3]) * wgt[1][k];
            out[(unsigned)((y * w + x0) * 3 + x3)] = (uint8_t)((acc + RESIZE_HALF) >> 22);
        }
    }
}

// src [n_img][stride] bytes, image b as [h_b, w_b, 3] at the start of its slot (any byte alignment), records from the
// DEVICE array recs[b] (no launch argument depends on a source size or on an operator) -> dst in the same layout: bytes
// [0, 3 h w) of the slot are written, the rest of it is left alone.  A record out of range, or an image that does not fit
// its slot, gets its WHOLE slot written as zeros and none of its source bytes are read.
// The blur is photo_blur above, with nothing done to a staged pixel.
__global__ __launch_bounds__(PHOTO_BLOCK) void photometric_u8hwc3_kernel(const uint8_t* __restrict__ src,
                                                                         uint8_t* __restrict__ dst, long long stride,
                                                                         const int* __restrict__ recs) {
    const int b = blockIdx.y;
    const int* rc = recs + (size_t)b * PHOTO_REC_INTS;
    const uint8_t* in = src + (long long)b * stride;
    uint8_t* out = dst + (long long)b * stride;
    if (!photo_record_ok(rc, stride)) {
        photo_zero_slot(out, stride);
        return;
    }
    const int h = rc[0], w = rc[1], op = rc[2];
    switch (op) {
        case 0: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<0>(rc, p, px); }); return;
        case 1: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<1>(rc, p, px); }); return;
        case 2: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<2>(rc, p, px); }); return;
        case 4: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<4>(rc, p, px); }); return;
        case 5: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<5>(rc, p, px); }); return;
        case 6: photo_point(in, out, h * w, [=](int p, int* px) { photo_pixel<6>(rc, p, px); }); return;
        default: break;
    }
    photo_blur<4>(in, out, rc, h, w, [](int, int*) {});
}

extern "C" int fgn_photometric_u8hwc3(const unsigned char* src, unsigned char* dst, long long stride_bytes,
                                      const int* recs, int n_img, hipStream_t stream) {
    if (!src || !dst || !recs) return FGN_ERR_ARG;
    if (n_img < 0 || n_img > 65535 || stride_bytes < 0 || stride_bytes > (1ll << 40)) return FGN_ERR_SHAPE;
    if (n_img == 0 || stride_bytes == 0) return FGN_OK;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t span = (uintptr_t)n_img * (uintptr_t)stride_bytes;
    if (a < d + span && d < a + span) return FGN_ERR_ARG;     // (the blur reads neighbours: never in place)
    const long long tile_bytes = 3ll * PHOTO_BLOCK * PHOTO_RUN;
    const int grid = (int)std::min<long long>((stride_bytes + tile_bytes - 1) / tile_bytes, PHOTO_GRID_CAP);
    hipLaunchKernelGGL(photometric_u8hwc3_kernel, dim3(grid, n_img), dim3(PHOTO_BLOCK), 0, stream, src, dst,
                       stride_bytes, recs);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// A chain of photometric operators in one pass (COCODS.augs_seq, coco_ds.py:45-59: one of AddToHue / AddToSaturation /
// AddToBrightness, then GaussianBlur): image b has n_ops records at recs[b][0..n_ops), applied in order, of the form
// "point operators, then at most one blur".  The rule is the left fold of photometric_image_u8 over the records
// (fgn_amd/fewshot_ds.py photometric_chain_u8) and the kernel agrees with it bit for bit.  Every
// operator but the blur is a function of (pixel index, the pixel's three bytes, record), so the point stages run on a
// pixel in registers one after the other - in the run of four pixels of photo_point where the chain has no blur, in the
// staging loop of photo_blur where it ends in one: one read and one write of the image either way.
// ----------------------------------------------------------------------------------
constexpr int PHOTO_CHAIN_MAX = 3;

// Every record inside its sets (photo_record_ok), one (h, w) for the image, and only operator-0 records behind a blur.
__device__ __forceinline__ bool photo_chain_ok(const int* __restrict__ rcs, int n_ops, long long stride) {
    bool ok = true, blurred = false;
    for (int s = 0; s < n_ops; ++s) {
        const int* rc = rcs + s * PHOTO_REC_INTS;
        ok = ok && photo_record_ok(rc, stride) && rc[0] == rcs[0] && rc[1] == rcs[1] && !(blurred && rc[2] != 0);
        blurred = blurred || rc[2] == 3;
    }
    return ok;
}

// One stage of a chain on a pixel in registers; the operator is workgroup-uniform.  Operator 0 and the blur (which the
// caller runs behind the point stages) leave the pixel as it is, and rc is then not read.
__device__ __forceinline__ void photo_stage(const int* __restrict__ rc, int op, int p, int px[3]) {
    switch (op) {
        case 1: photo_pixel<1>(rc, p, px); break;
        case 2: photo_pixel<2>(rc, p, px); break;
        case 4: photo_pixel<4>(rc, p, px); break;
        case 5: photo_pixel<5>(rc, p, px); break;
        case 6: photo_pixel<6>(rc, p, px); break;
        default: break;
    }
}

// Slots and zeroing as photometric_u8hwc3_kernel; recs [n_img][n_ops][64].  An image whose chain fails photo_chain_ok
// gets its WHOLE slot written as zeros and none of its source bytes are read.
__global__ __launch_bounds__(PHOTO_BLOCK) void photometric_chain_u8hwc3_kernel(const uint8_t* __restrict__ src,
                                                                               uint8_t* __restrict__ dst,
                                                                               long long stride,
                                                                               const int* __restrict__ recs, int n_ops) {
    const int b = blockIdx.y;
    const int* rcs = recs + (size_t)b * n_ops * PHOTO_REC_INTS;
    const uint8_t* in = src + (long long)b * stride;
    uint8_t* out = dst + (long long)b * stride;
    if (!photo_chain_ok(rcs, n_ops, stride)) {
        photo_zero_slot(out, stride);
        return;
    }
    const int h = rcs[0], w = rcs[1];
    const int* rc1 = rcs + PHOTO_REC_INTS;
    const int* rc2 = rcs + 2 * PHOTO_REC_INTS;
    const int op0 = rcs[2], op1 = n_ops > 1 ? rc1[2] : 0, op2 = n_ops > 2 ? rc2[2] : 0;
    auto stages = [=](int p, int* px) {
        photo_stage(rcs, op0, p, px);
        photo_stage(rc1, op1, p, px);
        photo_stage(rc2, op2, p, px);
    };
    const int* blur = op0 == 3 ? rcs : (op1 == 3 ? rc1 : (op2 == 3 ? rc2 : nullptr));
    if (!blur) {
        photo_point(in, out, h * w, stages);
        return;
    }
    photo_blur<1>(in, out, blur, h, w, stages);     // (one staged pixel at a time: an unrolled copy of the stages spills SGPRs)
}

extern "C" int fgn_photometric_chain_u8hwc3(const unsigned char* src, unsigned char* dst, long long stride_bytes,
                                            const int* recs, int n_ops, int n_img, hipStream_t stream) {
    if (!src || !dst || !recs) return FGN_ERR_ARG;
    if (n_img < 0 || n_img > 65535 || stride_bytes < 0 || stride_bytes > (1ll << 40)) return FGN_ERR_SHAPE;
    if (n_ops < 1 || n_ops > PHOTO_CHAIN_MAX) return FGN_ERR_SHAPE;
    if (n_img == 0 || stride_bytes == 0) return FGN_OK;
    const uintptr_t a = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t span = (uintptr_t)n_img * (uintptr_t)stride_bytes;
    if (a < d + span && d < a + span) return FGN_ERR_ARG;     // (the blur reads neighbours: never in place)
    const long long tile_bytes = 3ll * PHOTO_BLOCK * PHOTO_RUN;
    const int grid = (int)std::min<long long>((stride_bytes + tile_bytes - 1) / tile_bytes, PHOTO_GRID_CAP);
    hipLaunchKernelGGL(photometric_chain_u8hwc3_kernel, dim3(grid, n_img), dim3(PHOTO_BLOCK), 0, stream, src, dst,
                       stride_bytes, recs, n_ops);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// Supports from the source image behind the upload (BaseFewShotISEG.get_support, base_fst.py:1043-1167: get_crop with
// reflected context, bicubic resize of the longer side to S, centre pad).  The arithmetic is the integer rule of
// fgn_amd/fewshot_ds.py (cubic_taps / support_geometry / support_from_source) and the kernel agrees
// with support_from_source bit for bit.
//   tap of destination sample j on an axis of n_src -> n_dst samples (cubic convolution, A = -3/4):
//     num = (2j+1) * n_src - n_dst, den = 2 * n_dst, i0 = floor(num / den), rem = num - i0 * den,
//     u = (rem * 2048 + den) / (2 * den) (0..1024), v = 1024 - u; in units of 2^-32, int64:
//     w(-1) = -3 u v^2, w(+1) = 5 v^3 - 9216 v^2 + 2^32, w(+2) = -3 u^2 v; W(k) = (w(k) + 2^20) >> 21,
//     W(0) = 2048 - the other three; samples i0 - 1 .. i0 + 2 clamped into the crop.
//   |W| sums to at most 2816 per axis, so |acc| <= 255 * 2816^2 < 2^31: the accumulators are int32, rows first
//   (|row sum| <= 255 * 2816), which is exact and therefore the same number as the host's double sum.
// The geometry of every instance - sizes, crop origin, placement, border mode, uploaded window - is a 16-int record the
// kernel READS (no launch argument depends on it: one captured launch serves every support set).  As for the query
// kernel a wave takes 64 consecutive pixels of one output row: instance, row, the record and the row's four y taps are
// wave-uniform, the x taps are per lane.
// ----------------------------------------------------------------------------------
constexpr int SPP_REC_INTS = 16;      // H W y0 x0 ch cw nh nw top left reflect wy wx wh ww -

struct CubicTap { int i0; int w[4]; };
__device__ __forceinline__ CubicTap cubic_tap(int j, int n_src, int n_dst) {
    const unsigned den = 2u * (unsigned)n_dst;
    const unsigned nump = (2u * (unsigned)j + 1u) * (unsigned)n_src + (unsigned)n_dst;     // num + den, in [1, 2^30)
    const unsigned q = nump / den;                                                         // i0 + 1
    const unsigned rem = nump - q * den;
    const long long u = (long long)((rem * 2048u + den) / (2u * den)), v = 1024 - u;
    const long long one = 1ll << 32, half = 1ll << 20;
    CubicTap t;
    t.i0 = (int)q - 1;
    t.w[0] = (int)((-3 * u * v * v + half) >> 21);
    t.w[2] = (int)((5 * v * v * v - 9216 * v * v + one + half) >> 21);
    t.w[3] = (int)((-3 * u * u * v + half) >> 21);
    t.w[1] = 2048 - t.w[0] - t.w[2] - t.w[3];
    return t;
}

// Position t of the crop's axis in the source frame -> index into the uploaded window [w_lo, w_lo + w_len) of an axis of
// n samples, or -1 for "reads 0".  reflect: np.pad(mode='reflect') of any width = the periodic reflection of period
// 2 (n - 1) (index 0 for n = 1); otherwise outside the image is 0.  The result is clamped into the window: the host
// sends a window that holds every tap, a record that lies cannot make the kernel read outside its slot.
__device__ __forceinline__ int spp_src_index(int t, int n, bool reflect, int w_lo, int w_len) {
    if ((unsigned)t >= (unsigned)n) {
        if (!reflect) return -1;
        if (n == 1) {
            t = 0;
        } else {
            const int p = 2 * (n - 1);
            int m = t % p;
            m = m < 0 ? m + p : m;
            t = m < n ? m : p - m;
        }
    }
    return min(max(t - w_lo, 0), w_len - 1);
}

// y [n,S,S,4] fp32 = u8hwc3_to_nhwc4_kernel of support_from_source's crop, m [n,S,S] = its mask as 0 / 1 bytes.  A lane
// makes one output pixel: 16 taps x 3 image bytes and 16 mask bytes from four rows of the window (neighbouring lanes
// share cache lines; the windows of an episode are a few hundred KB and stay in L2), three table lookups in LDS, one
// 16-byte store (1 KB per wave, coalesced) and one mask byte (64 B per wave).  A pixel of the padding reads nothing.
// An instance whose record is out of range (see ok below) is written as padding with an empty mask and not read.
// U8: the byte-output form - the clamped bytes themselves go to crop [n,S,S,3] uint8 (three byte stores per lane, 192
// contiguous bytes per wave), the padding and an instance with a bad record as byte 0; no table, no LDS.  It feeds the
// support augmentation below, which works on bytes.  Record, taps, window reads, validity rule and mask are one body;
// t is the f32 form's table in LDS (lut_to_lds), unused by the byte form.
template <bool U8>
__device__ __forceinline__ void support_gather(const uint8_t* __restrict__ src, long long stride,
                                               const uint8_t* __restrict__ msk, long long mstride,
                                               const int* __restrict__ recs, const float* __restrict__ t,
                                               float4* __restrict__ y, uint8_t* __restrict__ crop,
                                               uint8_t* __restrict__ m, int S, int chunks, int units) {
    float4 pad = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!U8) pad = make_float4(t[0], t[256], t[512], 0.f);               // byte 0 through the table
    const WaveUnits wu = wave_units();
    for (int u = wu.first; u < units; u += wu.step) {
        const RowUnit q = row_unit(u, chunks, S);           // item: the instance
        const int r = q.r, b = q.item, oy = q.row;
        const int ox = q.chunk * 64 + wu.lane;
        if (ox >= S) continue;
        const int* rc = recs + (size_t)b * SPP_REC_INTS;
        const int H = rc[0], W = rc[1], y0 = rc[2], x0 = rc[3], ch = rc[4], cw = rc[5], nh = rc[6], nw = rc[7];
        const int top = rc[8], left = rc[9], mode = rc[10], wy = rc[11], wx = rc[12], wh = rc[13], ww = rc[14];
        const auto dim = [](int v) { return v >= 1 && v <= RESIZE_MAX_DIM; };
        const bool ok = dim(H) && dim(W) && dim(ch) && dim(cw) && dim(nh) && dim(nw) && top >= 0 && left >= 0 &&
                        nh <= S - top && nw <= S - left && (mode == 0 || mode == 1) &&
                        y0 >= -2 * RESIZE_MAX_DIM && y0 < RESIZE_MAX_DIM && x0 >= -2 * RESIZE_MAX_DIM && x0 < RESIZE_MAX_DIM &&
                        wy >= 0 && wx >= 0 && wh >= 1 && ww >= 1 && wh <= H - wy && ww <= W - wx &&
                        (long long)wh * ww * 3 <= stride && (long long)wh * ww <= mstride;
        float4* o = U8 ? nullptr : y + (size_t)r * S + ox;
        uint8_t* ob = U8 ? crop + ((size_t)r * S + ox) * 3 : nullptr;
        uint8_t* om = m + (size_t)r * S + ox;
        const int jy = oy - top, jx = ox - left;
        if (!ok || jy < 0 || jy >= nh || jx < 0 || jx >= nw) {
            if constexpr (U8) {
                ob[0] = 0; ob[1] = 0; ob[2] = 0;
            } else {
                *o = pad;
            }
            *om = 0;
            continue;
        }
        const bool reflect = mode == 1;
        const CubicTap ty = cubic_tap(jy, ch, nh), tx = cubic_tap(jx, cw, nw);
        int cx[4], cm[4];                                   // window columns of the image taps / of the mask taps (-1: 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = x0 + min(max(tx.i0 - 1 + k, 0), cw - 1);
            cx[k] = spp_src_index(c, W, reflect, wx, ww);
            cm[k] = spp_src_index(c, W, false, wx, ww);
        }
        const uint8_t* img = src + (long long)b * stride;
        const uint8_t* mk = msk + (long long)b * mstride;
        int acc[3] = {0, 0, 0}, macc = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int row = y0 + min(max(ty.i0 - 1 + a, 0), ch - 1);
            const int ry = spp_src_index(row, H, reflect, wy, wh), rm = spp_src_index(row, H, false, wy, wh);
            if (ry >= 0) {
                const uint8_t* p = img + (size_t)ry * ww * 3;
                int s[3] = {0, 0, 0};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (cx[k] >= 0) {
                        s[0] += (int)p[cx[k] * 3] * tx.w[k];
                        s[1] += (int)p[cx[k] * 3 + 1] * tx.w[k];
                        s[2] += (int)p[cx[k] * 3 + 2] * tx.w[k];
                    }
                acc[0] += s[0] * ty.w[a];
                acc[1] += s[1] * ty.w[a];
                acc[2] += s[2] * ty.w[a];
            }
            if (rm >= 0) {
                const uint8_t* p = mk + (size_t)rm * ww;
                int s = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (cm[k] >= 0 && p[cm[k]]) s += tx.w[k];
                macc += s * ty.w[a];
            }
        }
        int v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = min(max((acc[k] + RESIZE_HALF) >> 22, 0), 255);
        if constexpr (U8) {
            ob[0] = (uint8_t)v[0]; ob[1] = (uint8_t)v[1]; ob[2] = (uint8_t)v[2];
        } else {
            *o = make_float4(t[v[0]], t[256 + v[1]], t[512 + v[2]], 0.f);
        }
        *om = macc > RESIZE_HALF ? 1 : 0;
    }
}

__global__ __launch_bounds__(RESIZE_BLOCK) void support_from_source_kernel(const uint8_t* __restrict__ src,
                                                                           long long stride,
                                                                           const uint8_t* __restrict__ msk,
                                                                           long long mstride,
                                                                           const int* __restrict__ recs,
                                                                           const float* __restrict__ lut,
                                                                           float4* __restrict__ y,
                                                                           uint8_t* __restrict__ m, int S, int chunks,
                                                                           int units) {
    __shared__ float t[3 * 256];
    lut_to_lds(t, lut);
    support_gather<false>(src, stride, msk, mstride, recs, t, y, nullptr, m, S, chunks, units);
}

__global__ __launch_bounds__(RESIZE_BLOCK) void support_from_source_u8_kernel(const uint8_t* __restrict__ src,
                                                                              long long stride,
                                                                              const uint8_t* __restrict__ msk,
                                                                              long long mstride,
                                                                              const int* __restrict__ recs,
                                                                              uint8_t* __restrict__ crop,
                                                                              uint8_t* __restrict__ m, int S, int chunks,
                                                                              int units) {
    support_gather<true>(src, stride, msk, mstride, recs, nullptr, nullptr, crop, m, S, chunks, units);
}

template <class Launch>
static int support_gather_launch(bool pointers, long long src_stride_bytes, long long msk_stride_bytes, int n, int S,
                                 Launch launch) {
    if (!pointers) return FGN_ERR_ARG;
    if (n < 0 || S < 0 || S > RESIZE_MAX_DIM || src_stride_bytes < 0 || msk_stride_bytes < 0) return FGN_ERR_SHAPE;
    if ((long long)n * S == 0) return FGN_OK;
    RowGrid g;
    if (row_grid((long long)n * S, S, 64, RESIZE_GRID_CAP, &g) != FGN_OK) return FGN_ERR_SHAPE;
    launch(g);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_support_from_source_f32(const unsigned char* src, long long src_stride_bytes,
                                           const unsigned char* msk, long long msk_stride_bytes, const int* recs,
                                           const float* lut, float* y, unsigned char* m, int n, int S,
                                           hipStream_t stream) {
    return support_gather_launch(src && msk && recs && lut && y && m, src_stride_bytes, msk_stride_bytes, n, S,
                                 [&](const RowGrid& g) {
        hipLaunchKernelGGL(support_from_source_kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, src, src_stride_bytes,
                           msk, msk_stride_bytes, recs, lut, reinterpret_cast<float4*>(y), m, S, g.chunks, g.units);
    });
}

extern "C" int fgn_support_from_source_u8(const unsigned char* src, long long src_stride_bytes, const unsigned char* msk,
                                          long long msk_stride_bytes, const int* recs, unsigned char* crop,
                                          unsigned char* m, int n, int S, hipStream_t stream) {
    return support_gather_launch(src && msk && recs && crop && m, src_stride_bytes, msk_stride_bytes, n, S,
                                 [&](const RowGrid& g) {
        hipLaunchKernelGGL(support_from_source_u8_kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, src,
                           src_stride_bytes, msk, msk_stride_bytes, recs, crop, m, S, g.chunks, g.units);
    });
}

// ----------------------------------------------------------------------------------
// Support augmentation behind the cut (BaseFewShotISEG.get_support with augment_spp, base_fst.py:1151-1153:
// augment_with_imgaug once per instance on the S x S crop, its mask and its box, AFTER resize and pad).  The rule is the
// query's at equal size (fgn_amd/fewshot_ds.py augment_support): the photometric pass above on the n
// crops as n slots of 3 S S bytes, then this gather, which agrees with augment_image_u8 / augment_masks at S -> S
// followed by the table bit for bit.
//   crop [n,S,S,3] uint8, msk [n,S,S] (nonzero = set), recs [n][16] the records of query_augment_record with h = w = S,
//   READ on the device (no launch argument depends on an augmentation: one launch serves all n instances)
//   -> y [n,S,S,4] fp32 through the table and m [n,S,S] 0 / 1 bytes.
// Unit of work as above: a wave on 64 consecutive pixels of one output row; instance, row, record and the row terms are
// wave-uniform.  Kind 0: the equal-size taps of resize_tap are the identity (w1 = 0), so a lane copies pixel and mask
// byte of column ox, or S-1-ox under flip - one tap, no blend.  Kind 1: the taps of aug_tap per axis are computed once;
// image and mask share indices and weights, except that a mask tap outside the frame reads 0 whatever the border.  The
// symmetric border reflects the S x S frame, its pad bands included.  Stores as support_from_source_kernel's: one
// 16-byte store and one mask byte per lane.  An instance whose record is out of range (the sets of aug_record) or is
// for another size than S x S is written as the table's byte-0 pixel with an empty mask, and none of its bytes are read.
// ----------------------------------------------------------------------------------
__global__ __launch_bounds__(RESIZE_BLOCK) void support_augment_kernel(const uint8_t* __restrict__ crop,
                                                                       const uint8_t* __restrict__ msk,
                                                                       const int* __restrict__ recs,
                                                                       const float* __restrict__ lut,
                                                                       float4* __restrict__ y, uint8_t* __restrict__ m,
                                                                       int S, int chunks, int units) {
    __shared__ float t[3 * 256];
    lut_to_lds(t, lut);
    const float4 pad = make_float4(t[0], t[256], t[512], 0.f);
    const WaveUnits wu = wave_units();
    for (int u = wu.first; u < units; u += wu.step) {
        const RowUnit q = row_unit(u, chunks, S);           // item: the instance
        const AugRec g = aug_record<true>(recs + (size_t)q.item * AUG_REC_INTS);
        const int ox = q.chunk * 64 + wu.lane, oy = q.row;
        if (ox >= S) continue;
        float4* o = y + (size_t)q.r * S + ox;
        uint8_t* om = m + (size_t)q.r * S + ox;
        if (!g.ok || g.h != S || g.w != S) {
            *o = pad;
            *om = 0;
            continue;
        }
        const uint8_t* img = crop + (size_t)q.item * S * S * 3;         // (wave-uniform; the taps' offsets are 32-bit)
        const uint8_t* mk = msk + (size_t)q.item * S * S;
        int v[3];
        bool set;
        if (g.kind == 0) {
            const unsigned at = (unsigned)(oy * S + (g.flip ? S - 1 - ox : ox));
            const uint8_t* p = img + at * 3u;
            v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
            set = mk[at] != 0;
        } else {
            const long long ru = (long long)g.c01 * oy + g.c02, rv = (long long)g.c11 * oy + g.c12;     // wave-uniform
            const long long U = ru + (long long)g.c00 * ox, V = rv + (long long)g.c10 * ox;
            const ResizeTap mx = aug_tap(U, S, false), my = aug_tap(V, S, false);          // the mask's: outside reads 0
            const ResizeTap tx = g.border == 1 ? aug_tap(U, S, true) : mx, ty = g.border == 1 ? aug_tap(V, S, true) : my;
            int acc[3] = {0, 0, 0}, macc = 0;
            blend4<3, false, true>(img, S, ty, tx, acc);
            blend4<1, true, true>(mk, S, my, mx, &macc);
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = (acc[k] + RESIZE_HALF) >> 22;
            set = macc >= RESIZE_HALF;
        }
        // itertools.permutations(range(3))[perm] = (p0, p1, p2), two bits each
        const int p0 = (0xA50 >> (2 * g.perm)) & 3, p1 = (0x489 >> (2 * g.perm)) & 3, p2 = (0x126 >> (2 * g.perm)) & 3;
        *o = make_float4(t[aug_pick(v, p0)], t[256 + aug_pick(v, p1)], t[512 + aug_pick(v, p2)], 0.f);
        *om = set ? 1 : 0;
    }
}

extern "C" int fgn_support_augment_f32(const unsigned char* crop, const unsigned char* msk, const int* recs,
                                       const float* lut, float* y, unsigned char* m, int n, int S, hipStream_t stream) {
    if (!crop || !msk || !recs || !lut || !y || !m) return FGN_ERR_ARG;
    if (n < 0 || S < 0 || S > RESIZE_MAX_DIM) return FGN_ERR_SHAPE;
    if ((long long)n * S == 0) return FGN_OK;
    const uintptr_t px = (uintptr_t)n * S * S;              // pixels: 3 bytes of crop, 16 of y, 1 of msk and of m each
    const auto meet = [](const void* a, uintptr_t na, const void* b, uintptr_t nb) {
        const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
        return pa < pb + nb && pb < pa + na;
    };
    if (meet(crop, 3 * px, y, 16 * px) || meet(msk, px, m, px)) return FGN_ERR_ARG;       // (a gather: never in place)
    RowGrid g;
    if (row_grid((long long)n * S, S, 64, RESIZE_GRID_CAP, &g) != FGN_OK) return FGN_ERR_SHAPE;
    hipLaunchKernelGGL(support_augment_kernel, dim3(g.grid), dim3(RESIZE_BLOCK), 0, stream, crop, msk, recs, lut,
                       reinterpret_cast<float4*>(y), m, S, g.chunks, g.units);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// 3x3 / stride 2 / pad 1 max-pool, NHWC (mmdet ResNet stem; floor mode, -inf padding)
// ----------------------------------------------------------------------------------
__global__ void maxpool3x3s2_kernel(const float4* __restrict__ x, float4* __restrict__ y, int H, int W,
                                    int C4, int Ho, int Wo, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        long long r = i / C4;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho);
        const long long b = r / Ho;
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = oy * 2 - 1 + ky;
            if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = ox * 2 - 1 + kx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const float4 v = x[((b * H + iy) * W + ix) * C4 + c];
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y);
                m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        y[i] = m;
    }
}

extern "C" int fgn_maxpool3x3s2_nhwc_f32(const float* x, float* y, int n_img, int H, int W, int C,
                                         hipStream_t stream) {
    if (!x || !y) return FGN_ERR_ARG;
    if (C % 4) return FGN_ERR_SHAPE;
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const long long total = (long long)n_img * Ho * Wo * (C / 4);
    if (total == 0) return FGN_OK;
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(grid), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y), H, W, C / 4, Ho,
                       Wo, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// RoIAlign, average pooling, NHWC.  One workgroup per (roi, bin); lanes cover channels.
//   aligned=1, sampling_ratio=0 : mmcv.ops.RoIAlign as configured at
//                                 fgn_r50_c4_densecl.py:69-73 (fgn_roi_head.py:331,366)
//   aligned=0, sampling_ratio<=0: torchvision.ops.roi_align as called at
//                                 fgn_roi_head.py:429,432 (roi size clamped to >= 1)
// rois [R,5] = (batch_idx, x1, y1, x2, y2).  Sampling follows the upstream
// bilinear_interpolate: outside [-1,size] -> 0, coordinates clamped at 0, the last
// row/column snaps.
// ----------------------------------------------------------------------------------
// The geometry (box transform, grid, sample coordinates, axis_sample) is stated once, in roi_geom.h, for these
// kernels and for the adjoint in train_bwd.hip.
__global__ __launch_bounds__(256) void roi_align_kernel(const float* __restrict__ fmap,
                                                        const float* __restrict__ rois,
                                                        float* __restrict__ out,
                                                        const int32_t* __restrict__ n_rois_dev, int n_rois,
                                                        int H, int W, int C, int P, float spatial_scale,
                                                        int sampling_ratio, int aligned,
                                                        const float* __restrict__ post_shift, int relu,
                                                        const float* __restrict__ fmap2, float* __restrict__ out2, int C2,
                                                        const float* __restrict__ post_shift2, int relu2) {
    // (fmap2 / out2: an optional second map of the same spatial size pooled at the same RoIs by the same launch - the C4
    // map and the map of the shared head's commuted first conv; channel quads [C/4, (C + C2)/4) of the thread loop)
    const int bin = blockIdx.x;
    const int r = bin / (P * P);
    int nr = n_rois;
    if (n_rois_dev) nr = min(nr, *n_rois_dev);
    if (r >= nr) return;
    const int pb = bin - r * P * P;
    const int ph = pb / P, pw = pb - ph * P;

    const float* roi = rois + (size_t)r * 5;
    FGN_ROI_GEOMETRY(roi)
    const float* base1 = fmap + (size_t)b * H * W * C;
    const float* base2 = fmap2 ? fmap2 + (size_t)b * H * W * C2 : nullptr;
    const int c_all = C + (fmap2 ? C2 : 0);
    const int C1 = C;

    // The gh x gw samples of a bin form a grid and bilinear weights are separable, so the bin's value is
    //     sum_py sum_px WY[py] * WX[px] * v[py][px],   WY[py] = sum of the row weights of the samples touching row py
    // (likewise WX): (gh + 1) x (gw + 1) loads per channel quad instead of 4 * gh * gw (adaptive sampling takes up to
    // 8 x 8 samples per bin of a large RoI: 100 instead of 256 loads).  The two weight vectors are built once per bin
    // by two threads; samples outside [-1, size] carry no weight, as in the per-sample form.
    // (Measured on the 300 proposals of a cfg3 episode, two maps: 62.3 -> 55.0 us.  One workgroup per ROW of bins -
    // 2100 instead of 14 700 workgroups - was tried next and took 144 us: 10 serial items per thread.)
    constexpr int MAXS = 32;
    __shared__ float wy_sh[MAXS], wx_sh[MAXS];
    __shared__ int span_sh[4];       // y0, ny, x0, nx
    if (threadIdx.x < 2) {
        const bool is_y = threadIdx.x == 0;
        const int g = is_y ? gh : gw, size = is_y ? H : W;
        const float start = (is_y ? FGN_BIN_START(y1, ph, bin_h) : FGN_BIN_START(x1, pw, bin_w)), step = is_y ? bin_h : bin_w;
        float* w = is_y ? wy_sh : wx_sh;
        // (an empty sampling grid - a box of no extent - has no pixels: the bin is 0, as in the per-sample form)
        FGN_AXIS_SPAN(start, step, g, size)
        const int n = last - first + 1;
        span_sh[is_y ? 0 : 2] = first;
        span_sh[is_y ? 1 : 3] = n;
        if (n <= MAXS) {
            for (int i = 0; i < n; ++i) w[i] = 0.f;
            for (int i = 0; i < g; ++i) {
                const AxisSample sp = axis_sample(FGN_SAMPLE_COORD(start, i, step, g), size);
                if (sp.valid) {
                    w[sp.lo - first] += sp.h;
                    w[sp.hi - first] += sp.l;
                }
            }
        }
    }
    __syncthreads();
    const int y0 = span_sh[0], ny = span_sh[1], x0 = span_sh[2], nx = span_sh[3];
    const bool separable = ny <= MAXS && nx <= MAXS;

    for (int cc = threadIdx.x * 4; cc < c_all; cc += blockDim.x * 4) {
        const bool snd = cc >= C1;
        const float* base = snd ? base2 : base1;
        const int c = snd ? cc - C1 : cc;
        C = snd ? C2 : C1;
        if (snd) { out = out2; post_shift = post_shift2; relu = relu2; }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (separable) {
            for (int py = 0; py < ny; ++py) {
                const float wyv = wy_sh[py];
                const float* row = base + ((size_t)(y0 + py) * W + x0) * C + c;
                float4 racc = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int px = 0; px < nx; ++px) {
                    const float wv = wx_sh[px];
                    const float4 v = *reinterpret_cast<const float4*>(row + (size_t)px * C);
                    racc.x += wv * v.x; racc.y += wv * v.y; racc.z += wv * v.z; racc.w += wv * v.w;
                }
                acc.x += wyv * racc.x; acc.y += wyv * racc.y; acc.z += wyv * racc.z; acc.w += wyv * racc.w;
            }
        } else {
            for (int iy = 0; iy < gh; ++iy) {
                const float y = FGN_SAMPLE_COORD(FGN_BIN_START(y1, ph, bin_h), iy, bin_h, gh);
                const AxisSample sy = axis_sample(y, H);
                for (int ix = 0; ix < gw; ++ix) {
                    const float x = FGN_SAMPLE_COORD(FGN_BIN_START(x1, pw, bin_w), ix, bin_w, gw);
                    const AxisSample sx = axis_sample(x, W);
                    if (!(sy.valid && sx.valid)) continue;
                    const float w1 = sy.h * sx.h, w2 = sy.h * sx.l, w3 = sy.l * sx.h, w4 = sy.l * sx.l;
                    const float4 v1 = *reinterpret_cast<const float4*>(base + ((size_t)sy.lo * W + sx.lo) * C + c);
                    const float4 v2 = *reinterpret_cast<const float4*>(base + ((size_t)sy.lo * W + sx.hi) * C + c);
                    const float4 v3 = *reinterpret_cast<const float4*>(base + ((size_t)sy.hi * W + sx.lo) * C + c);
                    const float4 v4 = *reinterpret_cast<const float4*>(base + ((size_t)sy.hi * W + sx.hi) * C + c);
                    acc.x += w1 * v1.x + w2 * v2.x + w3 * v3.x + w4 * v4.x;
                    acc.y += w1 * v1.y + w2 * v2.y + w3 * v3.y + w4 * v4.y;
                    acc.z += w1 * v1.z + w2 * v2.z + w3 * v3.z + w4 * v4.z;
                    acc.w += w1 * v1.w + w2 * v2.w + w3 * v3.w + w4 * v4.w;
                }
            }
        }
        acc.x /= count; acc.y /= count; acc.z /= count; acc.w /= count;
        if (post_shift) {
            const float4 sh = *reinterpret_cast<const float4*>(post_shift + c);
            acc.x += sh.x; acc.y += sh.y; acc.z += sh.z; acc.w += sh.w;
        }
        if (relu) {
            acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
        }
        *reinterpret_cast<float4*>(out + ((size_t)r * P * P + pb) * C + c) = acc;
    }
}

// single-channel variant for the support masks (uint8/bool input [B,H,W]); one wavefront per bin,
// lanes stride over the (adaptive, up to ~37x37) sampling grid and combine with a shuffle reduction
__global__ __launch_bounds__(256) void roi_align_mask_kernel(const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ rois,
                                                             float* __restrict__ out, int n_rois, int H, int W,
                                                             int P, float spatial_scale, int sampling_ratio,
                                                             int aligned) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (i >= n_rois * P * P) return;
    const int r = i / (P * P);
    const int pb = i - r * P * P;
    const int ph = pb / P, pw = pb - ph * P;
    const float* roi = rois + (size_t)r * 5;
    FGN_ROI_GEOMETRY(roi)
    const uint8_t* base = mask + (size_t)b * H * W;
    float acc = 0.f;
    for (int s = lane; s < gh * gw; s += 64) {
        const int iy = s / gw, ix = s - iy * gw;
        const float y = FGN_SAMPLE_COORD(FGN_BIN_START(y1, ph, bin_h), iy, bin_h, gh);
        const float x = FGN_SAMPLE_COORD(FGN_BIN_START(x1, pw, bin_w), ix, bin_w, gw);
        const AxisSample sy = axis_sample(y, H);
        const AxisSample sx = axis_sample(x, W);
        if (!(sy.valid && sx.valid)) continue;
        const float v1 = base[(size_t)sy.lo * W + sx.lo] ? 1.f : 0.f;
        const float v2 = base[(size_t)sy.lo * W + sx.hi] ? 1.f : 0.f;
        const float v3 = base[(size_t)sy.hi * W + sx.lo] ? 1.f : 0.f;
        const float v4 = base[(size_t)sy.hi * W + sx.hi] ? 1.f : 0.f;
        acc += sy.h * sx.h * v1 + sy.h * sx.l * v2 + sy.l * sx.h * v3 + sy.l * sx.l * v4;
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) out[i] = acc / count;
}

extern "C" int fgn_roi_align_nhwc_f32(const float* fmap, const float* rois, float* out,
                                      const int32_t* n_rois_dev, int n_rois, int n_img, int H, int W, int C,
                                      int out_size, float spatial_scale, int sampling_ratio, int aligned,
                                      const float* post_shift, int relu, hipStream_t stream) {
    if (!fmap || !rois || !out) return FGN_ERR_ARG;
    if (C % 4 || out_size <= 0) return FGN_ERR_SHAPE;
    (void)n_img;
    if (n_rois == 0) return FGN_OK;
    const int threads = C >= 1024 ? 256 : (C >= 512 ? 128 : 64);
    hipLaunchKernelGGL(roi_align_kernel, dim3(n_rois * out_size * out_size), dim3(threads), 0, stream, fmap,
                       rois, out, n_rois_dev, n_rois, H, W, C, out_size, spatial_scale, sampling_ratio,
                       aligned, post_shift, relu, (const float*)nullptr, (float*)nullptr, 0, (const float*)nullptr, 0);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// Two maps of the same spatial size pooled at the same RoIs by one launch (fgn_roi_head.py:331,366 with the shared
// head's first 1x1 conv commuted in front of the pooling): out [R,P,P,C] from fmap, out2 [R,P,P,C2] from fmap2
// (+ post_shift2 [C2], ReLU).  Same arithmetic per channel as two fgn_roi_align_nhwc_f32 calls: identical bytes.
extern "C" int fgn_roi_align2_nhwc_f32(const float* fmap, const float* fmap2, const float* rois, float* out, float* out2,
                                       const int32_t* n_rois_dev, int n_rois, int n_img, int H, int W, int C, int C2,
                                       int out_size, float spatial_scale, int sampling_ratio, int aligned,
                                       const float* post_shift2, int relu2, hipStream_t stream) {
    if (!fmap || !fmap2 || !rois || !out || !out2) return FGN_ERR_ARG;
    if (C % 4 || C2 % 4 || out_size <= 0) return FGN_ERR_SHAPE;
    (void)n_img;
    if (n_rois == 0) return FGN_OK;
    // threads per bin, measured on the 300 proposals of a cfg3 episode (1024 + 512 channels = 384 quads; us per call):
    // 64: 92, 128: 61, 192: 52, 256: 55, 384: 67 - two whole items per thread on three waves
    const int quads = (C + C2) / 4;
    const int threads = quads % 192 == 0 ? 192 : (quads >= 256 ? 256 : (quads >= 128 ? 128 : 64));
    hipLaunchKernelGGL(roi_align_kernel, dim3(n_rois * out_size * out_size), dim3(threads), 0, stream, fmap,
                       rois, out, n_rois_dev, n_rois, H, W, C, out_size, spatial_scale, sampling_ratio,
                       aligned, (const float*)nullptr, 0, fmap2, out2, C2, post_shift2, relu2);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_roi_align_mask_u8(const uint8_t* mask, const float* rois, float* out, int n_rois, int n_img,
                                     int H, int W, int out_size, float spatial_scale, int sampling_ratio,
                                     int aligned, hipStream_t stream) {
    if (!mask || !rois || !out) return FGN_ERR_ARG;
    (void)n_img;
    if (n_rois == 0) return FGN_OK;
    const int total = n_rois * out_size * out_size;
    hipLaunchKernelGGL(roi_align_mask_kernel, dim3(cdiv(total, 4)), dim3(256), 0, stream, mask, rois, out,
                       n_rois, H, W, out_size, spatial_scale, sampling_ratio, aligned);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------
// Support-set reductions.
//   class vectors  out[g][c] = 1/(K*P) * sum_k sum_p x[g*K+k][p][c] * (w ? w[g*K+k][p] : 1)
//     - AG-RPN class-attentive vector, mean over (K,h,w)       fgn_ag_rpn_head.py:38-41
//     - mask-pooled vector, mean over (K,7,7) of feat*mask     fgn_roi_head.py:444-447
//   k-mean         out[g][p][c] = 1/K * sum_k x[g*K+k][p][c]   fgn_roi_head.py:439-442
// One workgroup per (group, 256-channel slab): lanes own 4 channels each, waves split
// the (k,p) range and combine through LDS.
// ----------------------------------------------------------------------------------
constexpr int CV_WAVES = 16;      // 12 workgroups in all at cfg3 and a serial K*P loop per wave: many waves keep it short
__global__ __launch_bounds__(64 * CV_WAVES) void class_vector_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ w,
                                                                     float* __restrict__ out, int K, int P, int C) {
    __shared__ float4 part[CV_WAVES][64];
    const int g = blockIdx.x;
    const int c = (blockIdx.y * 64 + (threadIdx.x & 63)) * 4;
    const int wv = threadIdx.x >> 6;
    const int KP = K * P;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
        for (int i = wv; i < KP; i += CV_WAVES) {
            const float4 v = *reinterpret_cast<const float4*>(x + ((size_t)g * KP + i) * C + c);
            const float s = w ? w[(size_t)g * KP + i] : 1.f;
            acc.x += v.x * s; acc.y += v.y * s; acc.z += v.z * s; acc.w += v.w * s;
        }
    }
    part[wv][threadIdx.x & 63] = acc;
    __syncthreads();
    if (wv == 0 && c < C) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < CV_WAVES; ++k) {            // fixed order
            const float4 a = part[k][threadIdx.x];
            o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
        }
        const float inv = 1.f / (float)KP;
        o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
        *reinterpret_cast<float4*>(out + (size_t)g * C + c) = o;
    }
}

extern "C" int fgn_support_class_vectors_f32(const float* x, const float* weights, float* out, int n_groups,
                                             int K, int P, int C, hipStream_t stream) {
    if (!x || !out) return FGN_ERR_ARG;
    if (C % 4) return FGN_ERR_SHAPE;
    if (n_groups == 0) return FGN_OK;
    hipLaunchKernelGGL(class_vector_kernel, dim3(n_groups, cdiv(C, 256)), dim3(64 * CV_WAVES), 0, stream, x, weights,
                       out, K, P, C);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

__global__ void kmean_kernel(const float4* __restrict__ x, float4* __restrict__ out, int K, long long PC4,
                             long long total) {
    const float inv = 1.f / (float)K;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long g = i / PC4, r = i - g * PC4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < K; ++k) {
            const float4 v = x[(g * K + k) * PC4 + r];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        out[i] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
    }
}

extern "C" int fgn_support_kmean_f32(const float* x, float* out, int n_groups, int K, int P, int C,
                                     hipStream_t stream) {
    if (!x || !out) return FGN_ERR_ARG;
    if (C % 4) return FGN_ERR_SHAPE;
    const long long pc4 = (long long)P * C / 4, total = pc4 * n_groups;
    if (total == 0) return FGN_OK;
    const int grid = (int)std::min<long long>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(kmean_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<float4*>(out), K, pc4, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// gather rows: out[i][:] = table[idx_base[i]][:]   (label -> support vector gather,
// fgn_roi_head.py:707-714; idx = label + n_ways * img)
__global__ void gather_rows_kernel(const float4* __restrict__ table, const int64_t* __restrict__ labels,
                                   const float* __restrict__ rois, float4* __restrict__ out,
                                   const int32_t* __restrict__ n_dev, int n, int n_ways, int C4) {
    int cnt = n;
    if (n_dev) cnt = min(cnt, *n_dev);
    const int i = blockIdx.x;
    if (i >= cnt) return;
    const int img = rois ? (int)rois[(size_t)i * 5] : 0;
    const long long row = labels[i] + (long long)n_ways * img;
    for (int c = threadIdx.x; c < C4; c += blockDim.x) out[(size_t)i * C4 + c] = table[row * C4 + c];
}

extern "C" int fgn_gather_support_vectors_f32(const float* table, const int64_t* labels, const float* rois,
                                              float* out, const int32_t* n_dev, int n, int n_ways, int C,
                                              hipStream_t stream) {
    if (!table || !labels || !out) return FGN_ERR_ARG;
    if (C % 4) return FGN_ERR_SHAPE;
    if (n == 0) return FGN_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, stream,
                       reinterpret_cast<const float4*>(table), labels, rois, reinterpret_cast<float4*>(out),
                       n_dev, n, n_ways, C / 4);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// out[n][p][c] = x[n / div][p][c] * v[n][c]: the AG-RPN guidance multiply materialised
// (fgn_ag_rpn_head.py:44-46) so that the 3x3 RPN conv can run on the LDS-DMA kernel when it does not take the Winograd form,
// which has no register stage to scale in.  HBM-bound: 1 read of x per class + 1 write.
__global__ void scale_channels_kernel(const float4* __restrict__ x, const float4* __restrict__ v,
                                      float4* __restrict__ out, int div, long long PC4, int C4, long long total) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long n = i / PC4, r = i - n * PC4;
        const float4 a = x[(n / div) * PC4 + r];
        const float4 s = v[n * C4 + (r % C4)];
        out[i] = make_float4(a.x * s.x, a.y * s.y, a.z * s.z, a.w * s.w);
    }
}

extern "C" int fgn_scale_channels_f32(const float* x, const float* v, float* out, int n_out, int div, int P, int C,
                                      hipStream_t stream) {
    if (C % 4 || div < 1 || n_out < 0 || P < 0) return FGN_ERR_SHAPE;
    const long long pc4 = (long long)P * C / 4, total = pc4 * n_out;
    if (total == 0) return FGN_OK;          // (the operands of an empty tensor are null pointers)
    if (!x || !v || !out) return FGN_ERR_ARG;
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(scale_channels_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(v), reinterpret_cast<float4*>(out), div, pc4, C / 4, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}
