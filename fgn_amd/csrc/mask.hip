// Mask-head tail: logits + sigmoid, and full-image paste + threshold.
//   mmdet FCNMaskHead: ... upsample (ConvTranspose2d 2x2/2) -> ReLU -> conv_logits 1x1
//   (fgn_roi_head.py:380), then get_seg_masks/_do_paste_mask (fgn_roi_head.py:668-671).
//
// The 2x2/stride-2 transposed conv is four independent 1x1 convs, one per output
// sub-position; it runs on the MFMA conv kernel as ONE 1x1 conv with 4*C output
// channels ordered n = (dy*2+dx)*C + co, leaving [D,7,7,(dy,dx),C] in memory.  Because
// conv_logits is point-wise it is applied directly on that layout, and the 14x14 pixel
// shuffle is folded into this kernel's output index - no shuffle pass.
#include "post_common.h"

// x : [D][P*P][4][C]  (post-ReLU upsample output);  w : [C], bias scalar
// prob/logit out : [D][2P][2P]
__global__ __launch_bounds__(256) void mask_logits_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          float bias, const float* __restrict__ bias_dev,
                                                          float* __restrict__ logits, float* __restrict__ prob,
                                                          const int32_t* __restrict__ n_dev, int n_det, int P,
                                                          int C) {
    if (bias_dev) bias = *bias_dev;          // device-resident bias (training: no host read of the updated parameter)
    int D = n_det;
    if (n_dev) D = min(D, *n_dev);
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int total = D * P * P * 4;
    if (wave >= total) return;
    const float* px = x + (size_t)wave * C;
    float acc = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4*>(px + c);
        const float4 k = *reinterpret_cast<const float4*>(w + c);
        acc += (v.x * k.x + v.y * k.y) + (v.z * k.z + v.w * k.w);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) {
        const int sub = wave & 3;
        const int cell = (wave >> 2) % (P * P);
        const int d = (wave >> 2) / (P * P);
        const int y = (cell / P) * 2 + (sub >> 1), xo = (cell % P) * 2 + (sub & 1);
        const float v = acc + bias;
        const size_t o = ((size_t)d * 2 * P + y) * 2 * P + xo;
        logits[o] = v;
        prob[o] = sigmoid32(v);
    }
}

extern "C" int fgn_mask_logits_f32(const float* x, const float* w, float bias, const float* bias_dev, float* logits, float* prob,
                                   const int32_t* n_dev, int n_det, int roi_size, int C, hipStream_t stream) {
    // (the per-detection operands of an empty detection set are null pointers: nothing is read or written then)
    if (!w || (n_det > 0 && (!x || !logits || !prob))) return FGN_ERR_ARG;
    if (C <= 0 || C % 4 || roi_size <= 0) return FGN_ERR_SHAPE;
    if (n_det <= 0) return FGN_OK;
    const int waves = n_det * roi_size * roi_size * 4;
    hipLaunchKernelGGL(mask_logits_kernel, dim3(cdiv(waves, 4)), dim3(256), 0, stream, x, w, bias, bias_dev, logits, prob,
                       n_dev, n_det, roi_size, C);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// paste: out[d][y][x] = bilinear(prob[d], grid(x,y)) >= thr.  grid_sample semantics: align_corners=False, zero
// padding.  HBM-bound: D*H*W bytes written, 4 pixels per lane.  Two region semantics, as in mmdet's _do_paste_mask:
//   skip_empty = 1 (its CPU path, one mask per chunk): only inside the integer-expanded box
//     (floor(x0)-1 .. ceil(x1)+1, clipped), 0 elsewhere - the oracle's and north_star's "CPU reference";
//   skip_empty = 0 (its CUDA path: the reference runs on cuda:0, main.py:365): the grid spans the whole image.  A
//     sample is non-zero only while its source coordinate lies inside (-1, M), i.e. within half a mask pixel =
//     box_w / (2 M) of the box, so the region computed here is that band (+1 px of slack), not the image; the two
//     semantics agree for thr >= 0.5 on boxes of positive width and height (the value on the box edge is half the
//     border pixel) and differ below it.
//     (thr <= 0 sets every pixel of the image under this semantic: the region is then the image.)
// ----------------------------------------------------------------------------------------------
// One mask sample, separable form shared by the dense paste kernel and the RLE kernel (so both
// produce the same bits): horizontal lerp of the two neighbouring mask rows, then vertical lerp.
// grid_sample semantics: pixel = ((g + 1) * size - 1) / 2, bilinear, zeros outside the map.
struct PasteBox {
    float bx0, by0, bx1, by1;
    int x0i, y0i, x1i, y1i;   // integer-expanded region [x0i,x1i) x [y0i,y1i)
};
__device__ __forceinline__ PasteBox make_paste_box(const float* b, int H, int W, int MS, int skip_empty, float thr) {
    PasteBox p;
    p.bx0 = b[0]; p.by0 = b[1]; p.bx1 = b[2]; p.by1 = b[3];
    if (skip_empty) {
        p.x0i = max((int)floorf(p.bx0) - 1, 0);
        p.y0i = max((int)floorf(p.by0) - 1, 0);
        p.x1i = min((int)ceilf(p.bx1) + 1, W);
        p.y1i = min((int)ceilf(p.by1) + 1, H);
        return p;
    }
    // whole-image grid: the band in which a sample can be non-zero; a degenerate axis (width <= 0: the grid
    // coordinate is inf -> 0, NaN where 0 / 0) samples the mask's centre line everywhere -> the whole axis
    const float bw = p.bx1 - p.bx0, bh = p.by1 - p.by0;
    const float mx = bw / (2.f * (float)MS), my = bh / (2.f * (float)MS);
    const bool all = !(thr > 0.f);
    const bool fx = all || !(bw > 0.f), fy = all || !(bh > 0.f);
    p.x0i = fx ? 0 : max((int)floorf(p.bx0 - mx) - 1, 0);
    p.x1i = fx ? W : min((int)ceilf(p.bx1 + mx) + 1, W);
    p.y0i = fy ? 0 : max((int)floorf(p.by0 - my) - 1, 0);
    p.y1i = fy ? H : min((int)ceilf(p.by1 + my) + 1, H);
    return p;
}
struct AxisLerp {
    int lo;        // low index (may be -1 .. MS-1); high = lo + 1
    float w_hi;    // weight of the high neighbour; low weight = 1 - w_hi
};
__device__ __forceinline__ AxisLerp paste_axis(int pix, float b0, float b1, int MS) {
    float g = ((float)pix + 0.5f - b0) / (b1 - b0) * 2.f - 1.f;
    if (isinf(g)) g = 0.f;
    const float c = ((g + 1.f) * (float)MS - 1.f) / 2.f;
    const float f = floorf(c);
    AxisLerp a;
    // clamp far-outside coordinates so the int conversion is defined; they contribute 0 anyway
    a.lo = (int)fminf(fmaxf(f, -2.f), (float)MS);
    a.w_hi = c - f;
    return a;
}
__device__ __forceinline__ float paste_row_lerp(const float* __restrict__ m, int MS, int row, const AxisLerp& ax) {
    if ((unsigned)row >= (unsigned)MS) return 0.f;
    const float v0 = ((unsigned)ax.lo < (unsigned)MS) ? m[row * MS + ax.lo] : 0.f;
    const float v1 = ((unsigned)(ax.lo + 1) < (unsigned)MS) ? m[row * MS + ax.lo + 1] : 0.f;
    return v0 * (1.f - ax.w_hi) + v1 * ax.w_hi;
}
__device__ __forceinline__ float paste_value(const float* __restrict__ m, int MS, const AxisLerp& ax,
                                             const AxisLerp& ay) {
    const float r0 = paste_row_lerp(m, MS, ay.lo, ax);
    const float r1 = paste_row_lerp(m, MS, ay.lo + 1, ax);
    return r0 * (1.f - ay.w_hi) + r1 * ay.w_hi;
}

__global__ __launch_bounds__(256) void mask_paste_kernel(const float* __restrict__ prob,
                                                         const float* __restrict__ boxes, int box_stride,
                                                         uint8_t* __restrict__ out,
                                                         const int32_t* __restrict__ n_dev, int n_det, int H, int W,
                                                         int MS, float thr, int skip_empty) {
    int D = n_det;
    if (n_dev) D = min(D, *n_dev);
    const long long HW = (long long)H * W;
    const long long total4 = ((long long)n_det * HW + 3) / 4;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total4;
         q += (long long)gridDim.x * blockDim.x) {
        uint32_t packed = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = q * 4 + k;
            if (i >= (long long)n_det * HW) break;
            const int d = (int)(i / HW);
            if (d >= D) continue;
            const int rem = (int)(i - (long long)d * HW);
            const int y = rem / W, x = rem - y * W;
            const PasteBox pb = make_paste_box(boxes + (size_t)d * box_stride, H, W, MS, skip_empty, thr);
            if (x < pb.x0i || x >= pb.x1i || y < pb.y0i || y >= pb.y1i) continue;
            const AxisLerp ax = paste_axis(x, pb.bx0, pb.bx1, MS);
            const AxisLerp ay = paste_axis(y, pb.by0, pb.by1, MS);
            if (paste_value(prob + (size_t)d * MS * MS, MS, ax, ay) >= thr) packed |= 1u << (8 * k);
        }
        if ((q + 1) * 4 <= (long long)n_det * HW) {
            reinterpret_cast<uint32_t*>(out)[q] = packed;
        } else {
            for (int k = 0; k < 4 && q * 4 + k < (long long)n_det * HW; ++k) out[q * 4 + k] = (packed >> (8 * k)) & 0xff;
        }
    }
}

extern "C" int fgn_mask_paste_u8(const float* prob, const float* boxes, int box_stride, uint8_t* out,
                                 const int32_t* n_dev, int n_det, int img_h, int img_w, int mask_size, float thr,
                                 int skip_empty, hipStream_t stream) {
    if (!prob || !boxes || !out) return FGN_ERR_ARG;
    if (n_det == 0) return FGN_OK;
    const long long total4 = ((long long)n_det * img_h * img_w + 3) / 4;
    const int grid = (int)std::min<long long>((total4 + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(mask_paste_kernel, dim3(grid), dim3(256), 0, stream, prob, boxes, box_stride, out, n_dev,
                       n_det, img_h, img_w, mask_size, thr, skip_empty);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// paste + threshold + COCO RLE, fused: the D x H x W masks are never materialised.
// Replaces get_seg_masks -> .cpu().numpy() -> pycocotools encode (fgn_roi_head.py:668-671,
// fgn.py:267,281): instead of writing D*H*W bytes, copying them over PCIe and run-length
// encoding on a host core, one workgroup per detection
//   1. counts the value transitions of every image column inside the pasted box
//      (column-major = pycocotools' Fortran order), one thread per column,
//   2. block-scans the counts and writes the transition positions in order,
//   3. turns positions into run lengths, delta-codes them against the run two back and
//      emits the COCO 5-bit/continuation ASCII string, again through a block scan.
// Only the strings (a few hundred bytes per detection) cross PCIe.
// Overflow of either cap sets overflow[d]; the host then falls back to the dense kernel for
// that detection, so results never depend on the caps.
// ----------------------------------------------------------------------------------------------
constexpr int RLE_THREADS = 1024;

__device__ inline int block_exclusive_scan(int v, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
    }
    __syncthreads();   // protects wave_sums reuse across calls
    if (lane == 63) wave_sums[wv] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < RLE_THREADS / 64; ++w) {
        const int s = wave_sums[w];
        if (w < wv) base += s;
        tot += s;
    }
    *total = tot;
    return base + incl - v;
}

__device__ __forceinline__ int rle_char_count(long long x) {
    int n = 0;
    bool more = true;
    while (more) {
        const int c = (int)(x & 0x1f);
        x >>= 5;
        more = (c & 0x10) ? (x != -1) : (x != 0);
        ++n;
    }
    return n;
}

// Step 3 of both RLE kernels: sorted transition positions tr[0..T) of the column-major pixel sequence -> run
// lengths -> COCO string (rleToString of pycocotools: delta against the run two back from the 4th run on, 5 data
// bits + continuation bit per character, +48).  Whole workgroup (RLE_THREADS); writes *out_len / *overflow.
__device__ inline void emit_coco_string(const uint32_t* __restrict__ tr, int T, long long HWl, uint8_t* __restrict__ ob,
                                        int byte_cap, int32_t* out_len, int32_t* overflow, int* wave_sums) {
    const int t = threadIdx.x;
    auto run_len = [&](int i) -> long long {   // i in [0, T]
        const long long hi = (i < T) ? (long long)tr[i] : HWl;
        const long long lo = (i > 0) ? (long long)tr[i - 1] : 0;
        return hi - lo;
    };
    const int n_runs = T + 1;
    const int rpt = (n_runs + RLE_THREADS - 1) / RLE_THREADS;
    int nchar = 0;
    for (int j = 0; j < rpt; ++j) {
        const int i = t * rpt + j;
        if (i < n_runs) {
            long long x = run_len(i);
            if (i > 2) x -= run_len(i - 2);
            nchar += rle_char_count(x);
        }
    }
    int total_chars;
    int o = block_exclusive_scan(nchar, wave_sums, &total_chars);
    if (total_chars > byte_cap) {
        if (t == 0) { *overflow = 1; *out_len = 0; }
        return;
    }
    for (int j = 0; j < rpt; ++j) {
        const int i = t * rpt + j;
        if (i < n_runs) {
            long long x = run_len(i);
            if (i > 2) x -= run_len(i - 2);
            bool more = true;
            while (more) {
                int c = (int)(x & 0x1f);
                x >>= 5;
                more = (c & 0x10) ? (x != -1) : (x != 0);
                if (more) c |= 0x20;
                ob[o++] = (uint8_t)(c + 48);
            }
        }
    }
    if (t == 0) { *out_len = total_chars; *overflow = 0; }
}

// Geometry of a source-size image under a network of (H, W) (results at source size): its size and the
// scale factors of mmdet's Resize, s_x = float32(W / w), s_y = float32(H / h) - the double quotient rounded once, which
// is numpy's np.float32(W / w) bit for bit.  At equal size both are exactly 1.  ok = the size is within 1..16384 (the
// contract of the resize kernel of spatial.hip); nothing is computed otherwise.
constexpr int SRC_MAX_DIM = 16384;
struct SrcGeom {
    int h, w;
    float sx, sy;
    bool ok;
};
__device__ __forceinline__ SrcGeom src_geom(int h, int w, int H, int W) {
    SrcGeom g;
    g.h = h; g.w = w;
    g.ok = h >= 1 && h <= SRC_MAX_DIM && w >= 1 && w <= SRC_MAX_DIM;
    g.sx = g.ok ? (float)((double)W / (double)w) : 1.f;
    g.sy = g.ok ? (float)((double)H / (double)h) : 1.f;
    return g;
}
// A network-frame box (x0, y0, x1, y1) in the source frame: each coordinate divided by its axis' scale, one correctly
// rounded f32 division (the translation unit is built without fast-math; mmdet: bboxes / scale_factor).  No clipping.
__device__ __forceinline__ void box_to_source(const float* __restrict__ b, const SrcGeom& g, float* __restrict__ o) {
    o[0] = __fdiv_rn(b[0], g.sx);
    o[1] = __fdiv_rn(b[1], g.sy);
    o[2] = __fdiv_rn(b[2], g.sx);
    o[3] = __fdiv_rn(b[3], g.sy);
}

// One detection, whole workgroup (RLE_THREADS): mask probabilities pm [MS][MS] pasted from box (x0, y0, x1, y1) into an
// H x W image, thresholded and run-length encoded (steps 1-3 above).  m: MS*MS floats of LDS, wave_sums: RLE_THREADS/64
// ints of LDS; tr / ob / out_len / overflow are the detection's own.  Every argument is workgroup-uniform.
__device__ __forceinline__ void rle_detection(const float* __restrict__ pm, const float* box,
                                              uint32_t* __restrict__ tr, uint8_t* __restrict__ ob, int32_t* out_len,
                                              int32_t* overflow, int H, int W, int MS, float thr, int trans_cap,
                                              int byte_cap, int skip_empty, float* m, int* wave_sums) {
    const int t = threadIdx.x;
    for (int i = t; i < MS * MS; i += RLE_THREADS) m[i] = pm[i];
    __syncthreads();
    const PasteBox pb = make_paste_box(box, H, W, MS, skip_empty, thr);
    // columns x0i .. min(x1i, W-1): one past the region closes a run that wraps a full-height column
    const int xs = pb.x0i, xe = min(pb.x1i, W - 1);
    const int ncols = max(xe - xs + 1, 0);
    const int cpt = (ncols + RLE_THREADS - 1) / RLE_THREADS;   // contiguous columns per thread
    // one row past the region closes a run; a region touching the bottom edge wraps into the next
    // column's row 0, so such columns are scanned from row 0
    const int ys = (pb.y1i >= H) ? 0 : pb.y0i, ye = min(pb.y1i, H - 1);

    auto value_at = [&](int x, int y, const AxisLerp& ax) -> int {
        if (x < pb.x0i || x >= pb.x1i || y < pb.y0i || y >= pb.y1i) return 0;
        const AxisLerp ay = paste_axis(y, pb.by0, pb.by1, MS);
        return paste_value(m, MS, ax, ay) >= thr ? 1 : 0;
    };
    auto scan_column = [&](int x, uint32_t* dst) -> int {   // dst == nullptr: count only
        const AxisLerp ax = paste_axis(x, pb.bx0, pb.bx1, MS);
        int prev = 0;
        if (ys == 0 && x > 0) {
            const AxisLerp axp = paste_axis(x - 1, pb.bx0, pb.bx1, MS);
            prev = value_at(x - 1, H - 1, axp);
        }
        int n = 0;
        for (int y = ys; y <= ye; ++y) {
            const int v = value_at(x, y, ax);
            if (v != prev) {
                if (dst) dst[n] = (uint32_t)x * (uint32_t)H + (uint32_t)y;
                ++n;
                prev = v;
            }
        }
        return n;
    };

    // ---- 1. count transitions per thread (contiguous columns) -------------------------------
    int cnt = 0;
    for (int j = 0; j < cpt; ++j) {
        const int c = t * cpt + j;
        if (c < ncols) cnt += scan_column(xs + c, nullptr);
    }
    int T;
    const int off = block_exclusive_scan(cnt, wave_sums, &T);
    if (T > trans_cap) {
        if (t == 0) { *overflow = 1; *out_len = 0; }
        return;
    }
    // ---- 2. write positions in order ----------------------------------------------------------
    {
        int o = off;
        for (int j = 0; j < cpt; ++j) {
            const int c = t * cpt + j;
            if (c < ncols) o += scan_column(xs + c, tr + o);
        }
    }
    __syncthreads();
    emit_coco_string(tr, T, (long long)H * W, ob, byte_cap, out_len, overflow, wave_sums);
}

__global__ __launch_bounds__(RLE_THREADS) void mask_rle_kernel(
    const float* __restrict__ prob, const float* __restrict__ boxes, int box_stride, uint32_t* __restrict__ trans,
    uint8_t* __restrict__ out_bytes, int32_t* __restrict__ out_len, int32_t* __restrict__ overflow,
    const int32_t* __restrict__ n_dev, int n_det, int H, int W, int MS, float thr, int trans_cap, int byte_cap,
    int skip_empty) {
    __shared__ float m[32 * 32];
    __shared__ int wave_sums[RLE_THREADS / 64];
    const int d = blockIdx.x, t = threadIdx.x;
    int D = n_det;
    if (n_dev) D = min(D, *n_dev);
    if (d >= D) {
        if (t == 0) { out_len[d] = 0; overflow[d] = 0; }
        return;
    }
    // (the network frame is the image: the box as it stands, no division)
    rle_detection(prob + (size_t)d * MS * MS, boxes + (size_t)d * box_stride, trans + (size_t)d * trans_cap,
                  out_bytes + (size_t)d * byte_cap, out_len + d, overflow + d, H, W, MS, thr, trans_cap, byte_cap,
                  skip_empty, m, wave_sums);
}

// The same for a batch at SOURCE size, one launch: grid (detection, image); row r = b * n_det + d of every array.
// Image b's size comes from the DEVICE array src_hw[b] = {h_b, w_b} and its detection count from n_dev[b] (null: n_det):
// no launch argument and no grid dimension depends on a source size, so one captured launch serves every source size.
// The box is divided by the image's scale (box_to_source) and pasted into h_b x w_b.  An image whose size is outside
// 1..16384 yields out_len = 0, overflow = 0 and zero boxes_src rows, and nothing of it is read.  boxes_src (optional)
// [B * n_det][4]: the scaled box of every row, written by one lane.  b, d and everything read at them are
// workgroup-uniform.
__global__ __launch_bounds__(RLE_THREADS) void mask_rle_src_kernel(
    const float* __restrict__ prob, const float* __restrict__ boxes, int box_stride, const int32_t* __restrict__ src_hw,
    uint32_t* __restrict__ trans, uint8_t* __restrict__ out_bytes, int32_t* __restrict__ out_len,
    int32_t* __restrict__ overflow, float* __restrict__ boxes_src, const int32_t* __restrict__ n_dev, int n_det, int H,
    int W, int MS, float thr, int trans_cap, int byte_cap, int skip_empty) {
    __shared__ float m[32 * 32];
    __shared__ int wave_sums[RLE_THREADS / 64];
    const int d = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const size_t r = (size_t)b * n_det + d;
    const SrcGeom g = src_geom(src_hw[2 * b], src_hw[2 * b + 1], H, W);
    int D = n_det;
    if (n_dev) D = min(D, n_dev[b]);
    float box[4] = {0.f, 0.f, 0.f, 0.f};
    if (g.ok) box_to_source(boxes + r * box_stride, g, box);
    if (boxes_src && t == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) boxes_src[r * 4 + k] = box[k];
    }
    if (!g.ok || d >= D) {
        if (t == 0) { out_len[r] = 0; overflow[r] = 0; }
        return;
    }
    rle_detection(prob + r * MS * MS, box, trans + r * trans_cap, out_bytes + r * byte_cap, out_len + r, overflow + r,
                  g.h, g.w, MS, thr, trans_cap, byte_cap, skip_empty, m, wave_sums);
}

extern "C" int fgn_mask_rle(const float* prob, const float* boxes, int box_stride, uint32_t* trans_scratch,
                            uint8_t* out_bytes, int32_t* out_len, int32_t* overflow, const int32_t* n_dev,
                            int n_det, int img_h, int img_w, int mask_size, float thr, int trans_cap, int byte_cap,
                            int skip_empty, hipStream_t stream) {
    if (!prob || !boxes || !trans_scratch || !out_bytes || !out_len || !overflow) return FGN_ERR_ARG;
    if (mask_size > 32 || mask_size < 1 || trans_cap < 1 || byte_cap < 8) return FGN_ERR_SHAPE;
    if ((long long)img_h * img_w >= (1ll << 32)) return FGN_ERR_SHAPE;
    if (n_det == 0) return FGN_OK;
    hipLaunchKernelGGL(mask_rle_kernel, dim3(n_det), dim3(RLE_THREADS), 0, stream, prob, boxes, box_stride,
                       trans_scratch, out_bytes, out_len, overflow, n_dev, n_det, img_h, img_w, mask_size, thr,
                       trans_cap, byte_cap, skip_empty);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_mask_rle_src(const float* prob, const float* boxes, int box_stride, const int32_t* src_hw,
                                uint32_t* trans_scratch, uint8_t* out_bytes, int32_t* out_len, int32_t* overflow,
                                float* boxes_src, const int32_t* n_dev, int batch, int n_det, int net_h, int net_w,
                                int mask_size, float thr, int trans_cap, int byte_cap, int skip_empty,
                                hipStream_t stream) {
    if (batch == 0 || n_det == 0) return FGN_OK;
    if (!prob || !boxes || !src_hw || !trans_scratch || !out_bytes || !out_len || !overflow) return FGN_ERR_ARG;
    if (batch < 0 || n_det < 0 || box_stride < 4) return FGN_ERR_ARG;
    if (mask_size > 32 || mask_size < 1 || trans_cap < 1 || byte_cap < 8 || net_h < 1 || net_w < 1 ||
        net_h > SRC_MAX_DIM || net_w > SRC_MAX_DIM || batch > 65535)
        return FGN_ERR_SHAPE;
    hipLaunchKernelGGL(mask_rle_src_kernel, dim3(n_det, batch), dim3(RLE_THREADS), 0, stream, prob, boxes, box_stride,
                       src_hw, trans_scratch, out_bytes, out_len, overflow, boxes_src, n_dev, n_det, net_h, net_w,
                       mask_size, thr, trans_cap, byte_cap, skip_empty);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// COCO RLE of DENSE binary masks: the ground-truth masks of the query image, which the reference moves to the
// GPU with the rest of the batch (fgn.py:92-99) and run-length encodes on the host at the end of simple_test
// (fgn.py:298, `qry_isegmaps_rle`).  Here they stay on the device: 4 host milliseconds of numpy per episode become
// four small kernels beside the network, and only the strings cross PCIe.
//   1. mask_to_columns_kernel: [n][H][W] bytes -> column-major [n][W][Hp] (Hp = H rounded up to 16, the pad rows
//      repeat the column's last pixel), i.e. pycocotools' Fortran scan order as contiguous 16-byte chunks;
//   2. dense_rle_walk_kernel (count, then emit; 32 workgroups per mask): value changes against the preceding pixel (the
//      pad makes "previous pixel of row 0" the last row of the previous column), positions x*H + y written in order;
//   3. dense_rle_string_kernel, one workgroup per mask: the shared string emitter.
// ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_to_columns_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                               int H, int W, int Hp) {
    __shared__ uint8_t tile[64][65];
    const int n = blockIdx.z;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    const uint8_t* src = in + (size_t)n * H * W;
    uint8_t* dst = out + (size_t)n * W * Hp;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int y = min(y0 + r, H - 1), x = x0 + tx;          // rows past H repeat row H-1 (the pad)
        tile[r][tx] = (x < W) ? (src[(size_t)y * W + x] != 0) : 0;
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int x = x0 + c, y = y0 + tx;
        if (x < W && y < Hp) dst[(size_t)x * Hp + y] = tile[tx][c];
    }
}

// The walk over a mask's change bits, split over DENSE_SEGS workgroups per mask (round 5: one 1024-thread workgroup per
// mask kept 4 of the 256 CUs busy for ~100 us - 66 steps of ~150 instructions per wave, two integer divisions among them -
// on the caller stream of the pipelined serving loop).  Three launches:
//   dense_rle_walk_kernel<false>  per (segment, mask): counts the transitions of its contiguous chunk range
//   dense_rle_walk_kernel<true>   ...: its offset = the counts of the segments before it; writes its transitions
//   dense_rle_string_kernel       one workgroup per mask: transitions -> COCO string (emit_coco_string)
// Inside a segment every wave owns a contiguous chunk range and walks it 64 chunks at a time (one contiguous kilobyte per
// wave-load, DENSE_U loads issued ahead); the column / chunk-in-column of a chunk advance incrementally (no division).
constexpr int DENSE_SEGS = 32;
constexpr int DENSE_THREADS = 256;
constexpr int DENSE_U = 4;

template <bool EMIT>
__global__ __launch_bounds__(DENSE_THREADS) void dense_rle_walk_kernel(const uint8_t* __restrict__ cols,
                                                                         uint32_t* __restrict__ trans,
                                                                         int32_t* __restrict__ seg_counts,
                                                                         int H, int W, int Hp, int trans_cap) {
    __shared__ int wave_sums[DENSE_THREADS / 64];
    const int seg = blockIdx.x, d = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint8_t* m = cols + (size_t)d * W * Hp;
    const int cpc = Hp / 16;                                   // chunks per column
    const int n_chunks = W * cpc;
    constexpr int NW = DENSE_THREADS / 64;
    const int per_seg = ((n_chunks + DENSE_SEGS - 1) / DENSE_SEGS + 64 * NW - 1) / (64 * NW) * (64 * NW);
    const int per_wave = per_seg / NW;                         // a multiple of 64
    const int w_lo = min(seg * per_seg + wv * per_wave, n_chunks), w_hi = min(w_lo + per_wave, n_chunks);
    int base = 0;
    if (EMIT) {
        int total = 0;
        for (int s2 = 0; s2 < DENSE_SEGS; ++s2) {
            const int c = seg_counts[d * DENSE_SEGS + s2];
            if (s2 < seg) base += c;
            total += c;
        }
        if (total > trans_cap) return;                         // (dense_rle_string_kernel flags the overflow)
    }
    auto load_chunk = [&](int c) -> uint4 {
        return c < w_hi ? *reinterpret_cast<const uint4*>(m + (size_t)c * 16) : make_uint4(0u, 0u, 0u, 0u);
    };
    // change bits of chunk c = chunk k of column x (its 16 bytes in v): bit r set iff pixel (x, 16 k + r) differs from its
    // predecessor in scan order (the last pixel of the previous chunk: the neighbouring lane's, or for lane 0 one byte load)
    auto chunk_bits = [&](int c, int k, const uint4& v) -> unsigned {
        const bool in = c < w_hi;
        // the 16 bytes are 0 / 1 (mask_to_columns_kernel normalises them): a multiply gathers the four low bits of a
        // word into one nibble (b0 | b1 << 1 | b2 << 2 | b3 << 3 lands in bits 24..27, the partial products never
        // carry), and "differs from its predecessor" is one XOR against the value shifted by a pixel
        const unsigned px = ((v.x * 0x01020408u) >> 24 & 0xfu) | ((v.y * 0x01020408u) >> 20 & 0xf0u) |
                            ((v.z * 0x01020408u) >> 16 & 0xf00u) | ((v.w * 0x01020408u) >> 12 & 0xf000u);
        unsigned prev = __shfl_up(px >> 15, 1, 64);
        if (lane == 0) prev = (in && c > 0) ? (unsigned)(m[(size_t)c * 16 - 1] & 1) : 0u;
        if (!in) return 0u;
        const unsigned bits = (px ^ ((px << 1) | prev)) & 0xffffu;
        const int valid = min(16, H - 16 * k);                  // pad rows never differ, but mask them anyway
        return valid >= 16 ? bits : (bits & ((1u << valid) - 1u));
    };
    // (x, k) of this lane's chunk, advanced by 64 chunks per step without a division
    int c = w_lo + lane;
    int x = c / cpc, k = c - x * cpc;
    const int dx = 64 / cpc, dk = 64 - dx * cpc;
    uint32_t* tr = trans + (size_t)d * trans_cap;
    int cnt = 0, run = 0;
    // ---- pass A (both variants): this thread's count (the emitting variant needs it for its offsets inside the segment)
    {
        int ca = c, ka = k;
        for (int c0 = w_lo; c0 < w_hi; c0 += 64 * DENSE_U) {
            uint4 v[DENSE_U];
#pragma unroll
            for (int u = 0; u < DENSE_U; ++u) v[u] = load_chunk(c0 + 64 * u + lane);
#pragma unroll
            for (int u = 0; u < DENSE_U; ++u) {
                if (c0 + 64 * u < w_hi) cnt += __popc(chunk_bits(ca, ka, v[u]));
                ca += 64; ka += dk;
                if (ka >= cpc) ka -= cpc;
            }
        }
    }
    // workgroup-level exclusive scan of the per-thread counts (thread order = wave-major); a wave's base = lane 0's
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_sums[wv] = incl;
    __syncthreads();
    int wave_base = 0, seg_total = 0;
    for (int w = 0; w < NW; ++w) {
        if (w < wv) wave_base += wave_sums[w];
        seg_total += wave_sums[w];
    }
    if (!EMIT) {
        if (t == 0) seg_counts[d * DENSE_SEGS + seg] = seg_total;
        return;
    }
    // ---- pass B: emit, in (step, lane) order inside the wave's range
    run = base + wave_base;
    for (int c0 = w_lo; c0 < w_hi; c0 += 64 * DENSE_U) {
        uint4 v[DENSE_U];
#pragma unroll
        for (int u = 0; u < DENSE_U; ++u) v[u] = load_chunk(c0 + 64 * u + lane);
#pragma unroll
        for (int u = 0; u < DENSE_U; ++u) {
            if (c0 + 64 * u < w_hi) {                            // (wave-uniform)
                unsigned bits = chunk_bits(c, k, v[u]);
                const int n = __popc(bits);
                int sc = n;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int up = __shfl_up(sc, off, 64);
                    if (lane >= off) sc += up;
                }
                int o = run + sc - n;
                run += __shfl(sc, 63, 64);
                while (bits) {
                    const int r = __ffs(bits) - 1;
                    bits &= bits - 1;
                    tr[o++] = (uint32_t)x * (uint32_t)H + (uint32_t)(16 * k + r);
                }
            }
            c += 64; x += dx; k += dk;
            if (k >= cpc) { k -= cpc; ++x; }
        }
    }
}

__global__ __launch_bounds__(RLE_THREADS) void dense_rle_string_kernel(const uint32_t* __restrict__ trans,
                                                                       const int32_t* __restrict__ seg_counts,
                                                                       uint8_t* __restrict__ out_bytes,
                                                                       int32_t* __restrict__ out_len,
                                                                       int32_t* __restrict__ overflow, int H, int W,
                                                                       int trans_cap, int byte_cap) {
    __shared__ int wave_sums[RLE_THREADS / 64];
    const int d = blockIdx.x, t = threadIdx.x;
    int T = 0;
    for (int s2 = 0; s2 < DENSE_SEGS; ++s2) T += seg_counts[d * DENSE_SEGS + s2];
    if (T > trans_cap) {
        if (t == 0) { overflow[d] = 1; out_len[d] = 0; }
        return;
    }
    emit_coco_string(trans + (size_t)d * trans_cap, T, (long long)H * W, out_bytes + (size_t)d * byte_cap, byte_cap,
                     out_len + d, overflow + d, wave_sums);
}

extern "C" size_t fgn_dense_rle_scratch_bytes(int n_masks, int img_h, int img_w, int trans_cap) {
    const size_t hp = (size_t)(img_h + 15) / 16 * 16;
    return (size_t)n_masks * img_w * hp + (size_t)n_masks * trans_cap * sizeof(uint32_t) + 256 +
           (size_t)n_masks * DENSE_SEGS * sizeof(int32_t) + 256;
}

extern "C" int fgn_dense_mask_rle(const uint8_t* masks, void* scratch, size_t scratch_bytes, uint8_t* out_bytes,
                                  int32_t* out_len, int32_t* overflow, int n_masks, int img_h, int img_w, int trans_cap,
                                  int byte_cap, hipStream_t stream) {
    if (!masks || !scratch || !out_bytes || !out_len || !overflow) return FGN_ERR_ARG;
    if (n_masks == 0) return FGN_OK;
    if (img_h < 1 || img_w < 1 || trans_cap < 1 || byte_cap < 8 || (long long)img_h * img_w >= (1ll << 32) ||
        n_masks > 65535)
        return FGN_ERR_SHAPE;
    if (scratch_bytes < fgn_dense_rle_scratch_bytes(n_masks, img_h, img_w, trans_cap)) return FGN_ERR_ARG;
    const int hp = (img_h + 15) / 16 * 16;
    uint8_t* cols = reinterpret_cast<uint8_t*>(scratch);
    const size_t cols_bytes = ((size_t)n_masks * img_w * hp + 255) / 256 * 256;
    uint32_t* trans = reinterpret_cast<uint32_t*>(cols + cols_bytes);
    const size_t trans_bytes = ((size_t)n_masks * trans_cap * sizeof(uint32_t) + 255) / 256 * 256;
    int32_t* seg_counts = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(trans) + trans_bytes);
    hipLaunchKernelGGL(mask_to_columns_kernel, dim3(cdiv(img_w, 64), cdiv(hp, 64), n_masks), dim3(256), 0, stream, masks,
                       cols, img_h, img_w, hp);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_rle_walk_kernel<false>, dim3(DENSE_SEGS, n_masks), dim3(DENSE_THREADS), 0, stream, cols, trans,
                       seg_counts, img_h, img_w, hp, trans_cap);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_rle_walk_kernel<true>, dim3(DENSE_SEGS, n_masks), dim3(DENSE_THREADS), 0, stream, cols, trans,
                       seg_counts, img_h, img_w, hp, trans_cap);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(dense_rle_string_kernel, dim3(n_masks), dim3(RLE_THREADS), 0, stream, trans, seg_counts, out_bytes,
                       out_len, overflow, img_h, img_w, trans_cap, byte_cap);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// COCO RLE as an INPUT: ground-truth and support masks that arrive as runs (the reference's COCO dataset holds nothing
// else, coco_ds.py:195-207, and decodes on the host per sample, get_isegmap coco_ds.py:265-278) become, on the device,
// exactly the bytes a dense upload would have put there.  The host sends the cumulative run ENDS of each mask
// (fgn_amd/rle.py: RleMasks) and one record per mask; pixel (y, x) sits at column-major position p = x * h + y and is
// set where an odd number of its mask's ends are <= p - zero-length runs (repeated ends) need no special case.
//   Mapping: one lane per window column, RLED_THREADS columns per workgroup, RLED_ROWS rows per blockIdx.y, masks and
//   column blocks flattened into blockIdx.x.  A lane finds r for its first p by one binary search, then walks down its
//   column: p grows by 1 per row, r advances while ends[r] <= p (one load per run crossed, the current end stays in a
//   register).  A row's store is 64 consecutive bytes per wave - one coalesced segment - and no pointer is cast, so the
//   output needs no alignment (the rows of a [rows, capacity] slot start at any byte).
//   Safety: r never leaves [0, n_runs], ends is read at run0 + r with r < n_runs only, and a record that fails a check
//   reads no run at all: whatever ends holds, no index leaves its slice.
// ----------------------------------------------------------------------------------------------
constexpr int RLED_THREADS = 256;   // window columns per workgroup
constexpr int RLED_ROWS = 32;       // window rows per blockIdx.y
constexpr int RLED_REC_INTS = 8;    // {h, w, wy, wx, wh, ww, run0, n_runs}

__global__ __launch_bounds__(RLED_THREADS) void rle_decode_kernel(const uint32_t* __restrict__ ends, long long n_ends,
                                                                  const int32_t* __restrict__ recs,
                                                                  uint8_t* __restrict__ out, long long out_stride,
                                                                  int col_blocks, int max_wh, int max_ww) {
    const int i = blockIdx.x / col_blocks, cb = blockIdx.x - i * col_blocks;      // (workgroup-uniform)
    const int32_t* rec = recs + (size_t)i * RLED_REC_INTS;
    const int h = rec[0], w = rec[1], wy = rec[2], wx = rec[3], wh = rec[4], ww = rec[5], run0 = rec[6], n_runs = rec[7];
    uint8_t* dst = out + (size_t)i * (size_t)out_stride;
    const bool window = wh >= 1 && ww >= 1;
    const bool fits = window && (long long)wh * ww <= out_stride;
    const bool ok = fits && h >= 1 && h <= SRC_MAX_DIM && w >= 1 && w <= SRC_MAX_DIM && wy >= 0 && wx >= 0 &&
                    wh <= h - wy && ww <= w - wx && wh <= max_wh && ww <= max_ww && n_runs >= 1 && run0 >= 0 &&
                    (long long)run0 + n_runs <= n_ends;
    if (!ok) {
        // an out-of-range record reads none of its runs; its window is zeros where it fits the slot (the workgroups of
        // this mask share the bytes), and nothing is written otherwise
        if (!fits) return;
        const long long total = (long long)wh * ww;
        const long long step = (long long)col_blocks * gridDim.y * RLED_THREADS;
        for (long long b = ((long long)blockIdx.y * col_blocks + cb) * RLED_THREADS + threadIdx.x; b < total; b += step)
            dst[b] = 0;
        return;
    }
    const int c = cb * RLED_THREADS + threadIdx.x;                                // window column of this lane
    const int y0 = blockIdx.y * RLED_ROWS;
    if (c >= ww || y0 >= wh) return;
    const int rows = min(RLED_ROWS, wh - y0);
    const uint32_t* e = ends + run0;
    uint32_t p = (uint32_t)(wx + c) * (uint32_t)h + (uint32_t)(wy + y0);          // < 2^28
    int lo = 0, hi = n_runs;                                                      // r = #{j : e[j] <= p}, in [0, n_runs]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    int r = lo;
    uint32_t cur = r < n_runs ? e[r] : 0xffffffffu;                               // the first end beyond p
    uint8_t* o = dst + (size_t)y0 * ww + c;
    for (int y = 0; y < rows; ++y, ++p, o += ww) {
        while (cur <= p) {                                                        // (a repeated end = a zero-length run)
            ++r;
            cur = r < n_runs ? e[r] : 0xffffffffu;
        }
        *o = (uint8_t)(r & 1);
    }
}

extern "C" int fgn_rle_decode_u8(const uint32_t* ends, long long n_ends, const int32_t* recs, uint8_t* out,
                                 long long out_stride_bytes, int n, int max_wh, int max_ww, hipStream_t stream) {
    if (n < 0 || out_stride_bytes < 0 || n_ends < 0 || max_wh < 0 || max_ww < 0 || max_wh > SRC_MAX_DIM ||
        max_ww > SRC_MAX_DIM)
        return FGN_ERR_SHAPE;
    if (n == 0 || max_wh == 0 || max_ww == 0) return FGN_OK;
    if (!ends || !recs || !out) return FGN_ERR_ARG;
    const int col_blocks = cdiv(max_ww, RLED_THREADS);
    if ((long long)n * col_blocks >= (1ll << 24)) return FGN_ERR_SHAPE;     // (grid.x * RLED_THREADS stays below 2^32)
    hipLaunchKernelGGL(rle_decode_kernel, dim3((unsigned)(n * col_blocks), cdiv(max_wh, RLED_ROWS)), dim3(RLED_THREADS), 0,
                       stream, ends, n_ends, recs, out, out_stride_bytes, col_blocks, max_wh, max_ww);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// Box + colour as an INPUT: the character datasets of the reference (cfg1 MNISTISEG, cfg2 OMNIISEG) store no mask, only
// a box and the RGB colour of every instance, and derive the mask from the image on the host for every sample
// (get_char_mask_by_color, create_img_from_chars.py:136-158; base_fst.py:836 for the query, :1107 per support
// instance): the pixels of the box inside the colour window, dilated 3x3 inside the box.  The image bytes are on the
// device already (qry_src / spp_src / the uint8 qry_img), so the mask is made here, right where a dense upload would
// have put its bytes, from 16 ints per mask.
//   p(y, x) = all_c(lo_c <= img[y][x][c] <= hi_c) inside the box, 0 outside; mask(y, x) = OR of p over the 3x3
//   neighbourhood for (y, x) inside the box, 0 outside.  No pixel outside the box (or the image) ever contributes.
//   Mapping: one workgroup of 4 waves per (mask, 64 x 32 tile of the IMAGE) - the output is written in full, zeros
//   outside the box included, so tiles that miss the box store zeros and read nothing.  A tile that meets it evaluates p
//   on its 34 rows (one halo row above and below): a wave takes a row, a lane a column, and the wave's ballot IS the
//   row's 64-bit word, kept in LDS; the two halo columns of the 34 rows are 68 single predicates.  Each image byte is
//   read once per tile (plus halo).  The dilation of a row is w | w << 1 | w >> 1 with the halo bits carried in at bit 0
//   and bit 63, ORed over three rows; a lane stores its bit as one byte: 64 consecutive bytes per wave and row, no
//   pointer cast, so neither the image row nor the output needs any alignment.  No atomics, no scratch.
//   Safety: every record field is checked against the capacities passed in before an address is formed; inside a valid
//   record a pixel is read only where it lies inside the box, and the box lies inside h x w, 3 * h * w <= src_cap.
// ----------------------------------------------------------------------------------------------
constexpr int CM_THREADS = 256;
constexpr int CM_TW = 64;           // tile columns: one ballot word
constexpr int CM_TH = 32;           // tile rows
constexpr int CM_REC_INTS = 16;     // {row, h, w, y0, x0, y1, x1, lo_r, lo_g, lo_b, hi_r, hi_g, hi_b, out, 0, 0}

__global__ __launch_bounds__(CM_THREADS) void color_mask_kernel(const uint8_t* __restrict__ src, long long src_stride,
                                                                long long src_cap, int src_rows,
                                                                const int32_t* __restrict__ recs,
                                                                uint8_t* __restrict__ out, long long out_stride,
                                                                int n_out, int tiles_x, int max_h, int max_w) {
    __shared__ unsigned long long words[CM_TH + 2];
    __shared__ uint8_t side[2][CM_TH + 2];
    const int i = blockIdx.x / tiles_x, tx = blockIdx.x - i * tiles_x;            // (workgroup-uniform)
    const int32_t* rec = recs + (size_t)i * CM_REC_INTS;
    const int row = rec[0], h = rec[1], w = rec[2], y0 = rec[3], x0 = rec[4], y1 = rec[5], x1 = rec[6], oi = rec[13];
    // the output must exist before anything is written: index inside the slot array, h * w bytes inside its stride
    if (!(oi >= 0 && oi < n_out && h >= 1 && w >= 1 && (long long)h * w <= out_stride)) return;
    uint8_t* dst = out + (size_t)oi * (size_t)out_stride;
    const bool ok = h <= max_h && w <= max_w && h <= SRC_MAX_DIM && w <= SRC_MAX_DIM && row >= 0 && row < src_rows &&
                    3ll * h * w <= src_cap && y0 >= 0 && y0 <= y1 && y1 <= h && x0 >= 0 && x0 <= x1 && x1 <= w;
    if (!ok) {
        // an out-of-range record reads no pixel; its output is zeros (the workgroups of this mask share the bytes)
        const long long total = (long long)h * w;
        const long long step = (long long)tiles_x * gridDim.y * CM_THREADS;
        for (long long b = ((long long)blockIdx.y * tiles_x + tx) * CM_THREADS + threadIdx.x; b < total; b += step)
            dst[b] = 0;
        return;
    }
    const int X0 = tx * CM_TW, Y0 = blockIdx.y * CM_TH;
    if (X0 >= w || Y0 >= h) return;
    const int rows = min(CM_TH, h - Y0), cols = min(CM_TW, w - X0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = X0 + lane;
    if (!(y0 < y1 && x0 < x1 && Y0 < y1 && Y0 + CM_TH > y0 && X0 < x1 && X0 + CM_TW > x0)) {
        if (lane < cols)                                                          // the tile misses the box: zeros
            for (int r = wave; r < rows; r += CM_THREADS / 64) dst[(size_t)(Y0 + r) * w + x] = 0;
        return;
    }
    const uint8_t* img = src + (size_t)row * (size_t)src_stride;
    const int lo0 = rec[7], lo1 = rec[8], lo2 = rec[9], hi0 = rec[10], hi1 = rec[11], hi2 = rec[12];
    auto pred = [&](int py, int px) -> bool {                                     // (inside the box => inside the image)
        if (py < y0 || py >= y1 || px < x0 || px >= x1) return false;
        const uint8_t* p = img + ((size_t)py * w + px) * 3;
        const int r = p[0], g = p[1], b = p[2];
        return r >= lo0 && r <= hi0 && g >= lo1 && g <= hi1 && b >= lo2 && b <= hi2;
    };
    for (int rr = wave; rr < CM_TH + 2; rr += CM_THREADS / 64) {                  // row Y0 - 1 + rr of the image
        const unsigned long long word = __ballot(pred(Y0 - 1 + rr, x));
        if (lane == 0) words[rr] = word;
    }
    if (threadIdx.x < 2 * (CM_TH + 2)) {                                          // the halo columns X0 - 1 and X0 + 64
        const int s = threadIdx.x / (CM_TH + 2), rr = threadIdx.x - s * (CM_TH + 2);
        side[s][rr] = pred(Y0 - 1 + rr, s ? X0 + CM_TW : X0 - 1) ? 1 : 0;
    }
    __syncthreads();
    for (int r = wave; r < rows; r += CM_THREADS / 64) {
        const int y = Y0 + r;
        unsigned long long acc = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned long long c = words[r + k];
            acc |= c | (c << 1) | (c >> 1) | (unsigned long long)side[0][r + k] |
                   ((unsigned long long)side[1][r + k] << 63);
        }
        const bool in = y >= y0 && y < y1 && x >= x0 && x < x1;
        if (lane < cols) dst[(size_t)y * w + x] = (uint8_t)(in ? (acc >> lane) & 1ull : 0ull);
    }
}

extern "C" int fgn_color_mask_u8(const uint8_t* src, long long src_stride_bytes, long long src_cap_bytes, int src_rows,
                                 const int32_t* recs, int n, uint8_t* out, long long out_stride_bytes, int n_out,
                                 int max_h, int max_w, hipStream_t stream) {
    if (n < 0 || src_rows < 0 || n_out < 0 || src_stride_bytes < 0 || src_cap_bytes < 0 || out_stride_bytes < 0 ||
        max_h < 0 || max_w < 0 || max_h > SRC_MAX_DIM || max_w > SRC_MAX_DIM)
        return FGN_ERR_SHAPE;
    if (n == 0 || max_h == 0 || max_w == 0) return FGN_OK;
    if (!src || !recs || !out) return FGN_ERR_ARG;
    const int tiles_x = cdiv(max_w, CM_TW);
    if ((long long)n * tiles_x >= (1ll << 24)) return FGN_ERR_SHAPE;        // (grid.x * CM_THREADS stays below 2^32)
    hipLaunchKernelGGL(color_mask_kernel, dim3((unsigned)(n * tiles_x), cdiv(max_h, CM_TH)), dim3(CM_THREADS), 0, stream,
                       src, src_stride_bytes, src_cap_bytes, src_rows, recs, out, out_stride_bytes, n_out, tiles_x, max_h,
                       max_w);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// Matching on the device: exact pixel counts |d & g|, |d|, |g| of every (detection, ground truth) pair.
// The evaluator (fgn_amd/fsiseg_eval.py) needs nothing else from the masks, and both operands are on the device while
// the episode is in flight: the ground-truth masks (uploaded for the RLE above) and the mask probabilities + boxes the
// RLE kernel pastes from.  Two kernels:
//   mask_bits_kernel     [G][H][W] bytes -> bit planes, one 64-bit word per 64 consecutive x of a row (a wave-wide
//                        ballot; bits of x >= W are zero), laid out [H][ceil(W/64)][G]: the words of all masks for
//                        one (row, x-word) are contiguous, which is what the consumer loads; + the areas |g|
//   mask_overlap_kernel  per (detection, block of rows): the pasted bits of a 64-pixel row segment are one ballot
//                        (lane = pixel; make_paste_box / paste_axis / paste_value of this file, so the bits are those of
//                        mask_paste_kernel and mask_rle_kernel), then lane = ground-truth index ANDs its own word with it
//                        and counts.  Integer atomics: the result does not depend on the order of the additions.
// Neither the D x H x W nor the bit form of the detections' masks is ever written.
// ----------------------------------------------------------------------------------------------
constexpr int BITS_THREADS = 256;
constexpr int BITS_ROWS = 8;        // image rows per workgroup of mask_bits_kernel
constexpr int OVL_THREADS = 256;
constexpr int OVL_WAVES = OVL_THREADS / 64;
constexpr int OVL_ROWS = 32;        // image rows per workgroup of mask_overlap_kernel

// a[0..na) = 0 and b[0..nb) = 0 (b may be null with nb = 0)
__global__ __launch_bounds__(256) void zero_i32_kernel(int32_t* __restrict__ a, long long na, int32_t* __restrict__ b,
                                                       long long nb) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < na + nb;
         i += (long long)gridDim.x * blockDim.x) {
        if (i < na) a[i] = 0;
        else b[i - na] = 0;
    }
}

// grid: row block * G + g.  area[] is zero on entry.
__global__ __launch_bounds__(BITS_THREADS) void mask_bits_kernel(const uint8_t* __restrict__ masks,
                                                                 unsigned long long* __restrict__ bits,
                                                                 int32_t* __restrict__ area, int G, int H, int W, int NW) {
    __shared__ int wave_cnt[BITS_THREADS / 64];
    const int g = blockIdx.x % G, rb = blockIdx.x / G;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int y0 = rb * BITS_ROWS, rows = min(BITS_ROWS, H - y0);
    const uint8_t* src = masks + (size_t)g * H * W;
    int cnt = 0;
    for (int i = wv; i < rows * NW; i += BITS_THREADS / 64) {     // (wave-uniform trip count)
        const int r = i / NW, xw = i - r * NW;
        const int y = y0 + r, x = xw * 64 + lane;
        const bool v = x < W && src[(size_t)y * W + x] != 0;
        const unsigned long long word = __ballot(v);
        if (lane == 0) bits[((size_t)y * NW + xw) * G + g] = word;
        cnt += __popcll(word);
    }
    if (lane == 0) wave_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < BITS_THREADS / 64; ++w) s += wave_cnt[w];
        if (s) atomicAdd(area + g, s);
    }
}

extern "C" int fgn_mask_bits_u64(const uint8_t* masks, uint64_t* bits, int32_t* area, int n_masks, int img_h, int img_w,
                                 hipStream_t stream) {
    if (n_masks == 0) return FGN_OK;
    if (!masks || !bits || !area) return FGN_ERR_ARG;
    if (n_masks < 0 || img_h < 1 || img_w < 1 || (long long)img_h * img_w >= (1ll << 31)) return FGN_ERR_SHAPE;
    const long long blocks = (long long)cdiv(img_h, BITS_ROWS) * n_masks;
    if (blocks >= (1ll << 31)) return FGN_ERR_SHAPE;
    hipLaunchKernelGGL(zero_i32_kernel, dim3(cdiv(n_masks, 256)), dim3(256), 0, stream, area, (long long)n_masks,
                       (int32_t*)nullptr, 0ll);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_bits_kernel, dim3((unsigned)blocks), dim3(BITS_THREADS), 0, stream, masks,
                       reinterpret_cast<unsigned long long*>(bits), area, n_masks, img_h, img_w, cdiv(img_w, 64));
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// One detection against the G ground-truth bit planes of an H x W image, rows of this workgroup's block (blockIdx.y):
// pm [MS][MS] pasted from box (x0, y0, x1, y1); inter_d [G] / det_area_d are the detection's own, zero on entry.
// m: MS*MS floats of LDS, red / red_area: the workgroup's reduction space.  Every argument is workgroup-uniform.
__device__ __forceinline__ void overlap_detection(const float* __restrict__ pm, const float* box,
                                                  const unsigned long long* __restrict__ gt_bits,
                                                  int32_t* __restrict__ inter_d, int32_t* __restrict__ det_area_d, int G,
                                                  int H, int W, int NW, int MS, float thr, int skip_empty, float* m,
                                                  int (*red)[64], int* red_area) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const PasteBox pb = make_paste_box(box, H, W, MS, skip_empty, thr);
    const int y_lo = max(pb.y0i, (int)blockIdx.y * OVL_ROWS), y_hi = min(pb.y1i, ((int)blockIdx.y + 1) * OVL_ROWS);
    if (y_lo >= y_hi || pb.x0i >= pb.x1i) return;          // rows outside the pasted region (workgroup-uniform)
    for (int i = t; i < MS * MS; i += OVL_THREADS) m[i] = pm[i];
    __syncthreads();
    const int w_lo = pb.x0i >> 6, w_hi = (pb.x1i - 1) >> 6;  // x-words of the region, inclusive; 0 <= x0i < x1i <= W
    for (int g0 = 0; g0 < G; g0 += 64) {                     // passes of 64 ground-truth masks (lane = mask)
        const int g = g0 + lane;
        int acc = 0, area = 0;
        for (int xw = w_lo; xw <= w_hi; ++xw) {
            const int x = xw * 64 + lane;                    // lane = pixel of the segment
            const bool in_x = x >= pb.x0i && x < pb.x1i;
            const AxisLerp ax = paste_axis(x, pb.bx0, pb.bx1, MS);
            for (int y = y_lo + wv; y < y_hi; y += OVL_WAVES) {
                const AxisLerp ay = paste_axis(y, pb.by0, pb.by1, MS);
                const bool v = in_x && paste_value(m, MS, ax, ay) >= thr;
                const unsigned long long det = __ballot(v);
                if (det) {                                   // (wave-uniform)
                    area += __popcll(det);
                    if (g < G) acc += __popcll(det & gt_bits[((size_t)y * NW + xw) * G + g]);
                }
            }
        }
        red[wv][lane] = acc;
        if (lane == 0) red_area[wv] = area;
        __syncthreads();
        if (wv == 0) {
            int s = 0, a = 0;
#pragma unroll
            for (int w = 0; w < OVL_WAVES; ++w) { s += red[w][lane]; a += red_area[w]; }
            if (g < G && s) atomicAdd(inter_d + g, s);
            if (g0 == 0 && lane == 0 && a) atomicAdd(det_area_d, a);   // |d| once, not once per pass
        }
        __syncthreads();
    }
}

// grid: (detection, block of OVL_ROWS rows).  inter / det_area are zero on entry.
__global__ __launch_bounds__(OVL_THREADS) void mask_overlap_kernel(
    const float* __restrict__ prob, const float* __restrict__ boxes, int box_stride,
    const unsigned long long* __restrict__ gt_bits, int32_t* __restrict__ inter, int32_t* __restrict__ det_area,
    const int32_t* __restrict__ n_dev, int n_det, int G, int H, int W, int NW, int MS, float thr, int skip_empty) {
    __shared__ float m[32 * 32];
    __shared__ int red[OVL_WAVES][64];
    __shared__ int red_area[OVL_WAVES];
    const int d = blockIdx.x;
    int D = n_det;
    if (n_dev) D = min(D, *n_dev);
    if (d >= D) return;
    overlap_detection(prob + (size_t)d * MS * MS, boxes + (size_t)d * box_stride, gt_bits, inter + (size_t)d * G,
                      det_area + d, G, H, W, NW, MS, thr, skip_empty, m, red, red_area);
}

// The same at SOURCE size: the boxes are network-frame boxes of an (H, W) network, divided by the scale of the h x w
// image (src_geom / box_to_source: the scale is formed where mask_rle_src_kernel forms it) and pasted into h x w, the
// size of gt_bits.  The launch is eager (G differs per image), so h and w are launch arguments and size the grid.
__global__ __launch_bounds__(OVL_THREADS) void mask_overlap_src_kernel(
    const float* __restrict__ prob, const float* __restrict__ boxes, int box_stride,
    const unsigned long long* __restrict__ gt_bits, int32_t* __restrict__ inter, int32_t* __restrict__ det_area,
    const int32_t* __restrict__ n_dev, int n_det, int G, int h, int w, int H, int W, int NW, int MS, float thr,
    int skip_empty) {
    __shared__ float m[32 * 32];
    __shared__ int red[OVL_WAVES][64];
    __shared__ int red_area[OVL_WAVES];
    const int d = blockIdx.x;
    int D = n_det;
    if (n_dev) D = min(D, *n_dev);
    const SrcGeom g = src_geom(h, w, H, W);
    if (d >= D || !g.ok) return;
    float box[4];
    box_to_source(boxes + (size_t)d * box_stride, g, box);
    overlap_detection(prob + (size_t)d * MS * MS, box, gt_bits, inter + (size_t)d * G, det_area + d, G, g.h, g.w, NW, MS,
                      thr, skip_empty, m, red, red_area);
}

extern "C" int fgn_mask_overlap_i32(const float* prob, const float* boxes, int box_stride, const uint64_t* gt_bits,
                                    int32_t* inter, int32_t* det_area, const int32_t* n_dev, int n_det, int n_gt,
                                    int img_h, int img_w, int mask_size, float thr, int skip_empty, hipStream_t stream) {
    if (n_det == 0 || n_gt == 0) return FGN_OK;
    if (!prob || !boxes || !gt_bits || !inter || !det_area) return FGN_ERR_ARG;
    if (n_det < 0 || n_gt < 0 || box_stride < 4) return FGN_ERR_ARG;
    if (mask_size > 32 || mask_size < 1 || img_h < 1 || img_w < 1 || (long long)img_h * img_w >= (1ll << 31) ||
        cdiv(img_h, OVL_ROWS) > 65535)
        return FGN_ERR_SHAPE;
    const long long n_out = (long long)n_det * n_gt;
    hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)std::min<long long>((n_out + n_det + 255) / 256, 1024)), dim3(256),
                       0, stream, inter, n_out, det_area, (long long)n_det);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_overlap_kernel, dim3(n_det, cdiv(img_h, OVL_ROWS)), dim3(OVL_THREADS), 0, stream, prob, boxes,
                       box_stride, reinterpret_cast<const unsigned long long*>(gt_bits), inter, det_area, n_dev, n_det,
                       n_gt, img_h, img_w, cdiv(img_w, 64), mask_size, thr, skip_empty);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_mask_overlap_src_i32(const float* prob, const float* boxes, int box_stride, const uint64_t* gt_bits,
                                        int32_t* inter, int32_t* det_area, const int32_t* n_dev, int n_det, int n_gt,
                                        int src_h, int src_w, int net_h, int net_w, int mask_size, float thr,
                                        int skip_empty, hipStream_t stream) {
    if (n_det == 0 || n_gt == 0) return FGN_OK;
    if (!prob || !boxes || !gt_bits || !inter || !det_area) return FGN_ERR_ARG;
    if (n_det < 0 || n_gt < 0 || box_stride < 4) return FGN_ERR_ARG;
    if (mask_size > 32 || mask_size < 1 || src_h < 1 || src_w < 1 || src_h > SRC_MAX_DIM || src_w > SRC_MAX_DIM ||
        net_h < 1 || net_w < 1 || net_h > SRC_MAX_DIM || net_w > SRC_MAX_DIM)
        return FGN_ERR_SHAPE;
    const long long n_out = (long long)n_det * n_gt;
    hipLaunchKernelGGL(zero_i32_kernel, dim3((unsigned)std::min<long long>((n_out + n_det + 255) / 256, 1024)), dim3(256),
                       0, stream, inter, n_out, det_area, (long long)n_det);
    FGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(mask_overlap_src_kernel, dim3(n_det, cdiv(src_h, OVL_ROWS)), dim3(OVL_THREADS), 0, stream, prob,
                       boxes, box_stride, reinterpret_cast<const unsigned long long*>(gt_bits), inter, det_area, n_dev,
                       n_det, n_gt, src_h, src_w, net_h, net_w, cdiv(src_w, 64), mask_size, thr, skip_empty);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ----------------------------------------------------------------------------------------------
// Matching on the device, second half: the evaluator's greedy matching (fgn_amd/fsiseg_eval.py, match_flags /
// FSISEGEval._evaluate_img) of one image's detections to its ground truth.  Per (IoU type, category): the detections of
// the category in descending score order (ties in index order), cut at max_dets; each in turn takes the still
// unmatched ground truth of the category with the largest IoU >= thr (among equal IoUs the largest index).  Output:
// one int32 per detection and IoU type, bit t = matched at thr[t]; -1 = beyond max_dets of its category; 0 = label
// outside 0..n_ways-1 or row at / beyond the device count.
//
// One workgroup per (IoU type, category) of T waves, ONE WAVE PER THRESHOLD.  The walk is sequential in the detections
// (at most max_dets steps, each a wave reduction), so its latency is what the launch costs: waves of different
// thresholds walk side by side instead of one wave walking T times.  They sit in one workgroup because they share the
// score order (formed once, by all threads) and because a detection's T bits are then combined from LDS by one thread
// and stored once - no two waves ever write the same word, so there is no atomic anywhere.
//   rank   rank_i = #{j of the category: s_j > s_i or (s_j == s_i and j < i)}: the stable descending order, by counting,
//          on scores and membership staged in LDS once; the detection of rank r leaves its operand (the box, divided to
//          the source frame where asked, or |d|) in LDS at r, so the walk reads no detection from global memory.
//   walk   lane = ground truth (passes of 64): its IoU in float64 with the expression of _bbox_iou / _count_iou (the
//          translation unit is built with -ffp-contract=off; the f64 division is correctly rounded), then - only where
//          more than one lane is at or above the threshold - a wave reduction to (max IoU, largest index among equals).
//          The matched set lives in registers: bit p of a lane's
//          word = its ground truth of pass p (the per-pass 64-bit masks, transposed).  The walk is a chain of dependent
//          steps, so the one global load a step needs (segm: the row of inter) is issued two steps ahead for pass 0.
// Scores are expected to be no NaN (a NaN has no rank); a rank left empty by one is skipped.
// ----------------------------------------------------------------------------------------------
constexpr int EVM_MAX_THRS = 16;
constexpr int EVM_MAX_DET = 2048;        // detections of an image: scores and membership live in LDS
constexpr int EVM_MAX_RANKS = 1024;      // min(D, max_dets) at most: the walk's order, operands and bits live in LDS
constexpr int EVM_MAX_GT = 4096;         // 64 passes: one bit each in a lane's matched word
constexpr int EVM_MIN_WAVES = 4;         // waves of a workgroup at least: the staging and ranking are shared work

struct EvmGt {                           // one ground truth as a lane holds it
    double x, y, w, h;                   // bbox: _xywh(qry_bboxes)
    double area;                         // segm: |g|
    bool ok;                             // of this workgroup's category
};

__device__ __forceinline__ EvmGt evm_load_gt(int g, int G, int k, int type, const double* __restrict__ gt_xywh,
                                             const int32_t* __restrict__ gt_cat, const int32_t* __restrict__ gt_area) {
    EvmGt v;
    v.x = v.y = v.w = v.h = v.area = 0.0;
    v.ok = g < G && gt_cat[g] == k;
    if (v.ok) {
        if (type == 0) {
            v.x = gt_xywh[4 * (size_t)g]; v.y = gt_xywh[4 * (size_t)g + 1];
            v.w = gt_xywh[4 * (size_t)g + 2]; v.h = gt_xywh[4 * (size_t)g + 3];
        } else {
            v.area = (double)gt_area[g];
        }
    }
    return v;
}

// grid: (category, IoU type: 0 bbox, 1 segm), max(T, EVM_MIN_WAVES) * 64 threads: with few thresholds the extra waves
// help to stage and rank, and walk nothing.  flags [2][D]; with has_segm == 0 the grid has one row
// and its category-0 workgroup zeroes row 1.  D <= EVM_MAX_DET, min(D, max_dets) <= EVM_MAX_RANKS, G <= EVM_MAX_GT.
__global__ __launch_bounds__(EVM_MAX_THRS * 64) void eval_match_kernel(
    const float* __restrict__ boxes, int box_stride, const long long* __restrict__ labels,
    const int32_t* __restrict__ n_dev, const int32_t* __restrict__ inter, const int32_t* __restrict__ det_area,
    const int32_t* __restrict__ gt_area, const double* __restrict__ gt_xywh, const int32_t* __restrict__ gt_cat,
    const double* __restrict__ thr, int32_t* __restrict__ flags, int D, int G, int T, int n_ways, int max_dets,
    int src_h, int src_w, int net_h, int net_w, int has_segm) {
    __shared__ float score[EVM_MAX_DET];
    __shared__ uint8_t member[EVM_MAX_DET];
    __shared__ int order[EVM_MAX_RANKS];
    __shared__ float4 operand[EVM_MAX_RANKS];               // of the detection at a rank: bbox x1 y1 x2 y2; segm .x = |d| (bits)
    __shared__ uint8_t hit[EVM_MAX_THRS][EVM_MAX_RANKS];
    __shared__ int wave_cnt[EVM_MAX_THRS];
    const int k = blockIdx.x, type = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6, nthreads = blockDim.x;
    int n = D;
    if (n_dev) n = max(0, min(D, *n_dev));
    int32_t* __restrict__ out = flags + (size_t)type * D;
    if (k == 0) {                                           // the words no category's workgroup owns
        for (int d = tid; d < D; d += nthreads) {
            bool outside = d >= n;
            if (!outside) { const long long l = labels[d]; outside = l < 0 || l >= n_ways; }
            if (outside) out[d] = 0;
            if (!has_segm) flags[(size_t)D + d] = 0;
        }
    }
    // ---- membership and scores into LDS; the category's detections are counted per wave (wave-uniform trip count)
    const int r_cap = min(min(n, max_dets), EVM_MAX_RANKS);
    for (int r = tid; r < r_cap; r += nthreads) order[r] = -1;
    int cnt = 0;
    for (int base = 0; base < n; base += nthreads) {
        const int d = base + tid;
        const bool m = d < n && labels[d] == k;
        if (d < n) {
            member[d] = m ? 1 : 0;
            score[d] = m ? boxes[(size_t)d * box_stride + 4] : 0.f;
        }
        cnt += __popcll(__ballot(m));
    }
    if (lane == 0) wave_cnt[t] = cnt;
    __syncthreads();
    int nk = 0;
    for (int w = 0; w < (nthreads >> 6); ++w) nk += wave_cnt[w];
    // ---- rank by counting; the detection of rank r leaves its operand at r
    const bool to_source = src_h > 0;
    const SrcGeom geom = src_geom(to_source ? src_h : 1, to_source ? src_w : 1, net_h, net_w);
    for (int d = tid; d < n; d += nthreads) {
        if (!member[d]) continue;
        const float s = score[d];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (member[j] && (score[j] > s || (score[j] == s && j < d))) ? 1 : 0;
        if (rank >= r_cap) {
            out[d] = -1;                                    // beyond max_dets of its category: not evaluated
            continue;
        }
        order[rank] = d;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (type == 0) {
            float b[4];
            const float* src = boxes + (size_t)d * box_stride;
            if (to_source) box_to_source(src, geom, b);
            else { b[0] = src[0]; b[1] = src[1]; b[2] = src[2]; b[3] = src[3]; }
            o = make_float4(b[0], b[1], b[2], b[3]);
        } else {
            o.x = __int_as_float(det_area[d]);
        }
        operand[rank] = o;
    }
    __syncthreads();
    const int n_ranked = min(nk, r_cap);

    // ---- the walk of threshold t (wave-uniform control flow throughout); a wave beyond T (see EVM_MIN_WAVES) has none
    const int nsel = t < T ? n_ranked : 0;
    const double th = thr[min(t, T - 1)];
    const int passes = (G + 63) >> 6;
    const EvmGt g_first = evm_load_gt(lane, G, k, type, gt_xywh, gt_cat, gt_area);      // pass 0, kept in registers
    // segm: inter[order[r]][lane], the one global load of a step, issued two steps ahead (0 where there is none)
    auto row_first = [&](int r) -> int {
        if (type != 1 || r >= nsel || !g_first.ok) return 0;
        const int d = order[r];
        return d >= 0 ? inter[(size_t)d * G + lane] : 0;
    };
    int ahead1 = row_first(0), ahead2 = row_first(1);
    unsigned long long matched = 0;                         // bit p: ground truth p * 64 + lane is matched
    for (int r = 0; r < nsel; ++r) {
        const int in_first = ahead1;
        ahead1 = ahead2;
        ahead2 = row_first(r + 2);
        const int d = order[r];
        if (d < 0) {
            if (lane == 0) hit[t][r] = 0;
            continue;
        }
        const float4 o = operand[r];
        double dx = 0, dy = 0, dx2 = 0, dy2 = 0, d_area;
        if (type == 0) {
            dx = (double)o.x; dy = (double)o.y;
            const double dw = (double)fmaxf(o.z - o.x, 1.f);           // the differences in the boxes' own float32 (_xywh)
            const double dh = (double)fmaxf(o.w - o.y, 1.f);
            dx2 = dx + dw; dy2 = dy + dh;
            d_area = dw * dh;
        } else {
            d_area = (double)__float_as_int(o.x);
        }
        double best = -1.0;                                 // (an IoU is never negative)
        int best_g = -1;
        for (int p = 0; p < passes; ++p) {
            const int g = p * 64 + lane;
            const EvmGt gt = p == 0 ? g_first : evm_load_gt(g, G, k, type, gt_xywh, gt_cat, gt_area);
            if (!gt.ok || ((matched >> p) & 1ull)) continue;
            double iou;
            if (type == 0) {
                const double w = fmax(fmin(dx2, gt.x + gt.w) - fmax(dx, gt.x), 0.0);
                const double h = fmax(fmin(dy2, gt.y + gt.h) - fmax(dy, gt.y), 0.0);
                const double in = w * h;
                const double un = d_area + gt.w * gt.h - in;
                iou = in / un;
            } else {
                const double in = (double)(p == 0 ? in_first : inter[(size_t)d * G + g]);
                const double un = d_area + gt.area - in;
                iou = un > 0.0 ? in / un : 0.0;
            }
            if (iou >= th && iou >= best) { best = iou; best_g = g; }     // a later pass holds the larger index
        }
        // most steps have no lane at or above the threshold, the others mostly one: the reduction runs for rivals only
        const unsigned long long rivals = __ballot(best_g >= 0);
        if (rivals == 0) {
            if (lane == 0) hit[t][r] = 0;
            continue;
        }
        if (rivals & (rivals - 1)) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ob = __shfl_xor(best, off);
                const int og = __shfl_xor(best_g, off);
                if (ob > best || (ob == best && og > best_g)) { best = ob; best_g = og; }
            }
        } else {
            best_g = __shfl(best_g, __ffsll(rivals) - 1);
        }
        if (best_g >= 0 && (best_g & 63) == lane) matched |= 1ull << (best_g >> 6);
        if (lane == 0) hit[t][r] = best_g >= 0 ? 1 : 0;
    }
    __syncthreads();
    for (int r = tid; r < n_ranked; r += nthreads) {
        const int d = order[r];
        if (d < 0) continue;
        int v = 0;
        for (int tt = 0; tt < T; ++tt) v |= (int)hit[tt][r] << tt;
        out[d] = v;
    }
}

extern "C" int fgn_eval_match_i32(const float* boxes, int box_stride, const int64_t* labels, const int32_t* n_dev,
                                  const int32_t* inter, const int32_t* det_area, const int32_t* gt_area,
                                  const double* gt_xywh, const int32_t* gt_cat, const double* thr, int32_t* flags,
                                  int n_det, int n_gt, int n_thr, int n_ways, int max_dets, int src_h, int src_w,
                                  int net_h, int net_w, hipStream_t stream) {
    if (n_thr < 1 || n_thr > EVM_MAX_THRS || n_det < 0 || n_gt < 0 || n_ways < 1 || max_dets < 1) return FGN_ERR_SHAPE;
    if (n_det == 0) return FGN_OK;
    const bool has_segm = det_area != nullptr;
    if (!boxes || !labels || !thr || !flags || box_stride < 5) return FGN_ERR_ARG;
    if (n_gt > 0 && (!gt_xywh || !gt_cat || (has_segm && (!inter || !gt_area)))) return FGN_ERR_ARG;
    if (n_det > EVM_MAX_DET || std::min(n_det, max_dets) > EVM_MAX_RANKS || n_gt > EVM_MAX_GT || n_ways > 65535)
        return FGN_ERR_SHAPE;
    const bool to_source = src_h != 0 || src_w != 0;
    if (to_source && (src_h < 1 || src_w < 1 || src_h > SRC_MAX_DIM || src_w > SRC_MAX_DIM || net_h < 1 || net_w < 1 ||
                      net_h > SRC_MAX_DIM || net_w > SRC_MAX_DIM))
        return FGN_ERR_SHAPE;
    hipLaunchKernelGGL(eval_match_kernel, dim3(n_ways, has_segm ? 2 : 1), dim3(std::max(n_thr, EVM_MIN_WAVES) * 64), 0,
                       stream, boxes, box_stride,
                       reinterpret_cast<const long long*>(labels), n_dev, inter, det_area, gt_area, gt_xywh, gt_cat, thr,
                       flags, n_det, n_gt, n_thr, n_ways, max_dets, to_source ? src_h : 0, to_source ? src_w : 0, net_h,
                       net_w, has_segm ? 1 : 0);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}
