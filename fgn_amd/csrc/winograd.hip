// Winograd transforms for the 3x3 / stride 1 / pad 1 convolutions whose reduction is deep
// enough to be MFMA-bound (AG-RPN conv, fgn_ag_rpn_head.py:48; the 3x3 of the shared_head bottlenecks,
// fgn_roi_head.py:236).  The convolution becomes
//     V = B^T d B   (input transform,  this file: HBM-bound, 16 B per lane)
//     Mo[g] = V[g] U[g]^T, g = 0..15 / 0..35   (one grouped GEMM launch, conv_igemm.hip)
//     y = A^T Mo A + shift, ReLU       (output transform, this file)
// with 2.25x fewer multiply-adds than the direct form.  fp32 throughout; F(2x2,3x3) uses only
// +-1 and 1/2 coefficients, its rounding error stays within a few ulp of the direct sum.
// Tile t = (img * ty + y) * tx + x covers outputs [2y, 2y+2) x [2x, 2x+2); V / Mo are laid out
// [16][t_pad][C] so each of the 16 positions is a contiguous row-major GEMM operand.
#include "common.h"
#include <cstdlib>

__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 f4mul(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }

// x [n_in, H, W, C]; logical image i reads x[i / a_img_div], scaled per channel by in_scale[i][c]
// (the AG-RPN guidance multiply, fgn_ag_rpn_head.py:44, fused here).
__global__ __launch_bounds__(256) void wg_input_kernel(const float4* __restrict__ x, const float4* __restrict__ in_scale,
                                                       float4* __restrict__ V, const int32_t* __restrict__ n_img_dev,
                                                       int n_img, int a_img_div, int H, int W, int C4, int ty, int tx,
                                                       int t_pad, long long total) {
    if (n_img_dev) n_img = min(n_img, *n_img_dev);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const int t = (int)(i / C4);
        const int xx = t % tx;
        const int r = t / tx;
        const int yy = r % ty;
        const int img = r / ty;
        if (img >= n_img) break;                      // images are the slowest index: nothing left for this thread
        const float4* src = x + (size_t)(img / a_img_div) * H * W * C4 + c;
        const int iy0 = 2 * yy - 1, ix0 = 2 * xx - 1;
        float4 d[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int iy = iy0 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int ix = ix0 + b;
                d[a][b] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                              ? src[((size_t)iy * W + ix) * C4] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        if (in_scale) {
            const float4 s = in_scale[(size_t)img * C4 + c];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) d[a][b] = f4mul(d[a][b], s);
        }
        float4 tt[4][4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {                 // B^T d  (columns)
            tt[0][b] = f4sub(d[0][b], d[2][b]);
            tt[1][b] = f4add(d[1][b], d[2][b]);
            tt[2][b] = f4sub(d[2][b], d[1][b]);
            tt[3][b] = f4sub(d[1][b], d[3][b]);
        }
        float4* dst = V + (size_t)t * C4 + c;
        const size_t gs = (size_t)t_pad * C4;
#pragma unroll
        for (int a = 0; a < 4; ++a) {                 // (B^T d) B  (rows)
            dst[(a * 4 + 0) * gs] = f4sub(tt[a][0], tt[a][2]);
            dst[(a * 4 + 1) * gs] = f4add(tt[a][1], tt[a][2]);
            dst[(a * 4 + 2) * gs] = f4sub(tt[a][2], tt[a][1]);
            dst[(a * 4 + 3) * gs] = f4sub(tt[a][1], tt[a][3]);
        }
    }
}

// Mo [16][t_pad][C] -> y [n_img, H, W, C] = A^T Mo A + shift (ReLU); odd H / W drop the last row / column
__global__ __launch_bounds__(256) void wg_output_kernel(const float4* __restrict__ Mo, float4* __restrict__ y,
                                                        const float4* __restrict__ shift,
                                                        const int32_t* __restrict__ n_img_dev, int n_img, int H, int W,
                                                        int C4, int ty, int tx, int t_pad, int relu, long long total) {
    if (n_img_dev) n_img = min(n_img, *n_img_dev);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        const int t = (int)(i / C4);
        const int xx = t % tx;
        const int r = t / tx;
        const int yy = r % ty;
        const int img = r / ty;
        if (img >= n_img) break;
        const float4* src = Mo + (size_t)t * C4 + c;
        const size_t gs = (size_t)t_pad * C4;
        float4 s0[4], s1[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {                 // A^T m (columns)
            const float4 m0 = src[(0 * 4 + b) * gs], m1 = src[(1 * 4 + b) * gs], m2 = src[(2 * 4 + b) * gs],
                         m3 = src[(3 * 4 + b) * gs];
            s0[b] = f4add(f4add(m0, m1), m2);
            s1[b] = f4sub(f4sub(m1, m2), m3);
        }
        float4 o[2][2];
        o[0][0] = f4add(f4add(s0[0], s0[1]), s0[2]);
        o[0][1] = f4sub(f4sub(s0[1], s0[2]), s0[3]);
        o[1][0] = f4add(f4add(s1[0], s1[1]), s1[2]);
        o[1][1] = f4sub(f4sub(s1[1], s1[2]), s1[3]);
        const float4 sh = shift ? shift[c] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int oy = 2 * yy + a;
            if (oy >= H) continue;
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ox = 2 * xx + b;
                if (ox >= W) continue;
                float4 v = f4add(o[a][b], sh);
                if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
                y[(((size_t)img * H + oy) * W + ox) * C4 + c] = v;
            }
        }
    }
}

extern "C" int fgn_winograd_input_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev,
                                      int n_img, int a_img_div, int H, int W, int C, int t_pad, hipStream_t stream) {
    if (!x || !V) return FGN_ERR_ARG;
    if (n_img <= 0) return FGN_OK;
    const int ty = (H + 1) / 2, tx = (W + 1) / 2;
    if (C % 4 != 0 || a_img_div < 1 || H < 1 || W < 1 || (long long)n_img * ty * tx > t_pad) return FGN_ERR_SHAPE;
    const long long total = (long long)n_img * ty * tx * (C / 4);
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 32);
    FGN_LAUNCH_TIMED(wg_input_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(x),
                       reinterpret_cast<const float4*>(in_scale), reinterpret_cast<float4*>(V), n_img_dev, n_img,
                       a_img_div, H, W, C / 4, ty, tx, t_pad, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_winograd_output_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev,
                                       int n_img, int H, int W, int C, int t_pad, int relu, hipStream_t stream) {
    if (!Mo || !y) return FGN_ERR_ARG;
    if (n_img <= 0) return FGN_OK;
    const int ty = (H + 1) / 2, tx = (W + 1) / 2;
    if (C % 4 != 0 || (long long)n_img * ty * tx > t_pad) return FGN_ERR_SHAPE;
    const long long total = (long long)n_img * ty * tx * (C / 4);
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 32);
    FGN_LAUNCH_TIMED(wg_output_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const float4*>(Mo),
                       reinterpret_cast<float4*>(y), reinterpret_cast<const float4*>(shift), n_img_dev, n_img, H, W,
                       C / 4, ty, tx, t_pad, relu, total);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// ------------------------------------------------------------------------------------------------
// F(4x4, 3x3): 36 products per 4x4 outputs instead of 144 (4x fewer multiply-adds than the direct form, 1.78x fewer
// than F(2x2,3x3)); V / Mo are [36][t_pad][C], 2.25 values per pixel instead of 4.  Cook-Toom with the interpolation
// points {0, 1, -1, 1/2, -2, inf}: every coefficient of B^T and A^T is a small dyadic rational (exact in fp32) and
// the point set keeps the fp32 error of a 512-deep 3x3 layer at 2.5e-6 of the output scale (the textbook points
// {0, +-1, +-2} give 7e-6, F(2x2) 4e-7, the direct form 2e-7); end to end the detector's scores move by 1.6e-6 and
// its mask probabilities by 2e-5 (tests/test_hip_e2e.py holds them to 1e-4).
//   B^T = [ 1 -3/2  -2   3/2   1   0 ]      A^T = [ 1  1   1   1     1   0 ]
//         [ 0  -1   1/2  5/2   1   0 ]            [ 0  1  -1   1/2  -2   0 ]
//         [ 0   1  -5/2  1/2   1   0 ]            [ 0  1   1   1/4   4   0 ]
//         [ 0  -2   -1    2    1   0 ]            [ 0  1  -1   1/8  -8   1 ]
//         [ 0  1/2  -1  -1/2   1   0 ]
//         [ 0   1  -3/2  -2   3/2  1 ]      (G, with thirds and fifteenths, is applied to the weights on the host in fp64)
// Tile t = (img * ty + y) * tx + x covers outputs [4y, 4y+4) x [4x, 4x+4) and reads inputs [4y-1, 4y+5) x [4x-1, 4x+5).
// ------------------------------------------------------------------------------------------------
// The F(4x4) transform kernels are templated on the channel vector width VEC of a thread (1, 2 or 4 floats): a thread owns
// (tile, VEC channels), loads the 6x6 patch / the 36 products and stores 36 / 16 values.  Most layers of an episode
// are small (70 k .. 800 k (tile, channel) elements): with 16-byte vectors they start 17 k .. 200 k threads on a chip
// that holds 524 k, and the kernel is a chain of dependent memory round trips - latency-bound at 2 TB/s.  With one
// channel per thread the same layer runs 4x the waves (a wave still moves 256 contiguous bytes per instruction) at a
// quarter of the registers; 16-byte vectors remain for the launches that fill the chip anyway (batched AG-RPN maps).
template <int V>
struct VF {
    typedef float type __attribute__((ext_vector_type(V)));
};
template <int V>
using vf = typename VF<V>::type;

template <int V>
__device__ __forceinline__ vf<V> vfma(float k, vf<V> a, vf<V> acc) {
    vf<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = fmaf(k, a[i], acc[i]);
    return r;
}
// The in_scale product a * s, rounded on its own: contracted into the first difference of wg4_bt (fma(d3, s, -(d1 * s)))
// it leaves x s - round(x s) where equal inputs must cancel to exactly 0 (tests/test_hip_wg_bound.py, the guided case).
template <int V>
__device__ __forceinline__ vf<V> vmul_rn(vf<V> a, vf<V> s) {
#pragma clang fp contract(off)
    return a * s;
}
template <int V>
__device__ __forceinline__ vf<V> vzero() {
    vf<V> r;
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = 0.f;
    return r;
}
template <int V>
__device__ __forceinline__ vf<V> vrelu(vf<V> a) {
#pragma unroll
    for (int i = 0; i < V; ++i) a[i] = fmaxf(a[i], 0.f);
    return a;
}
// r = B^T d for one column / row of six
template <int V>
__device__ __forceinline__ void wg4_bt(const vf<V> (&d)[6], vf<V> (&r)[6]) {
    r[0] = (vfma<V>(1.5f, d[3] - d[1], vfma<V>(-2.f, d[2], d[0]))) + d[4];
    r[1] = vfma<V>(2.5f, d[3], vfma<V>(0.5f, d[2], d[4] - d[1]));
    r[2] = vfma<V>(0.5f, d[3], vfma<V>(-2.5f, d[2], d[1] + d[4]));
    r[3] = vfma<V>(2.f, d[3] - d[1], d[4] - d[2]);
    r[4] = vfma<V>(0.5f, d[1] - d[3], d[4] - d[2]);
    r[5] = (vfma<V>(1.5f, d[4] - d[2], vfma<V>(-2.f, d[3], d[1]))) + d[5];
}
// r = A^T m for one column / row of six -> four
template <int V>
__device__ __forceinline__ void wg4_at(const vf<V> (&m)[6], vf<V> (&r)[4]) {
    const vf<V> s12 = m[1] + m[2], d12 = m[1] - m[2];
    r[0] = (m[0] + s12) + (m[3] + m[4]);
    r[1] = vfma<V>(-2.f, m[4], vfma<V>(0.5f, m[3], d12));
    r[2] = vfma<V>(4.f, m[4], vfma<V>(0.25f, m[3], s12));
    r[3] = (vfma<V>(-8.f, m[4], vfma<V>(0.125f, m[3], d12))) + m[5];
}

// A second tensor (`seg`: its own image count and size, no input scale, no device count) may follow the first in the
// tile index space - tiles [tiles0, ...) of V: the query and the support maps of one backbone layer share one launch.
struct WgSeg {
    const float* x;       // second input / output tensor (nullptr: none)
    int n_img, H, W, ty, tx;
    int tiles0;           // tiles of the first tensor
};

template <int V, bool EAGER>
__global__ __launch_bounds__(256) void wg4_input_kernel(const float* __restrict__ x_, const float* __restrict__ in_scale_,
                                                        float* __restrict__ V_, const int32_t* __restrict__ n_img_dev,
                                                        int n_img, int a_img_div, int H, int W, int CV, int ty, int tx,
                                                        int t_pad, long long total, const WgSeg seg) {
    typedef vf<V> T;
    const T* __restrict__ x = reinterpret_cast<const T*>(x_);
    const T* __restrict__ in_scale = reinterpret_cast<const T*>(in_scale_);
    T* __restrict__ Vo = reinterpret_cast<T*>(V_);
    if (n_img_dev) n_img = min(n_img, *n_img_dev);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        const int t = (int)(i / CV);
        const bool second = seg.x && t >= seg.tiles0;
        if (second) {
            x = reinterpret_cast<const T*>(seg.x);
            H = seg.H; W = seg.W; ty = seg.ty; tx = seg.tx; n_img = seg.n_img; a_img_div = 1;
        }
        const int tl = second ? t - seg.tiles0 : t;
        const int xx = tl % tx;
        const int r = tl / tx;
        const int yy = r % ty;
        const int img = r / ty;
        if (img >= n_img) {
            if (seg.x) continue;
            break;                                    // single tensor: images are the slowest index, nothing is left
        }
        const T* src = x + (size_t)(img / a_img_div) * H * W * CV + c;
        const int iy0 = 4 * yy - 1, ix0 = 4 * xx - 1;
        T s;
        if (in_scale) s = in_scale[(size_t)img * CV + c];
        else {
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] = 1.f;
        }
        T tt[6][6];
        if (EAGER) {
            // all 36 loads are issued before the first use (small layers are latency-bound: six dependent batches
            // of six loads cost six memory round trips)
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const int iy = iy0 + a;
#pragma unroll
                for (int b = 0; b < 6; ++b) {
                    const int ix = ix0 + b;
                    tt[a][b] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                                   ? src[((size_t)iy * W + ix) * CV] : vzero<V>();
                }
            }
#pragma unroll
            for (int b = 0; b < 6; ++b) {             // tt[.][b] = B^T (d * s)[.][b], in place
                T d[6], rr[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) d[a] = vmul_rn<V>(tt[a][b], s);
                wg4_bt<V>(d, rr);
#pragma unroll
                for (int a = 0; a < 6; ++a) tt[a][b] = rr[a];
            }
        } else {
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                const int ix = ix0 + b;
                T d[6], rr[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const int iy = iy0 + a;
                    d[a] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                               ? vmul_rn<V>(src[((size_t)iy * W + ix) * CV], s) : vzero<V>();
                }
                wg4_bt<V>(d, rr);
#pragma unroll
                for (int a = 0; a < 6; ++a) tt[a][b] = rr[a];
            }
        }
        T* dst = Vo + (size_t)t * CV + c;
        const size_t gs = (size_t)t_pad * CV;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            T rr[6];
            wg4_bt<V>(tt[a], rr);                      // (B^T d) B, row a
#pragma unroll
            for (int b = 0; b < 6; ++b) dst[(a * 6 + b) * gs] = rr[b];
        }
    }
}

// Mo [36][t_pad][C] -> y [n_img, H, W, C] = A^T Mo A + shift (ReLU); outputs beyond H / W are dropped
template <int V>
__global__ __launch_bounds__(256) void wg4_output_kernel(const float* __restrict__ Mo_, float* __restrict__ y_,
                                                         const float* __restrict__ shift_,
                                                         const int32_t* __restrict__ n_img_dev, int n_img, int H, int W,
                                                         int CV, int ty, int tx, int t_pad, int relu, long long total,
                                                         const WgSeg seg) {
    typedef vf<V> T;
    const T* __restrict__ Mo = reinterpret_cast<const T*>(Mo_);
    const T* __restrict__ shift = reinterpret_cast<const T*>(shift_);
    T* __restrict__ y = reinterpret_cast<T*>(y_);
    if (n_img_dev) n_img = min(n_img, *n_img_dev);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % CV);
        const int t = (int)(i / CV);
        const bool second = seg.x && t >= seg.tiles0;
        if (second) {
            y = reinterpret_cast<T*>(const_cast<float*>(seg.x));
            H = seg.H; W = seg.W; ty = seg.ty; tx = seg.tx; n_img = seg.n_img;
        }
        const int tl = second ? t - seg.tiles0 : t;
        const int xx = tl % tx;
        const int r = tl / tx;
        const int yy = r % ty;
        const int img = r / ty;
        if (img >= n_img) {
            if (seg.x) continue;
            break;
        }
        const T* src = Mo + (size_t)t * CV + c;
        const size_t gs = (size_t)t_pad * CV;
        T mm[6][6];                                    // all 36 loads in flight at once
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) mm[a][b] = src[(a * 6 + b) * gs];
        T st[4][6];                                    // st[i][b] = (A^T m)[i][b]
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            T m[6], rr[4];
#pragma unroll
            for (int a = 0; a < 6; ++a) m[a] = mm[a][b];
            wg4_at<V>(m, rr);
#pragma unroll
            for (int k = 0; k < 4; ++k) st[k][b] = rr[k];
        }
        const T sh = shift ? shift[c] : vzero<V>();
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int oy = 4 * yy + a;
            T rr[4];
            wg4_at<V>(st[a], rr);
            if (oy >= H) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int ox = 4 * xx + b;
                if (ox >= W) continue;
                T v = rr[b] + sh;
                if (relu) v = vrelu<V>(v);
                y[(((size_t)img * H + oy) * W + ox) * CV + c] = v;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The narrow instances: the same values through a short prologue.  Most layers of an episode start under one wave per
// SIMD, so nothing hides the instructions in front of the first load, and in the kernels above (the wide instances) they
// are many: two 64-bit and three 32-bit divisions per thread, 36 64-bit multiplies for the position addresses, 36 loads
// each under its own bounds branch, and the device count on the way to all of it.  Here
//   - a thread is one (tile, channel vector) of the grid, no loop; every offset is an unsigned 32-bit BYTE offset from a
//     wave-uniform base (the launcher shows that every tensor of the launch ends below 2 GiB, wg4_narrow_fits),
//   - the three divisions (channel vectors, tiles per row, tile rows per image) are a multiply-high each by a constant
//     of the launcher (WgDiv), whatever the channel count,
//   - the two tensors of a WgSeg launch own whole workgroups: which tensor a thread works on is a scalar,
//   - the patch loads go to the clamped coordinate and are issued without a condition, the zero fill is a select behind
//     them; position addresses advance by one add each,
//   - the device count is requested first and compared last: every tile below the capacity n_img loads (x, in_scale and
//     Mo are allocated at capacity), only the stores wait for the count.
// The arithmetic of a (tile, channel vector) - vmul_rn, wg4_bt / wg4_at, the order of the passes, shift, ReLU - is the
// code of the wide instances: the results are the same bytes (tests/test_hip_wg_index.py).
// ------------------------------------------------------------------------------------------------
// n / d for 0 <= n < 2^31 as (n * mul) >> (32 + shift); mul == 0 stands for d == 1.  With L = ceil(log2 d) and
// mul = ceil(2^(31 + L) / d) the quotient is exact: mul * d - 2^(31 + L) < d <= 2^L (Granlund & Montgomery 1994, thm 4.2).
struct WgDiv {
    uint32_t mul, shift;
};
static WgDiv wg_div(uint32_t d) {
    WgDiv r = {0u, 0u};
    if (d > 1) {
        const int L = 32 - __builtin_clz(d - 1);
        r.mul = (uint32_t)(((1ull << (31 + L)) + d - 1) / d);
        r.shift = (uint32_t)(L - 1);
    }
    return r;
}
__device__ __forceinline__ uint32_t wg_quot(uint32_t n, WgDiv d) { return d.mul ? __umulhi(n, d.mul) >> d.shift : n; }

struct WgMap {            // one tensor of a narrow launch
    const float* p;       // x of the input transform / y of the output transform
    int H, W;
    int n_img;            // capacity (logical images)
    uint32_t ty, tx;
    WgDiv dty, dtx;
    uint32_t elems;       // tiles * channel vectors
};
struct WgNarrow {
    WgMap m[2];
    uint32_t blocks0;     // workgroups of tensor 0 (all of them when there is no second tensor)
    uint32_t tiles0;      // tiles of tensor 0 = first tile of tensor 1 in V / Mo
    uint32_t CV;          // channel vectors per pixel
    WgDiv dcv, ddiv;      // by CV, by a_img_div
    uint32_t gs;          // bytes between two positions of V / Mo
};

template <typename T>
__device__ __forceinline__ T wg_ld(const void* base, uint32_t off) {
    return *reinterpret_cast<const T*>(static_cast<const char*>(base) + off);
}
template <typename T>
__device__ __forceinline__ void wg_st(void* base, uint32_t off, T v) {
    *reinterpret_cast<T*>(static_cast<char*>(base) + off) = v;
}

// The device count as a VECTOR load, first in the queue of the patch loads.  As a scalar load it shares the counter of
// the kernel-argument loads, which return out of order: the first late argument would make every wave wait for the
// count in front of its first patch load.  Vector loads return in order, so a wait for any patch covers the count.
__device__ __forceinline__ int wg_count_early(const int32_t* n_img_dev) {
    if (!n_img_dev) return 0x7fffffff;
    const int32_t* p = n_img_dev;
    asm volatile("" : "+v"(p));                        // keep the address in vector registers
    return *p;
}

template <int V>
__global__ __launch_bounds__(256) void wg4_input_narrow_kernel(const WgNarrow P, const float* __restrict__ in_scale,
                                                               float* __restrict__ Vo, const int32_t* __restrict__ n_img_dev) {
    typedef vf<V> T;
    const int dev_count = wg_count_early(n_img_dev);                   // requested now, needed at the stores
    const bool second = blockIdx.x >= P.blocks0;                       // scalar
    const float* __restrict__ x = second ? P.m[1].p : P.m[0].p;
    const int H = second ? P.m[1].H : P.m[0].H, W = second ? P.m[1].W : P.m[0].W;
    const uint32_t ty = second ? P.m[1].ty : P.m[0].ty, tx = second ? P.m[1].tx : P.m[0].tx;
    const WgDiv dty = second ? P.m[1].dty : P.m[0].dty, dtx = second ? P.m[1].dtx : P.m[0].dtx;
    const uint32_t elems = second ? P.m[1].elems : P.m[0].elems;
    const int n_cap = second ? P.m[1].n_img : P.m[0].n_img;
    const uint32_t i = (blockIdx.x - (second ? P.blocks0 : 0u)) * 256u + threadIdx.x;
    if (i >= elems) return;
    const uint32_t tl = wg_quot(i, P.dcv), c = i - tl * P.CV;
    const uint32_t r = wg_quot(tl, dtx), xx = tl - r * tx;
    const uint32_t img = wg_quot(r, dty), yy = r - img * ty;
    const uint32_t t = tl + (second ? P.tiles0 : 0u);
    const uint32_t px = (uint32_t)sizeof(T) * P.CV;                    // bytes of a pixel
    const int iy0 = 4 * (int)yy - 1, ix0 = 4 * (int)xx - 1;
    uint32_t ro[6], co[6];
    bool rok[6], cok[6];
    const uint32_t row0 = wg_quot(img, P.ddiv) * (uint32_t)H;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const int iy = iy0 + a, ix = ix0 + a;
        rok[a] = (unsigned)iy < (unsigned)H;
        cok[a] = (unsigned)ix < (unsigned)W;
        ro[a] = (row0 + (uint32_t)min(max(iy, 0), H - 1)) * (uint32_t)W * px;
        co[a] = (uint32_t)min(max(ix, 0), W - 1) * px + c * (uint32_t)sizeof(T);
    }
    T tt[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) tt[a][b] = wg_ld<T>(x, ro[a] + co[b]);
    T s;
    if (in_scale) s = wg_ld<T>(in_scale, (img * P.CV + c) * (uint32_t)sizeof(T));
    else {
#pragma unroll
        for (int k = 0; k < V; ++k) s[k] = 1.f;
    }
#pragma unroll
    for (int b = 0; b < 6; ++b) {                     // tt[.][b] = B^T (d * s)[.][b], in place
        T d[6], rr[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) d[a] = vmul_rn<V>((rok[a] && cok[b]) ? tt[a][b] : vzero<V>(), s);
        wg4_bt<V>(d, rr);
#pragma unroll
        for (int a = 0; a < 6; ++a) tt[a][b] = rr[a];
    }
    if ((int)img >= min(n_cap, dev_count)) return;
    uint32_t o = (t * P.CV + c) * (uint32_t)sizeof(T);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        T rr[6];
        wg4_bt<V>(tt[a], rr);                          // (B^T d) B, row a
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            wg_st<T>(Vo, o, rr[b]);
            o += P.gs;
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void wg4_output_narrow_kernel(const WgNarrow P, const float* __restrict__ Mo,
                                                                const float* __restrict__ shift,
                                                                const int32_t* __restrict__ n_img_dev, int relu) {
    typedef vf<V> T;
    const int dev_count = wg_count_early(n_img_dev);
    const bool second = blockIdx.x >= P.blocks0;                       // scalar
    float* __restrict__ y = const_cast<float*>(second ? P.m[1].p : P.m[0].p);
    const int H = second ? P.m[1].H : P.m[0].H, W = second ? P.m[1].W : P.m[0].W;
    const uint32_t ty = second ? P.m[1].ty : P.m[0].ty, tx = second ? P.m[1].tx : P.m[0].tx;
    const WgDiv dty = second ? P.m[1].dty : P.m[0].dty, dtx = second ? P.m[1].dtx : P.m[0].dtx;
    const uint32_t elems = second ? P.m[1].elems : P.m[0].elems;
    const int n_cap = second ? P.m[1].n_img : P.m[0].n_img;
    const uint32_t i = (blockIdx.x - (second ? P.blocks0 : 0u)) * 256u + threadIdx.x;
    if (i >= elems) return;
    const uint32_t tl = wg_quot(i, P.dcv), c = i - tl * P.CV;
    const uint32_t t = tl + (second ? P.tiles0 : 0u);
    T mm[6][6];                                        // all 36 loads in flight at once
    {
        uint32_t o = (t * P.CV + c) * (uint32_t)sizeof(T);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) {
                mm[a][b] = wg_ld<T>(Mo, o);
                o += P.gs;
            }
    }
    const T sh = shift ? wg_ld<T>(shift, c * (uint32_t)sizeof(T)) : vzero<V>();
    const uint32_t r = wg_quot(tl, dtx), xx = tl - r * tx;
    const uint32_t img = wg_quot(r, dty), yy = r - img * ty;
    T st[4][6];                                        // st[i][b] = (A^T m)[i][b]
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        T m[6], rr[4];
#pragma unroll
        for (int a = 0; a < 6; ++a) m[a] = mm[a][b];
        wg4_at<V>(m, rr);
#pragma unroll
        for (int k = 0; k < 4; ++k) st[k][b] = rr[k];
    }
    if ((int)img >= min(n_cap, dev_count)) return;
    const uint32_t px = (uint32_t)sizeof(T) * P.CV;
    const uint32_t oy0 = 4u * yy, ox0 = 4u * xx;
    uint32_t orow = ((img * (uint32_t)H + oy0) * (uint32_t)W + ox0) * px + c * (uint32_t)sizeof(T);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        T rr[4];
        wg4_at<V>(st[a], rr);
        if ((int)(oy0 + a) < H) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if ((int)(ox0 + b) >= W) continue;
                T v = rr[b] + sh;
                if (relu) v = vrelu<V>(v);
                wg_st<T>(y, orow + b * px, v);
            }
        }
        orow += (uint32_t)W * px;
    }
}

// Channel vector width of a thread for `elems` = tiles * channels (tile, channel) pairs, and whether the input transform
// issues its 36 loads up front.  Measured on MI355X at the cfg3 layer shapes (tools/wg4_ab.py, r03): loads up front wins
// at every size and width (AG-RPN map 55 -> 36 us at 16-byte vectors, shared_head on 300 RoIs 36 -> 20, layer1 31 -> 14:
// the column-by-column form is a chain of six dependent memory round trips); with it, 8-byte vectors are best or within
// 1.5 us of the best at every layer of an episode (34.0 / 21.7 / 16.5 / 13.7 us on the four large ones, 6-7 us - the
// floor of a launch whose every thread does one load and one store round trip - on the rest); 16-byte vectors are kept
// for launches with several million elements (batched AG-RPN maps).  (The A/B was driven by environment variables, removed
// since: the library reads none.)
// With the narrow instances (tools/wg4_ab.py, the vector width forced through fgn_winograd4_*_ix_f32; us per launch at
// 4 / 8 / 16 bytes, two runs, both within 0.5 us of each other; wide instance at 8 bytes in brackets):
//             input transform               output transform
//   AG-RPN    31.0 / 33.9 / 35.2  (34.5)    25.6 / 25.4 / 26.3  (32.3)
//   300 RoIs  22.2 / 21.3 / 20.0  (21.8)    19.8 / 18.7 / 18.2  (23.0)
//   100 RoIs   9.8 /  8.8 /  8.7   (9.5)     7.4 /  7.5 /  6.5   (9.9)
//   mask 0    14.2 / 16.0 / 13.4  (16.6)     4.4 /  4.3 /  4.8   (6.8)
//   mask 1     6.2 /  5.9 /  7.1   (6.9)     4.5 /  4.4 /  4.8   (6.8)
//   layer3     4.7 /  5.1 /  6.3   (6.9)     4.4 /  4.5 /  4.7   (6.8)
//   layer2     6.5 /  7.9 /  7.7   (9.5)     4.6 /  6.1 /  5.5   (8.3)
//   layer1    11.2 / 12.0 / 13.0  (13.4)     9.9 / 10.4 / 10.9  (13.2)
// 4 bytes now wins the input transform of the backbone layers and the AG-RPN map by 0.4-2.9 us and loses the shared head's
// by 1 us; the winners are not ordered by size, so no threshold on `elems` separates them: the rule stays (8 bytes is
// best or within 1.5 us of the best everywhere but the AG-RPN and mask-0 inputs: 2.9, 2.6).  (profiles/launch_fixed_cost_wg4_widths.txt)
static int wg4_vec(long long elems) { return elems >= (4ll << 20) ? 4 : 2; }
static bool wg4_eager(long long) { return true; }
// vec * 10 + eager of the input transform / vec * 10 of the output transform for a layer (lets a profiler name the
// kernel instance a launch uses)
extern "C" int fgn_winograd4_variant(int tiles_total, int C, int is_output) {
    const int v = wg4_vec((long long)tiles_total * C);
    return v * 10 + ((!is_output && wg4_eager((long long)tiles_total * (C / v))) ? 1 : 0);
}

// Whether the narrow instances can address a launch: every tensor it touches ends below 2 GiB, so a 32-bit byte offset
// reaches each element (the element count is then below 2^31 as well).  From the sizes alone: nothing is allocated.
static bool wg4_narrow_fits(long long imgs0, int H0, int W0, long long imgs1, int H1, int W1, long long n_scale, int C,
                            int t_pad) {
    const long long lim = 0x7fffffffll, cb = 4ll * C;
    return imgs0 * H0 * W0 * cb <= lim && imgs1 * H1 * W1 * cb <= lim && n_scale * cb <= lim && 36ll * t_pad * cb <= lim;
}
static void wg4_map(WgMap& m, const float* p, int n_img, int H, int W, int cv) {
    m.p = p; m.H = H; m.W = W; m.n_img = n_img;
    m.ty = (uint32_t)(H + 3) / 4; m.tx = (uint32_t)(W + 3) / 4;
    m.dty = wg_div(m.ty); m.dtx = wg_div(m.tx);
    m.elems = p ? (uint32_t)n_img * m.ty * m.tx * (uint32_t)cv : 0u;
}
static WgNarrow wg4_narrow(const float* p0, int n_img0, int a_img_div, int H0, int W0, const float* p1, int n_img1, int H1,
                           int W1, int C, int vec, int t_pad, int* grid) {
    WgNarrow P;
    const int cv = C / vec;
    wg4_map(P.m[0], p0, n_img0, H0, W0, cv);
    wg4_map(P.m[1], p1, n_img1, H1, W1, cv);
    P.blocks0 = (P.m[0].elems + 255u) / 256u;
    P.tiles0 = (uint32_t)n_img0 * P.m[0].ty * P.m[0].tx;
    P.CV = (uint32_t)cv;
    P.dcv = wg_div(P.CV);
    P.ddiv = wg_div((uint32_t)a_img_div);
    P.gs = (uint32_t)t_pad * (uint32_t)C * 4u;
    *grid = (int)(P.blocks0 + (P.m[1].elems + 255u) / 256u);
    return P;
}
// THE rule of the launchers below and of fgn_winograd4_index_bits: whether a launch of these sizes runs on the narrow
// instances.  n_img1 = 0: one tensor; input transform: x holds ceil(n_img / a_img_div) images and, with_scale, an
// in_scale of n_img rows is read; output transform: y holds n_img images (a_img_div 1, no scale).  The narrow input
// instances issue their loads up front: a launch that wg4_eager sends to the column-by-column form stays wide.
static bool wg4_takes_narrow(bool is_output, int n_img, int a_img_div, int H, int W, int n_img1, int H1, int W1, int C,
                             int t_pad, bool with_scale, int vec_force) {
    if (a_img_div < 1 || C < 4) return false;
    const long long tiles_all = (long long)n_img * ((H + 3) / 4) * ((W + 3) / 4) + (long long)n_img1 * ((H1 + 3) / 4) * ((W1 + 3) / 4);
    const int vec = vec_force ? vec_force : wg4_vec(tiles_all * C);
    if (!is_output && !wg4_eager(tiles_all * (C / vec))) return false;
    const long long imgs0 = is_output ? n_img : (n_img + a_img_div - 1) / a_img_div;
    return wg4_narrow_fits(imgs0, H, W, n_img1, H1, W1, (!is_output && with_scale) ? n_img : 0, C, t_pad);
}
// The index width a launch of these sizes takes: 32 (narrow instances: wg4_input_narrow_kernel / wg4_output_narrow_kernel)
// or 64 (wide: wg4_input_kernel / wg4_output_kernel).  Arguments as for fgn_winograd4_input_ix_f32 / _output_ix_f32.
extern "C" int fgn_winograd4_index_bits(int n_img, int a_img_div, int H, int W, int n_img1, int H1, int W1, int C, int t_pad,
                                        int with_scale, int is_output) {
    return wg4_takes_narrow(is_output != 0, n_img, a_img_div, H, W, n_img1, H1, W1, C, t_pad, with_scale != 0, 0) ? 32 : 64;
}

#define WG4_IN_LAUNCH(VV, EE)                                                                                          \
    FGN_LAUNCH_TIMED((wg4_input_kernel<VV, EE>), dim3(grid), dim3(256), 0, stream, x, in_scale, V, n_img_dev, n_img,  \
                     a_img_div, H, W, C / VV, ty, tx, t_pad, total, seg)
#define WG4_IN_NARROW(VV)                                                                                              \
    FGN_LAUNCH_TIMED((wg4_input_narrow_kernel<VV>), dim3(ngrid), dim3(256), 0, stream, P, in_scale, V, n_img_dev)

// index_bits: 0 = by the sizes, 32 / 64 = that instance (32 on sizes it cannot address: FGN_ERR_SHAPE);
// vec_force: 0 = wg4_vec's width, 1 / 2 / 4 = that many channels per thread (tools/wg4_ab.py)
static int wg4_input_launch(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev, int n_img,
                            int a_img_div, int H, int W, int C, int t_pad, const float* x1, int n_img1, int H1, int W1,
                            int index_bits, int vec_force, hipStream_t stream) {
    if (!x || !V) return FGN_ERR_ARG;
    if (index_bits != 0 && index_bits != 32 && index_bits != 64) return FGN_ERR_ARG;
    if (vec_force != 0 && vec_force != 1 && vec_force != 2 && vec_force != 4) return FGN_ERR_ARG;
    if (n_img <= 0) return FGN_OK;
    const int ty = (H + 3) / 4, tx = (W + 3) / 4;
    WgSeg seg;
    seg.x = x1; seg.n_img = n_img1; seg.H = H1; seg.W = W1; seg.ty = (H1 + 3) / 4; seg.tx = (W1 + 3) / 4;
    seg.tiles0 = n_img * ty * tx;
    const long long tiles_all = (long long)seg.tiles0 + (x1 ? (long long)n_img1 * seg.ty * seg.tx : 0);
    if (C % 4 != 0 || a_img_div < 1 || H < 1 || W < 1 || tiles_all > t_pad) return FGN_ERR_SHAPE;
    if (x1 && (in_scale || n_img_dev || a_img_div != 1 || n_img1 < 1 || H1 < 1 || W1 < 1)) return FGN_ERR_SHAPE;
    const int vec = vec_force ? vec_force : wg4_vec(tiles_all * C);
    const long long total = tiles_all * (C / vec);
    const bool eager = wg4_eager(total);
    const bool fits = wg4_takes_narrow(false, n_img, a_img_div, H, W, x1 ? n_img1 : 0, H1, W1, C, t_pad, in_scale != nullptr, vec_force);
    if (index_bits == 32 && !fits) return FGN_ERR_SHAPE;
    if (fits && index_bits != 64) {
        int ngrid = 0;
        const WgNarrow P = wg4_narrow(x, n_img, a_img_div, H, W, x1, n_img1, H1, W1, C, vec, t_pad, &ngrid);
        switch (vec) {
            case 1: WG4_IN_NARROW(1); break;
            case 2: WG4_IN_NARROW(2); break;
            default: WG4_IN_NARROW(4); break;
        }
        FGN_LAUNCH_CHECK();
        return FGN_OK;
    }
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 32);
    switch (vec * 10 + (eager ? 1 : 0)) {
        case 11: WG4_IN_LAUNCH(1, true); break;
        case 10: WG4_IN_LAUNCH(1, false); break;
        case 21: WG4_IN_LAUNCH(2, true); break;
        case 20: WG4_IN_LAUNCH(2, false); break;
        case 41: WG4_IN_LAUNCH(4, true); break;
        default: WG4_IN_LAUNCH(4, false); break;
    }
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_winograd4_input_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev,
                                       int n_img, int a_img_div, int H, int W, int C, int t_pad, hipStream_t stream) {
    return wg4_input_launch(x, in_scale, V, n_img_dev, n_img, a_img_div, H, W, C, t_pad, nullptr, 0, 1, 1, 0, 0, stream);
}
// two tensors (e.g. the query map and the support maps of a backbone layer) into consecutive tile ranges of one V
extern "C" int fgn_winograd4_input2_f32(const float* x0, int n_img0, int H0, int W0, const float* x1, int n_img1, int H1,
                                        int W1, float* V, int C, int t_pad, hipStream_t stream) {
    if (!x1) return FGN_ERR_ARG;
    return wg4_input_launch(x0, nullptr, V, nullptr, n_img0, 1, H0, W0, C, t_pad, x1, n_img1, H1, W1, 0, 0, stream);
}
// both forms with the index width and the vector width forced (tests, tools): x1 == nullptr is the one-tensor form
extern "C" int fgn_winograd4_input_ix_f32(const float* x, const float* in_scale, float* V, const int32_t* n_img_dev,
                                          int n_img, int a_img_div, int H, int W, int C, int t_pad, const float* x1,
                                          int n_img1, int H1, int W1, int index_bits, int vec, hipStream_t stream) {
    return wg4_input_launch(x, in_scale, V, n_img_dev, n_img, a_img_div, H, W, C, t_pad, x1, x1 ? n_img1 : 0, x1 ? H1 : 1,
                            x1 ? W1 : 1, index_bits, vec, stream);
}

#define WG4_OUT_LAUNCH(VV)                                                                                             \
    FGN_LAUNCH_TIMED((wg4_output_kernel<VV>), dim3(grid), dim3(256), 0, stream, Mo, y, shift, n_img_dev, n_img, H, W, \
                     C / VV, ty, tx, t_pad, relu, total, seg)
#define WG4_OUT_NARROW(VV)                                                                                             \
    FGN_LAUNCH_TIMED((wg4_output_narrow_kernel<VV>), dim3(ngrid), dim3(256), 0, stream, P, Mo, shift, n_img_dev, relu)

static int wg4_output_launch(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev, int n_img, int H,
                             int W, int C, int t_pad, int relu, float* y1, int n_img1, int H1, int W1, int index_bits,
                             int vec_force, hipStream_t stream) {
    if (!Mo || !y) return FGN_ERR_ARG;
    if (index_bits != 0 && index_bits != 32 && index_bits != 64) return FGN_ERR_ARG;
    if (vec_force != 0 && vec_force != 1 && vec_force != 2 && vec_force != 4) return FGN_ERR_ARG;
    if (n_img <= 0) return FGN_OK;
    const int ty = (H + 3) / 4, tx = (W + 3) / 4;
    WgSeg seg;
    seg.x = y1; seg.n_img = n_img1; seg.H = H1; seg.W = W1; seg.ty = (H1 + 3) / 4; seg.tx = (W1 + 3) / 4;
    seg.tiles0 = n_img * ty * tx;
    const long long tiles_all = (long long)seg.tiles0 + (y1 ? (long long)n_img1 * seg.ty * seg.tx : 0);
    if (C % 4 != 0 || H < 1 || W < 1 || tiles_all > t_pad) return FGN_ERR_SHAPE;
    if (y1 && (n_img_dev || n_img1 < 1 || H1 < 1 || W1 < 1)) return FGN_ERR_SHAPE;
    const int vec = vec_force ? vec_force : wg4_vec(tiles_all * C);
    const long long total = tiles_all * (C / vec);
    const bool fits = wg4_takes_narrow(true, n_img, 1, H, W, y1 ? n_img1 : 0, H1, W1, C, t_pad, false, vec_force);
    if (index_bits == 32 && !fits) return FGN_ERR_SHAPE;
    if (fits && index_bits != 64) {
        int ngrid = 0;
        const WgNarrow P = wg4_narrow(y, n_img, 1, H, W, y1, n_img1, H1, W1, C, vec, t_pad, &ngrid);
        switch (vec) {
            case 1: WG4_OUT_NARROW(1); break;
            case 2: WG4_OUT_NARROW(2); break;
            default: WG4_OUT_NARROW(4); break;
        }
        FGN_LAUNCH_CHECK();
        return FGN_OK;
    }
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 32);
    switch (vec) {
        case 1: WG4_OUT_LAUNCH(1); break;
        case 2: WG4_OUT_LAUNCH(2); break;
        default: WG4_OUT_LAUNCH(4); break;
    }
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

extern "C" int fgn_winograd4_output_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev,
                                        int n_img, int H, int W, int C, int t_pad, int relu, hipStream_t stream) {
    return wg4_output_launch(Mo, y, shift, n_img_dev, n_img, H, W, C, t_pad, relu, nullptr, 0, 1, 1, 0, 0, stream);
}
extern "C" int fgn_winograd4_output2_f32(const float* Mo, const float* shift, float* y0, int n_img0, int H0, int W0,
                                         float* y1, int n_img1, int H1, int W1, int C, int t_pad, int relu,
                                         hipStream_t stream) {
    if (!y1) return FGN_ERR_ARG;
    return wg4_output_launch(Mo, y0, shift, nullptr, n_img0, H0, W0, C, t_pad, relu, y1, n_img1, H1, W1, 0, 0, stream);
}
// both forms with the index width and the vector width forced (tests, tools): y1 == nullptr is the one-tensor form
extern "C" int fgn_winograd4_output_ix_f32(const float* Mo, float* y, const float* shift, const int32_t* n_img_dev,
                                           int n_img, int H, int W, int C, int t_pad, int relu, float* y1, int n_img1,
                                           int H1, int W1, int index_bits, int vec, hipStream_t stream) {
    return wg4_output_launch(Mo, y, shift, n_img_dev, n_img, H, W, C, t_pad, relu, y1, y1 ? n_img1 : 0, y1 ? H1 : 1,
                             y1 ? W1 : 1, index_bits, vec, stream);
}

// ----------------------------------------------------------------------------------------------
// Weight side of the Winograd forms: U[g = a * R + b][co][ci] = sum_ij G[a][i] * w[co][ci][i][j] * G[b][j], R = m + 2,
// computed in fp64 from the fp32 weights and rounded once - the transform `ops.pack_winograd` does with torch ops on
// the host when a model is built.  A training loop re-derives U from the updated master weights after EVERY step
// (fgn_amd.train.Trainer.refresh): there it was ~40 small torch kernels and 300 MB of fp64 intermediates per layer;
// here one launch writes U in place (rows [cout, cout_pad) of a group keep the zeros of the first pack).
// G [R][3] fp64 is handed over by the caller (the host's table is the single definition of the interpolation points).
// ----------------------------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(256) void wg_pack_weights_kernel(const float* __restrict__ w, const double* __restrict__ G,
                                                              float* __restrict__ U, int cout, int cin, int cout_pad) {
    __shared__ double g[R][3];
    if (threadIdx.x < R * 3) g[threadIdx.x / 3][threadIdx.x % 3] = G[threadIdx.x];
    __syncthreads();
    const long long total = (long long)cout * cin;
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < total; q += (long long)gridDim.x * blockDim.x) {
        const int co = (int)(q / cin), ci = (int)(q - (long long)co * cin);
        double k[3][3];
#pragma unroll
        for (int i = 0; i < 9; ++i) k[i / 3][i % 3] = (double)w[q * 9 + i];
        double t[R][3];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int j = 0; j < 3; ++j) t[a][j] = g[a][0] * k[0][j] + g[a][1] * k[1][j] + g[a][2] * k[2][j];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b)
                U[((size_t)(a * R + b) * cout_pad + co) * cin + ci] =
                    (float)(t[a][0] * g[b][0] + t[a][1] * g[b][1] + t[a][2] * g[b][2]);
    }
}

extern "C" int fgn_winograd_pack_weights_f32(const float* w, const double* G, float* U, int cout, int cin, int cout_pad,
                                             int m, hipStream_t stream) {
    if (!w || !G || !U) return FGN_ERR_ARG;
    if ((m != 2 && m != 4) || cout < 1 || cin < 1 || cout_pad < cout) return FGN_ERR_SHAPE;
    const long long total = (long long)cout * cin;
    const int grid = (int)std::min<long long>((total + 255) / 256, 256 * 16);
    if (m == 4)
        hipLaunchKernelGGL(wg_pack_weights_kernel<6>, dim3(grid), dim3(256), 0, stream, w, G, U, cout, cin, cout_pad);
    else
        hipLaunchKernelGGL(wg_pack_weights_kernel<4>, dim3(grid), dim3(256), 0, stream, w, G, U, cout, cin, cout_pad);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}
