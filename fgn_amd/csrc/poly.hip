// COCO polygons as an INPUT, rasterised on the device: almost every non-crowd annotation of COCO holds
// its mask as a list of polygons, which the reference turns into RLE once at dataset build through pycocotools
// (maskUtils.frPyObjects + merge, coco_ds.py:246-263).  Here the vertices go up - a few hundred bytes per instance - and
// the mask is made right where a dense upload would have put its bytes.  The rule is fgn_amd/polygon.py's, bit for bit.
//
// The host rounds the vertices to the 5x grid and makes one record per edge: its start after the flip, its step count,
// major axis, flip, slope s (the one division of an edge, a double) and the index of its first point in its part's path.
// The device only multiplies and adds.  This translation unit is built with -ffp-contract=off: the minor coordinate of
// a point is (int)(start + s * t + .5), a product rounded, then two sums rounded, never an fma.
//
//   poly_crossings_kernel  one workgroup per part.  Threads stride over the path indices j = 1..M-1; each finds its edge
//       by binary search over the part's edge offsets, forms (u, v) for j and j - 1 in closed form and, where u changes,
//       tests the crossing in integers (polygon.crossing_of).  Positions are appended to an LDS list - a wave ballot,
//       one LDS add per wave; the order is irrelevant because the list is sorted next -, the list is padded with
//       0xFFFFFFFF (above every position, so a pad never counts) to the part's capacity, a power of two <= 8192,
//       bitonic-sorted in LDS and written to the part's slice of the scratch buffer, all of it.
//   poly_fill_kernel       the mapping of rle_decode_kernel (mask.hip): one lane per window column, 256 columns per
//       workgroup, 32 rows per blockIdx.y.  For each part of its instance a lane finds the rank of its first position by
//       one binary search over the part's slice and walks down its column; the parity of the rank is the part's bit, the
//       bits of the parts are ORed in one 32-bit word per lane (one bit per row) and stored as bytes 0 / 1 at any
//       alignment; nothing is written behind a window in its row.
//
// Safety: every record field is checked before an index is formed from it, by ONE predicate per record kind that both
// kernels share.  An edge's index stays in its part's range, a position's in [0, capacity), a slice in the scratch; the
// contents of an edge record give at worst wrong bits (integer arithmetic wraps in unsigned, a double is clamped before
// it is converted).  A part whose record is out of range writes nothing and is read by nobody; a mask whose record is
// out of range is written as zeros where its window fits its output, and not at all otherwise.
#include "common.h"

constexpr int POLY_MAX_DIM = 16384;
constexpr int POLY_THREADS = 256;
constexpr int POLY_ROWS = 32;          // window rows per blockIdx.y: one bit each of a lane's word
constexpr int POLY_CAP = 8192;         // positions of one part (32 KB of LDS)
constexpr int POLY_POINTS = 1 << 20;   // path points of one part
constexpr int POLY_REC_INTS = 8;       // mask {h, w, wy, wx, wh, ww, part0, n_parts}
                                       // part {edge0, n_edges, points, ends0, cap, h, w, 0}
                                       // edge {xs, ys, steps, major | flip << 1, s lo, s hi, first, 0}

struct PolyPart {
    int edge0, n_edges, points, ends0, cap, h, w;
    bool ok;
};

__device__ __forceinline__ PolyPart poly_part(const int32_t* __restrict__ parts, int q, int n_edges_all,
                                              long long scratch_len) {
    const int32_t* r = parts + (size_t)q * POLY_REC_INTS;
    PolyPart p{r[0], r[1], r[2], r[3], r[4], r[5], r[6], false};
    p.ok = p.edge0 >= 0 && p.n_edges >= 1 && (long long)p.edge0 + p.n_edges <= n_edges_all && p.points >= 1 &&
           p.points <= POLY_POINTS && p.cap >= 1 && p.cap <= POLY_CAP && (p.cap & (p.cap - 1)) == 0 &&
           p.ends0 >= 0 && (long long)p.ends0 + p.cap <= scratch_len && p.h >= 1 && p.h <= POLY_MAX_DIM && p.w >= 1 &&
           p.w <= POLY_MAX_DIM;
    return p;
}

// point d of the path of edge e -> (u, v); any record contents are safe: unsigned wrap, clamp before conversion
__device__ __forceinline__ void poly_point(const int32_t* __restrict__ e, int d, int& u, int& v) {
    const int steps = e[2], flags = e[3];
    const int t = (flags & 2) ? (int)((unsigned)steps - (unsigned)d) : d;
    const double s = __hiloint2double(e[5], e[4]);
    const int major0 = (flags & 1) ? e[0] : e[1], minor0 = (flags & 1) ? e[1] : e[0];
    double m = (double)minor0 + s * (double)t + .5;            // (contraction is off: product, sum, sum)
    m = fmin(fmax(m, -1073741824.0), 1073741824.0);            // (NaN -> the first bound; never reached by a checked part)
    const int along = (int)((unsigned)major0 + (unsigned)t), across = (int)m;
    u = (flags & 1) ? along : across;
    v = (flags & 1) ? across : along;
}

__global__ __launch_bounds__(POLY_THREADS) void poly_crossings_kernel(const int32_t* __restrict__ parts, int n_parts,
                                                                      const int32_t* __restrict__ edges, int n_edges_all,
                                                                      uint32_t* __restrict__ scratch,
                                                                      long long scratch_len) {
    __shared__ uint32_t list[POLY_CAP];
    __shared__ int count;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const PolyPart p = poly_part(parts, q, n_edges_all, scratch_len);                 // (workgroup-uniform)
    if (!p.ok) return;
    const int32_t* ed = edges + (size_t)p.edge0 * POLY_REC_INTS;
    for (int k = tid; k < p.cap; k += POLY_THREADS) list[k] = 0xffffffffu;
    if (tid == 0) count = 0;
    __syncthreads();
    for (int base = 1; base < p.points; base += POLY_THREADS) {                       // (uniform trip count: the ballot)
        const int j = base + tid;
        bool hit = false;
        uint32_t pos = 0;
        if (j < p.points) {
            // the edge of point j: the last one whose first index is <= j (edge 0 where none is)
            int lo = 0, hi = p.n_edges - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (ed[(size_t)mid * POLY_REC_INTS + 6] <= j) lo = mid;
                else hi = mid - 1;
            }
            const int first = ed[(size_t)lo * POLY_REC_INTS + 6];
            int u1, v1, u0, v0;
            poly_point(ed + (size_t)lo * POLY_REC_INTS, (int)((unsigned)j - (unsigned)first), u1, v1);
            if (j - 1 >= first || lo == 0)
                poly_point(ed + (size_t)lo * POLY_REC_INTS, (int)((unsigned)j - 1u - (unsigned)first), u0, v0);
            else {                                                                    // the last point of the edge before
                const int32_t* pe = ed + (size_t)(lo - 1) * POLY_REC_INTS;
                poly_point(pe, (int)((unsigned)j - 1u - (unsigned)pe[6]), u0, v0);
            }
            if (u1 != u0) {
                const int m = u1 < u0 ? u1 : (int)((unsigned)u1 - 1u);
                const int n = min(v1, v0);
                if (m >= 2 && m % 5 == 2) {
                    const int cx = (m - 2) / 5;
                    if (cx <= p.w - 1) {
                        // floor((n + 2) / 5) clamped to [0, h]: n + 2 < 0 clamps to 0 whatever the quotient rounds to
                        const long long n2 = (long long)n + 2;
                        const int cy = n2 < 0 ? 0 : (int)min(n2 / 5, (long long)p.h);
                        pos = (uint32_t)cx * (uint32_t)p.h + (uint32_t)cy;            // <= (w - 1) * h + h < 2^29
                        hit = true;
                    }
                }
            }
        }
        const unsigned long long votes = __ballot(hit);
        int at = 0;
        if (lane == 0 && votes) at = atomicAdd(&count, __popcll(votes));
        at = __shfl(at, 0);
        if (hit) {
            const int k = at + __popcll(votes & ((1ull << lane) - 1ull));
            if (k >= 0 && k < p.cap) list[k] = pos;                                   // (a count beyond the capacity: dropped)
        }
    }
    __syncthreads();
    for (int size = 2; size <= p.cap; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int k = tid; k < p.cap; k += POLY_THREADS) {
                const int l = k ^ stride;
                if (l > k) {
                    const uint32_t a = list[k], b = list[l];
                    if (((k & size) == 0) == (a > b)) { list[k] = b; list[l] = a; }
                }
            }
            __syncthreads();
        }
    uint32_t* dst = scratch + p.ends0;
    for (int k = tid; k < p.cap; k += POLY_THREADS) dst[k] = list[k];
}

__global__ __launch_bounds__(POLY_THREADS) void poly_fill_kernel(const int32_t* __restrict__ recs,
                                                                 const int32_t* __restrict__ parts, int n_parts,
                                                                 int n_edges_all, const uint32_t* __restrict__ scratch,
                                                                 long long scratch_len, uint8_t* __restrict__ out,
                                                                 long long out_stride, int col_blocks, int max_wh,
                                                                 int max_ww) {
    const int i = blockIdx.x / col_blocks, cb = blockIdx.x - i * col_blocks;          // (workgroup-uniform)
    const int32_t* rec = recs + (size_t)i * POLY_REC_INTS;
    const int h = rec[0], w = rec[1], wy = rec[2], wx = rec[3], wh = rec[4], ww = rec[5], part0 = rec[6], np_ = rec[7];
    uint8_t* dst = out + (size_t)i * (size_t)out_stride;
    const bool window = wh >= 1 && ww >= 1;
    const bool fits = window && (long long)wh * ww <= out_stride;
    const bool ok = fits && h >= 1 && h <= POLY_MAX_DIM && w >= 1 && w <= POLY_MAX_DIM && wy >= 0 && wx >= 0 &&
                    wh <= h - wy && ww <= w - wx && wh <= max_wh && ww <= max_ww && np_ >= 1 && part0 >= 0 &&
                    (long long)part0 + np_ <= n_parts;
    if (!ok) {
        // an out-of-range record reads no part; its window is zeros where it fits the slot (the workgroups of this mask
        // share the bytes), and nothing is written otherwise
        if (!fits) return;
        const long long total = (long long)wh * ww;
        const long long step = (long long)col_blocks * gridDim.y * POLY_THREADS;
        for (long long b = ((long long)blockIdx.y * col_blocks + cb) * POLY_THREADS + threadIdx.x; b < total; b += step)
            dst[b] = 0;
        return;
    }
    const int c = cb * POLY_THREADS + threadIdx.x;                                    // window column of this lane
    const int y0 = blockIdx.y * POLY_ROWS;
    if (c >= ww || y0 >= wh) return;
    const int rows = min(POLY_ROWS, wh - y0);
    const uint32_t p0 = (uint32_t)(wx + c) * (uint32_t)h + (uint32_t)(wy + y0);       // < 2^28
    uint32_t bits = 0;
    for (int q = part0; q < part0 + np_; ++q) {
        const PolyPart p = poly_part(parts, q, n_edges_all, scratch_len);             // (workgroup-uniform)
        if (!p.ok || p.h != h || p.w != w) continue;                                  // (a part nobody wrote is not read)
        const uint32_t* e = scratch + p.ends0;
        int lo = 0, hi = p.cap;                                                       // r = #{j : e[j] <= p0}, in [0, cap]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (e[mid] <= p0) lo = mid + 1;
            else hi = mid;
        }
        int r = lo;
        uint32_t cur = r < p.cap ? e[r] : 0xffffffffu, pp = p0;
        for (int y = 0; y < rows; ++y, ++pp) {
            while (cur <= pp && r < p.cap) {
                ++r;
                cur = r < p.cap ? e[r] : 0xffffffffu;
            }
            bits |= (uint32_t)(r & 1) << y;
        }
    }
    uint8_t* o = dst + (size_t)y0 * ww + c;
    for (int y = 0; y < rows; ++y, o += ww) *o = (uint8_t)((bits >> y) & 1u);
}

extern "C" int fgn_poly_masks_u8(const int32_t* blob, long long blob_ints, int n, int n_parts, int n_edges,
                                 uint32_t* scratch, long long scratch_len, uint8_t* out, long long out_stride_bytes,
                                 int max_wh, int max_ww, hipStream_t stream) {
    if (n < 0 || n_parts < 0 || n_edges < 0 || blob_ints < 0 || scratch_len < 0 || out_stride_bytes < 0 || max_wh < 0 ||
        max_ww < 0 || max_wh > POLY_MAX_DIM || max_ww > POLY_MAX_DIM || scratch_len >= (1ll << 31) ||
        blob_ints < (long long)POLY_REC_INTS * ((long long)n + n_parts + n_edges))
        return FGN_ERR_SHAPE;
    if (n == 0 || max_wh == 0 || max_ww == 0) return FGN_OK;
    if (!blob || !out || (n_parts > 0 && !scratch)) return FGN_ERR_ARG;
    const int col_blocks = cdiv(max_ww, POLY_THREADS);
    if ((long long)n * col_blocks >= (1ll << 24)) return FGN_ERR_SHAPE;     // (grid.x * POLY_THREADS stays below 2^32)
    const int32_t* parts = blob + (size_t)n * POLY_REC_INTS;
    const int32_t* edges = parts + (size_t)n_parts * POLY_REC_INTS;
    if (n_parts > 0) {
        hipLaunchKernelGGL(poly_crossings_kernel, dim3((unsigned)n_parts), dim3(POLY_THREADS), 0, stream, parts, n_parts,
                           edges, n_edges, scratch, scratch_len);
        FGN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(poly_fill_kernel, dim3((unsigned)(n * col_blocks), cdiv(max_wh, POLY_ROWS)), dim3(POLY_THREADS), 0,
                       stream, (const int32_t*)blob, parts, n_parts, n_edges, (const uint32_t*)scratch, scratch_len, out,
                       out_stride_bytes, col_blocks, max_wh, max_ww);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}
