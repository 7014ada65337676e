// RoIAlign geometry shared by the forward kernels (spatial.hip) and the adjoint (train_bwd.hip): ONE statement of the
// box transform, the sampling grid, the sample coordinates and the per-axis bilinear weights, so that the backward
// pass distributes a gradient over exactly the pixels - and with exactly the weights - the forward pass read.
// The expressions are macros, not functions: the forward kernels must keep their code byte for byte (an inlined
// function schedules differently), and a macro hands the compiler the statements those kernels always had.
// They must be compiled without mul+add contraction (a fused `y1 + ph * bin_h` moves a sample coordinate by an ulp
// and, next to an integer, to another pixel): spatial.hip is built with -ffp-contract=off, the adjoint sets the pragma.
#pragma once
#include "common.h"

struct AxisSample {
    int lo, hi;
    float l, h;
    bool valid;
};

__device__ __forceinline__ AxisSample axis_sample(float c, int size) {
    AxisSample s;
    s.valid = !(c < -1.0f || c > (float)size);
    if (c <= 0.f) c = 0.f;
    int lo = (int)c;
    int hi;
    if (lo >= size - 1) {
        hi = lo = size - 1;
        c = (float)lo;
    } else {
        hi = lo + 1;
    }
    s.lo = lo; s.hi = hi;
    s.l = c - (float)lo;
    s.h = 1.f - s.l;
    return s;
}

// rois row `roi` (batch_idx, x1, y1, x2, y2) with the names P, spatial_scale, sampling_ratio, aligned in scope ->
// declares b, the box corner x1 / y1, the bin sizes, the sampling grid gh x gw and count = max(gh * gw, 1)
#define FGN_ROI_GEOMETRY(roi)                                                              \
    const int b = (int)roi[0];                                                             \
    const float off = aligned ? 0.5f : 0.f;                                                \
    const float x1 = roi[1] * spatial_scale - off;                                         \
    const float y1 = roi[2] * spatial_scale - off;                                         \
    const float x2 = roi[3] * spatial_scale - off;                                         \
    const float y2 = roi[4] * spatial_scale - off;                                         \
    float rw = x2 - x1, rh = y2 - y1;                                                      \
    if (!aligned) {                                                                        \
        rw = fmaxf(rw, 1.f);                                                               \
        rh = fmaxf(rh, 1.f);                                                               \
    }                                                                                      \
    const float bin_h = rh / (float)P, bin_w = rw / (float)P;                              \
    const int gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / (float)P);        \
    const int gw = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rw / (float)P);        \
    const float count = (float)max(gh * gw, 1);

// where bin p of an axis starts, and the coordinate of its sample i of g
#define FGN_BIN_START(box_start, p, step) ((box_start) + (float)(p) * (step))
#define FGN_SAMPLE_COORD(start, i, step, g) ((start) + ((float)(i) + 0.5f) * (step) / (float)(g))

// declares first, last: the pixels between the two end samples of the g samples of a bin (the samples run upwards
// from the first, or downwards where an aligned box has a negative extent and the grid is fixed: the span lies between
// the two end samples either way).  An empty sampling grid - a box of no extent - has no pixels: last < first.
#define FGN_AXIS_SPAN(start, step, g, size)                                                          \
    int first = 0, last = -1;                                                                        \
    if (g > 0) {                                                                                     \
        const AxisSample s0 = axis_sample(FGN_SAMPLE_COORD(start, 0, step, g), size);                \
        const AxisSample s1 = axis_sample(FGN_SAMPLE_COORD(start, g - 1, step, g), size);            \
        first = min(s0.lo, s1.lo);                                                                   \
        last = max(s0.hi, s1.hi);                                                                    \
    }
