// Optimiser side of a training step over the ~40 parameter tensors of the heads (~26 M elements): the update rules of
// torch.optim.Adam / SGD / Adagrad (single-tensor, non-fused forms), the global gradient norm of
// torch.nn.utils.clip_grad_norm_(norm_type=2) and the gradient accumulation of mmcv's GradientCumulativeOptimizerHook.
// All of it is bandwidth-bound element-wise work; every kernel follows adagrad_multi_kernel (train_bwd.hip): a table of
// up to 64 tensors travels as a kernel argument, block b works on 4096-element chunk b of the concatenation of the
// tensors, empty tensors take no slot and a longer list continues in the next launch where the previous one stopped.
//
// This translation unit is compiled with -ffp-contract=off: the arithmetic is as written, one rounding per operation
// (fp32 division and sqrtf are correctly rounded), which is what the rounding counts of tests/test_hip_optim.py rest on.
//
// Inside a chunk thread t (of 256) owns elements 1024 j + 4 t + {0,1,2,3}, j = 0..3.  A full chunk whose pointers are all
// 16-byte aligned moves them as float4 (16 B per lane, 1 KiB per wave instruction); a tail chunk or a misaligned tensor
// walks the SAME assignment element by element, so a reduction adds the same numbers in the same order on either path.
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

constexpr int OPT_MAX_TENSORS = 64;
constexpr int OPT_CHUNK = 4096;
constexpr int OPT_THREADS = 256;

enum OptRule { RULE_ADAGRAD = 0, RULE_ADAM = 1, RULE_SGD = 2 };

struct OptTable {                                   // 4 x 512 + 512 + 260 + 256 + 4 = 3080 B of the 4 KB argument space
    float* p[OPT_MAX_TENSORS];
    const float* g[OPT_MAX_TENSORS];
    float* s1[OPT_MAX_TENSORS];                     // Adagrad sum | Adam exp_avg | SGD momentum_buffer (null: no momentum)
    float* s2[OPT_MAX_TENSORS];                     // Adam exp_avg_sq
    long long n[OPT_MAX_TENSORS];
    int first_chunk[OPT_MAX_TENSORS + 1];
    float lr[OPT_MAX_TENSORS];                      // Adam: lr / (1 - beta1^t), formed on the host in double
    int count;
};

struct VecTable {                                   // gradient norm (a unused) and accumulation
    float* a[OPT_MAX_TENSORS];
    const float* g[OPT_MAX_TENSORS];
    long long n[OPT_MAX_TENSORS];
    int first_chunk[OPT_MAX_TENSORS + 1];
    int count;
};

struct OptHyper {
    float wd, eps;
    float b1, omb1, b2, omb2, rsq_bc2;              // Adam: beta, 1 - beta (host-formed), sqrt(1 - beta2^t)
    float mu;                                       // SGD momentum
    int nesterov;
    float gscale;                                   // host part of the gradient multiplier
    int use_mul;                                    // 0: the gradient is used as it is (coef null and gscale == 1)
};

template <class T>
__device__ __forceinline__ int find_tensor(const T& t, int chunk) {
    int k = 0;
    while (k + 1 < t.count && t.first_chunk[k + 1] <= chunk) ++k;          // block-uniform, <= 64 steps over SGPRs
    return k;
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// One element of one rule.  g' = g * mul + wd p (the product only where a multiplier is set).
template <int RULE>
__device__ __forceinline__ void update_one(float& p, float g, float& s1, float& s2, float lr, float mul, const OptHyper& h,
                                           bool has_s1) {
    if (h.use_mul) g = g * mul;
    const float gv = g + h.wd * p;
    if (RULE == RULE_ADAGRAD) {
        const float st = s1 + gv * gv;
        s1 = st;
        p = p - lr * gv / (sqrtf(st) + h.eps);
    } else if (RULE == RULE_ADAM) {
        const float m = h.b1 * s1 + h.omb1 * gv;
        const float v = h.b2 * s2 + h.omb2 * (gv * gv);
        s1 = m;
        s2 = v;
        p = p - lr * m / (sqrtf(v) / h.rsq_bc2 + h.eps);
    } else {
        float buf = gv;
        if (has_s1) {
            buf = h.mu * s1 + gv;
            s1 = buf;
        }
        p = p - lr * (h.nesterov ? gv + h.mu * buf : buf);
    }
}

template <int RULE>
__global__ __launch_bounds__(OPT_THREADS) void optim_multi_kernel(const OptTable t, const OptHyper h,
                                                                  const float* __restrict__ coef) {
    const int chunk = blockIdx.x;
    const int k = find_tensor(t, chunk);
    const long long base = (long long)(chunk - t.first_chunk[k]) * OPT_CHUNK;
    float* __restrict__ p = t.p[k];
    const float* __restrict__ g = t.g[k];
    float* __restrict__ s1 = t.s1[k];
    float* __restrict__ s2 = t.s2[k];
    const long long n = t.n[k];
    const float lr = t.lr[k];
    const bool has_s1 = s1 != nullptr, has_s2 = RULE == RULE_ADAM;
    float mul = h.gscale;
    if (coef) mul = coef[0] * h.gscale;             // one rounding; with gscale == 1 the coefficient itself
    const bool vec = base + OPT_CHUNK <= n && aligned16(p) && aligned16(g) && (!has_s1 || aligned16(s1)) &&
                     (!has_s2 || aligned16(s2));
    if (vec) {
#pragma unroll
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j) {
            const long long i = base + j * (4 * OPT_THREADS) + 4 * threadIdx.x;
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 a = has_s1 ? *reinterpret_cast<const float4*>(s1 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 b = has_s2 ? *reinterpret_cast<const float4*>(s2 + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            update_one<RULE>(pv.x, gv.x, a.x, b.x, lr, mul, h, has_s1);
            update_one<RULE>(pv.y, gv.y, a.y, b.y, lr, mul, h, has_s1);
            update_one<RULE>(pv.z, gv.z, a.z, b.z, lr, mul, h, has_s1);
            update_one<RULE>(pv.w, gv.w, a.w, b.w, lr, mul, h, has_s1);
            *reinterpret_cast<float4*>(p + i) = pv;
            if (has_s1) *reinterpret_cast<float4*>(s1 + i) = a;
            if (has_s2) *reinterpret_cast<float4*>(s2 + i) = b;
        }
    } else {
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j)
            for (int e = 0; e < 4; ++e) {
                const long long i = base + j * (4 * OPT_THREADS) + 4 * threadIdx.x + e;
                if (i >= n) continue;
                float pv = p[i], a = has_s1 ? s1[i] : 0.f, b = has_s2 ? s2[i] : 0.f;
                update_one<RULE>(pv, g[i], a, b, lr, mul, h, has_s1);
                p[i] = pv;
                if (has_s1) s1[i] = a;
                if (has_s2) s2[i] = b;
            }
    }
}

// acc = (first ? 0 : acc) + a g
__global__ __launch_bounds__(OPT_THREADS) void grad_accumulate_multi_kernel(const VecTable t, float a, int first) {
    const int chunk = blockIdx.x;
    const int k = find_tensor(t, chunk);
    const long long base = (long long)(chunk - t.first_chunk[k]) * OPT_CHUNK;
    float* __restrict__ acc = t.a[k];
    const float* __restrict__ g = t.g[k];
    const long long n = t.n[k];
    if (base + OPT_CHUNK <= n && aligned16(acc) && aligned16(g)) {
#pragma unroll
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j) {
            const long long i = base + j * (4 * OPT_THREADS) + 4 * threadIdx.x;
            const float4 gv = *reinterpret_cast<const float4*>(g + i);
            float4 r = make_float4(a * gv.x, a * gv.y, a * gv.z, a * gv.w);
            if (!first) {
                const float4 o = *reinterpret_cast<const float4*>(acc + i);
                r = make_float4(o.x + r.x, o.y + r.y, o.z + r.z, o.w + r.w);
            }
            *reinterpret_cast<float4*>(acc + i) = r;
        }
    } else {
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j)
            for (int e = 0; e < 4; ++e) {
                const long long i = base + j * (4 * OPT_THREADS) + 4 * threadIdx.x + e;
                if (i >= n) continue;
                const float r = a * g[i];
                acc[i] = first ? r : acc[i] + r;
            }
    }
}

// Stage 1 of the norm: partial[chunk0 + b] = sum of the squares of chunk b in fp64 (a square of an fp32 is exact there).
// Fixed order: a thread adds its 16 elements in ascending index, the 64 lanes of a wave combine in an xor butterfly,
// thread 0 adds the 4 wave sums in wave order.
__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_partial_kernel(const VecTable t, double* __restrict__ partial,
                                                                          int chunk0) {
    __shared__ double wave_sum[OPT_THREADS / 64];
    const int chunk = blockIdx.x;
    const int k = find_tensor(t, chunk);
    const long long base = (long long)(chunk - t.first_chunk[k]) * OPT_CHUNK;
    const float* __restrict__ g = t.g[k];
    const long long n = t.n[k];
    double acc = 0.0;
    if (base + OPT_CHUNK <= n && aligned16(g)) {
#pragma unroll
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j) {
            const float4 v = *reinterpret_cast<const float4*>(g + base + j * (4 * OPT_THREADS) + 4 * threadIdx.x);
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    } else {
        for (int j = 0; j < OPT_CHUNK / (4 * OPT_THREADS); ++j)
            for (int e = 0; e < 4; ++e) {
                const long long i = base + j * (4 * OPT_THREADS) + 4 * threadIdx.x + e;
                const double v = i < n ? (double)g[i] : 0.0;
                acc += v * v;
            }
    }
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < OPT_THREADS / 64; ++w) s += wave_sum[w];
        partial[chunk0 + chunk] = s;
    }
}

// Stage 2, one block: thread t adds partials t, t + 256, ... in index order, then the same fixed butterfly and wave order.
// out = {norm, coef}: norm = (float)(sqrt(sum) * grad_scale) (one rounding), coef = min(1, max_norm / (norm + 1e-6)) in fp32 as clip_grad_norm_ forms
// it; a NaN passes through the comparison (torch.clamp keeps NaN, fminf would not).
__global__ __launch_bounds__(OPT_THREADS) void grad_sqnorm_final_kernel(const double* __restrict__ partial, int count,
                                                                        float max_norm, float grad_scale,
                                                                        float* __restrict__ out) {
    __shared__ double wave_sum[OPT_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < count; i += OPT_THREADS) acc += partial[i];
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wave_sum[0];
        for (int w = 1; w < OPT_THREADS / 64; ++w) s += wave_sum[w];
        const float norm = (float)(sqrt(s) * (double)grad_scale);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.f ? 1.f : c;
    }
}

}  // namespace

// rule: 0 Adagrad (state1 = sum), 1 Adam (state1 = exp_avg, state2 = exp_avg_sq; h0 = beta1, h1 = beta2, bc1 = 1 - beta1^t,
// bc2 = 1 - beta2^t), 2 SGD (state1 = momentum_buffer or a null list when h0 = momentum is 0; flags bit 0: Nesterov).
// The gradient enters as g * (coef ? *coef * grad_scale : grad_scale); with coef null and grad_scale 1 as it is.
extern "C" int fgn_optim_multi_f32(int rule, float* const* params, const float* const* grads, float* const* state1,
                                   float* const* state2, const long long* n, const float* lr, int count, float weight_decay,
                                   float eps, float h0, float h1, double bc1, double bc2, int flags, const float* coef,
                                   float grad_scale, hipStream_t stream) {
    if (rule != RULE_ADAGRAD && rule != RULE_ADAM && rule != RULE_SGD) return FGN_ERR_ARG;
    if (count < 0 || (count > 0 && (!params || !grads || !n || !lr))) return FGN_ERR_ARG;
    const bool need1 = rule == RULE_ADAGRAD || rule == RULE_ADAM || (rule == RULE_SGD && h0 != 0.f);
    const bool need2 = rule == RULE_ADAM;
    if (count > 0 && ((need1 && !state1) || (need2 && !state2))) return FGN_ERR_ARG;
    if (rule == RULE_ADAM && !(bc1 > 0.0 && bc2 > 0.0)) return FGN_ERR_ARG;
    OptHyper h = {};
    h.wd = weight_decay;
    h.eps = eps;
    h.gscale = grad_scale;
    h.use_mul = (coef != nullptr || grad_scale != 1.f) ? 1 : 0;
    if (rule == RULE_ADAM) {
        h.b1 = h0; h.omb1 = 1.f - h0;
        h.b2 = h1; h.omb2 = 1.f - h1;
        h.rsq_bc2 = (float)sqrt(bc2);
    } else if (rule == RULE_SGD) {
        h.mu = h0;
        h.nesterov = flags & 1;
    }
    int i = 0;
    while (i < count) {
        OptTable t;
        t.count = 0;
        int chunks = 0;
        for (; i < count && t.count < OPT_MAX_TENSORS; ++i) {
            if (n[i] <= 0) continue;
            if (!params[i] || !grads[i] || (need1 && !state1[i]) || (need2 && !state2[i])) return FGN_ERR_ARG;
            const int k = t.count++;
            t.p[k] = params[i]; t.g[k] = grads[i];
            t.s1[k] = need1 ? state1[i] : nullptr;
            t.s2[k] = need2 ? state2[i] : nullptr;
            t.n[k] = n[i];
            t.lr[k] = rule == RULE_ADAM ? (float)((double)lr[i] / bc1) : lr[i];
            t.first_chunk[k] = chunks;
            chunks += (int)((n[i] + OPT_CHUNK - 1) / OPT_CHUNK);
        }
        t.first_chunk[t.count] = chunks;
        if (t.count == 0) continue;
        if (rule == RULE_ADAGRAD)
            hipLaunchKernelGGL(optim_multi_kernel<RULE_ADAGRAD>, dim3(chunks), dim3(OPT_THREADS), 0, stream, t, h, coef);
        else if (rule == RULE_ADAM)
            hipLaunchKernelGGL(optim_multi_kernel<RULE_ADAM>, dim3(chunks), dim3(OPT_THREADS), 0, stream, t, h, coef);
        else
            hipLaunchKernelGGL(optim_multi_kernel<RULE_SGD>, dim3(chunks), dim3(OPT_THREADS), 0, stream, t, h, coef);
        FGN_LAUNCH_CHECK();
    }
    return FGN_OK;
}

// out[0] = grad_scale * ||concat(grads)||_2 (the norm of the rescaled gradient), out[1] = min(1, max_norm / (out[0] + 1e-6)).  partials: fp64 scratch of
// partials_capacity >= sum_i ceil(n_i / 4096) entries.  No atomics, no host synchronisation: the same input gives the
// same bits on every run.
extern "C" int fgn_grad_sqnorm_multi_f32(const float* const* grads, const long long* n, int count, float max_norm,
                                         float grad_scale, double* partials, long long partials_capacity, float* out,
                                         hipStream_t stream) {
    if (count < 0 || (count > 0 && (!grads || !n)) || !out || !(max_norm >= 0.f) || !(grad_scale >= 0.f))
        return FGN_ERR_ARG;
    long long total = 0;
    for (int i = 0; i < count; ++i)
        if (n[i] > 0) total += (n[i] + OPT_CHUNK - 1) / OPT_CHUNK;
    if (total > partials_capacity || total > 0x7fffffffLL) return FGN_ERR_SHAPE;
    if (total > 0 && !partials) return FGN_ERR_ARG;
    int i = 0, chunk0 = 0;
    while (i < count) {
        VecTable t;
        t.count = 0;
        int chunks = 0;
        for (; i < count && t.count < OPT_MAX_TENSORS; ++i) {
            if (n[i] <= 0) continue;
            if (!grads[i]) return FGN_ERR_ARG;
            const int k = t.count++;
            t.a[k] = nullptr; t.g[k] = grads[i]; t.n[k] = n[i];
            t.first_chunk[k] = chunks;
            chunks += (int)((n[i] + OPT_CHUNK - 1) / OPT_CHUNK);
        }
        t.first_chunk[t.count] = chunks;
        if (t.count == 0) continue;
        hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(chunks), dim3(OPT_THREADS), 0, stream, t, partials, chunk0);
        FGN_LAUNCH_CHECK();
        chunk0 += chunks;
    }
    hipLaunchKernelGGL(grad_sqnorm_final_kernel, dim3(1), dim3(OPT_THREADS), 0, stream, partials, chunk0, max_norm,
                       grad_scale, out);
    FGN_LAUNCH_CHECK();
    return FGN_OK;
}

// accs[i] = (first ? 0 : accs[i]) + a * grads[i]
extern "C" int fgn_grad_accumulate_multi_f32(float* const* accs, const float* const* grads, const long long* n, int count,
                                             float a, int first, hipStream_t stream) {
    if (count < 0 || (count > 0 && (!accs || !grads || !n))) return FGN_ERR_ARG;
    int i = 0;
    while (i < count) {
        VecTable t;
        t.count = 0;
        int chunks = 0;
        for (; i < count && t.count < OPT_MAX_TENSORS; ++i) {
            if (n[i] <= 0) continue;
            if (!accs[i] || !grads[i]) return FGN_ERR_ARG;
            const int k = t.count++;
            t.a[k] = accs[i]; t.g[k] = grads[i]; t.n[k] = n[i];
            t.first_chunk[k] = chunks;
            chunks += (int)((n[i] + OPT_CHUNK - 1) / OPT_CHUNK);
        }
        t.first_chunk[t.count] = chunks;
        if (t.count == 0) continue;
        hipLaunchKernelGGL(grad_accumulate_multi_kernel, dim3(chunks), dim3(OPT_THREADS), 0, stream, t, a, first ? 1 : 0);
        FGN_LAUNCH_CHECK();
    }
    return FGN_OK;
}
