// GroupNorm (+ SiLU) of the diffusion half for MI355X (gfx950), binary16 in and out, fp32 arithmetic in registers;
// Part 10 of include/mi3d.h, which states the contract.  Replaces, per conv(silu(norm(x))) of the stock route, the chain
// x.float() -> var_mean -> addcmul -> silu -> autocast's cast (32 B per element) by two kernels that move 6 B per element,
// and the backward chain (about 48 B per element) by two kernels that move 10 B.
//
// Work decomposition (the same in all four kernels): x is NCHW-contiguous, so a (sample, channel) ROW is HW contiguous
// elements and the rows of a group are adjacent.  Every row is cut into Sc = ceil(HW / kChunk) chunks; one workgroup owns
// one (row, chunk).  A group therefore has S = C/G * Sc chunks, whose partial results lie contiguously in the workspace
// (index (row * Sc + chunk)); B * C * Sc workgroups fill the chip even when B * G = 32.
//
// Kernels (all memory-bound; nothing staged in LDS beyond the cross-wave reduction):
//   k_groupnorm_stats        (row, chunk) -> (count, mean, M2), Chan's merge in the thread (one merge per 16-byte vector,
//                            the vector's own moments by two passes over its 8 registers), in the wave and across waves
//   k_groupnorm_apply<ACT>   merges its group's S triples -> mean, rstd (stored by the group's first workgroup), then
//                            y = act(x * a_c + b_c), a_c = rstd * w_c, b_c = bias_c - mean * a_c, rounded once to binary16
//   k_groupnorm_bwd_sums<ACT>(row, chunk) -> (sum dz, sum dz * x), dz = dy * act'(z) with z recomputed
//   k_groupnorm_bwd<ACT>     merges its group's partial sums, weighted by w_c, into ATen's c2, c3;
//                            dx = rstd * w_c * dz + c2 * x + c3
// No atomics anywhere: every reduction has a fixed order, results are bit-reproducible.
//
// Vector access: a chunk starts (row * HW + chunk * kChunk) elements into the tensor; kChunk is a multiple of 8, so with
// 16-byte aligned base pointers the chunk's misalignment is (row * HW) mod 8 elements.  Up to 7 head elements and up to 7
// tail elements go one by one, the rest as 16-byte vectors.  If any base pointer is not 16-byte aligned the whole chunk
// goes element by element.
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr uint32_t kChunk = 8192;            // elements per (row, chunk): 16 KiB, four 16-byte loads per thread
constexpr uint32_t kMaxGroupElems = 1u << 24;  // counts are carried as fp32: exact up to 2^24

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

struct Mom {
    float n, mean, m2;
};

// Chan et al.: the moments of the union of two disjoint sets
__device__ __forceinline__ Mom merge(Mom a, Mom b) {
    if (b.n == 0.0f) return a;
    if (a.n == 0.0f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean, r = b.n / n;
    return {n, a.mean + d * r, a.m2 + b.m2 + d * d * a.n * r};
}

// Every thread returns the merge of all threads' values: lane 0 of each wave holds its wave's (shfl_down tree), then every
// thread merges the kWaves wave results in the same fixed order.
__device__ __forceinline__ Mom block_merge(Mom v, Mom *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const Mom o = {__shfl_down(v.n, off), __shfl_down(v.mean, off), __shfl_down(v.m2, off)};
        v = merge(v, o);
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    Mom r = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = merge(r, lds[w]);
    return r;
}

__device__ __forceinline__ float2 block_sum2(float2 v, float2 *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v.x += __shfl_down(v.x, off);
        v.y += __shfl_down(v.y, off);
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float2 r = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        r.x += lds[w].x;
        r.y += lds[w].y;
    }
    return r;
}

// The elements [off, off + len) of a tensor, dealt to the workgroup's threads: fs(e) for a single element index e,
// fv(e) for 8 consecutive elements starting at the 16-byte aligned index e.
template <class FV, class FS>
__device__ __forceinline__ void for_span(size_t off, uint32_t len, bool vec_ok, FV fv, FS fs) {
    const uint32_t mis = (uint32_t)(off & 7);
    uint32_t head = vec_ok ? ((8u - mis) & 7u) : len;
    if (head > len) head = len;
    const uint32_t nvec = (len - head) >> 3, tail0 = head + (nvec << 3);
    for (uint32_t i = threadIdx.x; i < head; i += kBlock) fs(off + i);
    for (uint32_t v = threadIdx.x; v < nvec; v += kBlock) fv(off + head + ((size_t)v << 3));
    for (uint32_t i = tail0 + threadIdx.x; i < len; i += kBlock) fs(off + i);
}

struct Shape {
    uint32_t C, HW, G, per, Sc;
};

// what a workgroup owns: row = sample * C + channel, its chunk, and the span of elements
struct Work {
    uint32_t row, chunk, c, bg;  // bg = sample * G + group
    size_t off;
    uint32_t len;
    size_t group_first;  // index of the group's first (row, chunk) in a per-chunk workspace
};

__device__ __forceinline__ Work work_of(const Shape &s) {
    Work w;
    w.row = blockIdx.x / s.Sc;
    w.chunk = blockIdx.x - w.row * s.Sc;
    const uint32_t b = w.row / s.C;
    w.c = w.row - b * s.C;
    const uint32_t g = w.c / s.per;
    w.bg = b * s.G + g;
    const uint32_t start = w.chunk * kChunk;
    w.off = (size_t)w.row * s.HW + start;
    w.len = s.HW - start < kChunk ? s.HW - start : kChunk;
    w.group_first = ((size_t)b * s.C + (size_t)g * s.per) * s.Sc;
    return w;
}

__global__ __launch_bounds__(kBlock) void k_groupnorm_stats(const half_t *__restrict__ x, Shape s, bool vec_ok,
                                                            float *__restrict__ ws) {
    __shared__ Mom lds[kWaves];
    const Work w = work_of(s);
    Mom m = {0.0f, 0.0f, 0.0f};
    for_span(
        w.off, w.len, vec_ok,
        [&](size_t e) {
            const half8 v = *reinterpret_cast<const half8 *>(x + e);
            float f[8], sum = 0.0f, m2 = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                f[i] = (float)v[i];
                sum += f[i];
            }
            const float mu = sum * 0.125f;
#pragma unroll
            for (int i = 0; i < 8; ++i) m2 += (f[i] - mu) * (f[i] - mu);
            m = merge(m, Mom{8.0f, mu, m2});
        },
        [&](size_t e) { m = merge(m, Mom{1.0f, (float)x[e], 0.0f}); });
    m = block_merge(m, lds);
    if (threadIdx.x == 0) {
        float *o = ws + 3 * (size_t)blockIdx.x;
        o[0] = m.n;
        o[1] = m.mean;
        o[2] = m.m2;
    }
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float z) {
    if (ACT == 0) return z;
    return z / (1.0f + expf(-z));
}

// dy * act'(z); silu'(z) = s (1 + z (1 - s)), s = sigmoid(z) (ATen's silu_backward)
template <int ACT>
__device__ __forceinline__ float act_bwd(float dy, float z) {
    if (ACT == 0) return dy;
    const float sg = 1.0f / (1.0f + expf(-z));
    return dy * sg * (1.0f + z * (1.0f - sg));
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_apply(const half_t *__restrict__ x, const float *__restrict__ ws,
                                                            const float *__restrict__ weight,
                                                            const float *__restrict__ bias, Shape s, float eps, bool vec_ok,
                                                            half_t *__restrict__ y, float *__restrict__ mean_out,
                                                            float *__restrict__ rstd_out) {
    __shared__ Mom lds[kWaves];
    const Work w = work_of(s);
    const uint32_t S = s.per * s.Sc;
    const float *t = ws + 3 * w.group_first;
    Mom m = {0.0f, 0.0f, 0.0f};
    for (uint32_t i = threadIdx.x; i < S; i += kBlock) m = merge(m, Mom{t[3 * i], t[3 * i + 1], t[3 * i + 2]});
    m = block_merge(m, lds);
    const float mean = m.mean, rstd = 1.0f / sqrtf(m.m2 / m.n + eps);
    if (threadIdx.x == 0 && w.chunk == 0 && w.c % s.per == 0) {
        mean_out[w.bg] = mean;
        rstd_out[w.bg] = rstd;
    }
    const float a = rstd * weight[w.c], b = bias[w.c] - mean * a;
    for_span(
        w.off, w.len, vec_ok,
        [&](size_t e) {
            const half8 v = *reinterpret_cast<const half8 *>(x + e);
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = (half_t)act_fwd<ACT>(fmaf((float)v[i], a, b));
            *reinterpret_cast<half8 *>(y + e) = o;
        },
        [&](size_t e) { y[e] = (half_t)act_fwd<ACT>(fmaf((float)x[e], a, b)); });
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_bwd_sums(const half_t *__restrict__ x, const half_t *__restrict__ dy,
                                                               const float *__restrict__ mean,
                                                               const float *__restrict__ rstd,
                                                               const float *__restrict__ weight,
                                                               const float *__restrict__ bias, Shape s, bool vec_ok,
                                                               float *__restrict__ partial) {
    __shared__ float2 lds[kWaves];
    const Work w = work_of(s);
    const float mu = mean[w.bg], a = rstd[w.bg] * weight[w.c], b = bias[w.c] - mu * a;
    float2 acc = {0.0f, 0.0f};
    for_span(
        w.off, w.len, vec_ok,
        [&](size_t e) {
            const half8 v = *reinterpret_cast<const half8 *>(x + e);
            const half8 g = *reinterpret_cast<const half8 *>(dy + e);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float xf = (float)v[i], dz = act_bwd<ACT>((float)g[i], fmaf(xf, a, b));
                acc.x += dz;
                acc.y = fmaf(dz, xf, acc.y);
            }
        },
        [&](size_t e) {
            const float xf = (float)x[e], dz = act_bwd<ACT>((float)dy[e], fmaf(xf, a, b));
            acc.x += dz;
            acc.y = fmaf(dz, xf, acc.y);
        });
    acc = block_sum2(acc, lds);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = acc.x;
        partial[2 * (size_t)blockIdx.x + 1] = acc.y;
    }
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_bwd(const half_t *__restrict__ x, const half_t *__restrict__ dy,
                                                          const float *__restrict__ mean, const float *__restrict__ rstd,
                                                          const float *__restrict__ weight, const float *__restrict__ bias,
                                                          const float *__restrict__ partial, Shape s, bool vec_ok,
                                                          half_t *__restrict__ dx) {
    __shared__ float2 lds[kWaves];
    const Work w = work_of(s);
    const uint32_t S = s.per * s.Sc, c0 = w.c - w.c % s.per;
    const float *p = partial + 2 * w.group_first;
    float2 acc = {0.0f, 0.0f};  // (db, ds) of ATen's GroupNorm backward: sums over the group of w_c dz and w_c dz x
    for (uint32_t i = threadIdx.x; i < S; i += kBlock) {
        const float wc = weight[c0 + i / s.Sc];
        acc.x = fmaf(wc, p[2 * i], acc.x);
        acc.y = fmaf(wc, p[2 * i + 1], acc.y);
    }
    acc = block_sum2(acc, lds);
    const float mu = mean[w.bg], r = rstd[w.bg], inv_n = 1.0f / ((float)s.per * (float)s.HW);
    const float c2 = (acc.x * mu - acc.y) * r * r * r * inv_n, c3 = -c2 * mu - acc.x * r * inv_n;
    const float a = r * weight[w.c], b = bias[w.c] - mu * a;
    for_span(
        w.off, w.len, vec_ok,
        [&](size_t e) {
            const half8 v = *reinterpret_cast<const half8 *>(x + e);
            const half8 g = *reinterpret_cast<const half8 *>(dy + e);
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float xf = (float)v[i], dz = act_bwd<ACT>((float)g[i], fmaf(xf, a, b));
                o[i] = (half_t)fmaf(a, dz, fmaf(c2, xf, c3));
            }
            *reinterpret_cast<half8 *>(dx + e) = o;
        },
        [&](size_t e) {
            const float xf = (float)x[e], dz = act_bwd<ACT>((float)dy[e], fmaf(xf, a, b));
            dx[e] = (half_t)fmaf(a, dz, fmaf(c2, xf, c3));
        });
}

inline uint32_t chunks_of(uint32_t HW) { return (HW + kChunk - 1) / kChunk; }

// false = refuse: a null shape, groups that do not divide the channels, a group too large for fp32 counts, or more
// workgroups than a 1-D grid holds
bool make_shape(uint32_t B, uint32_t C, uint32_t HW, uint32_t G, Shape &s, uint32_t &blocks) {
    if (B == 0 || C == 0 || HW == 0 || G == 0 || C % G != 0) return false;
    s.C = C; s.HW = HW; s.G = G; s.per = C / G; s.Sc = chunks_of(HW);
    if ((unsigned long long)s.per * HW > kMaxGroupElems) return false;
    const unsigned long long n = (unsigned long long)B * C * s.Sc;
    if (n > 0x7FFFFFFFull) return false;
    blocks = (uint32_t)n;
    return true;
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

uint32_t mi3d_groupnorm_chunks(uint32_t HW) { return chunks_of(HW); }

int mi3d_groupnorm_stats(const void *x, uint32_t B, uint32_t C, uint32_t HW, uint32_t G, float *ws, void *stream) {
    Shape s;
    uint32_t blocks;
    if (!make_shape(B, C, HW, G, s, blocks) || x == nullptr || ws == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groupnorm_stats, dim3(blocks), dim3(kBlock), 0, as_stream(stream), (const half_t *)x, s,
                       aligned16(x), ws);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_act_forward(const void *x, const float *ws, const float *weight, const float *bias, uint32_t B,
                               uint32_t C, uint32_t HW, uint32_t G, float eps, int act, void *y, float *mean, float *rstd,
                               void *stream) {
    Shape s;
    uint32_t blocks;
    if (!make_shape(B, C, HW, G, s, blocks) || x == nullptr || ws == nullptr || weight == nullptr || bias == nullptr ||
        y == nullptr || mean == nullptr || rstd == nullptr || (act != 0 && act != 1))
        return (int)hipErrorInvalidValue;
    const bool vec_ok = aligned16(x) && aligned16(y);
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_apply<0>, grid, block, 0, st, (const half_t *)x, ws, weight, bias, s, eps, vec_ok,
                           (half_t *)y, mean, rstd);
    else
        hipLaunchKernelGGL(k_groupnorm_apply<1>, grid, block, 0, st, (const half_t *)x, ws, weight, bias, s, eps, vec_ok,
                           (half_t *)y, mean, rstd);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_act_backward_sums(const void *x, const void *dy, const float *mean, const float *rstd,
                                     const float *weight, const float *bias, uint32_t B, uint32_t C, uint32_t HW,
                                     uint32_t G, int act, float *partial, void *stream) {
    Shape s;
    uint32_t blocks;
    if (!make_shape(B, C, HW, G, s, blocks) || x == nullptr || dy == nullptr || mean == nullptr || rstd == nullptr ||
        weight == nullptr || bias == nullptr || partial == nullptr || (act != 0 && act != 1))
        return (int)hipErrorInvalidValue;
    const bool vec_ok = aligned16(x) && aligned16(dy);
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_bwd_sums<0>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, s, vec_ok, partial);
    else
        hipLaunchKernelGGL(k_groupnorm_bwd_sums<1>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, s, vec_ok, partial);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_act_backward(const void *x, const void *dy, const float *mean, const float *rstd, const float *weight,
                                const float *bias, const float *partial, uint32_t B, uint32_t C, uint32_t HW, uint32_t G,
                                int act, void *dx, void *stream) {
    Shape s;
    uint32_t blocks;
    if (!make_shape(B, C, HW, G, s, blocks) || x == nullptr || dy == nullptr || mean == nullptr || rstd == nullptr ||
        weight == nullptr || bias == nullptr || partial == nullptr || dx == nullptr || (act != 0 && act != 1))
        return (int)hipErrorInvalidValue;
    const bool vec_ok = aligned16(x) && aligned16(dy) && aligned16(dx);
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_bwd<0>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, partial, s, vec_ok, (half_t *)dx);
    else
        hipLaunchKernelGGL(k_groupnorm_bwd<1>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, partial, s, vec_ok, (half_t *)dx);
    return (int)hipGetLastError();
}

}  // extern "C"
