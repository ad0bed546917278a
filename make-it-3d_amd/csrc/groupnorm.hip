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
//
// The same four kernels for channels-last tensors ([B][HW][C], k_groupnorm_nhwc_*) follow the NCHW ones below, with
// their own decomposition (spans of whole pixels x slabs of whole groups) described there.
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

// ------------------------------------------------------------------------------------------------ NHWC (channels-last)
// x is [B][HW][C] with C contiguous and C % 8 == 0, so every 16-byte vector holds 8 channels of one pixel.  The channels
// are cut into SLABS of whole groups, slabC = the smallest multiple of lcm(C/G, 8) that is >= 64 channels (128 bytes of a
// pixel; the last slab may be shorter), and a sample's pixels into Sc spans of P whole pixels: one workgroup owns one
// (sample, span, slab).  Its threads form a (pixel row, vector) tile - vt = slabC / 8 vectors wide, 256 / vt pixels high -
// that walks down the span, so a thread keeps the same 8 channels throughout and carries their 8 partial results in
// registers.  The partials are folded per channel over the tile's rows through LDS, then per group over the group's
// channels (a vector of 8 may straddle two groups - 10 or 20 channels per group - which is why the fold is per channel
// first), both with the k-set form of Chan's merge: mean = sum n_i mean_i / n, M2 = sum M2_i + sum n_i (mean_i - mean)^2.
// The workspaces hold one entry per (sample, span, group); the second kernel of each direction merges its slab's groups
// over the Sc spans, at most kNhwcMerge entries per workgroup.  Orders are fixed everywhere, there are no atomics.
constexpr uint32_t kNhwcChunk = 8192;     // elements per workgroup aimed at, as kChunk
constexpr uint32_t kNhwcMerge = 4096;     // entries (groups of the slab x spans) a workgroup of the second kernel merges
constexpr uint32_t kNhwcRatio = 16;       // elements of a workgroup per workspace entry it merges, at least
constexpr uint32_t kNhwcMaxSlab = 2048;   // channels per slab the LDS fold buffers hold (256 threads x 8 channels)

struct NShape {
    uint32_t C, HW, G, per, slabC, nslab, P, Sc, tpg;  // tpg: threads per group in the merge over spans, a power of two
};

struct NWork {
    uint32_t b, span, c0, nc, g0, ng, len;  // the slab's first channel / channel count / first group / group count
    size_t off;                             // element index of (sample, first pixel of the span, c0)
    size_t entry0;                          // workspace entry of (sample, span 0, group 0)
};

__device__ __forceinline__ NWork nwork_of(const NShape &s) {
    NWork w;
    const uint32_t slab = blockIdx.x % s.nslab, rest = blockIdx.x / s.nslab;
    w.b = rest / s.Sc;
    w.span = rest - w.b * s.Sc;
    w.c0 = slab * s.slabC;
    w.nc = s.C - w.c0 < s.slabC ? s.C - w.c0 : s.slabC;
    w.g0 = w.c0 / s.per;
    w.ng = w.nc / s.per;
    const uint32_t p0 = w.span * s.P;
    w.len = s.HW - p0 < s.P ? s.HW - p0 : s.P;
    w.off = ((size_t)w.b * s.HW + p0) * s.C + w.c0;
    w.entry0 = (size_t)w.b * s.Sc * s.G;
    return w;
}

// the thread's place in the (pixel row, vector) tile; rows r >= rows own nothing
struct NTile {
    uint32_t vt, rows, tc, r;
    bool active;
};

__device__ __forceinline__ NTile ntile_of(const NWork &w) {
    NTile t;
    t.vt = w.nc >> 3;
    t.rows = kBlock / t.vt;
    t.r = threadIdx.x / t.vt;
    t.tc = threadIdx.x - t.r * t.vt;
    t.active = t.r < t.rows;
    return t;
}

// pixels of a span of len that row r of a tile with `rows` rows visits: r, r + rows, ...
__device__ __forceinline__ float row_count(uint32_t len, uint32_t r, uint32_t rows) {
    return (float)(len / rows + (r < len % rows ? 1u : 0u));
}

// a_c, b_c and the group mean of the thread's 8 channels c .. c + 7 from the per-group mean / rstd (indexed by
// group - g_base)
__device__ __forceinline__ void chan_affine(const float (&wv)[8], const float (&bv)[8], const float *mean,
                                            const float *rstd, uint32_t c, uint32_t per, uint32_t g_base, float (&a)[8],
                                            float (&b)[8], float (&mu)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t g = (c + i) / per - g_base;
        mu[i] = mean[g];
        a[i] = rstd[g] * wv[i];
        b[i] = bv[i] - mu[i] * a[i];
    }
}

__device__ __forceinline__ void load8(const float *__restrict__ p, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[i];
}

constexpr uint32_t kNhwcPre = 2;  // pixels per thread whose loads the second kernels issue ahead of the merge over spans

__global__ __launch_bounds__(kBlock) void k_groupnorm_nhwc_stats(const half_t *__restrict__ x, NShape s,
                                                                 float *__restrict__ ws) {
    __shared__ float rmean[kNhwcMaxSlab], rm2[kNhwcMaxSlab], cmean[kNhwcMaxSlab], cm2[kNhwcMaxSlab];
    const NWork w = nwork_of(s);
    const NTile t = ntile_of(w);
    if (t.active) {
        float mean[8], m2[8], cnt = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) mean[i] = m2[i] = 0.0f;
        const half_t *px = x + w.off + (t.tc << 3);
#pragma unroll 8
        for (uint32_t p = t.r; p < w.len; p += t.rows) {
            const half8 v = *reinterpret_cast<const half8 *>(px + (size_t)p * s.C);
            cnt += 1.0f;
            const float inv = 1.0f / cnt;
#pragma unroll
            for (int i = 0; i < 8; ++i) {  // Welford: one element joins the channel's set
                const float f = (float)v[i], d = f - mean[i];
                mean[i] += d * inv;
                m2[i] = fmaf(d, f - mean[i], m2[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rmean[t.r * w.nc + (t.tc << 3) + i] = mean[i];
            rm2[t.r * w.nc + (t.tc << 3) + i] = m2[i];
        }
    }
    __syncthreads();
    const float n = (float)w.len;
    for (uint32_t c = threadIdx.x; c < w.nc; c += kBlock) {  // the channel over the tile's rows
        float sum = 0.0f;
#pragma unroll 8
        for (uint32_t r = 0; r < t.rows; ++r) sum = fmaf(row_count(w.len, r, t.rows), rmean[r * w.nc + c], sum);
        const float mu = sum / n;
        float q = 0.0f;
#pragma unroll 8
        for (uint32_t r = 0; r < t.rows; ++r) {
            const float d = rmean[r * w.nc + c] - mu;
            q += fmaf(row_count(w.len, r, t.rows) * d, d, rm2[r * w.nc + c]);
        }
        cmean[c] = mu;
        cm2[c] = q;
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < w.ng; g += kBlock) {  // the group over its channels, all of count n
        float sum = 0.0f;
#pragma unroll 8
        for (uint32_t c = g * s.per; c < (g + 1) * s.per; ++c) sum += cmean[c];
        const float mu = sum / (float)s.per;
        float q = 0.0f;
#pragma unroll 8
        for (uint32_t c = g * s.per; c < (g + 1) * s.per; ++c) {
            const float d = cmean[c] - mu;
            q += fmaf(n * d, d, cm2[c]);
        }
        float *o = ws + 3 * (w.entry0 + (size_t)w.span * s.G + w.g0 + g);
        o[0] = n * (float)s.per;
        o[1] = mu;
        o[2] = q;
    }
}

// The workgroup's threads as (group of the slab, lane j of tpg): the entries of group w.g0 + gl over the spans
// j, j + tpg, ...; four loads in flight per thread.  f(entry index) -> value, acc(value) folds it.
template <class LOAD, class ACC>
__device__ __forceinline__ void over_spans(const NShape &s, const NWork &w, uint32_t gl, uint32_t j, LOAD load, ACC acc) {
    if (gl >= w.ng) return;
    const size_t e0 = w.entry0 + w.g0 + gl;
    for (uint32_t k0 = j; k0 < s.Sc; k0 += 4 * s.tpg) {
        decltype(load((size_t)0, true)) v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            const uint32_t k = k0 + u * s.tpg;
            v[u] = load(e0 + (size_t)(k < s.Sc ? k : 0u) * s.G, k < s.Sc);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) acc(v[u]);
    }
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_nhwc_apply(const half_t *__restrict__ x, const float *__restrict__ ws,
                                                                 const float *__restrict__ weight,
                                                                 const float *__restrict__ bias, NShape s, float eps,
                                                                 half_t *__restrict__ y, float *__restrict__ mean_out,
                                                                 float *__restrict__ rstd_out) {
    __shared__ float gmean[kBlock], grstd[kBlock];
    const NWork w = nwork_of(s);
    const NTile t = ntile_of(w);
    const uint32_t gl = threadIdx.x / s.tpg, j = threadIdx.x - gl * s.tpg;
    const uint32_t c = w.c0 + (t.tc << 3);
    const size_t base = w.off + (t.tc << 3);
    float wv[8], bv[8];
    half8 pre[kNhwcPre];
    if (t.active) {  // issued ahead of the merge: their latency runs beside it
        load8(weight + c, wv);
        load8(bias + c, bv);
#pragma unroll
        for (uint32_t u = 0; u < kNhwcPre; ++u)
            if (t.r + u * t.rows < w.len) pre[u] = *reinterpret_cast<const half8 *>(x + base + (size_t)(t.r + u * t.rows) * s.C);
    }
    Mom m = {0.0f, 0.0f, 0.0f};
    over_spans(
        s, w, gl, j,
        [&](size_t e, bool ok) { return ok ? Mom{ws[3 * e], ws[3 * e + 1], ws[3 * e + 2]} : Mom{0.0f, 0.0f, 0.0f}; },
        [&](Mom v) { m = merge(m, v); });
    for (uint32_t off = s.tpg >> 1; off > 0; off >>= 1) {
        const Mom o = {__shfl_down(m.n, off, s.tpg), __shfl_down(m.mean, off, s.tpg), __shfl_down(m.m2, off, s.tpg)};
        m = merge(m, o);
    }
    if (j == 0 && gl < w.ng) {
        const float mean = m.mean, rstd = 1.0f / sqrtf(m.m2 / m.n + eps);
        gmean[gl] = mean;
        grstd[gl] = rstd;
        if (w.span == 0) {
            mean_out[w.b * s.G + w.g0 + gl] = mean;
            rstd_out[w.b * s.G + w.g0 + gl] = rstd;
        }
    }
    __syncthreads();
    if (!t.active) return;
    float a[8], b[8], mu[8];
    chan_affine(wv, bv, gmean, grstd, c, s.per, w.g0, a, b, mu);
    auto pixel = [&](uint32_t p, half8 v) {
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (half_t)act_fwd<ACT>(fmaf((float)v[i], a[i], b[i]));
        *reinterpret_cast<half8 *>(y + base + (size_t)p * s.C) = o;
    };
#pragma unroll
    for (uint32_t u = 0; u < kNhwcPre; ++u)
        if (t.r + u * t.rows < w.len) pixel(t.r + u * t.rows, pre[u]);
#pragma unroll 8
    for (uint32_t p = t.r + kNhwcPre * t.rows; p < w.len; p += t.rows)
        pixel(p, *reinterpret_cast<const half8 *>(x + base + (size_t)p * s.C));
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_nhwc_bwd_sums(const half_t *__restrict__ x,
                                                                    const half_t *__restrict__ dy,
                                                                    const float *__restrict__ mean,
                                                                    const float *__restrict__ rstd,
                                                                    const float *__restrict__ weight,
                                                                    const float *__restrict__ bias, NShape s,
                                                                    float *__restrict__ partial) {
    __shared__ float rdz[kNhwcMaxSlab], rdzx[kNhwcMaxSlab], cdz[kNhwcMaxSlab], cdzx[kNhwcMaxSlab];
    const NWork w = nwork_of(s);
    const NTile t = ntile_of(w);
    if (t.active) {
        float a[8], b[8], mu[8], sdz[8], sdzx[8];
        float wv[8], bv[8];
        load8(weight + w.c0 + (t.tc << 3), wv);
        load8(bias + w.c0 + (t.tc << 3), bv);
        chan_affine(wv, bv, mean + (size_t)w.b * s.G, rstd + (size_t)w.b * s.G, w.c0 + (t.tc << 3), s.per, 0u, a, b, mu);
#pragma unroll
        for (int i = 0; i < 8; ++i) sdz[i] = sdzx[i] = 0.0f;
        const size_t base = w.off + (t.tc << 3);
#pragma unroll 8
        for (uint32_t p = t.r; p < w.len; p += t.rows) {
            const size_t e = base + (size_t)p * s.C;
            const half8 v = *reinterpret_cast<const half8 *>(x + e);
            const half8 g = *reinterpret_cast<const half8 *>(dy + e);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float xf = (float)v[i], dz = act_bwd<ACT>((float)g[i], fmaf(xf, a[i], b[i]));
                sdz[i] += dz;
                sdzx[i] = fmaf(dz, xf - mu[i], sdzx[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            rdz[t.r * w.nc + (t.tc << 3) + i] = sdz[i];
            rdzx[t.r * w.nc + (t.tc << 3) + i] = sdzx[i];
        }
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < w.nc; c += kBlock) {
        float u = 0.0f, v = 0.0f;
#pragma unroll 8
        for (uint32_t r = 0; r < t.rows; ++r) {
            u += rdz[r * w.nc + c];
            v += rdzx[r * w.nc + c];
        }
        const float wc = weight[w.c0 + c];
        cdz[c] = wc * u;
        cdzx[c] = wc * v;
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < w.ng; g += kBlock) {  // this span's share of (db, ds - db mean) of ATen's backward
        float u = 0.0f, v = 0.0f;
#pragma unroll 8
        for (uint32_t c = g * s.per; c < (g + 1) * s.per; ++c) {
            u += cdz[c];
            v += cdzx[c];
        }
        float *o = partial + 2 * (w.entry0 + (size_t)w.span * s.G + w.g0 + g);
        o[0] = u;
        o[1] = v;
    }
}

template <int ACT>
__global__ __launch_bounds__(kBlock) void k_groupnorm_nhwc_bwd(const half_t *__restrict__ x, const half_t *__restrict__ dy,
                                                               const float *__restrict__ mean,
                                                               const float *__restrict__ rstd,
                                                               const float *__restrict__ weight,
                                                               const float *__restrict__ bias,
                                                               const float *__restrict__ partial, NShape s,
                                                               half_t *__restrict__ dx) {
    __shared__ float gc2[kBlock], gc3[kBlock];
    const NWork w = nwork_of(s);
    const NTile t = ntile_of(w);
    const uint32_t gl = threadIdx.x / s.tpg, j = threadIdx.x - gl * s.tpg;
    const uint32_t c = w.c0 + (t.tc << 3);
    const size_t base = w.off + (t.tc << 3);
    float wv[8], bv[8];
    half8 prex[kNhwcPre], preg[kNhwcPre];
    if (t.active) {  // issued ahead of the merge, as in the apply kernel
        load8(weight + c, wv);
        load8(bias + c, bv);
#pragma unroll
        for (uint32_t u = 0; u < kNhwcPre; ++u)
            if (t.r + u * t.rows < w.len) {
                prex[u] = *reinterpret_cast<const half8 *>(x + base + (size_t)(t.r + u * t.rows) * s.C);
                preg[u] = *reinterpret_cast<const half8 *>(dy + base + (size_t)(t.r + u * t.rows) * s.C);
            }
    }
    float2 acc = {0.0f, 0.0f};
    over_spans(
        s, w, gl, j,
        [&](size_t e, bool ok) { return ok ? float2{partial[2 * e], partial[2 * e + 1]} : float2{0.0f, 0.0f}; },
        [&](float2 v) {
            acc.x += v.x;
            acc.y += v.y;
        });
    for (uint32_t off = s.tpg >> 1; off > 0; off >>= 1) {
        acc.x += __shfl_down(acc.x, off, s.tpg);
        acc.y += __shfl_down(acc.y, off, s.tpg);
    }
    const float *mu_b = mean + (size_t)w.b * s.G, *r_b = rstd + (size_t)w.b * s.G;
    if (j == 0 && gl < w.ng) {
        // ATen's c2 = (db mean - ds) rstd^3 / n with the difference summed centred (acc.y = ds - db mean), and its
        // c2 x + c3, c3 = -c2 mean - db rstd / n, as c2 (x - mean) - db rstd / n: the same value without the two large
        // terms that cancel when a group's spread is small against its mean
        const float r = r_b[w.g0 + gl], inv_n = 1.0f / ((float)s.per * (float)s.HW);
        gc2[gl] = -acc.y * r * r * r * inv_n;
        gc3[gl] = -acc.x * r * inv_n;
    }
    __syncthreads();
    if (!t.active) return;
    float a[8], b[8], mu[8], c2[8], c3[8];
    chan_affine(wv, bv, mu_b, r_b, c, s.per, 0u, a, b, mu);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c2[i] = gc2[(c + i) / s.per - w.g0];
        c3[i] = gc3[(c + i) / s.per - w.g0];
    }
    auto pixel = [&](uint32_t p, half8 v, half8 g) {
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float xf = (float)v[i], dz = act_bwd<ACT>((float)g[i], fmaf(xf, a[i], b[i]));
            o[i] = (half_t)fmaf(a[i], dz, fmaf(c2[i], xf - mu[i], c3[i]));
        }
        *reinterpret_cast<half8 *>(dx + base + (size_t)p * s.C) = o;
    };
#pragma unroll
    for (uint32_t u = 0; u < kNhwcPre; ++u)
        if (t.r + u * t.rows < w.len) pixel(t.r + u * t.rows, prex[u], preg[u]);
#pragma unroll 8
    for (uint32_t p = t.r + kNhwcPre * t.rows; p < w.len; p += t.rows)
        pixel(p, *reinterpret_cast<const half8 *>(x + base + (size_t)p * s.C),
              *reinterpret_cast<const half8 *>(dy + base + (size_t)p * s.C));
}

inline uint32_t gcd_u32(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// false = refuse: what make_shape refuses, channels that are no multiple of 8, or groups whose lcm with a vector of 8
// channels exceeds the slab the LDS buffers hold
bool make_nshape(uint32_t B, uint32_t C, uint32_t HW, uint32_t G, NShape &s, uint32_t &blocks) {
    if (B == 0 || C == 0 || HW == 0 || G == 0 || C % G != 0 || C % 8 != 0) return false;
    s.C = C; s.HW = HW; s.G = G; s.per = C / G;
    if ((unsigned long long)s.per * HW > kMaxGroupElems) return false;
    const unsigned long long lcm = (unsigned long long)s.per / gcd_u32(s.per, 8u) * 8u;
    if (lcm > kNhwcMaxSlab) return false;
    s.slabC = (uint32_t)lcm * (uint32_t)((64u + lcm - 1) / lcm);
    if (s.slabC > C) s.slabC = C;  // (C is a multiple of the lcm)
    s.nslab = (C + s.slabC - 1) / s.slabC;
    const uint32_t gs = s.slabC / s.per;  // groups per slab: at most kNhwcMaxSlab / 8 = kBlock
    const uint32_t cap = kNhwcMerge / gs > 0 ? kNhwcMerge / gs : 1u;
    const uint32_t pmin = (kNhwcChunk + s.slabC - 1) / s.slabC, pcap = (HW + cap - 1) / cap;
    s.P = pmin > pcap ? pmin : pcap;
    // a workgroup of the second kernels reads gs * Sc workspace entries for its P * slabC elements: keep the entries below
    // 1 / kNhwcRatio of the elements, P^2 >= kNhwcRatio * HW / per (measured: at 1 / 2 the merge costs as much as the data)
    while ((unsigned long long)s.P * s.P * s.per < (unsigned long long)kNhwcRatio * HW) ++s.P;
    if (s.P > HW) s.P = HW;
    s.Sc = (HW + s.P - 1) / s.P;
    uint32_t tpg = 1;  // no more lanes per group than there are spans to merge: a short shuffle tree for the small tensors
    while (tpg * 2 <= 64u && tpg * 2 * gs <= (uint32_t)kBlock && tpg < s.Sc) tpg *= 2;
    s.tpg = tpg;
    const unsigned long long n = (unsigned long long)B * s.Sc * s.nslab;
    if (n > 0x7FFFFFFFull) return false;
    blocks = (uint32_t)n;
    return true;
}

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

uint32_t mi3d_groupnorm_nhwc_span(uint32_t C, uint32_t HW, uint32_t G) {
    NShape s;
    uint32_t blocks;
    return make_nshape(1, C, HW, G, s, blocks) ? s.P : 0u;
}

uint32_t mi3d_groupnorm_nhwc_spans(uint32_t C, uint32_t HW, uint32_t G) {
    NShape s;
    uint32_t blocks;
    return make_nshape(1, C, HW, G, s, blocks) ? s.Sc : 0u;
}

int mi3d_groupnorm_nhwc_stats(const void *x, uint32_t B, uint32_t C, uint32_t HW, uint32_t G, float *ws, void *stream) {
    NShape s;
    uint32_t blocks;
    if (!make_nshape(B, C, HW, G, s, blocks) || x == nullptr || ws == nullptr || !aligned16(x))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groupnorm_nhwc_stats, dim3(blocks), dim3(kBlock), 0, as_stream(stream), (const half_t *)x, s, ws);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_nhwc_act_forward(const void *x, const float *ws, const float *weight, const float *bias, uint32_t B,
                                    uint32_t C, uint32_t HW, uint32_t G, float eps, int act, void *y, float *mean,
                                    float *rstd, void *stream) {
    NShape s;
    uint32_t blocks;
    if (!make_nshape(B, C, HW, G, s, blocks) || x == nullptr || ws == nullptr || weight == nullptr || bias == nullptr ||
        y == nullptr || mean == nullptr || rstd == nullptr || (act != 0 && act != 1) || !aligned16(x) || !aligned16(y))
        return (int)hipErrorInvalidValue;
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_nhwc_apply<0>, grid, block, 0, st, (const half_t *)x, ws, weight, bias, s, eps,
                           (half_t *)y, mean, rstd);
    else
        hipLaunchKernelGGL(k_groupnorm_nhwc_apply<1>, grid, block, 0, st, (const half_t *)x, ws, weight, bias, s, eps,
                           (half_t *)y, mean, rstd);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_nhwc_act_backward_sums(const void *x, const void *dy, const float *mean, const float *rstd,
                                          const float *weight, const float *bias, uint32_t B, uint32_t C, uint32_t HW,
                                          uint32_t G, int act, float *partial, void *stream) {
    NShape s;
    uint32_t blocks;
    if (!make_nshape(B, C, HW, G, s, blocks) || x == nullptr || dy == nullptr || mean == nullptr || rstd == nullptr ||
        weight == nullptr || bias == nullptr || partial == nullptr || (act != 0 && act != 1) || !aligned16(x) ||
        !aligned16(dy))
        return (int)hipErrorInvalidValue;
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_nhwc_bwd_sums<0>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean,
                           rstd, weight, bias, s, partial);
    else
        hipLaunchKernelGGL(k_groupnorm_nhwc_bwd_sums<1>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean,
                           rstd, weight, bias, s, partial);
    return (int)hipGetLastError();
}

int mi3d_groupnorm_nhwc_act_backward(const void *x, const void *dy, const float *mean, const float *rstd,
                                     const float *weight, const float *bias, const float *partial, uint32_t B, uint32_t C,
                                     uint32_t HW, uint32_t G, int act, void *dx, void *stream) {
    NShape s;
    uint32_t blocks;
    if (!make_nshape(B, C, HW, G, s, blocks) || x == nullptr || dy == nullptr || mean == nullptr || rstd == nullptr ||
        weight == nullptr || bias == nullptr || partial == nullptr || dx == nullptr || (act != 0 && act != 1) ||
        !aligned16(x) || !aligned16(dy) || !aligned16(dx))
        return (int)hipErrorInvalidValue;
    const dim3 grid(blocks), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (act == 0)
        hipLaunchKernelGGL(k_groupnorm_nhwc_bwd<0>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, partial, s, (half_t *)dx);
    else
        hipLaunchKernelGGL(k_groupnorm_nhwc_bwd<1>, grid, block, 0, st, (const half_t *)x, (const half_t *)dy, mean, rstd,
                           weight, bias, partial, s, (half_t *)dx);
    return (int)hipGetLastError();
}

}  // extern "C"
