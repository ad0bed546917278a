// Taubin lambda | mu smoothing of a mesh's vertices for MI355X (gfx950, wave64); Part 16 of include/mi3d.h, which states
// the contract: usable triangles, the umbrella, the fixed-point neighbour sums, one pass, the border rule, max_move, the
// counts.  The passes repeat 2 x iterations times, so they pay for no atomic: the vertex -> triangle incidence is built
// once, and a pass is one thread per vertex that walks its row, sums in registers and stores to the other buffer.
//
// Compiled with -ffp-contract=off: p + k * (m - p) is a binary64 subtraction, a multiplication and an addition, each
// rounded on its own.
//
// ORDER.  A triangle claims a slot of each corner's row by an atomic cursor, so the order of a row depends on
// scheduling.  Nothing read from a row does: S is a sum of 64-bit integers, the border rule counts equal entries.
//
// Launches of mi3d_mesh_smooth (no host synchronisation, no allocation):
//   k_sm_init       cursors = 0 (grid stride); counts = 0
//   k_sm_degree     per triangle: usable (else counts[0]) -> one int32 atomic per corner: the degrees
//   k_sm_block_sums per vertex: the degrees of a workgroup summed -> block[b]
//   k_sm_scan       one workgroup: exclusive scan of the block sums in place (scan_row of mi3d_scan.h); the total ->
//                   offs[nv]
//   k_sm_offsets    per vertex: block scan of the degrees + block[b] -> offs[v]; the cursor back to 0
//   k_sm_fill       per usable triangle and corner: slot = cursor++ (atomic); inside the row: the pair of the other two
//                   corners -> pairs[offs + slot]; outside: counts[6], nothing stored
//   k_sm_flags      per vertex: finite, degree, border -> moves[v]; counts[1 .. 4]
//   k_sm_pass       2 x iterations times (passes with k == 0 left out): src -> dst, the last one into out_vertices;
//                   the last one counts what the clamp held (counts[5])
//   k_sm_copy       only if no pass is launched (lambda = mu = 0)
// The events counted are rare on the meshes this is made for (unusable triangles, border vertices of a closed surface):
// one atomic per wave that has any.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mi3d.h"
#include "mi3d_incidence.h"

namespace {

using namespace mi3d_scan;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr unsigned long long kMaxVertices = 0x7FFFFFFFull;  // indices are int32
constexpr unsigned long long kMaxTriangles = 1ull << 30;    // 3 nt row slots, offsets are uint32
constexpr uint32_t kMaxDegree = MI3D_SMOOTH_MAX_DEGREE;
constexpr uint32_t kMaxIterations = 1000, kMaxFractionBits = 40;
constexpr uint32_t kInitBlocks = 2048;
constexpr double kSaturate = 1099511627776.0;  // 2^40

// counts (device uint64[8]): see Part 16
enum { kUnusable = 0, kNonFinite = 1, kIsolated = 2, kBorder = 3, kOverDegree = 4, kClamped = 5, kErrors = 6 };

// workspace: smooth_layout of mi3d_workspace.h, the one statement of its arrays and its size
using mi3d_incidence::usable;
using namespace mi3d_workspace;
static_assert(kBlock == kLayoutBlock, "smooth_layout sizes its row of block sums by this workgroup");

// ------------------------------------------------------------------------------------------------ the incidence, once

__global__ __launch_bounds__(kBlock) void k_sm_init(int32_t *__restrict__ cur, uint32_t nv,
                                                    unsigned long long *__restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x < 8) counts[threadIdx.x] = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < nv; i += gridDim.x * kBlock) cur[i] = 0;
}

__global__ __launch_bounds__(kBlock) void k_sm_degree(const float *__restrict__ vertices, uint32_t nv,
                                                      const int32_t *__restrict__ tri, uint32_t nt, int32_t *cur,
                                                      unsigned long long *__restrict__ counts) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < nt;
    int32_t c[3];
    const bool ok = live && usable(vertices, nv, tri, t, c);
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(cur + c[k], 1);
    }
    wave_count(live && !ok, &counts[kUnusable]);
}

// the three scan steps of mi3d_incidence.h, which meshcollapse.hip shares
__global__ __launch_bounds__(kBlock) void k_sm_block_sums(uint32_t nv, SmoothWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    mi3d_incidence::block_sums(w.cur, nv, w.block, wave_sum);
}

__global__ __launch_bounds__(kRowThreads) void k_sm_scan(SmoothWorkspace w, uint32_t nv, uint32_t nb) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    mi3d_incidence::scan_blocks(w.block, nb, w.offs, nv, wave_sum, &base);
}

__global__ __launch_bounds__(kBlock) void k_sm_offsets(uint32_t nv, SmoothWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    mi3d_incidence::offsets(w.cur, nv, w.block, w.offs, wave_sum);
}

__global__ __launch_bounds__(kBlock) void k_sm_fill(const float *__restrict__ vertices, uint32_t nv,
                                                    const int32_t *__restrict__ tri, uint32_t nt, SmoothWorkspace w,
                                                    unsigned long long *__restrict__ counts) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    int32_t c[3];
    uint32_t lost = 0;
    if (t < nt && usable(vertices, nv, tri, t, c)) {
#pragma unroll
        for (int k = 0; k < 3; ++k)  // lost: the mesh changed since k_sm_degree
            lost += mi3d_incidence::fill(w.cur, w.offs, (uint32_t)c[k], [&](size_t i) {
                w.pairs[i] = IndexPair{c[(k + 1) % 3], c[(k + 2) % 3]};
            });
    }
    if (lost != 0) atomicAdd(&counts[kErrors], (unsigned long long)lost);  // never, on a mesh that stays as it is
}

// moves[v] = 1 iff a pass moves vertex v: finite, 0 < deg <= kMaxDegree, not a pinned border vertex.
__global__ __launch_bounds__(kBlock) void k_sm_flags(const float *__restrict__ vertices, uint32_t nv, SmoothWorkspace w,
                                                     int pin_border, unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool live = v < nv;
    bool finite = false, isolated = false, over = false, border = false;
    if (live) {
        finite = finite3(vertices + (size_t)v * 3);
        const uint32_t begin = w.offs[v], deg = w.offs[v + 1] - begin;
        isolated = deg == 0;
        over = deg > kMaxDegree;
        if (pin_border && !isolated && !over) {
            const int32_t *row = reinterpret_cast<const int32_t *>(w.pairs + begin);
            const uint32_t n = 2 * deg;  // <= 2048 entries
            for (uint32_t i = 0; i < n && !border; ++i) {
                const int32_t x = row[i];
                uint32_t shared = 0;
                for (uint32_t j = 0; j < n; ++j) shared += row[j] == x ? 1u : 0u;
                border = shared == 1;  // one usable triangle holds both v and x: an open edge
            }
        }
        w.moves[v] = finite && !isolated && !over && !border ? 1 : 0;
    }
    wave_count(live && !finite, &counts[kNonFinite]);
    wave_count(isolated, &counts[kIsolated]);
    wave_count(border, &counts[kBorder]);
    wave_count(over, &counts[kOverDegree]);
}

// ------------------------------------------------------------------------------------------------ the passes

// q of Part 16: the coordinate in units of 2^-e, saturated at +-2^40, 0 for NaN
__device__ __forceinline__ long long quantise(float p, double scale) {
    const double x = (double)p * scale;
    if (x >= kSaturate) return 1ll << 40;
    if (x <= -kSaturate) return -(1ll << 40);
    return x == x ? __double2ll_rn(x) : 0ll;
}

__global__ __launch_bounds__(kBlock) void k_sm_pass(const float *__restrict__ src, const float *__restrict__ input,
                                                    float *__restrict__ dst, uint32_t nv, SmoothWorkspace w, double k,
                                                    double scale, double inv_scale, float max_move, int clamp,
                                                    int count_held, unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool live = v < nv;
    bool held = false;
    if (live) {
        float p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = src[(size_t)v * 3 + a];
        if (w.moves[v]) {
            const uint32_t begin = w.offs[v], end = w.offs[v + 1];  // 0 < end - begin <= kMaxDegree
            long long S[3] = {0, 0, 0};
            for (uint32_t r = begin; r < end; ++r) {
                const IndexPair pr = w.pairs[r];  // two vertices of a usable triangle: in range
                if (!in_range(pr.x, nv) || !in_range(pr.y, nv)) continue;  // a slot k_sm_fill lost (counts[6]): no fault
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    S[a] += quantise(src[(size_t)pr.x * 3 + a], scale) + quantise(src[(size_t)pr.y * 3 + a], scale);
            }
            const double wsum = (double)(2ll * (long long)(end - begin));
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double m = (double)S[a] / wsum;  // -ffp-contract=off: every operation rounded on its own
                m = m * inv_scale;               // exact
                double d = m - (double)p[a];
                d = k * d;
                const float moved = (float)((double)p[a] + d);
                float kept = moved;
                if (clamp) {
                    const float p0 = input[(size_t)v * 3 + a];
                    const float lo = p0 - max_move, hi = p0 + max_move;
                    kept = moved < lo ? lo : moved > hi ? hi : moved;
                    held = held || kept != moved;
                }
                p[a] = kept;
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) dst[(size_t)v * 3 + a] = p[a];
    }
    if (count_held) wave_count(held, &counts[kClamped]);
}

__global__ __launch_bounds__(kBlock) void k_sm_copy(const float *__restrict__ src, float *__restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

bool factor_ok(double k) { return std::isfinite(k) && k >= -1.0 && k <= 1.0; }

}  // namespace

extern "C" {

size_t mi3d_mesh_smooth_workspace(unsigned long long nv, unsigned long long nt) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles) || nv == 0) return 0;
    return bytes_of(smooth_layout, (uint32_t)nv, (uint32_t)nt);
}

int mi3d_mesh_smooth(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                     uint32_t iterations, double lambda, double mu, int pin_border, float max_move,
                     uint32_t fraction_bits, void *ws, size_t ws_bytes, float *out_vertices, unsigned long long *counts,
                     void *stream) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles) || iterations < 1 || iterations > kMaxIterations || fraction_bits > kMaxFractionBits ||
        !factor_ok(lambda) || !factor_ok(mu) || !(max_move >= 0.f))
        return (int)hipErrorInvalidValue;
    if (nv == 0) return (int)hipSuccess;
    if (vertices == nullptr || out_vertices == nullptr || out_vertices == vertices ||
        !state_ok(ws, ws_bytes, bytes_of(smooth_layout, (uint32_t)nv, (uint32_t)nt), counts) ||
        (nt > 0 && triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt, nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const SmoothWorkspace w = at(ws, smooth_layout, n, m);
    hipLaunchKernelGGL(k_sm_init, dim3(nb < kInitBlocks ? nb : kInitBlocks), dim3(kBlock), 0, st, w.cur, n, counts);
    if (m) hipLaunchKernelGGL(k_sm_degree, dim3(nbt), dim3(kBlock), 0, st, vertices, n, triangles, m, w.cur, counts);
    hipLaunchKernelGGL(k_sm_block_sums, dim3(nb), dim3(kBlock), 0, st, n, w);
    hipLaunchKernelGGL(k_sm_scan, dim3(1), dim3(kRowThreads), 0, st, w, n, nb);
    hipLaunchKernelGGL(k_sm_offsets, dim3(nb), dim3(kBlock), 0, st, n, w);
    if (m) hipLaunchKernelGGL(k_sm_fill, dim3(nbt), dim3(kBlock), 0, st, vertices, n, triangles, m, w, counts);
    hipLaunchKernelGGL(k_sm_flags, dim3(nb), dim3(kBlock), 0, st, vertices, n, w, pin_border ? 1 : 0, counts);

    const double factor[2] = {lambda, mu};
    const uint32_t per_iteration = (lambda != 0.0 ? 1u : 0u) + (mu != 0.0 ? 1u : 0u);
    const uint32_t passes = iterations * per_iteration;
    if (passes == 0) {
        const size_t words = (size_t)n * 3;
        hipLaunchKernelGGL(k_sm_copy, dim3((uint32_t)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, vertices,
                           out_vertices, words);
        return (int)hipGetLastError();
    }
    const double scale = std::ldexp(1.0, (int)fraction_bits), inv_scale = std::ldexp(1.0, -(int)fraction_bits);
    const int clamp = std::isfinite(max_move) ? 1 : 0;
    const float *src = vertices;
    uint32_t left = passes;  // the pass with `left` == 1 is the last: the buffers alternate so that it writes the output
    for (uint32_t it = 0; it < iterations; ++it) {
        for (int half = 0; half < 2; ++half) {
            if (factor[half] == 0.0) continue;
            float *dst = (left & 1u) ? out_vertices : w.tmp;
            hipLaunchKernelGGL(k_sm_pass, dim3(nb), dim3(kBlock), 0, st, src, vertices, dst, n, w, factor[half], scale,
                               inv_scale, max_move, clamp, left == 1 ? 1 : 0, counts);
            src = dst;
            --left;
        }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
