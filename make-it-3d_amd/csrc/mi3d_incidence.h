// The vertex -> row scaffolding meshsmooth.hip and meshcollapse.hip share: per-vertex counts (the degrees, or a 0 / 1
// flag) become row offsets by "sum per workgroup / one workgroup scans the sums / offsets = block base + rank".  The
// three steps are device functions; each unit wraps them in its own kernels, which decide whether the step runs at all.
// With them the rule that says which triangles take part (usable) and the claim of a row slot by its cursor (fill).
#pragma once
#include "mi3d_scan.h"

namespace mi3d_incidence {

using namespace mi3d_scan;

constexpr int kBlock = 256, kWaves = kBlock / 64;  // the workgroup block_sums and offsets run in

// the counts of a workgroup's vertices summed -> block[blockIdx.x].  wave_sum: kWaves words of LDS.
__device__ __forceinline__ void block_sums(const int32_t *__restrict__ cur, uint32_t nv, uint32_t *__restrict__ block,
                                           uint32_t *wave_sum) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    block_scan<kWaves>(v < nv ? (uint32_t)cur[v] : 0u, wave_sum, total);
    if (threadIdx.x == 0) block[blockIdx.x] = total;
}

// exclusive scan of the row of block sums in place, by one workgroup of kRowThreads; the total -> offs[nv].
// wave_sum: kRowWaves words of LDS, base: one.
__device__ __forceinline__ void scan_blocks(uint32_t *block, uint32_t nb, uint32_t *offs, uint32_t nv,
                                            uint32_t *wave_sum, uint32_t *base) {
    const uint32_t total = scan_row(block, nb, wave_sum, base);
    if (threadIdx.x == 0) offs[nv] = total;
}

// block scan of the counts + block[b] -> offs[v]; the count back to 0: from here on the cursor of the row
__device__ __forceinline__ void offsets(int32_t *__restrict__ cur, uint32_t nv, const uint32_t *__restrict__ block,
                                        uint32_t *__restrict__ offs, uint32_t *wave_sum) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(v < nv ? (uint32_t)cur[v] : 0u, wave_sum, total);
    if (v >= nv) return;
    offs[v] = block[blockIdx.x] + rank;
    cur[v] = 0;
}

// The corners of triangle t if it is usable (include/mi3d.h Part 16): indices in range, pairwise distinct, three finite
// vertices.  Nothing is dereferenced before the index check.
__device__ __forceinline__ bool usable(const float *__restrict__ vertices, uint32_t nv, const int32_t *__restrict__ tri,
                                       uint32_t t, int32_t c[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = tri[(size_t)t * 3 + k];
    if (!(in_range(c[0], nv) && in_range(c[1], nv) && in_range(c[2], nv))) return false;
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return false;
    for (int k = 0; k < 3; ++k)
        if (!finite3(vertices + (size_t)c[k] * 3)) return false;
    return true;
}

// One entry of v's row [offs[v], offs[v + 1]): the cursor hands out the slot, put(index) stores the payload there.
// Returns 1, and stores nothing, for a slot beyond the row (the degrees were counted on another mesh), else 0.
template <typename Put>
__device__ __forceinline__ uint32_t fill(int32_t *cur, const uint32_t *offs, uint32_t v, Put put) {
    const uint32_t begin = offs[v], len = offs[v + 1] - begin;
    const uint32_t slot = (uint32_t)atomicAdd(cur + v, 1);
    if (slot >= len) return 1u;
    put((size_t)begin + slot);
    return 0u;
}

}  // namespace mi3d_incidence
