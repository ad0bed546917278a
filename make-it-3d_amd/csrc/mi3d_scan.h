// The compaction scaffolding of the mesh, point-cloud and raster units (wave64): the exclusive scan over a workgroup,
// the looped scan of a row of block sums by one workgroup of 1024, and the small predicates and host helpers those
// units share.  Every "count per workgroup / scan the block sums / emit at block base + rank" pipeline in mesh.hip,
// meshclean.hip, meshsimplify.hip, meshsmooth.hip, meshcollapse.hip, pointcloud.hip and raster.hip goes through the two
// scans here (the vertex -> row steps meshsmooth.hip and meshcollapse.hip share are mi3d_incidence.h); the scans of
// raymarching.hip and hashgrid.hip have other shapes and stay where they are.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mi3d_workspace.h"

namespace mi3d_scan {

constexpr int kRowThreads = 1024, kRowWaves = kRowThreads / 64;  // the workgroup scan_row runs in

// inclusive scan of v over the wave's lanes
template <typename T>
__device__ __forceinline__ T wave_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(v, off, 64);
        if (lane >= off) v += up;
    }
    return v;
}

// exclusive scan over a workgroup of WAVES waves; returns the thread's rank, `total` the block sum.  wave_sum: WAVES
// words of LDS.  Every thread of the workgroup calls it.  The trailing barrier lets the next scan reuse wave_sum.
template <int WAVES>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sum, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_scan(v);
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        before += w < wave ? wave_sum[w] : 0u;
        total += wave_sum[w];
    }
    __syncthreads();
    return before + incl - v;
}

// Exclusive scan of row[0 .. nb) by ONE workgroup of kRowThreads threads, kRowThreads elements a round: element i's
// offset goes to put(i, offset), called once per i by the thread that read row[i] (so put may store to row itself);
// returns the total to every thread.  wave_sum: kRowWaves elements of LDS, base: one.  The running base lives in LDS
// and is advanced by thread 0 between two barriers, so a ragged last round and nb == 0 need no special case.  A caller
// that hands the same wave_sum / base to a second call puts a __syncthreads() between the two: a thread may still be
// reading the total of the first.
template <typename T, typename Put>
__device__ __forceinline__ T scan_row(const T *row, uint32_t nb, T *wave_sum, T *base, Put put) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) *base = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nb; b0 += kRowThreads) {
        const uint32_t b = b0 + threadIdx.x;
        const T cnt = b < nb ? row[b] : T(0);
        const T incl = wave_scan(cnt);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        T before = 0, sum = 0;
#pragma unroll
        for (int q = 0; q < kRowWaves; ++q) {
            before += q < wave ? wave_sum[q] : T(0);
            sum += wave_sum[q];
        }
        if (b < nb) put(b, *base + before + incl - cnt);
        __syncthreads();
        if (threadIdx.x == 0) *base += sum;
        __syncthreads();
    }
    return *base;
}

// the same in place: row[i] = the sum of the elements before it
template <typename T>
__device__ __forceinline__ T scan_row(T *row, uint32_t nb, T *wave_sum, T *base) {
    return scan_row(row, nb, wave_sum, base, [row](uint32_t i, T offset) { row[i] = offset; });
}

__device__ __forceinline__ bool in_range(int32_t i, uint32_t nv) { return i >= 0 && (uint32_t)i < nv; }

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }  // false for NaN, +-inf

// the three coordinates of a vertex row
__device__ __forceinline__ bool finite3(const float *__restrict__ row) {
    return is_finite(row[0]) && is_finite(row[1]) && is_finite(row[2]);
}

// one atomic per wave that has any; reached by every lane of the wave (no lane has returned)
__device__ __forceinline__ void wave_count(bool pred, unsigned long long *counter) {
    const unsigned long long m = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// ------------------------------------------------------------------------------------------------ host side

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

using mi3d_workspace::blocks_of;
using mi3d_workspace::bytes_of;
using mi3d_workspace::pad8;

inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// the sizes of a mesh within what the unit's indices hold
inline bool sizes_ok(unsigned long long nv, unsigned long long nt, unsigned long long max_nv, unsigned long long max_nt) {
    return nv <= max_nv && nt <= max_nt;
}

// what an entry point asks of its workspace and its counts: present, 8-byte aligned, the workspace of `need` bytes
inline bool state_ok(const void *ws, size_t ws_bytes, size_t need, const void *counts) {
    return counts != nullptr && aligned8(counts) && ws != nullptr && aligned8(ws) && ws_bytes >= need;
}

}  // namespace mi3d_scan
