// Marching cubes for MI355X (gfx950): a dense scalar volume -> a welded, indexed triangle mesh in a deterministic order;
// Part 8 of include/mi3d.h, which states the contract (inside = value >= iso, the vertex formula, the output order).
// What `mcubes.marching_cubes` does for the reference's export_mesh (nerf/renderer.py:182 of the reference); PyMCubes is on
// no machine this project builds on, so the conventions are this project's own - PARITY UNPINNED.
//
// Compiled with -ffp-contract=off: a vertex coordinate is origin + spacing * (a + t), three separately rounded binary32
// operations behind a correctly rounded division, so that a NumPy float32 restatement gives the same bits.
//
// Passes (no host synchronisation, no allocation, no atomic appends; thread = grid point, linear index, z fastest, so a
// wave reads 64 consecutive floats and its +y / +x neighbours are two more contiguous rows that the caches serve):
//   k_mc_count     per point: the 3-bit mask of the crossing edges it OWNS (towards +x, +y, +z) and, where it is the min
//                  corner of a cell, the triangle count of its case; block sums of both -> workspace
//   k_mc_scan      one workgroup: exclusive scan of the block sums in place (scan_row of mi3d_scan.h, once per row),
//                  totals -> counts
//   k_mc_vertices  masks again, block scan, vertex `block base + rank` written, first vertex id of every point -> workspace
//   k_mc_triangles cases again, block scan, triangles written; a corner on cube edge e is vertex
//                  first_id[owner] + popcount(mask[owner] & ((1 << axis) - 1)), the owner's lower mask bits recomputed
//                  from the volume (cached loads: the owner is a corner of the cell or one step beyond it)
// What does not fit the caller's buffers is counted in counts[2], never written.
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_mc_tables.h"
#include "mi3d_scan.h"

namespace {

using namespace mi3d_scan;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr uint32_t kMinDim = 2, kMaxDim = 1024;

__constant__ int8_t d_tri[256][16] = MI3D_MC_TRI_INIT;
__constant__ uint8_t d_ntri[256] = MI3D_MC_NTRI_INIT;
__constant__ uint8_t d_corners[8][3] = MI3D_MC_CORNERS_INIT;
__constant__ uint8_t d_edges[12][2] = MI3D_MC_EDGES_INIT;
const int8_t h_tri[256][16] = MI3D_MC_TRI_INIT;
const uint8_t h_ntri[256] = MI3D_MC_NTRI_INIT;

struct McDims {
    uint32_t Rx, Ry, Rz, n;  // n = Rx Ry Rz <= 2^30
};

// workspace: mc_layout of mi3d_workspace.h, the one statement of its arrays and its size
using namespace mi3d_workspace;
static_assert(kBlock == kLayoutBlock, "mc_layout sizes its rows of block sums by this workgroup");

__host__ __device__ inline uint32_t mc_blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

__device__ __forceinline__ bool inside(float v, float iso) { return v >= iso; }  // NaN: outside

// mask of the crossing edges grid point (i, j, k) owns: bit a = the edge towards +axis a exists and changes side
__device__ __forceinline__ uint32_t owned_mask(const float *__restrict__ vol, McDims d, uint32_t p, uint32_t i, uint32_t j,
                                               uint32_t k, float iso, uint32_t upto = 3) {
    const bool in0 = inside(vol[p], iso);
    uint32_t m = 0;
    if (upto > 0 && i + 1 < d.Rx && inside(vol[p + d.Ry * d.Rz], iso) != in0) m |= 1u;
    if (upto > 1 && j + 1 < d.Ry && inside(vol[p + d.Rz], iso) != in0) m |= 2u;
    if (upto > 2 && k + 1 < d.Rz && inside(vol[p + 1], iso) != in0) m |= 4u;
    return m;
}

// case index of the cell whose min corner is (i, j, k); the caller guarantees that the cell exists
__device__ __forceinline__ uint32_t cell_case(const float *__restrict__ vol, McDims d, uint32_t p, float iso) {
    uint32_t c = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t o = (d_corners[q][0] * d.Ry + d_corners[q][1]) * d.Rz + d_corners[q][2];
        c |= inside(vol[p + o], iso) ? 1u << q : 0u;
    }
    return c;
}

__device__ __forceinline__ void split(McDims d, uint32_t p, uint32_t &i, uint32_t &j, uint32_t &k) {
    k = p % d.Rz;
    const uint32_t r = p / d.Rz;
    j = r % d.Ry;
    i = r / d.Ry;
}

__global__ __launch_bounds__(kBlock) void k_mc_count(const float *__restrict__ vol, McDims d, float iso, McWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t nv = 0, nt = 0;
    if (p < d.n) {
        uint32_t i, j, k;
        split(d, p, i, j, k);
        nv = __popc(owned_mask(vol, d, p, i, j, k, iso));
        if (i + 1 < d.Rx && j + 1 < d.Ry && k + 1 < d.Rz) nt = d_ntri[cell_case(vol, d, p, iso)];
    }
    uint32_t tv, tt;
    block_scan<kWaves>(nv, wave_sum, tv);
    block_scan<kWaves>(nt, wave_sum, tt);
    if (threadIdx.x == 0) {
        w.block_v[blockIdx.x] = tv;
        w.block_t[blockIdx.x] = tt;
    }
}

// exclusive scan of both rows of block sums in place (at most 4 M sums each); counts = {vertices, triangles, 0
// (elements emit could not place), 0}.  The vertex offsets fit 32 bits without a clamp: a grid point owns at most 3
// edges and n <= 2^30 (kMaxDim), so they end at 3 * 2^30 < 2^32 at most.  Triangles: up to 5 per cell, 64 bits.
__global__ __launch_bounds__(kRowThreads) void k_mc_scan(McWorkspace w, uint32_t nb,
                                                         unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_v[kRowWaves], base_v;
    __shared__ unsigned long long wave_t[kRowWaves], base_t;
    const uint32_t nv = scan_row(w.block_v, nb, wave_v, &base_v);
    const unsigned long long nt = scan_row(w.block_t, nb, wave_t, &base_t);
    if (threadIdx.x == 0) { counts[0] = nv; counts[1] = nt; counts[2] = 0; counts[3] = 0; }
}

struct McFrame {
    float ox, oy, oz, sx, sy, sz;
};

__global__ __launch_bounds__(kBlock) void k_mc_vertices(const float *__restrict__ vol, McDims d, float iso, McFrame f,
                                                        McWorkspace w, float *__restrict__ vertices, uint32_t nv_cap,
                                                        unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t i = 0, j = 0, k = 0, mask = 0;
    if (p < d.n) {
        split(d, p, i, j, k);
        mask = owned_mask(vol, d, p, i, j, k, iso);
    }
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(__popc(mask), wave_sum, total);
    if (p >= d.n) return;
    uint32_t id = w.block_v[blockIdx.x] + rank;  // at most 3 * 2^30 (see k_mc_scan): the three steps below fit too
    w.first_id[p] = id;
    if (mask == 0) return;
    const float va = vol[p];
    const uint32_t stride[3] = {d.Ry * d.Rz, d.Rz, 1u};
    uint32_t dropped = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1u)) continue;
        if (id >= nv_cap) { ++dropped; ++id; continue; }
        const float vb = vol[p + stride[a]];
        float t = (iso - va) / (vb - va);
        if (!(t >= 0.f && t <= 1.f)) t = 0.5f;  // also NaN: a non-finite end value
        const float gx = (float)i + (a == 0 ? t : 0.f), gy = (float)j + (a == 1 ? t : 0.f),
                    gz = (float)k + (a == 2 ? t : 0.f);
        float *o = vertices + (size_t)id * 3;
        o[0] = f.ox + f.sx * gx;
        o[1] = f.oy + f.sy * gy;
        o[2] = f.oz + f.sz * gz;
        ++id;
    }
    if (dropped) atomicAdd(&counts[2], (unsigned long long)dropped);
}

__global__ __launch_bounds__(kBlock) void k_mc_triangles(const float *__restrict__ vol, McDims d, float iso, McWorkspace w,
                                                         int32_t *__restrict__ triangles, unsigned long long nt_cap,
                                                         unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    uint32_t i = 0, j = 0, k = 0, cs = 0, nt = 0;
    if (p < d.n) {
        split(d, p, i, j, k);
        if (i + 1 < d.Rx && j + 1 < d.Ry && k + 1 < d.Rz) {
            cs = cell_case(vol, d, p, iso);
            nt = d_ntri[cs];
        }
    }
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(nt, wave_sum, total);
    if (nt == 0) return;
    const unsigned long long first = w.block_t[blockIdx.x] + rank;
    uint32_t dropped = 0;
    for (uint32_t t = 0; t < nt; ++t) {
        if (first + t >= nt_cap) { ++dropped; continue; }
        int32_t *o = triangles + (size_t)(first + t) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int e = d_tri[cs][3 * t + c];
            // the edge's lower corner owns it; the axis is the coordinate in which its two corners differ
            const int c0 = d_edges[e][0], c1 = d_edges[e][1];
            const int lo = d_corners[c0][0] + d_corners[c0][1] + d_corners[c0][2] <
                                   d_corners[c1][0] + d_corners[c1][1] + d_corners[c1][2] ? c0 : c1;
            const int hi = lo == c0 ? c1 : c0;
            const uint32_t axis = d_corners[hi][0] != d_corners[lo][0] ? 0u : d_corners[hi][1] != d_corners[lo][1] ? 1u : 2u;
            const uint32_t oi = i + d_corners[lo][0], oj = j + d_corners[lo][1], ok = k + d_corners[lo][2];
            const uint32_t op = (oi * d.Ry + oj) * d.Rz + ok;
            const uint32_t below = axis == 0 ? 0u : owned_mask(vol, d, op, oi, oj, ok, iso, axis);
            o[c] = (int32_t)(w.first_id[op] + __popc(below));
        }
    }
    if (dropped) atomicAdd(&counts[2], (unsigned long long)dropped);
}

bool mc_dims(uint32_t Rx, uint32_t Ry, uint32_t Rz, McDims &d) {
    if (Rx < kMinDim || Ry < kMinDim || Rz < kMinDim || Rx > kMaxDim || Ry > kMaxDim || Rz > kMaxDim) return false;
    d.Rx = Rx; d.Ry = Ry; d.Rz = Rz; d.n = Rx * Ry * Rz;
    return true;
}

bool mc_args(const void *vol, uint32_t Rx, uint32_t Ry, uint32_t Rz, const void *ws, size_t ws_bytes, const void *counts,
             McDims &d) {
    return mc_dims(Rx, Ry, Rz, d) && vol != nullptr && state_ok(ws, ws_bytes, bytes_of(mc_layout, d.n), counts);
}

}  // namespace

extern "C" {

size_t mi3d_mc_workspace(uint32_t Rx, uint32_t Ry, uint32_t Rz) {
    McDims d;
    return mc_dims(Rx, Ry, Rz, d) ? bytes_of(mc_layout, d.n) : 0;
}

int mi3d_mc_case(uint32_t case_index, int8_t *edges_host) {
    if (case_index > 255u || edges_host == nullptr) return -1;
    for (int q = 0; q < 16; ++q) edges_host[q] = h_tri[case_index][q];
    return (int)h_ntri[case_index];
}

int mi3d_mc_count(const float *vol, uint32_t Rx, uint32_t Ry, uint32_t Rz, float iso, void *ws, size_t ws_bytes,
                  unsigned long long *counts, void *stream) {
    McDims d;
    if (!mc_args(vol, Rx, Ry, Rz, ws, ws_bytes, counts, d) || iso != iso) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mc_count, dim3(mc_blocks(d.n)), dim3(kBlock), 0, as_stream(stream), vol, d, iso, at(ws, mc_layout, d.n));
    return (int)hipGetLastError();
}

int mi3d_mc_scan(uint32_t Rx, uint32_t Ry, uint32_t Rz, void *ws, size_t ws_bytes, unsigned long long *counts,
                 void *stream) {
    McDims d;
    if (!mc_args(ws /* no volume here */, Rx, Ry, Rz, ws, ws_bytes, counts, d)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mc_scan, dim3(1), dim3(kRowThreads), 0, as_stream(stream), at(ws, mc_layout, d.n), mc_blocks(d.n),
                       counts);
    return (int)hipGetLastError();
}

int mi3d_mc_emit(const float *vol, uint32_t Rx, uint32_t Ry, uint32_t Rz, float iso, const float *origin_host,
                 const float *spacing_host, void *ws, size_t ws_bytes, unsigned long long *counts, float *vertices,
                 unsigned long long nv_cap, int32_t *triangles, unsigned long long nt_cap, void *stream) {
    McDims d;
    if (!mc_args(vol, Rx, Ry, Rz, ws, ws_bytes, counts, d) || iso != iso || origin_host == nullptr ||
        spacing_host == nullptr || (nv_cap > 0 && vertices == nullptr) || (nt_cap > 0 && triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const McFrame f = {origin_host[0], origin_host[1], origin_host[2], spacing_host[0], spacing_host[1], spacing_host[2]};
    const uint32_t vcap = nv_cap > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)nv_cap;  // ids are int32 in `triangles`
    const McWorkspace w = at(ws, mc_layout, d.n);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_mc_vertices, dim3(mc_blocks(d.n)), dim3(kBlock), 0, st, vol, d, iso, f, w, vertices, vcap, counts);
    hipLaunchKernelGGL(k_mc_triangles, dim3(mc_blocks(d.n)), dim3(kBlock), 0, st, vol, d, iso, w, triangles, nt_cap,
                       counts);
    return (int)hipGetLastError();
}

}  // extern "C"
