// Mesh simplification by vertex clustering (Rossignac-Borrel) for MI355X (gfx950, wave64); Part 14 of include/mi3d.h,
// which states the contract: the cluster of a vertex, its leader (the smallest vertex index of the cluster), the
// fixed-point mean that places it, degenerate and duplicate triangles, the output order.  One pass over the vertices and
// one over the triangles: no priority queue, no sorting, integer atomics only, so that two runs - and a NumPy
// restatement - give the same bytes.
//
// Compiled with -ffp-contract=off: g = (v - o) / cell is a binary32 subtraction and a binary32 division, the position
// o + cell * (c + (S / n) * 2^-20) four separately rounded binary64 operations.
//
// TABLES.  Two open-addressing tables whose slots hold an INDEX (-1: empty), never a packed key: a vertex index in the
// cluster table, a triangle index in the duplicate table.  The key of a slot is re-derived from the element it holds,
// out of read-only input (the vertex's coordinates; the triangle's corners through `lead`, which the launch before
// completed).  A slot is claimed by atomicCAS(-1 -> index) and from then on only ever lowered by atomicMin to an
// element of the SAME key: the key of a slot never changes and a slot never becomes empty again.  Hence a stale read of
// a slot (the eight XCDs have separate L2s, a CU's L1 is never refreshed) is harmless: a stale -1 is found out by the
// compare-and-swap, which is performed on memory, and a stale index still carries the slot's key and is not below its
// present content.  The probes read with relaxed agent-scope loads (past L1), linear probing, at most `capacity` steps;
// a thread that runs out adds to counts[3] and leaves - a bug is an error, never a hang.  The hash is private to this
// file: nothing in the result depends on it, nor on the capacity.
//
// Passes of mi3d_mesh_simplify_count (thread = vertex or triangle, no host synchronisation, no allocation):
//   k_sp_init      tables = -1, accumulators and reference marks = 0 (8 bytes per step, grid stride); counts = 0
//   k_sp_insert_v  per vertex: cluster -> probe, claim or lower; its slot -> lead[v] (non-finite: -1, counts[4])
//   k_sp_accum     per vertex: lead[v] = the slot's final content = the leader; S (3 axes) and n added to the leader's
//                  row by 64-bit integer atomics
//   k_sp_insert_t  per triangle: indices checked (counts[2]), corners -> leaders, degenerate or inserted under its
//                  sorted leader triple; its slot -> tslot[t]; degenerate ones counted per workgroup
//   k_sp_flag_t    per triangle: survivor iff its slot ended up holding it, else a duplicate; survivors mark their three
//                  leaders (same-value plain stores); both counted per workgroup
//   k_sp_count_v   per vertex: a leader with a mark is emitted; leaders and emitted leaders counted per workgroup
//   k_sp_scan      one workgroup: exclusive scan of both rows of block sums in place; totals -> counts[0], counts[1];
//                  the rows of leaders, degenerate and duplicate triangles summed -> counts[5], [6], [7]
// Passes of mi3d_mesh_simplify_emit:
//   k_sp_emit_v    emitted leaders: block scan, position from the accumulators, vertex_map[leader]
//   k_sp_map       every other vertex: vertex_map[v] = vertex_map[lead[v]] (-1 without a cluster)
//   k_sp_emit_t    survivors: block scan, corners through vertex_map
// The common events (leaders, degenerate, duplicate) are counted per workgroup and summed by k_sp_scan: one atomic per
// wave on a single address retires at under 100 per microsecond, which was 9 of the first version's 16 ms on the 256^3
// noise surface.  The rare ones (counts[2], [3], [4]) are one atomic per wave that has any.  The scans
// (block_scan, scan_row) and wave_count are those of mi3d_scan.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

using namespace mi3d_scan;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr unsigned long long kMaxCount = 0x7FFFFFFFull;  // nv, nt <= 2^31 - 1: indices are int32
constexpr uint32_t kInitBlocks = 2048;

// counts (device uint64[8]): 0 emitted vertices, 1 surviving triangles, 2 triangles with an index outside [0, nv) or a
// corner without a cluster, 3 threads that gave up, 4 non-finite vertices, 5 clusters, 6 degenerate triangles,
// 7 duplicate triangles
enum { kOutV = 0, kOutT = 1, kBad = 2, kGaveUp = 3, kNonFinite = 4, kClusters = 5, kDegenerate = 6, kDuplicate = 7 };

struct Lattice {
    float o[3];
    float cell;
};

// workspace: simplify_layout of mi3d_workspace.h, the one statement of its arrays, of the region k_sp_init fills with -1
// and the one it zeroes behind it, and of its size for either table capacity
using namespace mi3d_workspace;
static_assert(kBlock == kLayoutBlock, "simplify_layout sizes its rows of block sums by this workgroup");

// the capacities are the largest the caller's bytes hold: recommended (shift 1) or tight (shift 0)
inline SimplifyWorkspace simplify_carve(void *ws, size_t ws_bytes, uint32_t nv, uint32_t nt) {
    return at(ws, simplify_layout, nv, nt, ws_bytes >= bytes_of(simplify_layout, nv, nt, 1) ? 1 : 0);
}

// relaxed, agent scope: past the CU's L1
__device__ __forceinline__ int32_t load_slot(const int32_t *table, uint32_t s) {
    return __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t mix3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ c * 0xC2B2AE3Du;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}

// The cluster c and the fraction f of vertex v (Part 14); false: a non-finite coordinate, no cluster.
__device__ __forceinline__ bool cluster_of(const float *__restrict__ vertices, uint32_t v, const Lattice &L, int32_t c[3],
                                           float f[3]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float x = vertices[(size_t)v * 3 + k];
        finite = finite && is_finite(x);
        const float d = x - L.o[k];
        const float g = d / L.cell;
        const float fl = floorf(g);
        c[k] = fl >= 1073741824.f ? 1073741823 : fl < -1073741824.f ? -1073741824 : (int32_t)fl;
        const float fr = g - (float)c[k];
        f[k] = fminf(fmaxf(fr, 0.f), 1.f);  // moves nothing unless c was clamped
    }
    return finite;
}

// ------------------------------------------------------------------------------------------------ the count phase

__global__ __launch_bounds__(kBlock) void k_sp_init(unsigned long long *__restrict__ words, unsigned long long fill_words,
                                                    unsigned long long zero_words,
                                                    unsigned long long *__restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x < 8) counts[threadIdx.x] = 0;
    const unsigned long long total = fill_words + zero_words;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; i < total;
         i += (unsigned long long)gridDim.x * kBlock)
        words[i] = i < fill_words ? ~0ull : 0ull;
}

__global__ __launch_bounds__(kBlock) void k_sp_insert_v(const float *__restrict__ vertices, uint32_t nv, Lattice L,
                                                        SimplifyWorkspace w, unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool live = v < nv;
    int32_t c[3] = {0, 0, 0};
    float f[3];
    const bool finite = live && cluster_of(vertices, v, L, c, f);
    int32_t found = -1;
    bool gave_up = false;
    if (finite) {
        const uint32_t mask = w.cap_v - 1;
        uint32_t s = mix3((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2]) & mask;
        gave_up = true;
        for (uint32_t step = 0; step < w.cap_v; ++step, s = (s + 1) & mask) {
            int32_t cur = load_slot(w.table_v, s);
            if (cur == -1) {
                cur = atomicCAS(w.table_v + s, -1, (int32_t)v);
                if (cur == -1) { found = (int32_t)s; gave_up = false; break; }
            }
            int32_t oc[3];
            float of[3];
            cluster_of(vertices, (uint32_t)cur, L, oc, of);  // cur was inserted: it is a finite vertex below nv
            if (oc[0] == c[0] && oc[1] == c[1] && oc[2] == c[2]) {
                if ((int32_t)v < cur) atomicMin(w.table_v + s, (int32_t)v);  // cur >= the present content
                found = (int32_t)s;
                gave_up = false;
                break;
            }
        }
    }
    if (live) w.lead[v] = found;
    wave_count(live && !finite, &counts[kNonFinite]);
    wave_count(gave_up, &counts[kGaveUp]);
}

__global__ __launch_bounds__(kBlock) void k_sp_accum(const float *__restrict__ vertices, uint32_t nv, Lattice L,
                                                     SimplifyWorkspace w) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int32_t s = w.lead[v];  // the slot, written by this thread's predecessor in k_sp_insert_v
    if (s < 0) return;
    const int32_t leader = w.table_v[s];
    w.lead[v] = leader;
    int32_t c[3];
    float f[3];
    cluster_of(vertices, v, L, c, f);
    unsigned long long *row = w.acc + (size_t)leader * 4;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(row + k, (unsigned long long)(long long)floorf(f[k] * 1048576.f));
    atomicAdd(row + 3, 1ull);
}

__device__ __forceinline__ void sort3(int32_t &a, int32_t &b, int32_t &c) {
    int32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

__global__ __launch_bounds__(kBlock) void k_sp_insert_t(const int32_t *__restrict__ tri, uint32_t nt, uint32_t nv,
                                                        SimplifyWorkspace w, unsigned long long *__restrict__ counts) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool live = t < nt;
    bool bad = false, degenerate = false, gave_up = false;
    int32_t found = -1;
    if (live) {
        const int32_t a = tri[(size_t)t * 3], b = tri[(size_t)t * 3 + 1], c = tri[(size_t)t * 3 + 2];
        bad = !(in_range(a, nv) && in_range(b, nv) && in_range(c, nv));
        int32_t x = -1, y = -1, z = -1;
        if (!bad) {
            x = w.lead[a];
            y = w.lead[b];
            z = w.lead[c];
            bad = x < 0 || y < 0 || z < 0;  // a corner without a cluster
        }
        degenerate = !bad && (x == y || y == z || x == z);
        if (!bad && !degenerate) {
            sort3(x, y, z);
            const uint32_t mask = w.cap_t - 1;
            uint32_t s = mix3((uint32_t)x, (uint32_t)y, (uint32_t)z) & mask;
            gave_up = true;
            for (uint32_t step = 0; step < w.cap_t; ++step, s = (s + 1) & mask) {
                int32_t cur = load_slot(w.table_t, s);
                if (cur == -1) {
                    cur = atomicCAS(w.table_t + s, -1, (int32_t)t);
                    if (cur == -1) { found = (int32_t)s; gave_up = false; break; }
                }
                // cur was inserted: its indices are in range and its corners have leaders
                int32_t p = w.lead[tri[(size_t)cur * 3]], q = w.lead[tri[(size_t)cur * 3 + 1]],
                        r = w.lead[tri[(size_t)cur * 3 + 2]];
                sort3(p, q, r);
                if (p == x && q == y && r == z) {
                    if ((int32_t)t < cur) atomicMin(w.table_t + s, (int32_t)t);
                    found = (int32_t)s;
                    gave_up = false;
                    break;
                }
            }
        }
        w.tslot[t] = found;
    }
    wave_count(bad, &counts[kBad]);
    wave_count(gave_up, &counts[kGaveUp]);
    __shared__ uint32_t wave_sum[kWaves];
    uint32_t total;
    // most triangles are degenerate: a row of block sums, not one hot address
    block_scan<kWaves>(degenerate ? 1u : 0u, wave_sum, total);
    if (threadIdx.x == 0) w.degenerate_t[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_sp_flag_t(const int32_t *__restrict__ tri, uint32_t nt, SimplifyWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const int32_t s = t < nt ? w.tslot[t] : -1;
    const bool survives = s >= 0 && w.table_t[s] == (int32_t)t;
    if (s >= 0 && !survives) w.tslot[t] = -1;  // from here on tslot[t] >= 0 means "survives"
    if (survives) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w.ref[w.lead[tri[(size_t)t * 3 + k]]] = 1;
    }
    uint32_t total;  // two counts of at most 256 in one scan: survivors low, duplicates high
    block_scan<kWaves>((survives ? 1u : 0u) | (s >= 0 && !survives ? 1u << 16 : 0u), wave_sum, total);
    if (threadIdx.x == 0) {
        w.block_t[blockIdx.x] = total & 0xFFFFu;
        w.duplicate_t[blockIdx.x] = total >> 16;
    }
}

__device__ __forceinline__ bool is_leader(const SimplifyWorkspace &w, uint32_t v, uint32_t nv) {
    return v < nv && w.lead[v] == (int32_t)v;
}

__global__ __launch_bounds__(kBlock) void k_sp_count_v(uint32_t nv, SimplifyWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool leader = is_leader(w, v, nv);
    uint32_t total;  // emitted leaders low, all leaders high
    block_scan<kWaves>((leader && w.ref[v] ? 1u : 0u) | (leader ? 1u << 16 : 0u), wave_sum, total);
    if (threadIdx.x == 0) {
        w.block_v[blockIdx.x] = total & 0xFFFFu;
        w.clusters_v[blockIdx.x] = total >> 16;
    }
}

// the sum of a row of per-workgroup counts, to every thread (one workgroup of 1024)
__device__ unsigned long long sum_row(const uint32_t *row, uint32_t nb, unsigned long long *wave_total) {
    unsigned long long s = 0;
    for (uint32_t b = threadIdx.x; b < nb; b += kRowThreads) s += row[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = s;
    __syncthreads();
    unsigned long long sum = 0;
#pragma unroll
    for (int q = 0; q < kRowWaves; ++q) sum += wave_total[q];
    return sum;
}

__global__ __launch_bounds__(kRowThreads) void k_sp_scan(SimplifyWorkspace w, uint32_t nbv, uint32_t nbt,
                                                  unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    const uint32_t kv = scan_row(w.block_v, nbv, wave_sum, &base);
    __syncthreads();
    const uint32_t kt = scan_row(w.block_t, nbt, wave_sum, &base);
    __shared__ unsigned long long wave_total[kRowWaves];
    const unsigned long long clusters = sum_row(w.clusters_v, nbv, wave_total);
    const unsigned long long degenerate = sum_row(w.degenerate_t, nbt, wave_total);
    const unsigned long long duplicate = sum_row(w.duplicate_t, nbt, wave_total);
    if (threadIdx.x == 0) {
        counts[kOutV] = kv;
        counts[kOutT] = kt;
        counts[kClusters] = clusters;
        counts[kDegenerate] = degenerate;
        counts[kDuplicate] = duplicate;
    }
}

// ------------------------------------------------------------------------------------------------ the emit phase

__global__ __launch_bounds__(64) void k_sp_zero_lost(unsigned long long *__restrict__ lost) {
    if (threadIdx.x == 0) *lost = 0;
}

__global__ __launch_bounds__(kBlock) void k_sp_emit_v(const float *__restrict__ vertices, uint32_t nv, Lattice L,
                                                      SimplifyWorkspace w, float *__restrict__ out, uint32_t nv_cap,
                                                      int32_t *__restrict__ vertex_map,
                                                      unsigned long long *__restrict__ lost) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool leader = is_leader(w, v, nv);
    const uint32_t emitted = leader && w.ref[v] ? 1u : 0u;
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(emitted, wave_sum, total);
    if (!leader) return;  // the others: k_sp_map
    const uint32_t id = w.block_v[blockIdx.x] + rank;
    vertex_map[v] = emitted ? (int32_t)id : -1;
    if (!emitted) return;
    if (id >= nv_cap) { atomicAdd(lost, 1ull); return; }
    int32_t c[3];
    float f[3];
    cluster_of(vertices, v, L, c, f);
    const unsigned long long *row = w.acc + (size_t)v * 4;
    const double n = (double)row[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = (double)row[k] / n;    // -ffp-contract=off: every operation rounded on its own
        s = s * (1.0 / 1048576.0);        // exact
        s = (double)c[k] + s;
        s = (double)L.cell * s;
        s = (double)L.o[k] + s;
        out[(size_t)id * 3 + k] = (float)s;
    }
}

__global__ __launch_bounds__(kBlock) void k_sp_map(uint32_t nv, SimplifyWorkspace w, int32_t *vertex_map) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const int32_t leader = w.lead[v];
    if (leader == (int32_t)v) return;  // written by k_sp_emit_v; only such rows are read here
    vertex_map[v] = leader < 0 ? -1 : vertex_map[leader];
}

__global__ __launch_bounds__(kBlock) void k_sp_emit_t(const int32_t *__restrict__ tri, uint32_t nt, SimplifyWorkspace w,
                                                      const int32_t *__restrict__ vertex_map, int32_t *__restrict__ out,
                                                      uint32_t nt_cap, unsigned long long *__restrict__ lost) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t survives = t < nt && w.tslot[t] >= 0 ? 1u : 0u;
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(survives, wave_sum, total);
    if (!survives) return;
    const uint32_t id = w.block_t[blockIdx.x] + rank;
    if (id >= nt_cap) { atomicAdd(lost, 1ull); return; }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)id * 3 + k] = vertex_map[tri[(size_t)t * 3 + k]];  // a survivor's indices are valid
}

bool lattice_ok(const float *origin_host, float cell) {
    if (origin_host == nullptr || !(cell > 0.f) || !std::isfinite(cell)) return false;
    return std::isfinite(origin_host[0]) && std::isfinite(origin_host[1]) && std::isfinite(origin_host[2]);
}

}  // namespace

extern "C" {

size_t mi3d_mesh_simplify_workspace(unsigned long long nv, unsigned long long nt, int tight) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount) || (nv == 0 && nt == 0)) return 0;
    return bytes_of(simplify_layout, (uint32_t)nv, (uint32_t)nt, tight ? 0 : 1);
}

int mi3d_mesh_simplify_count(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             const float *origin_host, float cell, void *ws, size_t ws_bytes, unsigned long long *counts,
                             void *stream) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount) || !lattice_ok(origin_host, cell)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, bytes_of(simplify_layout, (uint32_t)nv, (uint32_t)nt, 0), counts) ||
        (nt > 0 && triangles == nullptr) || (nv > 0 && vertices == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    const uint32_t nbv = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const SimplifyWorkspace w = simplify_carve(ws, ws_bytes, n, m);
    const Lattice L = {{origin_host[0], origin_host[1], origin_host[2]}, cell};
    const unsigned long long words = w.fill_words + w.zero_words;
    const uint32_t init_blocks = (uint32_t)((words + kBlock - 1) / kBlock < kInitBlocks ? (words + kBlock - 1) / kBlock
                                                                                         : kInitBlocks);
    hipLaunchKernelGGL(k_sp_init, dim3(init_blocks), dim3(kBlock), 0, st, reinterpret_cast<unsigned long long *>(ws),
                       w.fill_words, w.zero_words, counts);
    if (n) {
        hipLaunchKernelGGL(k_sp_insert_v, dim3(nbv), dim3(kBlock), 0, st, vertices, n, L, w, counts);
        hipLaunchKernelGGL(k_sp_accum, dim3(nbv), dim3(kBlock), 0, st, vertices, n, L, w);
    }
    if (m) {
        hipLaunchKernelGGL(k_sp_insert_t, dim3(nbt), dim3(kBlock), 0, st, triangles, m, n, w, counts);
        hipLaunchKernelGGL(k_sp_flag_t, dim3(nbt), dim3(kBlock), 0, st, triangles, m, w);
    }
    if (n) hipLaunchKernelGGL(k_sp_count_v, dim3(nbv), dim3(kBlock), 0, st, n, w);
    hipLaunchKernelGGL(k_sp_scan, dim3(1), dim3(kRowThreads), 0, st, w, nbv, nbt, counts);
    return (int)hipGetLastError();
}

int mi3d_mesh_simplify_emit(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                            const float *origin_host, float cell, void *ws, size_t ws_bytes, float *out_vertices,
                            unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap,
                            int32_t *vertex_map, unsigned long long *lost, void *stream) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount) || !lattice_ok(origin_host, cell)) return (int)hipErrorInvalidValue;
    if (nv == 0) return (int)hipSuccess;  // nothing to map, and no triangle survives
    if (!state_ok(ws, ws_bytes, bytes_of(simplify_layout, (uint32_t)nv, (uint32_t)nt, 0), lost) || vertices == nullptr ||
        vertex_map == nullptr || (nt > 0 && triangles == nullptr) || (nv_cap > 0 && out_vertices == nullptr) ||
        (nt_cap > 0 && out_triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    const uint32_t nbv = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const uint32_t vcap = nv_cap > kMaxCount ? (uint32_t)kMaxCount : (uint32_t)nv_cap;
    const uint32_t tcap = nt_cap > kMaxCount ? (uint32_t)kMaxCount : (uint32_t)nt_cap;
    const hipStream_t st = as_stream(stream);
    const SimplifyWorkspace w = simplify_carve(ws, ws_bytes, n, m);
    const Lattice L = {{origin_host[0], origin_host[1], origin_host[2]}, cell};
    hipLaunchKernelGGL(k_sp_zero_lost, dim3(1), dim3(64), 0, st, lost);
    hipLaunchKernelGGL(k_sp_emit_v, dim3(nbv), dim3(kBlock), 0, st, vertices, n, L, w, out_vertices, vcap,
                       vertex_map, lost);
    hipLaunchKernelGGL(k_sp_map, dim3(nbv), dim3(kBlock), 0, st, n, w, vertex_map);
    if (m) hipLaunchKernelGGL(k_sp_emit_t, dim3(nbt), dim3(kBlock), 0, st, triangles, m, w, vertex_map,
                              out_triangles, tcap, lost);
    return (int)hipGetLastError();
}

}  // extern "C"
