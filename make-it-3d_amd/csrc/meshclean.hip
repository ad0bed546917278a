// Connected components of an indexed triangle mesh and the floater filter on top of them, for MI355X (gfx950, wave64);
// Part 13 of include/mi3d.h, which states the contract (connectivity by shared vertex INDEX, label = the smallest vertex
// index of the component, the keep rule, stable compaction).  What the `clean_mesh` step of projects of this family does
// on the CPU through pymeshlab (min_f / min_d), which is on no machine this project builds on.
//
// Compiled with -ffp-contract=off: diag2 = dx*dx + dy*dy + dz*dz is five separately rounded binary32 operations, so that
// a NumPy float32 restatement gives the same bits.
//
// Union-find with MONOTONE PARENTS.  `label` doubles as the parent array: parent[v] <= v always, and a parent only ever
// decreases.  Hence (a) a find walks a strictly decreasing chain, (b) the root of a component is its smallest index
// whatever the interleaving of the hooks, (c) a failed compare-and-swap means the root got a smaller parent, and the
// retry goes on from the value the compare-and-swap RETURNED.  No wave waits for another: no locks, no grid barriers,
// no spinning on a flag.  Every loop carries a step budget the invariant makes unreachable (nv + 1 per chain); a thread
// that exhausts it adds to counts[3] and leaves, so that a bug surfaces as an error and never as a hang.
//
// VISIBILITY.  The eight XCDs have separate L2s and a CU's L1 is never refreshed by another CU's stores: within one
// launch a load may return a parent that has since been overwritten.  Neither the result nor termination needs fresh
// values: every value a location ever held is a smaller-or-equal member of the same component (equal only while it was a
// root), so a walk over stale values still strictly descends inside the component, and a root that is one no longer is
// found out by the compare-and-swap, which is performed on memory and returns the present parent - the hook goes on from
// THAT value, never from a re-read.  k_cc_hook reads `parent` with relaxed agent-scope atomic loads (no L1) and hooks and
// splits with atomics only - that is what the code relies on for progress without re-reading; flattening is a launch of
// its own behind the hooks (the stream orders them), so its plain, cached loads see every hook.
//
// Passes of mi3d_mesh_components (thread = vertex or triangle, no host synchronisation, no allocation):
//   k_cc_init       parent[v] = v, faces[v] = 0, the box rows = the empty interval in key space; counts = 0
//   k_cc_hook       per triangle: indices checked (a bad one is counted in counts[2] and connects nothing), then the
//                   pairs (a, b) and (a, c) united: the larger root hooked under the smaller by atomicCAS; the finds
//                   split their paths by atomicMin
//   k_cc_flatten    per vertex: walk to the root, label[v] = root (in place: a half-flattened chain is still a chain)
//   k_cc_faces      per triangle: faces[label[a]] += 1    } integer atomics, order-independent; accumulated per
//   k_cc_boxes      per vertex: atomicMin / atomicMax of   } workgroup in an LDS table keyed by label first (see
//                   the coordinates' order-preserving keys } "statistics" below)
//   k_cc_finish     per vertex: label rows: keys -> floats, other rows: box = 0; per wave: 64-bit atomicMax of
//                   (faces << 32) | ~label into counts[4], counts[5] += its components with a face
// Passes of mi3d_mesh_clean_count / _emit (the structure of k_mc_count / k_mc_scan / k_mc_emit; no atomic appends):
//   k_cl_flags      per vertex: the keep rule at label rows -> flag (workspace)
//   k_cl_count_v/_t kept vertices / triangles per workgroup -> workspace
//   k_cl_scan       one workgroup: exclusive scan of both rows of block sums in place; totals -> counts[0], counts[1]
//                   (scan_row of mi3d_scan.h, which also holds block_scan)
//   k_cl_emit_v     kept again, block scan, vertex row copied to `block base + rank`, vertex_map written
//   k_cl_emit_t     kept again, block scan, triangle written with its indices mapped
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

using namespace mi3d_scan;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr unsigned long long kMaxCount = 0x7FFFFFFFull;  // nv, nt <= 2^31 - 1: indices are int32

// counts (device uint64[8]): 0 kept vertices, 1 kept triangles, 2 triangles with an index outside [0, nv), 3 threads
// that gave up, 4 (faces << 32) | ~label of the largest component, 5 components with a face, 6 elements emit could not
// place, 7 unused (0)
enum { kKeptV = 0, kKeptT = 1, kBad = 2, kGaveUp = 3, kLargest = 4, kComponents = 5, kLost = 6 };

// workspace: clean_layout of mi3d_workspace.h, the one statement of its arrays and its size
using namespace mi3d_workspace;
static_assert(kBlock == kLayoutBlock, "clean_layout sizes its rows of block sums by this workgroup");

// the order-preserving integer image of a binary32: a < b as floats <=> key(a) < key(b) as unsigned (-0 below +0).
// NaNs are never inserted, so 0xFFFFFFFF / 0 are free to mean "no minimum / no maximum yet".
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

constexpr uint32_t kNoMin = 0xFFFFFFFFu, kNoMax = 0u;

__device__ __forceinline__ bool valid_triangle(const int32_t *__restrict__ tri, uint32_t t, uint32_t nv, int32_t &a,
                                               int32_t &b, int32_t &c) {
    a = tri[(size_t)t * 3];
    b = tri[(size_t)t * 3 + 1];
    c = tri[(size_t)t * 3 + 2];
    return in_range(a, nv) && in_range(b, nv) && in_range(c, nv);
}

__device__ __forceinline__ void give_up(unsigned long long *counts) { atomicAdd(&counts[kGaveUp], 1ull); }

// ------------------------------------------------------------------------------------------------ components

__global__ __launch_bounds__(64) void k_cc_zero(unsigned long long *__restrict__ counts) {
    if (threadIdx.x < 8) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kBlock) void k_cc_init(uint32_t nv, int32_t *__restrict__ parent, uint32_t *__restrict__ faces,
                                                    uint32_t *__restrict__ key_min, uint32_t *__restrict__ key_max) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    faces[v] = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        key_min[(size_t)v * 3 + c] = kNoMin;
        key_max[(size_t)v * 3 + c] = kNoMax;
    }
}

// relaxed, agent scope: past the CU's L1, which no other CU's hook would ever refresh
__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t v) {
    return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, splitting the path on the way: every vertex passed gets its grandparent for a parent, by atomicMin, so
// that a parent still only decreases whatever another wave stored meanwhile (only a non-root is written, and a non-root
// never becomes a root again: no hook is lost).  Shorter chains for every later find: the hook pass of the 256^3 noise
// surface of DESIGN.md 17 went from 5.8 to 4.1 ms.  false = out of budget.
__device__ __forceinline__ bool find_root(int32_t *parent, int32_t &x, unsigned long long &budget) {
    int32_t p = load_parent(parent, x);
    while (p != x) {
        if (budget-- == 0) return false;
        const int32_t g = load_parent(parent, p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return true;
}

// Both chains only descend (a find step and a failed hook each move one of them to a smaller index), so 2 (nv + 1)
// steps - nv + 1 per chain - cannot be used up.  false = gave up.
__device__ bool unite(int32_t *parent, int32_t a, int32_t b, unsigned long long budget) {
    for (;;) {
        if (!find_root(parent, a, budget) || !find_root(parent, b, budget)) return false;
        if (a == b) return true;
        if (a < b) { const int32_t s = a; a = b; b = s; }
        const int32_t old = atomicCAS(parent + a, a, b);  // device scope; the larger root under the smaller
        if (old == a) return true;
        if (budget-- == 0) return false;
        a = old;  // the root got a smaller parent meanwhile: go on from it, not from a value read again
    }
}

__global__ __launch_bounds__(kBlock) void k_cc_hook(const int32_t *__restrict__ tri, uint32_t nt, uint32_t nv,
                                                    int32_t *parent, unsigned long long *__restrict__ counts) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    int32_t a, b, c;
    if (!valid_triangle(tri, t, nv, a, b, c)) {
        atomicAdd(&counts[kBad], 1ull);
        return;
    }
    const unsigned long long budget = 2ull * ((unsigned long long)nv + 1);
    if (!unite(parent, a, b, budget) || !unite(parent, a, c, budget)) give_up(counts);
}

// In place: label[v] is overwritten by the root while other threads may still walk through v - they read the old parent
// or the root, both ancestors.  Roots do not change in this launch (no hooks), so every walk ends at the minimum.
__global__ __launch_bounds__(kBlock) void k_cc_flatten(uint32_t nv, int32_t *label, unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    int32_t r = (int32_t)v;
    uint32_t budget = nv + 1;
    for (int32_t p; (p = label[r]) != r; r = p)
        if (budget-- == 0) { give_up(counts); return; }
    label[v] = r;
}

// ---- statistics.  A large component is cited by most triangles and owns most vertices, and a few million atomics on
// one address take hundreds of milliseconds (measured: DESIGN.md 17).  So every workgroup first accumulates in a table
// of its own in LDS, keyed by label (open addressing, kProbes probes; what finds no slot goes to global memory at
// once - those are the small components, spread over many addresses), walks the input with a grid stride from at most
// kStatBlocks workgroups, and adds its table to global memory once at the end: a hot address sees at most kStatBlocks
// atomics per launch.  Inside a wave the lanes that share the first live lane's label are reduced by shuffles before
// they touch the table.  Integer add / min / max throughout: the result does not depend on any of this.

constexpr int kSlots = 512, kProbes = 4;
constexpr uint32_t kStatBlocks = 512;

__device__ __forceinline__ void table_init(int32_t *keys) {
    for (int s = threadIdx.x; s < kSlots; s += kBlock) keys[s] = -1;
}

// the slot of `label` in the workgroup's table, claimed if need be; -1: no room within kProbes
__device__ __forceinline__ int slot_of(int32_t *keys, int32_t label) {
    const uint32_t h = ((uint32_t)label * 2654435761u) >> 16;
    for (int probe = 0; probe < kProbes; ++probe) {
        const int s = (int)((h + probe) & (kSlots - 1));
        int32_t k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == -1) k = atomicCAS(&keys[s], -1, label);
        if (k == -1 || k == label) return s;
    }
    return -1;
}

__global__ __launch_bounds__(kBlock) void k_cc_faces(const int32_t *__restrict__ tri, uint32_t nt, uint32_t nv,
                                                     const int32_t *__restrict__ label, uint32_t *__restrict__ faces) {
    __shared__ int32_t keys[kSlots];
    __shared__ uint32_t sums[kSlots];
    table_init(keys);
    for (int s = threadIdx.x; s < kSlots; s += kBlock) sums[s] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * kBlock; base < nt; base += gridDim.x * kBlock) {  // uniform over the workgroup
        const uint32_t t = base + threadIdx.x;
        int32_t a, b, c;
        const bool ok = t < nt && valid_triangle(tri, t, nv, a, b, c);
        const int32_t l = ok ? label[a] : -1;
        const unsigned long long live = __ballot(ok);
        if (live == 0) continue;
        const int leader = __ffsll(live) - 1;
        const int32_t first = __shfl(l, leader, 64);
        const bool same = ok && l == first;
        const uint32_t group = (uint32_t)__popcll(__ballot(same));  // by all lanes, ahead of the divergence
        const uint32_t n = lane == leader ? group : 1u;
        if (ok && (!same || lane == leader)) {
            const int s = slot_of(keys, l);
            if (s >= 0) atomicAdd(&sums[s], n);
            else atomicAdd(&faces[l], n);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots; s += kBlock)
        if (keys[s] >= 0 && sums[s] != 0) atomicAdd(&faces[keys[s]], sums[s]);
}

// atomicMin / atomicMax into global memory unless the value read there is already as good: the extremes only move
// outwards during the launch, so a value that was good enough - however stale - stays good enough
__device__ __forceinline__ void global_min(uint32_t *p, uint32_t k) {
    if (k != kNoMin && k < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, k);
}

__device__ __forceinline__ void global_max(uint32_t *p, uint32_t k) {
    if (k != kNoMax && k > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, k);
}

__global__ __launch_bounds__(kBlock) void k_cc_boxes(const float *__restrict__ vertices, uint32_t nv,
                                                     const int32_t *__restrict__ label, uint32_t *key_min,
                                                     uint32_t *key_max) {
    __shared__ int32_t keys[kSlots];
    __shared__ uint32_t los[kSlots][3], his[kSlots][3];
    table_init(keys);
    for (int s = threadIdx.x; s < kSlots * 3; s += kBlock) {
        los[s / 3][s % 3] = kNoMin;
        his[s / 3][s % 3] = kNoMax;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * kBlock; base < nv; base += gridDim.x * kBlock) {  // uniform over the workgroup
        const uint32_t v = base + threadIdx.x;
        const bool ok = v < nv;
        const int32_t l = ok ? label[v] : -1;
        const int32_t first = __shfl(l, 0, 64);  // lane 0 is live: vertices fill a wave from its first lane
        const bool same = ok && l == first;
        uint32_t lo[3], hi[3], glo[3], ghi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = ok ? vertices[(size_t)v * 3 + c] : __uint_as_float(0x7FC00000u);
            const bool num = x == x;  // a NaN coordinate is ignored
            lo[c] = num ? float_key(x) : kNoMin;
            hi[c] = num ? float_key(x) : kNoMax;
            glo[c] = same ? lo[c] : kNoMin;  // the first lane's group: all 64 lanes take part, the others hold the
            ghi[c] = same ? hi[c] : kNoMax;  // neutral keys
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                glo[c] = min(glo[c], (uint32_t)__shfl_xor(glo[c], off, 64));
                ghi[c] = max(ghi[c], (uint32_t)__shfl_xor(ghi[c], off, 64));
            }
        if (!ok || (same && lane != 0)) continue;
        const int s = slot_of(keys, l);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t kl = same ? glo[c] : lo[c], kh = same ? ghi[c] : hi[c];
            if (s >= 0) {
                if (kl != kNoMin) atomicMin(&los[s][c], kl);
                if (kh != kNoMax) atomicMax(&his[s][c], kh);
            } else {
                global_min(&key_min[(size_t)l * 3 + c], kl);
                global_max(&key_max[(size_t)l * 3 + c], kh);
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kSlots * 3; s += kBlock) {
        const int32_t row = keys[s / 3];
        if (row < 0) continue;
        global_min(&key_min[(size_t)row * 3 + s % 3], los[s / 3][s % 3]);
        global_max(&key_max[(size_t)row * 3 + s % 3], his[s / 3][s % 3]);
    }
}

// Grid stride from at most kStatBlocks workgroups, like the two kernels above: the largest component and the component
// count are kept in registers and reach counts with one atomic each per wave (a quarter of a million components sending
// theirs one by one took 3.5 ms).
__global__ __launch_bounds__(kBlock) void k_cc_finish(uint32_t nv, const int32_t *__restrict__ label,
                                                      const uint32_t *__restrict__ faces, uint32_t *__restrict__ box_min,
                                                      uint32_t *__restrict__ box_max,
                                                      unsigned long long *__restrict__ counts) {
    unsigned long long key = 0;
    uint32_t faced = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < nv; base += gridDim.x * kBlock) {
        const uint32_t v = base + threadIdx.x;
        if (v >= nv) break;
        const bool root = label[v] == (int32_t)v;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t lo = box_min[(size_t)v * 3 + c], hi = box_max[(size_t)v * 3 + c];
            const bool any = root && lo != kNoMin;  // an axis without a number: the interval [0, 0]
            box_min[(size_t)v * 3 + c] = any ? __float_as_uint(key_float(lo)) : 0u;
            box_max[(size_t)v * 3 + c] = any ? __float_as_uint(key_float(hi)) : 0u;
        }
        const uint32_t f = root ? faces[v] : 0u;
        if (f >= 1) {
            const unsigned long long mine = ((unsigned long long)f << 32) | (uint32_t)~v;
            key = mine > key ? mine : key;
            ++faced;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {  // all 64 lanes are back here
        const unsigned long long other = __shfl_xor(key, off, 64);
        key = other > key ? other : key;
        faced += __shfl_xor(faced, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && faced != 0) {
        atomicMax(&counts[kLargest], key);
        atomicAdd(&counts[kComponents], (unsigned long long)faced);
    }
}

// ------------------------------------------------------------------------------------------------ the filter

struct KeepRule {
    uint32_t min_faces;
    float min_diag2;  // min_diagonal * min_diagonal, rounded once (on the host: one binary32 multiply)
    int largest;
};

__global__ __launch_bounds__(kBlock) void k_cl_flags(uint32_t nv, const int32_t *__restrict__ label,
                                                     const uint32_t *__restrict__ faces, const float *__restrict__ box_min,
                                                     const float *__restrict__ box_max, KeepRule rule,
                                                     const unsigned long long *__restrict__ counts,
                                                     uint8_t *__restrict__ flag) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    bool keep = false;
    if (label[v] == (int32_t)v) {
        const uint32_t f = faces[v];
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d[c] = box_max[(size_t)v * 3 + c] - box_min[(size_t)v * 3 + c];
            if (d[c] != d[c]) d[c] = 0.f;  // both ends the same infinity
        }
        const float diag2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];  // -ffp-contract=off: left to right, no fma
        keep = f >= 1 && f >= rule.min_faces && diag2 >= rule.min_diag2;
        if (rule.largest) keep = keep && counts[kLargest] == (((unsigned long long)f << 32) | (uint32_t)~v);
    }
    flag[v] = keep ? 1 : 0;
}

__device__ __forceinline__ uint32_t kept_vertex(uint32_t v, uint32_t nv, const int32_t *__restrict__ label,
                                                const uint8_t *__restrict__ flag) {
    return v < nv ? flag[label[v]] : 0u;
}

__device__ __forceinline__ uint32_t kept_triangle(const int32_t *__restrict__ tri, uint32_t t, uint32_t nt, uint32_t nv,
                                                  const int32_t *__restrict__ label, const uint8_t *__restrict__ flag,
                                                  int32_t &a, int32_t &b, int32_t &c) {
    return t < nt && valid_triangle(tri, t, nv, a, b, c) ? flag[label[a]] : 0u;
}

__global__ __launch_bounds__(kBlock) void k_cl_count_v(uint32_t nv, const int32_t *__restrict__ label, CleanWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    uint32_t total;
    block_scan<kWaves>(kept_vertex(blockIdx.x * kBlock + threadIdx.x, nv, label, w.flag), wave_sum, total);
    if (threadIdx.x == 0) w.block_v[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_cl_count_t(const int32_t *__restrict__ tri, uint32_t nt, uint32_t nv,
                                                       const int32_t *__restrict__ label, CleanWorkspace w) {
    __shared__ uint32_t wave_sum[kWaves];
    int32_t a, b, c;
    uint32_t total;
    block_scan<kWaves>(kept_triangle(tri, blockIdx.x * kBlock + threadIdx.x, nt, nv, label, w.flag, a, b, c), wave_sum,
                       total);
    if (threadIdx.x == 0) w.block_t[blockIdx.x] = total;
}

// both rows of block sums scanned in place (at most 8 M sums each).  Sums are at most 2^31 - 1: 32 bits hold every
// offset.
__global__ __launch_bounds__(kRowThreads) void k_cl_scan(CleanWorkspace w, uint32_t nbv, uint32_t nbt,
                                                  unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    const uint32_t kv = scan_row(w.block_v, nbv, wave_sum, &base);
    __syncthreads();
    const uint32_t kt = scan_row(w.block_t, nbt, wave_sum, &base);
    if (threadIdx.x == 0) { counts[kKeptV] = kv; counts[kKeptT] = kt; counts[kLost] = 0; }
}

__global__ __launch_bounds__(kBlock) void k_cl_emit_v(const float *__restrict__ vertices, uint32_t nv,
                                                      const int32_t *__restrict__ label, CleanWorkspace w,
                                                      float *__restrict__ out, uint32_t nv_cap,
                                                      int32_t *__restrict__ vertex_map,
                                                      unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t kept = kept_vertex(v, nv, label, w.flag);
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(kept, wave_sum, total);
    if (v >= nv) return;
    const uint32_t id = w.block_v[blockIdx.x] + rank;
    vertex_map[v] = kept ? (int32_t)id : -1;
    if (!kept) return;
    if (id >= nv_cap) { atomicAdd(&counts[kLost], 1ull); return; }
    const uint32_t *src = reinterpret_cast<const uint32_t *>(vertices) + (size_t)v * 3;  // bit for bit
    uint32_t *dst = reinterpret_cast<uint32_t *>(out) + (size_t)id * 3;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
}

__global__ __launch_bounds__(kBlock) void k_cl_emit_t(const int32_t *__restrict__ tri, uint32_t nt, uint32_t nv,
                                                      const int32_t *__restrict__ label, CleanWorkspace w,
                                                      const int32_t *__restrict__ vertex_map, int32_t *__restrict__ out,
                                                      uint32_t nt_cap, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    int32_t a = 0, b = 0, c = 0;
    const uint32_t kept = kept_triangle(tri, t, nt, nv, label, w.flag, a, b, c);
    uint32_t total;
    const uint32_t rank = block_scan<kWaves>(kept, wave_sum, total);
    if (!kept) return;
    const uint32_t id = w.block_t[blockIdx.x] + rank;
    if (id >= nt_cap) { atomicAdd(&counts[kLost], 1ull); return; }
    int32_t *o = out + (size_t)id * 3;  // a kept triangle's three vertices lie in its kept component
    o[0] = vertex_map[a];
    o[1] = vertex_map[b];
    o[2] = vertex_map[c];
}

}  // namespace

extern "C" {

size_t mi3d_mesh_components_workspace(unsigned long long nv, unsigned long long nt) {
    return sizes_ok(nv, nt, kMaxCount, kMaxCount) ? bytes_of(clean_layout, (uint32_t)nv, (uint32_t)nt) : 0;
}

int mi3d_mesh_components(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         int32_t *label, uint32_t *faces, float *box_min, float *box_max, unsigned long long *counts,
                         void *stream) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (counts == nullptr || !aligned8(counts) || (nt > 0 && triangles == nullptr) ||
        (nv > 0 && (vertices == nullptr || label == nullptr || faces == nullptr || box_min == nullptr || box_max == nullptr)))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    const uint32_t nbv = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    uint32_t *kmin = reinterpret_cast<uint32_t *>(box_min), *kmax = reinterpret_cast<uint32_t *>(box_max);
    hipLaunchKernelGGL(k_cc_zero, dim3(1), dim3(64), 0, st, counts);
    if (n) hipLaunchKernelGGL(k_cc_init, dim3(nbv), dim3(kBlock), 0, st, n, label, faces, kmin, kmax);
    if (m) hipLaunchKernelGGL(k_cc_hook, dim3(nbt), dim3(kBlock), 0, st, triangles, m, n, label, counts);
    if (n) hipLaunchKernelGGL(k_cc_flatten, dim3(nbv), dim3(kBlock), 0, st, n, label, counts);
    if (m && n)
        hipLaunchKernelGGL(k_cc_faces, dim3(min(nbt, kStatBlocks)), dim3(kBlock), 0, st, triangles, m, n, label,
                           faces);
    if (n) {
        hipLaunchKernelGGL(k_cc_boxes, dim3(min(nbv, kStatBlocks)), dim3(kBlock), 0, st, vertices, n, label, kmin,
                           kmax);
        hipLaunchKernelGGL(k_cc_finish, dim3(min(nbv, kStatBlocks)), dim3(kBlock), 0, st, n, label, faces, kmin,
                           kmax, counts);
    }
    return (int)hipGetLastError();
}

int mi3d_mesh_clean_count(const int32_t *triangles, unsigned long long nv, unsigned long long nt, const int32_t *label,
                          const uint32_t *faces, const float *box_min, const float *box_max, uint32_t min_faces,
                          float min_diagonal, int largest, void *ws, size_t ws_bytes, unsigned long long *counts,
                          void *stream) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount) || !(min_diagonal >= 0.f)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, bytes_of(clean_layout, (uint32_t)nv, (uint32_t)nt), counts) ||
        (nt > 0 && triangles == nullptr) ||
        (nv > 0 && (label == nullptr || faces == nullptr || box_min == nullptr || box_max == nullptr)))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    const uint32_t nbv = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const CleanWorkspace w = at(ws, clean_layout, n, m);
    const KeepRule rule = {min_faces, min_diagonal * min_diagonal, largest != 0};
    if (n) {
        hipLaunchKernelGGL(k_cl_flags, dim3(nbv), dim3(kBlock), 0, st, n, label, faces, box_min, box_max, rule,
                           counts, w.flag);
        hipLaunchKernelGGL(k_cl_count_v, dim3(nbv), dim3(kBlock), 0, st, n, label, w);
    }
    if (m && n) hipLaunchKernelGGL(k_cl_count_t, dim3(nbt), dim3(kBlock), 0, st, triangles, m, n, label, w);
    // without vertices no triangle is valid: its row of block sums is not scanned (and never read)
    hipLaunchKernelGGL(k_cl_scan, dim3(1), dim3(kRowThreads), 0, st, w, nbv, n ? nbt : 0u, counts);
    return (int)hipGetLastError();
}

int mi3d_mesh_clean_emit(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         const int32_t *label, void *ws, size_t ws_bytes, unsigned long long *counts, float *out_vertices,
                         unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap, int32_t *vertex_map,
                         void *stream) {
    if (!sizes_ok(nv, nt, kMaxCount, kMaxCount)) return (int)hipErrorInvalidValue;
    if (nv == 0) return (int)hipSuccess;  // nothing to map, and no triangle is valid
    if (!state_ok(ws, ws_bytes, bytes_of(clean_layout, (uint32_t)nv, (uint32_t)nt), counts) || vertices == nullptr ||
        label == nullptr || vertex_map == nullptr || (nt > 0 && triangles == nullptr) ||
        (nv_cap > 0 && out_vertices == nullptr) || (nt_cap > 0 && out_triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    const uint32_t nbv = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const uint32_t vcap = nv_cap > kMaxCount ? (uint32_t)kMaxCount : (uint32_t)nv_cap;
    const uint32_t tcap = nt_cap > kMaxCount ? (uint32_t)kMaxCount : (uint32_t)nt_cap;
    const hipStream_t st = as_stream(stream);
    const CleanWorkspace w = at(ws, clean_layout, n, m);
    hipLaunchKernelGGL(k_cl_emit_v, dim3(nbv), dim3(kBlock), 0, st, vertices, n, label, w, out_vertices, vcap,
                       vertex_map, counts);
    if (m) hipLaunchKernelGGL(k_cl_emit_t, dim3(nbt), dim3(kBlock), 0, st, triangles, m, n, label, w, vertex_map,
                              out_triangles, tcap, counts);
    return (int)hipGetLastError();
}

}  // extern "C"
