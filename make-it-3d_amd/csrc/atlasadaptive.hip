// The area-adaptive texture atlas for MI355X (gfx950): Part 20 of include/mi3d.h, which states the contract (bins, the
// ladder of legs, the plan, the sort, ownership, UV corners, the point formula).  Part 9's atlas (texture.hip) gives
// every triangle the same patch; here a triangle's patch has legs that follow its two shorter edges, so that a mesh
// after edge collapse gets about the same number of texels per unit length everywhere.  vt, xyz and owner keep Part 9's
// formats: mi3d_texture_pack, mi3d_texture_project and the mesh render consume them unchanged.
//
// Compiled with -ffp-contract=off: squared edge lengths are (dx dx + dy dy) + dz dz and a texel's point is
// A' + s (B' - A') + t (C' - A') as separately rounded binary32 operations, so that a NumPy float32 restatement gives
// the same bits.  All counters are integers; no float atomics: two runs give the same bytes.
//
// Kernels:
//   k_measure    thread = triangle: rot and the two bins -> the shape word; a 64 x 64 histogram in LDS per workgroup,
//                merged with one integer atomic per occupied bin
//   k_sort<0>    per workgroup and key (kb * 16 + ka) the number of its triangles -> counts[key][workgroup]
//   k_sort_scan  workgroup = key: the exclusive scan of its row of counts (mi3d_scan.h's scan_row) on top of the class's
//                start in the plan
//   k_sort<1>    slot = the row's offset + the rank among the workgroup's triangles of the same key (stable)
//   k_uv         thread = triangle: its three unshared vt, rows in the ORIGINAL corner order
//   k_positions  thread = texel of a band of image rows: height group by row, class by position in the group's strip of
//                shelves, cell, half, triangle; owner and the ssaa^2 sample points as texture.hip writes them
// The plan itself is host arithmetic (mi3d_atlas_adaptive.h), uploaded by the caller: 3472 words are too many for kernel
// arguments.  Whatever the plan holds, no kernel writes outside its outputs: every index that addresses an output or
// triangle_of is compared with its bound first.
#include <hip/hip_runtime.h>

#define MI3D_HD __host__ __device__
#include "../../include/mi3d.h"
#include "mi3d_atlas_adaptive.h"
#include "mi3d_scan.h"

namespace {

namespace at = mi3d_atlas;
using mi3d_scan::as_stream;
using mi3d_scan::in_range;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr unsigned long long kMaxCount = 0x7FFFFFFFull;

static_assert(at::kPlanWords == MI3D_ATLAS_PLAN_WORDS, "mi3d.h states the plan's size");

__device__ __forceinline__ float sq_len(const float *p, const float *q) {
    const float dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(kBlock) void k_measure(const float *__restrict__ vertices, uint32_t nv,
                                                    const int32_t *__restrict__ triangles, uint32_t nt,
                                                    uint32_t *__restrict__ shape, uint32_t *__restrict__ hist,
                                                    unsigned long long *__restrict__ bad) {
    __shared__ uint32_t h[at::kBins * at::kBins];
    for (int j = threadIdx.x; j < at::kBins * at::kBins; j += kBlock) h[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool is_bad = false;
    if (i < nt) {
        const int32_t *t = triangles + (size_t)i * 3;
        const int32_t id[3] = {t[0], t[1], t[2]};
        int rot = 0, binAB = 0, binAC = 0;
        is_bad = !(in_range(id[0], nv) && in_range(id[1], nv) && in_range(id[2], nv));  // never dereferenced
        if (!is_bad) {
            float p[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int d = 0; d < 3; ++d) p[k][d] = vertices[(size_t)id[k] * 3 + d];
            // edge k is the one opposite corner k
            const float l0 = sq_len(p[1], p[2]), l1 = sq_len(p[2], p[0]), l2 = sq_len(p[0], p[1]);
            float longest = l0;
            if (l1 > longest) { rot = 1; longest = l1; }
            if (l2 > longest) rot = 2;
            // A'B' is the edge opposite corner rot + 2, A'C' the one opposite corner rot + 1
            const float lAB = rot == 0 ? l2 : rot == 1 ? l0 : l1, lAC = rot == 0 ? l1 : rot == 1 ? l2 : l0;
            binAB = at::bin_of_bits(__float_as_uint(lAB));
            binAC = at::bin_of_bits(__float_as_uint(lAC));
        }
        shape[i] = at::shape_word(rot, binAB, binAC, is_bad);
        atomicAdd(&h[binAC * at::kBins + binAB], 1u);
    }
    mi3d_scan::wave_count(is_bad, bad);
    __syncthreads();
    for (int j = threadIdx.x; j < at::kBins * at::kBins; j += kBlock)
        if (h[j] != 0) atomicAdd(&hist[j], h[j]);
}

struct PlanHead {
    int shift, kmax;
};

// what the kernels take from the plan's head, kept inside the ranges the keys assume
__device__ __forceinline__ PlanHead plan_head(const int32_t *__restrict__ plan) {
    const int s = plan[at::H_SHIFT], k = plan[at::H_KMAX];
    return {s & 63, k < 0 ? 0 : k > at::kClasses - 1 ? at::kClasses - 1 : k};
}

// the record of a key, or null
__device__ __forceinline__ const int32_t *class_record(const int32_t *__restrict__ plan, int key) {
    const int rec = plan[at::kIndex + key];
    return (uint32_t)rec < 256u ? plan + at::kRecords + rec * at::kClassWords : nullptr;
}

template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void k_sort(const uint32_t *__restrict__ shape, uint32_t nt,
                                                 const int32_t *__restrict__ plan, uint32_t nb,
                                                 uint32_t *__restrict__ counts, uint32_t *__restrict__ slot,
                                                 uint32_t *__restrict__ triangle_of) {
    __shared__ uint32_t wc[kWaves][256];  // triangles per wave and key
    for (int j = threadIdx.x; j < kWaves * 256; j += kBlock) (&wc[0][0])[j] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool valid = i < nt;
    const PlanHead ph = plan_head(plan);
    const int key = valid ? at::shape_key(shape[i], ph.shift, ph.kmax) : 0;
    unsigned long long same = __ballot(valid);  // the wave's lanes with this lane's key
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool set = (key >> bit) & 1;
        const unsigned long long m = __ballot(set);
        same &= set ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wc[wave][key] = (uint32_t)__popcll(same);
    __syncthreads();
    if (!SCATTER) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) n += wc[w][threadIdx.x];
        counts[(size_t)threadIdx.x * nb + blockIdx.x] = n;
    } else if (valid) {
        uint32_t off = counts[(size_t)key * nb + blockIdx.x] + rank;
        for (int w = 0; w < wave; ++w) off += wc[w][key];
        if (off < nt) {
            slot[i] = off;
            triangle_of[off] = i;
        }
    }
}

__global__ __launch_bounds__(mi3d_scan::kRowThreads) void k_sort_scan(uint32_t *__restrict__ counts, uint32_t nb,
                                                                      const int32_t *__restrict__ plan) {
    __shared__ uint32_t wave_sum[mi3d_scan::kRowWaves], base;
    const int key = blockIdx.x;
    const int32_t *c = class_record(plan, key);
    const uint32_t start = c != nullptr ? (uint32_t)c[at::C_START] : 0u;
    uint32_t *row = counts + (size_t)key * nb;
    mi3d_scan::scan_row(row, nb, wave_sum, &base, [row, start](uint32_t b, uint32_t offset) { row[b] = start + offset; });
}

__global__ __launch_bounds__(kBlock) void k_uv(const uint32_t *__restrict__ shape, const uint32_t *__restrict__ slot,
                                               uint32_t nt, const int32_t *__restrict__ plan, uint32_t T,
                                               float *__restrict__ vt) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nt) return;
    const PlanHead ph = plan_head(plan);
    const uint32_t w = shape[i];
    const int32_t *c = class_record(plan, at::shape_key(w, ph.shift, ph.kmax));
    float *o = vt + (size_t)i * 6;
    if (c == nullptr) {  // a plan made for another histogram
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = 0.0f;
        return;
    }
    const uint32_t r = slot[i] - (uint32_t)c[at::C_START], a = (uint32_t)c[at::C_A], b = (uint32_t)c[at::C_B];
    uint32_t X0, Y0;
    at::cell_origin(c, T, r >> 1, X0, Y0);
    const bool half = r & 1u;
    const int rot = at::shape_rot(w) % 3;
    const float fT = (float)T;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // original corner k is A', B', C' for j = 0, 1, 2: at the centres of local texels (0, 0) (a, 0) (0, b)
        const int j = (k - rot + 3) % 3;
        const uint32_t lx = j == 1 ? a : 0u, ly = j == 2 ? b : 0u;
        const uint32_t x = half ? a + 2 - lx : lx, y = half ? b + 2 - ly : ly;
        o[2 * k] = ((float)(X0 + x) + 0.5f) / fT;
        o[2 * k + 1] = 1.0f - ((float)(Y0 + y) + 0.5f) / fT;
    }
}

__device__ __forceinline__ float clamp_box(float p) { return fminf(fmaxf(p, -1.0f), 1.0f); }

template <int SS>
__global__ __launch_bounds__(kBlock) void k_positions(const float *__restrict__ vertices, uint32_t nv,
                                                      const int32_t *__restrict__ triangles, uint32_t nt,
                                                      const uint32_t *__restrict__ shape,
                                                      const uint32_t *__restrict__ triangle_of,
                                                      const int32_t *__restrict__ plan, uint32_t T, uint32_t row0,
                                                      float *__restrict__ xyz, int32_t *__restrict__ owner) {
    const uint32_t X = blockIdx.x * kBlock + threadIdx.x, ry = blockIdx.y;
    if (X >= T) return;
    const uint32_t Y = row0 + ry;
    const size_t texel = (size_t)ry * T + X;
    float *o = xyz + texel * (size_t)(3 * SS * SS);

    int32_t own = -1;
    uint32_t u = 0, v = 0, a = 1, b = 1;
    int32_t id[3] = {0, 0, 0};
    // the height group by row: at most 16 steps
    const int groups = min(max(plan[at::H_GROUPS], 0), at::kClasses);
    const int32_t *gr = nullptr;
    for (int g = 0; g < groups; ++g) {
        const int32_t *cand = plan + at::kGroups + g * at::kGroupWords;
        const uint32_t y0 = (uint32_t)cand[at::G_Y0], h = (uint32_t)cand[at::G_HEIGHT], n = (uint32_t)cand[at::G_SHELVES];
        if (Y >= y0 && (unsigned long long)(Y - y0) < (unsigned long long)n * h) gr = cand;
    }
    if (gr != nullptr && gr[at::G_HEIGHT] > 0) {
        const uint32_t h = (uint32_t)gr[at::G_HEIGHT], shelf = (Y - (uint32_t)gr[at::G_Y0]) / h;
        const uint32_t y = (Y - (uint32_t)gr[at::G_Y0]) - shelf * h;
        const unsigned long long pos = (unsigned long long)shelf * T + X;
        // the class by position in the group's strip of shelves: the last one that starts at or before this texel
        const int first = min(max(gr[at::G_FIRST], 0), 256), last = min(first + max(gr[at::G_COUNT], 0), 256);
        const int32_t *c = nullptr;
        for (int j = first; j < last; ++j) {
            const int32_t *cand = plan + at::kRecords + j * at::kClassWords;
            if ((unsigned long long)(uint32_t)cand[at::C_SHELF0] * T + (uint32_t)cand[at::C_X0] <= pos) c = cand;
        }
        if (c != nullptr && c[at::C_A] > 0 && c[at::C_B] > 0 && (uint32_t)c[at::C_B] + 3u == h && c[at::C_PER] > 0) {
            a = (uint32_t)c[at::C_A];
            b = (uint32_t)c[at::C_B];
            const uint32_t w = a + 3, sh0 = (uint32_t)c[at::C_SHELF0], n0 = (uint32_t)c[at::C_N0];
            uint32_t q, x;
            bool inside;
            if (shelf == sh0) {
                const uint32_t xr = X - (uint32_t)c[at::C_X0];
                q = xr / w;
                x = xr - q * w;
                inside = q < n0;
            } else {
                const uint32_t col = X / w;
                x = X - col * w;
                inside = col < (uint32_t)c[at::C_PER];
                q = n0 + (shelf - sh0 - 1) * (uint32_t)c[at::C_PER] + col;
            }
            const int half = at::half_of((int)a, (int)b, (int)x, (int)y);
            if (inside && q < (uint32_t)c[at::C_CELLS] && half >= 0) {
                const uint32_t r = 2 * q + (uint32_t)half;
                const unsigned long long idx = (unsigned long long)(uint32_t)c[at::C_START] + r;
                if (r < (uint32_t)c[at::C_COUNT] && idx < nt) {  // the missing partner of an odd count owns nothing
                    const uint32_t i = triangle_of[idx];
                    if (i < nt) {
                        const uint32_t word = shape[i];
                        const int rot = at::shape_rot(word) % 3;
                        const int32_t *t = triangles + (size_t)i * 3;
                        id[0] = t[rot]; id[1] = t[(rot + 1) % 3]; id[2] = t[(rot + 2) % 3];
                        // an index outside [0, nv) is never dereferenced: the triangle owns nothing (k_measure counted it)
                        if (in_range(id[0], nv) && in_range(id[1], nv) && in_range(id[2], nv)) own = (int32_t)i;
                        u = half ? a + 2 - x : x;
                        v = half ? b + 2 - y : y;
                    }
                }
            }
        }
    }
    if (owner != nullptr) owner[texel] = own;
    if (own < 0) {
#pragma unroll
        for (int k = 0; k < 3 * SS * SS; ++k) o[k] = 0.0f;
        return;
    }
    const float *A = vertices + (size_t)id[0] * 3, *B = vertices + (size_t)id[1] * 3, *Cc = vertices + (size_t)id[2] * 3;
    float pa[3], e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        pa[d] = A[d];
        e1[d] = B[d] - pa[d];
        e2[d] = Cc[d] - pa[d];
    }
    const float fa = (float)a, fb = (float)b;
#pragma unroll
    for (int j = 0; j < SS; ++j) {
#pragma unroll
        for (int i = 0; i < SS; ++i) {
            // (i + 0.5) / SS - 0.5 is exact in binary32 for SS in {1, 2, 4}, and so is its sum with a small integer
            const float s = ((float)u + ((i + 0.5f) / SS - 0.5f)) / fa, t = ((float)v + ((j + 0.5f) / SS - 0.5f)) / fb;
#pragma unroll
            for (int d = 0; d < 3; ++d) o[(j * SS + i) * 3 + d] = clamp_box((pa[d] + s * e1[d]) + t * e2[d]);
        }
    }
}

size_t sort_workspace(unsigned long long nt) {
    if (nt == 0 || nt > kMaxCount) return 0;
    return mi3d_scan::pad8((size_t)256 * mi3d_scan::blocks_of((uint32_t)nt, kBlock) * sizeof(uint32_t));
}

bool size_ok(uint32_t T) { return T >= at::kMinT && T <= at::kMaxT; }

}  // namespace

extern "C" {

size_t mi3d_atlas_adaptive_workspace(unsigned long long nt) { return sort_workspace(nt); }

uint32_t mi3d_atlas_adaptive_plan(const uint32_t *hist_host, uint32_t T, int32_t *plan_host) {
    return at::make_plan(hist_host, T, plan_host);
}

int mi3d_atlas_adaptive_owner(uint32_t ka, uint32_t kb, uint32_t x, uint32_t y) {
    if (ka >= (uint32_t)at::kClasses || kb >= (uint32_t)at::kClasses) return -2;
    const int a = at::leg((int)ka), b = at::leg((int)kb);
    if (x > (uint32_t)a + 2u || y > (uint32_t)b + 2u) return -2;
    return at::half_of(a, b, (int)x, (int)y);
}

int mi3d_atlas_adaptive_measure(const float *vertices, unsigned long long nv, const int32_t *triangles,
                                unsigned long long nt, uint32_t *shape, uint32_t *hist, unsigned long long *bad,
                                void *stream) {
    if (vertices == nullptr || triangles == nullptr || shape == nullptr || hist == nullptr || bad == nullptr ||
        !mi3d_scan::aligned8(bad) || nv == 0 || nv > kMaxCount || nt == 0 || nt > kMaxCount)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_measure, dim3(mi3d_scan::blocks_of((uint32_t)nt, kBlock)), dim3(kBlock), 0, as_stream(stream),
                       vertices, (uint32_t)nv, triangles, (uint32_t)nt, shape, hist, bad);
    return (int)hipGetLastError();
}

int mi3d_atlas_adaptive_sort(const uint32_t *shape, unsigned long long nt, const int32_t *plan, void *ws, size_t ws_bytes,
                             uint32_t *slot, uint32_t *triangle_of, void *stream) {
    const size_t need = sort_workspace(nt);
    if (need == 0 || shape == nullptr || plan == nullptr || slot == nullptr || triangle_of == nullptr || ws == nullptr ||
        !mi3d_scan::aligned8(ws) || ws_bytes < need)
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nt, nb = mi3d_scan::blocks_of(n, kBlock);
    uint32_t *counts = static_cast<uint32_t *>(ws);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_sort<false>, dim3(nb), dim3(kBlock), 0, st, shape, n, plan, nb, counts, slot, triangle_of);
    hipLaunchKernelGGL(k_sort_scan, dim3(256), dim3(mi3d_scan::kRowThreads), 0, st, counts, nb, plan);
    hipLaunchKernelGGL(k_sort<true>, dim3(nb), dim3(kBlock), 0, st, shape, n, plan, nb, counts, slot, triangle_of);
    return (int)hipGetLastError();
}

int mi3d_atlas_adaptive_uv(const uint32_t *shape, const uint32_t *slot, unsigned long long nt, const int32_t *plan,
                           uint32_t T, float *vt, void *stream) {
    if (shape == nullptr || slot == nullptr || plan == nullptr || vt == nullptr || nt == 0 || nt > kMaxCount || !size_ok(T))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_uv, dim3(mi3d_scan::blocks_of((uint32_t)nt, kBlock)), dim3(kBlock), 0, as_stream(stream), shape,
                       slot, (uint32_t)nt, plan, T, vt);
    return (int)hipGetLastError();
}

int mi3d_atlas_adaptive_positions(const float *vertices, unsigned long long nv, const int32_t *triangles,
                                  unsigned long long nt, const uint32_t *shape, const uint32_t *triangle_of,
                                  const int32_t *plan, uint32_t T, uint32_t ssaa, uint32_t row0, uint32_t rows, float *xyz,
                                  int32_t *owner, void *stream) {
    if (vertices == nullptr || triangles == nullptr || shape == nullptr || triangle_of == nullptr || plan == nullptr ||
        xyz == nullptr || nv == 0 || nv > kMaxCount || nt == 0 || nt > kMaxCount || !size_ok(T) ||
        (ssaa != 1 && ssaa != 2 && ssaa != 4) || rows < 1 || row0 >= T || rows > T - row0)
        return (int)hipErrorInvalidValue;
    const dim3 grid((T + kBlock - 1) / kBlock, rows), block(kBlock);
    const hipStream_t st = as_stream(stream);
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt;
    if (ssaa == 1)
        hipLaunchKernelGGL(k_positions<1>, grid, block, 0, st, vertices, n, triangles, m, shape, triangle_of, plan, T, row0,
                           xyz, owner);
    else if (ssaa == 2)
        hipLaunchKernelGGL(k_positions<2>, grid, block, 0, st, vertices, n, triangles, m, shape, triangle_of, plan, T, row0,
                           xyz, owner);
    else
        hipLaunchKernelGGL(k_positions<4>, grid, block, 0, st, vertices, n, triangles, m, shape, triangle_of, plan, T, row0,
                           xyz, owner);
    return (int)hipGetLastError();
}

}  // extern "C"
