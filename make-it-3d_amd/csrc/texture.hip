// Texture baking for MI355X (gfx950): the per-triangle atlas of a marching-cubes mesh, the texel -> surface point map and
// the 8-bit packing of the evaluated albedo; Part 9 of include/mi3d.h, which states the contract (cell layout, ownership,
// UV corners, the point formula, supersampling, quantisation).  What xatlas + nvdiffrast + the kd-tree inpainting do for the
// reference's export_mesh (nerf/renderer.py:193-299 of the reference); neither exists for this hardware, so the layout is
// this project's own - PARITY UNPINNED.
//
// Compiled with -ffp-contract=off: a texel's point is A + s (B - A) + t (C - A) as separately rounded binary32 operations,
// so that a NumPy float32 restatement gives the same bits.
//
// Kernels (all memory-trivial; nothing staged in LDS):
//   k_atlas_uv         thread = triangle: its three unshared vt
//   k_atlas_positions  thread = texel of a band of image rows, consecutive lanes on consecutive x: owner and the ssaa^2
//                      sample points, 12 ssaa^2 contiguous bytes per lane; the triangle's indices and vertices come through
//                      the caches (about c / 2 neighbouring lanes share a triangle)
//   k_texture_pack     thread = four texels = three 32-bit words of RGB; the ssaa^2 mean and the quantisation
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMinT = 64, kMaxT = 16384, kMinCell = 4;

using mi3d_scan::as_stream;

struct Atlas {
    uint32_t T, c, cols, rows, nt;  // cols x rows cells of (c + 1) x c texels; triangle i in cell i / 2 as half i & 1
};

inline unsigned long long atlas_capacity(uint32_t T, uint32_t c) {
    return 2ull * (T / (c + 1)) * (T / c);
}

// the largest c >= 4 whose capacity holds nt triangles (the capacity is non-increasing in c); 0 if none
uint32_t atlas_cell(unsigned long long nt, uint32_t T) {
    if (T < kMinT || T > kMaxT || atlas_capacity(T, kMinCell) < nt) return 0;
    uint32_t lo = kMinCell, hi = T - 1;  // capacity(lo) >= nt; c + 1 <= T keeps one column
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (atlas_capacity(T, mid) >= nt) lo = mid; else hi = mid - 1;
    }
    return lo;
}

bool make_atlas(unsigned long long nt, uint32_t T, Atlas &a) {
    const uint32_t c = atlas_cell(nt, T);
    if (c == 0 || nt == 0 || nt > 0x7FFFFFFFull) return false;
    a.T = T; a.c = c; a.cols = T / (c + 1); a.rows = T / c; a.nt = (uint32_t)nt;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_atlas_uv(Atlas a, float *__restrict__ vt) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.nt) return;
    const uint32_t q = i >> 1, half = i & 1u, c = a.c;
    const uint32_t X0 = (q % a.cols) * (c + 1), Y0 = (q / a.cols) * c;
    // half 0: centres of local texels (0, 0) (c - 2, 0) (0, c - 2); half 1: their reflection (x, y) -> (c - x, c - 1 - y)
    const uint32_t lx[3] = {0u, c - 2, 0u}, ly[3] = {0u, 0u, c - 2};
    const float fT = (float)a.T;
    float *o = vt + (size_t)i * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t x = half ? c - lx[k] : lx[k], y = half ? c - 1 - ly[k] : ly[k];
        o[2 * k] = ((float)(X0 + x) + 0.5f) / fT;
        o[2 * k + 1] = 1.0f - ((float)(Y0 + y) + 0.5f) / fT;
    }
}

__device__ __forceinline__ float clamp_box(float p) { return fminf(fmaxf(p, -1.0f), 1.0f); }

template <int SS>
__global__ __launch_bounds__(kBlock) void k_atlas_positions(const float *__restrict__ vertices, uint32_t nv,
                                                            const int32_t *__restrict__ triangles, Atlas a, uint32_t row0,
                                                            float *__restrict__ xyz, int32_t *__restrict__ owner,
                                                            unsigned long long *__restrict__ bad) {
    const uint32_t X = blockIdx.x * kBlock + threadIdx.x, ry = blockIdx.y;
    if (X >= a.T) return;
    const uint32_t Y = row0 + ry, c = a.c;
    const uint32_t col = X / (c + 1), x = X - col * (c + 1), row = Y / c, y = Y - row * c;
    const size_t texel = (size_t)ry * a.T + X;
    float *o = xyz + texel * (size_t)(3 * SS * SS);

    int32_t own = -1;
    uint32_t u = 0, v = 0;
    int32_t ia = 0, ib = 0, ic = 0;
    if (col < a.cols && row < a.rows) {
        const uint32_t half = (x <= c - 1 && x + y <= c - 1) ? 0u : 1u;
        const uint32_t i = 2 * (row * a.cols + col) + half;
        if (i < a.nt) {
            u = half ? c - x : x;
            v = half ? c - 1 - y : y;
            const int32_t *t = triangles + (size_t)i * 3;
            ia = t[0]; ib = t[1]; ic = t[2];
            // an index outside [0, nv) is never dereferenced: the triangle owns nothing and is counted once, by the
            // texel of its vertex 0 (every triangle has exactly one, in exactly one band)
            const bool ok = (uint32_t)ia < nv && (uint32_t)ib < nv && (uint32_t)ic < nv;
            if (ok) own = (int32_t)i;
            else if (u == 0 && v == 0) atomicAdd(bad, 1ull);
        }
    }
    if (owner != nullptr) owner[texel] = own;
    if (own < 0) {
#pragma unroll
        for (int k = 0; k < 3 * SS * SS; ++k) o[k] = 0.0f;
        return;
    }
    const float *A = vertices + (size_t)ia * 3, *B = vertices + (size_t)ib * 3, *Cc = vertices + (size_t)ic * 3;
    float pa[3], e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        pa[d] = A[d];
        e1[d] = B[d] - pa[d];
        e2[d] = Cc[d] - pa[d];
    }
    const float span = (float)(c - 2);
#pragma unroll
    for (int j = 0; j < SS; ++j) {
#pragma unroll
        for (int i = 0; i < SS; ++i) {
            // (i + 0.5) / SS - 0.5 is exact in binary32 for SS in {1, 2, 4}, and so is its sum with a small integer
            const float s = ((float)u + ((i + 0.5f) / SS - 0.5f)) / span, t = ((float)v + ((j + 0.5f) / SS - 0.5f)) / span;
#pragma unroll
            for (int d = 0; d < 3; ++d) o[(j * SS + i) * 3 + d] = clamp_box((pa[d] + s * e1[d]) + t * e2[d]);
        }
    }
}

__device__ __forceinline__ uint32_t quantise(float a) {
    const float v = a * 255.0f;
    return v >= 255.0f ? 255u : v >= 0.0f ? (uint32_t)floorf(v) : 0u;  // NaN and negatives: 0
}

// the RGB bytes of one texel as the low 24 bits of a word (R lowest); 0 where no triangle owns it
template <int SS>
__device__ __forceinline__ uint32_t texel_rgb(const float *__restrict__ albedo, const int32_t *__restrict__ owner, size_t texel) {
    if (owner[texel] < 0) return 0u;
    const float *a = albedo + texel * (size_t)(3 * SS * SS);
    uint32_t rgb = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float sum = a[d];
#pragma unroll
        for (int k = 1; k < SS * SS; ++k) sum += a[3 * k + d];
        rgb |= quantise(sum * (1.0f / (SS * SS))) << (8 * d);
    }
    return rgb;
}

template <int SS>
__global__ __launch_bounds__(kBlock) void k_texture_pack(const float *__restrict__ albedo, const int32_t *__restrict__ owner,
                                                         size_t texels, uint8_t *__restrict__ image) {
    const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x, first = g * 4;
    if (first >= texels) return;
    if (first + 4 <= texels) {
        const uint32_t p0 = texel_rgb<SS>(albedo, owner, first), p1 = texel_rgb<SS>(albedo, owner, first + 1),
                       p2 = texel_rgb<SS>(albedo, owner, first + 2), p3 = texel_rgb<SS>(albedo, owner, first + 3);
        uint32_t *w = reinterpret_cast<uint32_t *>(image) + g * 3;  // 12 bytes: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
        w[0] = p0 | (p1 << 24);
        w[1] = (p1 >> 8) | (p2 << 16);
        w[2] = (p2 >> 16) | (p3 << 8);
        return;
    }
    for (size_t t = first; t < texels; ++t) {  // the last one to three texels of a band whose size is no multiple of 4
        const uint32_t p = texel_rgb<SS>(albedo, owner, t);
        image[3 * t] = (uint8_t)p;
        image[3 * t + 1] = (uint8_t)(p >> 8);
        image[3 * t + 2] = (uint8_t)(p >> 16);
    }
}

bool band_ok(uint32_t T, uint32_t ssaa, uint32_t row0, uint32_t rows) {
    if (T < kMinT || T > kMaxT || (ssaa != 1 && ssaa != 2 && ssaa != 4)) return false;
    return rows >= 1 && row0 < T && rows <= T - row0;
}

}  // namespace

extern "C" {

uint32_t mi3d_atlas_cell(unsigned long long nt, uint32_t T) { return atlas_cell(nt, T); }

int mi3d_atlas_uv(unsigned long long nt, uint32_t T, float *vt, void *stream) {
    Atlas a;
    if (!make_atlas(nt, T, a) || vt == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_atlas_uv, dim3((a.nt + kBlock - 1) / kBlock), dim3(kBlock), 0, as_stream(stream), a, vt);
    return (int)hipGetLastError();
}

int mi3d_atlas_positions(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         uint32_t T, uint32_t ssaa, uint32_t row0, uint32_t rows, float *xyz, int32_t *owner,
                         unsigned long long *bad, void *stream) {
    Atlas a;
    if (!make_atlas(nt, T, a) || !band_ok(T, ssaa, row0, rows) || vertices == nullptr || triangles == nullptr ||
        xyz == nullptr || bad == nullptr || (reinterpret_cast<uintptr_t>(bad) & 7u) != 0 || nv == 0 || nv > 0x7FFFFFFFull)
        return (int)hipErrorInvalidValue;
    const dim3 grid((T + kBlock - 1) / kBlock, rows), block(kBlock);
    const hipStream_t st = as_stream(stream);
    const uint32_t n = (uint32_t)nv;
    if (ssaa == 1)
        hipLaunchKernelGGL(k_atlas_positions<1>, grid, block, 0, st, vertices, n, triangles, a, row0, xyz, owner, bad);
    else if (ssaa == 2)
        hipLaunchKernelGGL(k_atlas_positions<2>, grid, block, 0, st, vertices, n, triangles, a, row0, xyz, owner, bad);
    else
        hipLaunchKernelGGL(k_atlas_positions<4>, grid, block, 0, st, vertices, n, triangles, a, row0, xyz, owner, bad);
    return (int)hipGetLastError();
}

int mi3d_texture_pack(const float *albedo, const int32_t *owner, uint32_t T, uint32_t ssaa, uint32_t rows, uint8_t *image,
                      void *stream) {
    if (!band_ok(T, ssaa, 0, rows) || albedo == nullptr || owner == nullptr || image == nullptr ||
        (reinterpret_cast<uintptr_t>(image) & 3u) != 0)
        return (int)hipErrorInvalidValue;
    const size_t texels = (size_t)rows * T, groups = (texels + 3) / 4;
    const dim3 grid((uint32_t)((groups + kBlock - 1) / kBlock)), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (ssaa == 1)
        hipLaunchKernelGGL(k_texture_pack<1>, grid, block, 0, st, albedo, owner, texels, image);
    else if (ssaa == 2)
        hipLaunchKernelGGL(k_texture_pack<2>, grid, block, 0, st, albedo, owner, texels, image);
    else
        hipLaunchKernelGGL(k_texture_pack<4>, grid, block, 0, st, albedo, owner, texels, image);
    return (int)hipGetLastError();
}

}  // extern "C"
