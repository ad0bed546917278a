// Projective texturing for MI355X (gfx950): a depth map of the mesh per view, and per atlas sample a visibility-tested,
// angle-weighted blend of the views' colours; Part 15 of include/mi3d.h, which states the arithmetic operation by
// operation.  The reference bakes the field only (nerf/renderer.py:193-299 of the reference); this contract is this
// project's own - PARITY UNPINNED.
//
// Compiled with -ffp-contract=off: everything is binary32 with separately rounded operations, sums in index order, no
// sqrt and no transcendental function, so that a NumPy float32 restatement gives the same bits - the visibility decisions
// are discrete, and only bit-equal inputs make them testable.
//
// Kernels (memory-trivial; nothing staged in LDS, nothing waits on another workgroup):
//   k_depth_fill      thread = pixel of a view: +inf; thread 0 zeroes the two counters
//   k_mesh_depth      thread = (triangle, view): walks the pixel centres of the clipped bounding box, atomicMin on the
//                     uint32 bits of the perspective-correct depth (positive floats order like their bits)
//   k_texture_project thread = texel of a band (k_atlas_positions' mapping), its ssaa^2 samples in turn; the views in
//                     order, the 24-float view record read wave-uniformly; eight cached taps per view; no atomics
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_meshraster.h"
#include "mi3d_scan.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMinT = 64, kMaxT = 16384;

// the view record, the projection, the watertight edge function and the bounding-box walk: shared with meshrender.hip
using namespace mi3d_meshraster;

using mi3d_scan::as_stream;

__global__ __launch_bounds__(kBlock) void k_depth_fill(float *__restrict__ depth, size_t n,
                                                       unsigned long long *__restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        counts[0] = 0ull;
        counts[1] = 0ull;
    }
    if (i < n) depth[i] = __builtin_inff();
}

__global__ __launch_bounds__(kBlock) void k_mesh_depth(const float *__restrict__ vertices, uint32_t nv,
                                                       const int32_t *__restrict__ triangles, uint32_t nt,
                                                       const float *__restrict__ views, uint32_t H, uint32_t W,
                                                       float *__restrict__ depth, unsigned long long *__restrict__ counts) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x, v = blockIdx.y;
    if (i >= nt) return;
    uint32_t *out = reinterpret_cast<uint32_t *>(depth) + (size_t)v * H * W;
    raster_triangle(vertices, nv, triangles, i, v, views, H, W, counts,
                    [out](size_t at, float d) { atomicMin(out + at, __float_as_uint(d)); });
}

struct ProjectArgs {
    const float *xyz, *vertices, *views, *depth, *images, *weights, *base;
    const int32_t *owner, *triangles;
    const uint8_t *masks;
    float *colour;
    uint8_t *hits;
    uint32_t nv, nt, T, V, H, W, power;
    float min_cos2, depth_tol;
};

template <int SS>
__global__ __launch_bounds__(kBlock) void k_texture_project(ProjectArgs a) {
    const uint32_t X = blockIdx.x * kBlock + threadIdx.x, ry = blockIdx.y;
    if (X >= a.T) return;
    const size_t texel = (size_t)ry * a.T + X;
    const int32_t own = a.owner[texel];
    float N[3] = {0.0f, 0.0f, 0.0f}, nn = 0.0f;
    if ((uint32_t)own < a.nt) {  // own < 0 fails as a uint32 too
        const int32_t *t = a.triangles + (size_t)own * 3;
        const int32_t ia = t[0], ib = t[1], ic = t[2];
        if ((uint32_t)ia < a.nv && (uint32_t)ib < a.nv && (uint32_t)ic < a.nv) {
            const float *A = a.vertices + (size_t)ia * 3, *B = a.vertices + (size_t)ib * 3, *Cc = a.vertices + (size_t)ic * 3;
            float e1[3], e2[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                e1[d] = B[d] - A[d];
                e2[d] = Cc[d] - A[d];
            }
            N[0] = e1[1] * e2[2] - e1[2] * e2[1];
            N[1] = e1[2] * e2[0] - e1[0] * e2[2];
            N[2] = e1[0] * e2[1] - e1[1] * e2[0];
            nn = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2];
        }
    }
    const bool live = nn > 0.0f && finite_f(nn);  // a degenerate triangle and an unowned texel contribute nothing
    const float xmax = (float)a.W - 0.5f, ymax = (float)a.H - 0.5f;
    const size_t plane = (size_t)a.H * a.W;
    for (int k = 0; k < SS * SS; ++k) {
        const size_t sample = texel * (size_t)(SS * SS) + k;
        const float *p = a.xyz + sample * 3;
        const float p0 = p[0], p1 = p[1], p2 = p[2];
        float sw = 0.0f, sc[3] = {0.0f, 0.0f, 0.0f};
        uint32_t hits = 0;
        for (uint32_t v = 0; live && v < a.V; ++v) {
            const float *view = a.views + (size_t)v * kView;
            const Projected q = project(view, p0, p1, p2);
            if (!(q.z > 0.0f)) continue;                                                            // (a)
            if (!(q.x >= 0.5f && q.x <= xmax && q.y >= 0.5f && q.y <= ymax)) continue;              // (b)
            const float gx = q.x - 0.5f, gy = q.y - 0.5f;
            const uint32_t i0 = min((uint32_t)floorf(gx), a.W - 2), j0 = min((uint32_t)floorf(gy), a.H - 2);
            const size_t at = (size_t)v * plane + (size_t)j0 * a.W + i0;
            const float d00 = a.depth[at], d10 = a.depth[at + 1], d01 = a.depth[at + a.W], d11 = a.depth[at + a.W + 1];
            if (!(finite_f(d00) && finite_f(d10) && finite_f(d01) && finite_f(d11))) continue;      // (c)
            if (!(q.z <= fminf(fminf(d00, d10), fminf(d01, d11)) + a.depth_tol)) continue;
            if (a.masks != nullptr) {                                                               // (d)
                const uint8_t *m = a.masks + at;
                if (m[0] == 0 || m[1] == 0 || m[a.W] == 0 || m[a.W + 1] == 0) continue;
            }
            const float dx = view[21] - p0, dy = view[22] - p1, dz = view[23] - p2;                 // (e)
            const float nd = (N[0] * dx + N[1] * dy) + N[2] * dz;
            if (!(nd > 0.0f)) continue;
            const float dd = (dx * dx + dy * dy) + dz * dz;
            const float cos2 = (nd * nd) / (nn * dd);
            if (!(cos2 >= a.min_cos2)) continue;
            float cp = cos2;                                                                        // cos^power
            for (uint32_t e = 2; e < a.power; e *= 2) cp = cp * cp;
            const float w = a.weights[v] * cp;
            const float fx = gx - (float)i0, fy = gy - (float)j0, hx = 1.0f - fx, hy = 1.0f - fy;
            const float *c00 = a.images + at * 3, *c01 = c00 + (size_t)a.W * 3;
            sw = sw + w;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const float top = c00[d] * hx + c00[3 + d] * fx, bot = c01[d] * hx + c01[3 + d] * fx;
                sc[d] = sc[d] + w * (top * hy + bot * fy);
            }
            ++hits;
        }
        float *o = a.colour + sample * 3;
        const float *b = a.base + sample * 3;
        const bool seen = sw > 0.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) o[d] = seen ? sc[d] / sw : b[d];
        a.hits[sample] = (uint8_t)hits;
    }
}

}  // namespace

extern "C" {

int mi3d_mesh_depth(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                    const float *views, uint32_t V, uint32_t H, uint32_t W, float *depth, unsigned long long *counts,
                    void *stream) {
    if (!views_ok(V, H, W) || views == nullptr || depth == nullptr || counts == nullptr ||
        (reinterpret_cast<uintptr_t>(counts) & 7u) != 0 || nv > 0x7FFFFFFFull || nt > 0x7FFFFFFFull ||
        (nt != 0 && triangles == nullptr) || (nt != 0 && nv != 0 && vertices == nullptr))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = as_stream(stream);
    const size_t n = (size_t)V * H * W;
    hipLaunchKernelGGL(k_depth_fill, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, depth, n, counts);
    if (nt != 0)
        hipLaunchKernelGGL(k_mesh_depth, dim3((uint32_t)((nt + kBlock - 1) / kBlock), V), dim3(kBlock), 0, st, vertices,
                           (uint32_t)nv, triangles, (uint32_t)nt, views, H, W, depth, counts);
    return (int)hipGetLastError();
}

int mi3d_texture_project(const float *xyz, const int32_t *owner, const float *vertices, unsigned long long nv,
                         const int32_t *triangles, unsigned long long nt, uint32_t T, uint32_t ssaa, uint32_t rows,
                         const float *views, uint32_t V, uint32_t H, uint32_t W, const float *depth, const float *images,
                         const uint8_t *masks, const float *weights, uint32_t power, float min_cos2, float depth_tol,
                         const float *base, float *colour, uint8_t *hits, void *stream) {
    if (!views_ok(V, H, W) || T < kMinT || T > kMaxT || (ssaa != 1 && ssaa != 2 && ssaa != 4) || rows < 1 || rows > T ||
        (power != 2 && power != 4 && power != 8 && power != 16) || !(min_cos2 >= 0.0f && min_cos2 <= 1.0f) ||
        !(depth_tol >= 0.0f && depth_tol < __builtin_inff()) || xyz == nullptr || owner == nullptr || vertices == nullptr ||
        triangles == nullptr || views == nullptr || depth == nullptr || images == nullptr || weights == nullptr ||
        base == nullptr || colour == nullptr || hits == nullptr || nv == 0 || nv > 0x7FFFFFFFull || nt == 0 ||
        nt > 0x7FFFFFFFull)
        return (int)hipErrorInvalidValue;
    ProjectArgs a;
    a.xyz = xyz; a.vertices = vertices; a.views = views; a.depth = depth; a.images = images; a.weights = weights;
    a.base = base; a.owner = owner; a.triangles = triangles; a.masks = masks; a.colour = colour; a.hits = hits;
    a.nv = (uint32_t)nv; a.nt = (uint32_t)nt; a.T = T; a.V = V; a.H = H; a.W = W; a.power = power;
    a.min_cos2 = min_cos2; a.depth_tol = depth_tol;
    const dim3 grid((T + kBlock - 1) / kBlock, rows), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (ssaa == 1)
        hipLaunchKernelGGL(k_texture_project<1>, grid, block, 0, st, a);
    else if (ssaa == 2)
        hipLaunchKernelGGL(k_texture_project<2>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_texture_project<4>, grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
