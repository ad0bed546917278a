// A rasteriser for the exported mesh on MI355X (gfx950): per view a visibility buffer - the nearest triangle at every pixel
// centre - and a shading pass that turns it into an image from vertex colours or from Part 9's atlas; Part 17 of
// include/mi3d.h, which states the arithmetic operation by operation.  The forward half of what nvdiffrast does for the
// reference's export (nerf/renderer.py:193-299 of the reference rasterises in UV space only); the conventions are Part
// 15's and this project's own - PARITY UNPINNED.
//
// Compiled with -ffp-contract=off: everything is binary32 with separately rounded operations, sums in index order, no
// sqrt and no transcendental function, so that a NumPy float32 restatement gives the same bits.  The projection, the
// edge function, the bounding-box walk, the coverage test and the depth are the ones textureviews.hip uses
// (mi3d_meshraster.h): the visibility pass visits exactly the pixels mi3d_mesh_depth writes, with the same d.
//
// Kernels (memory-trivial; nothing staged in LDS, nothing waits on another workgroup):
//   k_vis_fill    thread = pixel of a view: all-ones; thread 0 zeroes the two counters
//   k_visibility  thread = (triangle, view): the walk of k_mesh_depth, a no-return 64-bit atomicMin of
//                 (bits(d) << 32) | triangle per covered pixel - one vector atomic per covered pixel into 8 V H W bytes
//   k_shade       thread = pixel of [V][H][W]: re-projects the winning triangle, the perspective-correct weights, the
//                 colour from vertex colours or four texture taps; plain stores, no atomics
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_meshraster.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMinT = 64, kMaxT = 16384;  // Part 9's range
constexpr unsigned long long kEmpty = ~0ull;

using namespace mi3d_meshraster;

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

__global__ __launch_bounds__(kBlock) void k_vis_fill(unsigned long long *__restrict__ vis, size_t n,
                                                     unsigned long long *__restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) {
        counts[0] = 0ull;
        counts[1] = 0ull;
    }
    if (i < n) vis[i] = kEmpty;
}

__global__ __launch_bounds__(kBlock) void k_visibility(const float *__restrict__ vertices, uint32_t nv,
                                                       const int32_t *__restrict__ triangles, uint32_t nt,
                                                       const float *__restrict__ views, uint32_t H, uint32_t W,
                                                       unsigned long long *__restrict__ vis,
                                                       unsigned long long *__restrict__ counts) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x, v = blockIdx.y;
    if (i >= nt) return;
    unsigned long long *out = vis + (size_t)v * H * W;
    // the depth in the upper word orders the keys (positive floats order like their bits); the triangle index in the
    // lower one breaks a tie towards the smaller index.  The result is not used: a no-return atomic.
    raster_triangle(vertices, nv, triangles, i, v, views, H, W, counts, [out, i](size_t at, float d) {
        atomicMin(out + at, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)i);
    });
}

struct ShadeArgs {
    const float *vertices, *views, *colors, *vt, *vn;
    const int32_t *triangles;
    const unsigned long long *vis;
    const uint8_t *texture;
    float *image, *normal, *depth, *bary;
    int32_t *tri;
    uint8_t *alpha;
    uint32_t nv, nt, T, H, W;
    size_t n;  // V * H * W
    float background[3];
};

// ((l0 a0 + l1 a1) + l2 a2)
__device__ __forceinline__ float mix3(const float l[3], float a0, float a1, float a2) {
    return (l[0] * a0 + l[1] * a1) + l[2] * a2;
}

// the lower tap index and the fraction of a texel coordinate g = u T - 0.5: i0 = min(max(floor(g), 0), T - 2),
// f = min(max(g - i0, 0), 1); a NaN gives tap 0 and fraction 0 (fmaxf returns its other argument)
__device__ __forceinline__ uint32_t tap(float g, uint32_t T, float &f) {
    const float i0 = fminf(fmaxf(floorf(g), 0.0f), (float)(T - 2));
    f = fminf(fmaxf(g - i0, 0.0f), 1.0f);
    return (uint32_t)i0;
}

template <bool TEXTURED>
__global__ __launch_bounds__(kBlock) void k_shade(ShadeArgs a) {
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= a.n) return;
    const size_t plane = (size_t)a.H * a.W;
    const uint32_t v = (uint32_t)(pix / plane);
    const uint32_t at = (uint32_t)(pix - (size_t)v * plane), j = at / a.W, ii = at - j * a.W;
    const unsigned long long key = a.vis[pix];
    const uint32_t t = (uint32_t)key;
    int32_t id[3] = {0, 0, 0};
    // an all-ones key: nothing was drawn.  A key no visibility pass of this mesh wrote (a triangle or a vertex index
    // out of range) is never dereferenced: background too.
    const bool hit = key != kEmpty && t < a.nt && load_triangle(a.triangles, t, a.nv, id);
    float col[3] = {a.background[0], a.background[1], a.background[2]}, nrm[3] = {0.0f, 0.0f, 0.0f};
    float lam[3] = {0.0f, 0.0f, 0.0f}, d = __builtin_inff();
    if (hit) {
        Projected P[3];
        project_triangle(a.vertices, id, a.views + (size_t)v * kView, P);
        const Weights e = edge_weights(id, P, (float)ii + 0.5f, (float)j + 0.5f);  // the visibility pass' operations
        float r[3];
        d = depth_terms(e, P, r);
#pragma unroll
        for (int k = 0; k < 3; ++k) lam[k] = r[k] * d;
        if (TEXTURED) {
            const float *uv = a.vt + (size_t)t * 6;  // Part 9's unshared corners: vt index 3 t + k
            const float u = mix3(lam, uv[0], uv[2], uv[4]), w = mix3(lam, uv[1], uv[3], uv[5]);
            const float T = (float)a.T;
            float fx, fy;
            const uint32_t i0 = tap(u * T - 0.5f, a.T, fx), j0 = tap((1.0f - w) * T - 0.5f, a.T, fy);  // row 0 is the top
            const float hx = 1.0f - fx, hy = 1.0f - fy;
            const uint8_t *c00 = a.texture + ((size_t)j0 * a.T + i0) * 3, *c01 = c00 + (size_t)a.T * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = (float)c00[c] * hx + (float)c00[3 + c] * fx, bot = (float)c01[c] * hx + (float)c01[3 + c] * fx;
                col[c] = (top * hy + bot * fy) / 255.0f;
            }
        } else {
            const float *c0 = a.colors + (size_t)id[0] * 3, *c1 = a.colors + (size_t)id[1] * 3, *c2 = a.colors + (size_t)id[2] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) col[c] = mix3(lam, c0[c], c1[c], c2[c]);
        }
        if (a.normal != nullptr) {
            const float *n0 = a.vn + (size_t)id[0] * 3, *n1 = a.vn + (size_t)id[1] * 3, *n2 = a.vn + (size_t)id[2] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) nrm[c] = mix3(lam, n0[c], n1[c], n2[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a.image[pix * 3 + c] = col[c];
    if (a.normal != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normal[pix * 3 + c] = nrm[c];
    }
    if (a.bary != nullptr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.bary[pix * 3 + c] = lam[c];
    }
    if (a.depth != nullptr) a.depth[pix] = d;
    if (a.tri != nullptr) a.tri[pix] = hit ? (int32_t)t : -1;
    if (a.alpha != nullptr) a.alpha[pix] = hit ? 1 : 0;
}

bool mesh_ok(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt) {
    return nv <= 0x7FFFFFFFull && nt <= 0x7FFFFFFFull && (nt == 0 || triangles != nullptr) &&
           (nt == 0 || nv == 0 || vertices != nullptr);
}

}  // namespace

extern "C" {

int mi3d_mesh_visibility(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         const float *views, uint32_t V, uint32_t H, uint32_t W, unsigned long long *vis,
                         unsigned long long *counts, void *stream) {
    if (!views_ok(V, H, W) || views == nullptr || vis == nullptr || counts == nullptr ||
        (reinterpret_cast<uintptr_t>(counts) & 7u) != 0 || (reinterpret_cast<uintptr_t>(vis) & 7u) != 0 ||
        !mesh_ok(vertices, nv, triangles, nt))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = as_stream(stream);
    const size_t n = (size_t)V * H * W;
    hipLaunchKernelGGL(k_vis_fill, dim3((uint32_t)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, vis, n, counts);
    if (nt != 0)
        hipLaunchKernelGGL(k_visibility, dim3((uint32_t)((nt + kBlock - 1) / kBlock), V), dim3(kBlock), 0, st, vertices,
                           (uint32_t)nv, triangles, (uint32_t)nt, views, H, W, vis, counts);
    return (int)hipGetLastError();
}

int mi3d_mesh_shade(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                    const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                    const float *colors, const float *vt, const uint8_t *texture, uint32_t T, const float *vn,
                    const float *background, float *image, float *normal, float *depth, int32_t *tri, float *bary,
                    uint8_t *alpha, void *stream) {
    const bool by_vertex = colors != nullptr, textured = vt != nullptr || texture != nullptr;
    if (!views_ok(V, H, W) || views == nullptr || vis == nullptr || (reinterpret_cast<uintptr_t>(vis) & 7u) != 0 ||
        background == nullptr || image == nullptr || !mesh_ok(vertices, nv, triangles, nt) || by_vertex == textured ||
        (textured && (vt == nullptr || texture == nullptr || T < kMinT || T > kMaxT)) || (normal != nullptr && vn == nullptr))
        return (int)hipErrorInvalidValue;
    ShadeArgs a;
    a.vertices = vertices; a.views = views; a.colors = colors; a.vt = vt; a.vn = vn; a.triangles = triangles; a.vis = vis;
    a.texture = texture; a.image = image; a.normal = normal; a.depth = depth; a.bary = bary; a.tri = tri; a.alpha = alpha;
    a.nv = (uint32_t)nv; a.nt = (uint32_t)nt; a.T = T; a.H = H; a.W = W; a.n = (size_t)V * H * W;
    for (int c = 0; c < 3; ++c) a.background[c] = background[c];
    const dim3 grid((uint32_t)((a.n + kBlock - 1) / kBlock)), block(kBlock);
    const hipStream_t st = as_stream(stream);
    if (textured)
        hipLaunchKernelGGL(k_shade<true>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_shade<false>, grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
