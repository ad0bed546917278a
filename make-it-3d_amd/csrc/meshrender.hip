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
//                 colour from vertex colours or four texture taps (uint8 or float texels: one template); plain stores,
//                 no atomics
//
// The adjoint of k_shade in its colour source (Part 18; visibility and geometry stay fixed).  The sums are 64-bit
// integers in units of 2^e, e chosen from the largest |dimage| and the pixel count, so that arrival order cannot change a
// bit and a NumPy restatement gives the same bytes:
//   k_grad_amax       thread strides over dimage: one unsigned atomicMax of bits(|g|) per workgroup (a fill zeroed the
//                     accumulators and the amax word before it)
//   k_shade_backward  thread = pixel: the key test, the weights and the taps of k_shade, one no-return 64-bit integer
//                     atomicAdd per non-zero contribution; leaves at once if amax is zero or not finite
//   k_grad_finish     thread = element: (float)ldexp((double)sum, e)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/mi3d.h"
#include "mi3d_dev.h"
#include "mi3d_meshraster.h"
#include "mi3d_scan.h"

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kMinT = 64, kMaxT = 16384;  // Part 9's range
constexpr unsigned long long kEmpty = ~0ull;

using namespace mi3d_meshraster;

using mi3d_scan::as_stream;
using mi3d_scan::aligned8;

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
    const void *texture;  // uint8_t or float [T][T][3]: k_shade's Texel
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

// What the shading pass and its adjoint share per pixel.  An all-ones key: nothing was drawn.  A key no visibility pass
// of this mesh wrote (a triangle or a vertex index out of range) is never dereferenced: no hit either.  On a hit: the
// triangle t, its indices, the perspective-correct weights lam and the depth d - the visibility pass' operations.
__device__ __forceinline__ bool pixel_weights(const unsigned long long *__restrict__ vis, size_t pix,
                                              const float *__restrict__ vertices, uint32_t nv,
                                              const int32_t *__restrict__ triangles, uint32_t nt,
                                              const float *__restrict__ views, uint32_t H, uint32_t W, uint32_t &t,
                                              int32_t id[3], float lam[3], float &d) {
    const size_t plane = (size_t)H * W;
    const uint32_t v = (uint32_t)(pix / plane);
    const uint32_t at = (uint32_t)(pix - (size_t)v * plane), j = at / W, ii = at - j * W;
    const unsigned long long key = vis[pix];
    t = (uint32_t)key;
    if (!(key != kEmpty && t < nt && load_triangle(triangles, t, nv, id))) return false;
    Projected P[3];
    project_triangle(vertices, id, views + (size_t)v * kView, P);
    const Weights e = edge_weights(id, P, (float)ii + 0.5f, (float)j + 0.5f);
    float r[3];
    d = depth_terms(e, P, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) lam[k] = r[k] * d;
    return true;
}

// the upper-left texel (i0, j0) of the four taps and the fractions (fx, fy) at the interpolated (u, v) of triangle t
__device__ __forceinline__ void texel_taps(const float *__restrict__ vt, uint32_t t, const float lam[3], uint32_t Tn,
                                           uint32_t &i0, uint32_t &j0, float &fx, float &fy) {
    const float *uv = vt + (size_t)t * 6;  // Part 9's unshared corners: vt index 3 t + k
    const float u = mix3(lam, uv[0], uv[2], uv[4]), w = mix3(lam, uv[1], uv[3], uv[5]);
    const float T = (float)Tn;
    i0 = tap(u * T - 0.5f, Tn, fx);
    j0 = tap((1.0f - w) * T - 0.5f, Tn, fy);  // row 0 is the top
}

template <bool TEXTURED, class Texel>
__global__ __launch_bounds__(kBlock) void k_shade(ShadeArgs a) {
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= a.n) return;
    uint32_t t;
    int32_t id[3] = {0, 0, 0};
    float col[3] = {a.background[0], a.background[1], a.background[2]}, nrm[3] = {0.0f, 0.0f, 0.0f};
    float lam[3] = {0.0f, 0.0f, 0.0f}, d = __builtin_inff();
    const bool hit = pixel_weights(a.vis, pix, a.vertices, a.nv, a.triangles, a.nt, a.views, a.H, a.W, t, id, lam, d);
    if (hit) {
        if (TEXTURED) {
            uint32_t i0, j0;
            float fx, fy;
            texel_taps(a.vt, t, lam, a.T, i0, j0, fx, fy);
            const float hx = 1.0f - fx, hy = 1.0f - fy;
            const Texel *c00 = static_cast<const Texel *>(a.texture) + ((size_t)j0 * a.T + i0) * 3, *c01 = c00 + (size_t)a.T * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = (float)c00[c] * hx + (float)c00[3 + c] * fx, bot = (float)c01[c] * hx + (float)c01[3 + c] * fx;
                const float blend = top * hy + bot * fy;
                col[c] = std::is_same<Texel, uint8_t>::value ? blend / 255.0f : blend;  // float texels: the blend itself
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

// ------------------------------------------------------------------------------------------------ Part 18: the adjoint

constexpr uint32_t kInfBits = 0x7F800000u;
constexpr int kAmaxBlocks = 2048;  // k_grad_amax strides: at most this many workgroups, one atomic each

struct GradArgs {
    const float *vertices, *views, *vt, *dimage;
    const int32_t *triangles;
    const unsigned long long *vis;
    unsigned long long *acc;  // int64 sums in units of 2^e, two's complement
    const uint32_t *amax;
    uint32_t nv, nt, T, H, W;
    int L;     // 2^L >= V H W
    size_t n;  // V * H * W
};

// e = (E + 1) + L - 60 with E = the exponent field of amax's bits less 127: 2^(E + 1) > amax, denormals included
__device__ __forceinline__ int grad_exponent(uint32_t amax, int L) { return ((int)(amax >> 23) - 127 + 1) + L - 60; }

__global__ __launch_bounds__(kBlock) void k_grad_amax(const float *__restrict__ g, size_t count, uint32_t *__restrict__ amax) {
    __shared__ uint32_t part[kBlock / 64];
    uint32_t m = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (size_t)gridDim.x * kBlock)
        m = max(m, __float_as_uint(g[i]) & 0x7FFFFFFFu);  // positive floats order like their bits; a NaN exceeds infinity
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) m = max(m, part[w]);
        if (m != 0) atomicMax(amax, m);
    }
}

// one contribution w * g in units of 2^e, saturated at +-2^(61 - L) so that not even a key no visibility pass wrote (its
// weights are then arbitrary) can carry a sum out of int64: at most 3 contributions per pixel and accumulator, 2^L pixels
__device__ __forceinline__ void contribute(unsigned long long *acc, float w, float g, int e, double cap) {
    const float t = w * g;
    double x = ldexp((double)t, -e);
    x = x != x ? 0.0 : fmin(fmax(x, -cap), cap);
    const long long q = llrint(x);
    if (q != 0) atomicAdd(acc, (unsigned long long)q);  // the result is not used: a no-return atomic
}

template <bool TEXTURED>
__global__ __launch_bounds__(kBlock) void k_shade_backward(GradArgs a) {
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (pix >= a.n) return;
    const uint32_t amax = *a.amax;  // the same word for every thread
    if (amax == 0 || amax >= kInfBits) return;  // nothing to add; k_grad_finish writes +0 or NaN
    const int e = grad_exponent(amax, a.L);
    const double cap = ldexp(1.0, 61 - a.L);
    uint32_t t;
    int32_t id[3];
    float lam[3], d;
    if (!pixel_weights(a.vis, pix, a.vertices, a.nv, a.triangles, a.nt, a.views, a.H, a.W, t, id, lam, d)) return;
    const float g[3] = {a.dimage[pix * 3], a.dimage[pix * 3 + 1], a.dimage[pix * 3 + 2]};
    if (TEXTURED) {
        uint32_t i0, j0;
        float fx, fy;
        texel_taps(a.vt, t, lam, a.T, i0, j0, fx, fy);
        const float hx = 1.0f - fx, hy = 1.0f - fy;
        const float w[4] = {hx * hy, fx * hy, hx * fy, fx * fy};  // the taps (i0, j0), (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1)
        unsigned long long *top = a.acc + ((size_t)j0 * a.T + i0) * 3, *bot = top + (size_t)a.T * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            contribute(top + c, w[0], g[c], e, cap);
            contribute(top + 3 + c, w[1], g[c], e, cap);
            contribute(bot + c, w[2], g[c], e, cap);
            contribute(bot + 3 + c, w[3], g[c], e, cap);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) contribute(a.acc + (size_t)id[k] * 3 + c, lam[k], g[c], e, cap);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_grad_finish(const unsigned long long *__restrict__ acc, size_t count,
                                                        const uint32_t *__restrict__ amax, int L, float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t m = *amax;
    float r = 0.0f;  // amax == 0: nothing was added
    if (m >= kInfBits)
        r = __uint_as_float(0x7FC00000u);  // a poisoned upstream gradient poisons the result
    else if (m != 0)
        r = (float)ldexp((double)(long long)acc[i], grad_exponent(m, L));
    out[i] = r;
}

bool mesh_ok(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt) {
    return nv <= 0x7FFFFFFFull && nt <= 0x7FFFFFFFull && (nt == 0 || triangles != nullptr) &&
           (nt == 0 || nv == 0 || vertices != nullptr);
}

constexpr unsigned long long kMaxGradElements = 3ull * 0x7FFFFFFFull;  // 3 nv at the largest nv; 3 T^2 lies below it

template <class Texel>
int shade(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt, const float *views,
          uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis, const float *colors, const float *vt,
          const Texel *texture, uint32_t T, const float *vn, const float *background, float *image, float *normal,
          float *depth, int32_t *tri, float *bary, uint8_t *alpha, void *stream) {
    const bool by_vertex = colors != nullptr, textured = vt != nullptr || texture != nullptr;
    if (!views_ok(V, H, W) || views == nullptr || vis == nullptr || !aligned8(vis) ||
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
        hipLaunchKernelGGL((k_shade<true, Texel>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((k_shade<false, Texel>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mi3d_mesh_visibility(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         const float *views, uint32_t V, uint32_t H, uint32_t W, unsigned long long *vis,
                         unsigned long long *counts, void *stream) {
    if (!views_ok(V, H, W) || views == nullptr || vis == nullptr || counts == nullptr || !aligned8(counts) ||
        !aligned8(vis) || !mesh_ok(vertices, nv, triangles, nt))
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
    return shade<uint8_t>(vertices, nv, triangles, nt, views, V, H, W, vis, colors, vt, texture, T, vn, background, image,
                          normal, depth, tri, bary, alpha, stream);
}

int mi3d_mesh_shade_f32(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                        const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                        const float *colors, const float *vt, const float *texture, uint32_t T, const float *vn,
                        const float *background, float *image, float *normal, float *depth, int32_t *tri, float *bary,
                        uint8_t *alpha, void *stream) {
    return shade<float>(vertices, nv, triangles, nt, views, V, H, W, vis, colors, vt, texture, T, vn, background, image,
                        normal, depth, tri, bary, alpha, stream);
}

size_t mi3d_mesh_shade_backward_workspace(unsigned long long elements) {
    if (elements > kMaxGradElements) return 0;
    return (size_t)(elements + 1) * 8;  // the int64 sums, then the amax word (in a slot of 8 bytes)
}

int mi3d_mesh_shade_backward(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                             const float *dimage, const float *vt, uint32_t T, float *grad_colors, float *grad_texture,
                             void *ws, size_t ws_bytes, void *stream) {
    const bool by_vertex = grad_colors != nullptr, textured = grad_texture != nullptr;
    if (!views_ok(V, H, W) || views == nullptr || vis == nullptr || !aligned8(vis) ||
        dimage == nullptr || !mesh_ok(vertices, nv, triangles, nt) || by_vertex == textured || (vt != nullptr) != (T != 0) ||
        (textured && (vt == nullptr || T < kMinT || T > kMaxT)) || (by_vertex && vt != nullptr) || ws == nullptr ||
        !aligned8(ws))
        return (int)hipErrorInvalidValue;
    const size_t count = textured ? (size_t)T * T * 3 : (size_t)nv * 3;
    if (ws_bytes < mi3d_mesh_shade_backward_workspace(count)) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;  // no vertex: no gradient to write
    GradArgs a;
    a.vertices = vertices; a.views = views; a.vt = vt; a.dimage = dimage; a.triangles = triangles; a.vis = vis;
    a.acc = static_cast<unsigned long long *>(ws);
    uint32_t *amax = reinterpret_cast<uint32_t *>(a.acc + count);
    a.amax = amax;
    a.nv = (uint32_t)nv; a.nt = (uint32_t)nt; a.T = T; a.H = H; a.W = W; a.n = (size_t)V * H * W;
    a.L = 0;
    while (((size_t)1 << a.L) < a.n) ++a.L;
    const hipStream_t st = as_stream(stream);
    const int launches = MI3D_TUNE(MI3D_T_SHADE_BACKWARD_LAUNCHES, 7);
    const size_t floats = a.n * 3;
    if (launches & 1) {
        const hipError_t err = hipMemsetAsync(ws, 0, (count + 1) * 8, st);  // the fill: the sums and the amax word
        if (err != hipSuccess) return (int)err;
        const size_t blocks = (floats + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(k_grad_amax, dim3((uint32_t)(blocks < (size_t)kAmaxBlocks ? blocks : (size_t)kAmaxBlocks)),
                           dim3(kBlock), 0, st, dimage, floats, amax);
    }
    if (launches & 2) {
        const dim3 grid((uint32_t)((a.n + kBlock - 1) / kBlock)), block(kBlock);
        if (textured)
            hipLaunchKernelGGL(k_shade_backward<true>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_shade_backward<false>, grid, block, 0, st, a);
    }
    if (launches & 4)
        hipLaunchKernelGGL(k_grad_finish, dim3((uint32_t)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a.acc, count,
                           amax, a.L, textured ? grad_texture : grad_colors);
    return (int)hipGetLastError();
}

}  // extern "C"
