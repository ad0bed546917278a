// Refine-stage point renderer for MI355X (gfx950): the pytorch3d calls of the reference's `render_point`
// (/root/reference/nerf/refine_utils.py:306-333) - `rasterize_points(pointcloud, image_size, radius, points_per_pixel)`
// and `compositing.alpha_composite(idx, alphas, features)` with alphas = 1 - sqrt(clamp(0.1 dist / radius^2, 1e-3, 1))
// (:321-326) - as hand-written HIP kernels; Part 7 of include/mi3d.h.  SURVEY 8(f1) / BASELINE config 5.
//
// pytorch3d itself is an un-pinned dependency absent from this image: the semantics are restated from its published
// naive rasteriser and compositor (see oracle/raster_ref.py for the provenance note) - PARITY UNPINNED.
//
// Pipeline (no host synchronisation, no allocation: the caller provides the tile lists' storage):
//   k_raster_count / k_raster_scan / k_raster_fill   points -> per-tile index lists (16 x 16 pixel tiles; a point goes
//       to every tile its radius-disc's bounding box overlaps).  Plain global atomics: a few per point.  The scan is
//       scan_row of mi3d_scan.h with a put that clamps to the caller's capacity.
//   k_raster_tiles   one 256-thread workgroup per tile, thread = pixel; the tile's points stream through LDS 256 at a
//       time and every pixel keeps its K nearest covering points sorted by (z, point index) in registers - the index
//       tie-break makes the result independent of the (atomic) order of the tile lists.
//   k_points_composite_fwd / _bwd   thread = pixel, front-to-back over the K slots, C feature channels in registers;
//       the backward adds w_k * dout into the 76-byte feature row of each hit point with float atomics (a few million
//       requests per 512^2 image - far below the rate that forced the hash-grid scatter through memory).
//   k_points_composite_bwd_dists / k_raster_bwd_points   the position gradient, launched only when something upstream
//       of the projection requires grad: d out / d dists with plain stores (reproducible), then two float atomics per
//       slot into the (x, y) of the hit point - 2/C of the feature gradient's requests.
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

using mi3d_scan::kRowThreads;
using mi3d_scan::kRowWaves;

constexpr int kTilePx = 16, kTileThreads = kTilePx * kTilePx, kMaxK = 8, kMaxC = 32;

using mi3d_scan::as_stream;

// pytorch3d rasterization_utils.cuh PixToNonSquareNdc: centre of pixel i along an axis of S1 pixels (other axis S2)
__host__ __device__ inline float pix_to_ndc(int i, int S1, int S2) {
    float range = 2.0f;
    if (S1 > S2) range = ((float)S1 * range) / (float)S2;
    const float offset = range / 2.0f;
    return -offset + (range * (float)i + offset) / (float)S1;
}

struct RasterGeom {
    int H, W, tiles_x, tiles_y;
    float radius, radius2;
    float range_x, range_y;  // NDC extent of the two axes (2 for the longer... see pix_to_ndc)
};

__host__ __device__ inline RasterGeom make_geom(int H, int W, float radius) {
    RasterGeom g;
    g.H = H; g.W = W; g.tiles_x = (W + kTilePx - 1) / kTilePx; g.tiles_y = (H + kTilePx - 1) / kTilePx;
    g.radius = radius; g.radius2 = radius * radius;
    g.range_x = W > H ? (2.0f * (float)W) / (float)H : 2.0f;
    g.range_y = H > W ? (2.0f * (float)H) / (float)W : 2.0f;
    return g;
}

// Conservative pixel bounding box of a point's disc: output pixel xi looks at NDC pix_to_ndc(W-1-xi, W, H), i.e.
// x_ndc = range/2 - range (xi + 0.5) / W  ->  xi = (range/2 - x_ndc) W / range - 0.5; one pixel of margin either side.
__device__ __forceinline__ bool point_bbox(const RasterGeom &g, float x, float y, float z, int &x0, int &x1, int &y0,
                                           int &y1) {
    if (!(z >= 0.f)) return false;  // behind the camera (or NaN): skipped, as pytorch3d does
    const float cx = (g.range_x * 0.5f - x) * (float)g.W / g.range_x - 0.5f;
    const float cy = (g.range_y * 0.5f - y) * (float)g.H / g.range_y - 0.5f;
    const float rx = g.radius * (float)g.W / g.range_x + 1.0f, ry = g.radius * (float)g.H / g.range_y + 1.0f;
    if (!(cx + rx >= 0.f) || !(cx - rx <= (float)(g.W - 1)) || !(cy + ry >= 0.f) || !(cy - ry <= (float)(g.H - 1)))
        return false;
    x0 = (int)fmaxf(0.f, floorf(cx - rx)); x1 = (int)fminf((float)(g.W - 1), ceilf(cx + rx));
    y0 = (int)fmaxf(0.f, floorf(cy - ry)); y1 = (int)fminf((float)(g.H - 1), ceilf(cy + ry));
    return x0 <= x1 && y0 <= y1;
}

__global__ void k_raster_count(const float *__restrict__ ndc, uint32_t P, RasterGeom g, uint32_t *__restrict__ counts) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int x0, x1, y0, y1;
    if (!point_bbox(g, ndc[(size_t)p * 3], ndc[(size_t)p * 3 + 1], ndc[(size_t)p * 3 + 2], x0, x1, y0, y1)) return;
    for (int ty = y0 / kTilePx; ty <= y1 / kTilePx; ++ty)
        for (int tx = x0 / kTilePx; tx <= x1 / kTilePx; ++tx) atomicAdd(&counts[ty * g.tiles_x + tx], 1u);
}

// exclusive scan of the tile counts (a few thousand tiles) into `offsets`, cursors reset for the fill pass
__global__ __launch_bounds__(kRowThreads) void k_raster_scan(const uint32_t *__restrict__ counts, uint32_t n_tiles,
                                                             uint32_t capacity, uint32_t *__restrict__ offsets,
                                                             uint32_t *__restrict__ cursors) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    const uint32_t total = mi3d_scan::scan_row(counts, n_tiles, wave_sum, &base, [=](uint32_t i, uint32_t o) {
        offsets[i] = o < capacity ? o : capacity;  // a list that would overrun the caller's storage is cut
        cursors[i] = 0;
    });
    if (threadIdx.x == 0) offsets[n_tiles] = total < capacity ? total : capacity;
}

__global__ void k_raster_fill(const float *__restrict__ ndc, uint32_t P, RasterGeom g, const uint32_t *__restrict__ offsets,
                              uint32_t *__restrict__ cursors, uint32_t capacity, uint32_t *__restrict__ list) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int x0, x1, y0, y1;
    if (!point_bbox(g, ndc[(size_t)p * 3], ndc[(size_t)p * 3 + 1], ndc[(size_t)p * 3 + 2], x0, x1, y0, y1)) return;
    for (int ty = y0 / kTilePx; ty <= y1 / kTilePx; ++ty)
        for (int tx = x0 / kTilePx; tx <= x1 / kTilePx; ++tx) {
            const uint32_t t = ty * g.tiles_x + tx;
            const uint32_t slot = offsets[t] + atomicAdd(&cursors[t], 1u);
            if (slot < offsets[t + 1] && slot < capacity) list[slot] = p;
        }
}

__global__ __launch_bounds__(kTileThreads) void k_raster_tiles(const float *__restrict__ ndc, RasterGeom g, uint32_t K,
                                                               const uint32_t *__restrict__ offsets,
                                                               const uint32_t *__restrict__ list,
                                                               int32_t *__restrict__ idx_out, float *__restrict__ zbuf_out,
                                                               float *__restrict__ dist_out) {
    __shared__ float sx[kTileThreads], sy[kTileThreads], sz[kTileThreads];
    __shared__ uint32_t si[kTileThreads];
    const uint32_t tile = blockIdx.x;
    const int tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    const int xi = tx * kTilePx + (threadIdx.x % kTilePx), yi = ty * kTilePx + (threadIdx.x / kTilePx);
    const bool inside = xi < g.W && yi < g.H;
    // the reversed axes of pytorch3d's camera convention (+X left, +Y up)
    const float xf = pix_to_ndc(g.W - 1 - xi, g.W, g.H), yf = pix_to_ndc(g.H - 1 - yi, g.H, g.W);
    float bz[kMaxK], bd[kMaxK];
    uint32_t bi[kMaxK];
    uint32_t n = 0;
    const uint32_t begin = offsets[tile], end = offsets[tile + 1];
    for (uint32_t c0 = begin; c0 < end; c0 += kTileThreads) {
        const uint32_t j = c0 + threadIdx.x;
        if (j < end) {
            const uint32_t p = list[j];
            si[threadIdx.x] = p;
            sx[threadIdx.x] = ndc[(size_t)p * 3]; sy[threadIdx.x] = ndc[(size_t)p * 3 + 1];
            sz[threadIdx.x] = ndc[(size_t)p * 3 + 2];
        }
        __syncthreads();
        const uint32_t m = end - c0 < (uint32_t)kTileThreads ? end - c0 : (uint32_t)kTileThreads;
        if (inside) {
            for (uint32_t q = 0; q < m; ++q) {
                const float dx = xf - sx[q], dy = yf - sy[q];
                const float d2 = dx * dx + dy * dy;
                if (!(d2 < g.radius2)) continue;
                const float z = sz[q];
                const uint32_t p = si[q];
                // K nearest by (z, point index): the tie-break makes the result independent of the list order
                if (n == K && !(z < bz[K - 1] || (z == bz[K - 1] && p < bi[K - 1]))) continue;
                uint32_t pos = n < K ? n : K - 1;
#pragma unroll
                for (int s = kMaxK - 1; s > 0; --s) {
                    if ((uint32_t)s <= pos && (z < bz[s - 1] || (z == bz[s - 1] && p < bi[s - 1]))) {
                        bz[s] = bz[s - 1]; bd[s] = bd[s - 1]; bi[s] = bi[s - 1];
                        pos = s - 1;
                    }
                }
                bz[pos] = z; bd[pos] = d2; bi[pos] = p;
                if (n < K) ++n;
            }
        }
        __syncthreads();
    }
    if (!inside) return;
    const size_t o = ((size_t)yi * g.W + xi) * K;
    for (uint32_t k = 0; k < K; ++k) {
        const bool used = k < n;
        idx_out[o + k] = used ? (int32_t)bi[k] : -1;
        if (zbuf_out != nullptr) zbuf_out[o + k] = used ? bz[k] : -1.0f;
        dist_out[o + k] = used ? bd[k] : -1.0f;
    }
}

// refine_utils.py:321-326: dist = 0.1 * dist / pow(radius, 2); alpha = 1 - clamp(dist, 1e-3, 1) ** 0.5
__device__ __forceinline__ float point_alpha(float dist, float radius2) {
    const float d = (0.1f * dist) / radius2;
    return 1.0f - sqrtf(fminf(1.0f, fmaxf(1e-3f, d)));
}

__global__ void k_points_composite_fwd(const int32_t *__restrict__ idx, const float *__restrict__ dists, uint32_t n_pix,
                                       uint32_t K, const float *__restrict__ feats, uint32_t C, float radius2,
                                       float *__restrict__ out) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    float acc[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) acc[c] = 0.f;
    float T = 1.0f;
    for (uint32_t k = 0; k < K; ++k) {
        const int32_t p = idx[(size_t)pix * K + k];
        if (p < 0) continue;
        const float a = point_alpha(dists[(size_t)pix * K + k], radius2);
        const float w = T * a;
        const float *f = feats + (size_t)p * C;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if ((uint32_t)c < C) acc[c] += w * f[c];
        T *= 1.0f - a;
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
        if ((uint32_t)c < C) out[(size_t)c * n_pix + pix] = acc[c];
}

__global__ void k_points_composite_bwd(const int32_t *__restrict__ idx, const float *__restrict__ dists, uint32_t n_pix,
                                       uint32_t K, const float *__restrict__ dout, uint32_t C, float radius2,
                                       float *__restrict__ grad_feats) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    float g[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) g[c] = (uint32_t)c < C ? dout[(size_t)c * n_pix + pix] : 0.f;
    float T = 1.0f;
    for (uint32_t k = 0; k < K; ++k) {
        const int32_t p = idx[(size_t)pix * K + k];
        if (p < 0) continue;
        const float a = point_alpha(dists[(size_t)pix * K + k], radius2);
        const float w = T * a;
        float *dst = grad_feats + (size_t)p * C;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if ((uint32_t)c < C && g[c] != 0.f) unsafeAtomicAdd(dst + c, w * g[c]);
        T *= 1.0f - a;
    }
}

// d out / d dists for fixed idx (include/mi3d.h Part 7, "gradient for the point positions"): thread = pixel.  Pass 1
// walks the slots front to back as the forward does and keeps a_k, s_k = <dout, features[idx_k]>, T_k and the clamp's
// own derivative factor in registers; pass 2 runs R back to front.  No division by 1 - a anywhere, plain stores only.
__global__ __launch_bounds__(256) void k_points_composite_bwd_dists(const int32_t *__restrict__ idx, const float *__restrict__ dists,
                                             uint32_t n_pix, uint32_t K, const float *__restrict__ dout,
                                             const float *__restrict__ feats, uint32_t C, float radius2,
                                             float *__restrict__ grad_dists) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pix) return;
    float g[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) g[c] = (uint32_t)c < C ? dout[(size_t)c * n_pix + pix] : 0.f;
    float a[kMaxK], s[kMaxK], Tk[kMaxK], da[kMaxK];  // da = d a_k / d dist_k (0: unused slot or the clamp binds)
    float T = 1.0f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        a[k] = 0.f; s[k] = 0.f; Tk[k] = 0.f; da[k] = 0.f;
        if ((uint32_t)k >= K) continue;
        const int32_t p = idx[(size_t)pix * K + k];
        if (p < 0) continue;
        const float u = (0.1f * dists[(size_t)pix * K + k]) / radius2;  // point_alpha's own operations
        const float r = sqrtf(fminf(1.0f, fmaxf(1e-3f, u)));
        a[k] = 1.0f - r;
        if (u >= 1e-3f && u <= 1.0f) da[k] = -0.05f / (radius2 * r);
        const float *f = feats + (size_t)p * C;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxC; ++c)
            if ((uint32_t)c < C) dot += g[c] * f[c];
        s[k] = dot;
        Tk[k] = T;
        T *= 1.0f - a[k];
    }
    float R = 0.f;
#pragma unroll
    for (int k = kMaxK - 1; k >= 0; --k) {
        if ((uint32_t)k >= K) continue;
        // an unused slot has a = s = 0: it leaves R as it is, and its da = 0 writes the 0 the contract asks for
        grad_dists[(size_t)pix * K + k] = da[k] != 0.f ? Tk[k] * (s[k] - R) * da[k] : 0.f;
        R = a[k] * s[k] + (1.0f - a[k]) * R;
    }
}

// d dists / d (x, y) of the points: dist = (x_p - xf)^2 + (y_p - yf)^2 with (xf, yf) the pixel centre k_raster_tiles
// uses.  Thread = pixel, two float atomics per slot that carries a gradient; idx is the truth (no disc test), z is never
// written.  An index outside [0, P) is skipped.
__global__ __launch_bounds__(256) void k_raster_bwd_points(const float *__restrict__ ndc, uint32_t P, const int32_t *__restrict__ idx,
                                    const float *__restrict__ grad_dists, int H, int W, uint32_t K,
                                    float *__restrict__ grad_points) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= (uint32_t)H * (uint32_t)W) return;
    const int xi = (int)(pix % (uint32_t)W), yi = (int)(pix / (uint32_t)W);
    const float xf = pix_to_ndc(W - 1 - xi, W, H), yf = pix_to_ndc(H - 1 - yi, H, W);
    for (uint32_t k = 0; k < K; ++k) {
        const int32_t p = idx[(size_t)pix * K + k];
        if (p < 0 || (uint32_t)p >= P) continue;
        const float gd = grad_dists[(size_t)pix * K + k];
        if (gd == 0.f) continue;
        const float x = ndc[(size_t)p * 3], y = ndc[(size_t)p * 3 + 1];
        unsafeAtomicAdd(grad_points + (size_t)p * 3, 2.0f * (x - xf) * gd);
        unsafeAtomicAdd(grad_points + (size_t)p * 3 + 1, 2.0f * (y - yf) * gd);
    }
}

uint32_t tiles_per_point_max(const RasterGeom &g) {
    const float rx = g.radius * (float)g.W / g.range_x + 1.0f, ry = g.radius * (float)g.H / g.range_y + 1.0f;
    const uint32_t nx = (uint32_t)((2.0f * rx + 2.0f) / kTilePx) + 2u, ny = (uint32_t)((2.0f * ry + 2.0f) / kTilePx) + 2u;
    return nx * ny;
}

}  // namespace

extern "C" {

size_t mi3d_points_rasterize_workspace(uint32_t P, uint32_t H, uint32_t W, float radius) {
    if (H == 0 || W == 0) return 0;
    const RasterGeom g = make_geom((int)H, (int)W, radius);
    const size_t n_tiles = (size_t)g.tiles_x * g.tiles_y;
    // counts, offsets (+1), cursors, then the tile lists: every point can sit in tiles_per_point_max tiles.  An empty
    // cloud still needs the tile table (every list is empty, every slot -1) and the one list entry the launch asks for
    const size_t entries = P ? (size_t)P * tiles_per_point_max(g) : 1;
    return (3 * n_tiles + 4) * sizeof(uint32_t) + entries * sizeof(uint32_t);
}

int mi3d_points_rasterize(const float *points_ndc, uint32_t P, uint32_t H, uint32_t W, float radius,
                          uint32_t points_per_pixel, void *workspace, size_t workspace_bytes, int32_t *idx, float *zbuf,
                          float *dists, void *stream) {
    if (H == 0 || W == 0 || points_per_pixel == 0 || points_per_pixel > (uint32_t)kMaxK || !(radius > 0.f))
        return (int)hipErrorInvalidValue;
    const RasterGeom g = make_geom((int)H, (int)W, radius);
    const uint32_t n_tiles = (uint32_t)(g.tiles_x * g.tiles_y);
    const size_t head = (3 * (size_t)n_tiles + 4) * sizeof(uint32_t);
    if (workspace == nullptr || workspace_bytes < head + sizeof(uint32_t)) return (int)hipErrorInvalidValue;
    const size_t cap64 = (workspace_bytes - head) / sizeof(uint32_t);
    const uint32_t capacity = cap64 > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)cap64;
    uint32_t *counts = reinterpret_cast<uint32_t *>(workspace), *offsets = counts + n_tiles,
             *cursors = offsets + n_tiles + 1, *list = cursors + n_tiles + 3;
    hipStream_t st = as_stream(stream);
    (void)hipMemsetAsync(counts, 0, n_tiles * sizeof(uint32_t), st);
    if (P > 0) hipLaunchKernelGGL(k_raster_count, dim3((P + 255) / 256), dim3(256), 0, st, points_ndc, P, g, counts);
    hipLaunchKernelGGL(k_raster_scan, dim3(1), dim3(kRowThreads), 0, st, counts, n_tiles, capacity, offsets, cursors);
    if (P > 0)
        hipLaunchKernelGGL(k_raster_fill, dim3((P + 255) / 256), dim3(256), 0, st, points_ndc, P, g, offsets, cursors,
                           capacity, list);
    hipLaunchKernelGGL(k_raster_tiles, dim3(n_tiles), dim3(kTileThreads), 0, st, points_ndc, g, points_per_pixel, offsets,
                       list, idx, zbuf, dists);
    return (int)hipGetLastError();
}

int mi3d_points_composite_forward(const int32_t *idx, const float *dists, uint32_t H, uint32_t W, uint32_t points_per_pixel,
                                  const float *features, uint32_t C, double radius, float *out, void *stream) {
    if (C == 0 || C > (uint32_t)kMaxC || !(radius > 0.f)) return (int)hipErrorInvalidValue;
    const uint32_t n_pix = H * W;
    if (n_pix == 0) return 0;
    hipLaunchKernelGGL(k_points_composite_fwd, dim3((n_pix + 255) / 256), dim3(256), 0, as_stream(stream), idx, dists,
                       n_pix, points_per_pixel, features, C, (float)(radius * radius), out);
    return (int)hipGetLastError();
}

int mi3d_points_composite_backward(const int32_t *idx, const float *dists, uint32_t H, uint32_t W,
                                   uint32_t points_per_pixel, const float *grad_out, uint32_t C, double radius,
                                   float *grad_features, void *stream) {
    if (C == 0 || C > (uint32_t)kMaxC || !(radius > 0.f)) return (int)hipErrorInvalidValue;
    const uint32_t n_pix = H * W;
    if (n_pix == 0) return 0;
    hipLaunchKernelGGL(k_points_composite_bwd, dim3((n_pix + 255) / 256), dim3(256), 0, as_stream(stream), idx, dists,
                       n_pix, points_per_pixel, grad_out, C, (float)(radius * radius), grad_features);
    return (int)hipGetLastError();
}

int mi3d_points_composite_backward_dists(const int32_t *idx, const float *dists, uint32_t H, uint32_t W,
                                         uint32_t points_per_pixel, const float *grad_out, const float *features,
                                         uint32_t C, double radius, float *grad_dists, void *stream) {
    if (C == 0 || C > (uint32_t)kMaxC || !(radius > 0.f)) return (int)hipErrorInvalidValue;
    if (points_per_pixel > (uint32_t)kMaxK) return (int)hipErrorInvalidValue;  // the slots live in registers here
    const uint32_t n_pix = H * W;
    if (n_pix == 0 || points_per_pixel == 0) return 0;
    hipLaunchKernelGGL(k_points_composite_bwd_dists, dim3((n_pix + 255) / 256), dim3(256), 0, as_stream(stream), idx,
                       dists, n_pix, points_per_pixel, grad_out, features, C, (float)(radius * radius), grad_dists);
    return (int)hipGetLastError();
}

int mi3d_points_rasterize_backward(const float *points_ndc, uint32_t P, const int32_t *idx, const float *grad_dists,
                                   uint32_t H, uint32_t W, uint32_t points_per_pixel, float *grad_points, void *stream) {
    if (H == 0 || W == 0 || points_per_pixel == 0 || points_per_pixel > (uint32_t)kMaxK)
        return (int)hipErrorInvalidValue;  // mi3d_points_rasterize's own checks on these arguments
    if (P == 0) return 0;
    const uint32_t n_pix = H * W;
    hipLaunchKernelGGL(k_raster_bwd_points, dim3((n_pix + 255) / 256), dim3(256), 0, as_stream(stream), points_ndc, P, idx,
                       grad_dists, (int)H, (int)W, points_per_pixel, grad_points);
    return (int)hipGetLastError();
}

}  // extern "C"
