// The refine stage's point cloud from depth views, for MI355X (gfx950, wave64): Part 11 of include/mi3d.h, which states
// the contract.  What `depth2point`, `multidepth2point_mask`, `z_buffer` and `project` of the reference's
// nerf/refine_utils.py (:61-208) compute in NumPy, two Python loops over every point and cv2.erode.
//
// Compiled with -ffp-contract=off.  Geometry is binary64 with every operation rounded separately and three-term sums in
// index order, as a NumPy restatement evaluates them; the sampled colours and the canonical-depth lookup are binary32
// from the point where the reference hands its coordinates to torch (F.grid_sample's defaults restated in `bilinear`).
// The binary64 arithmetic does not bound these kernels: each reads 24 bytes per point and does a few dozen operations.
//
// Kernels (thread = pixel or point; no host synchronisation, no allocation, no atomic appends):
//   k_pc_count / k_pc_scan / k_pc_unproject   kept pixels per workgroup (wave ballot + popcount), exclusive scan of the
//                  workgroup sums by one workgroup, then pixel -> world point written at `base + rank`: row-major pixel
//                  order, the scheme of k_mc_count / k_mc_scan / k_mc_vertices in mesh.hip (scan_row of mi3d_scan.h)
//   k_pc_fill / k_pc_zmin / k_pc_visible      [H, W] buffer of order-preserving 64-bit keys of the depth, one atomicMin
//                  per in-bounds point; then z - zmin[pixel] <= 1 / H per point
//   k_box_morph    rows then columns of a kh x kw box minimum / maximum through an LDS tile with its halo, one launch
//   k_pc_cano_filter, k_pc_colour             projection, then the binary32 bilinear lookup
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

using mi3d_scan::kRowThreads;
using mi3d_scan::kRowWaves;

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr uint32_t kMaxSide = 16384;           // H, W: H * W <= 2^28 pixels, every pixel index fits 32 bits
constexpr unsigned long long kMaxPoints = 0x7FFFFFFFull * kBlock;  // one thread per point, grid.x < 2^31
constexpr int kTile = 32, kMaxBox = 31, kMaxTile = kTile + kMaxBox - 1;

using mi3d_scan::as_stream;

// world -> camera rows [R | t] (3 x 4, row-major) and the intrinsics (3 x 3, row-major), by value in the kernel arguments
struct Camera {
    double rt[12], k[9];
};

struct Unproject {
    double kinv[9], c2w[12];
};

__host__ __device__ inline uint32_t pc_blocks(unsigned long long n) { return (uint32_t)((n + kBlock - 1) / kBlock); }

// refine_utils.py:154-158 `project`: cam = p . RT[:, :3]^T + RT[:, 3], q = cam . K^T, xy = q[:2] / q[2], z = q[2]
__device__ __forceinline__ void project(const double *__restrict__ p, const Camera &c, double &x, double &y, double &z) {
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    double cam[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = ((p0 * c.rt[4 * r] + p1 * c.rt[4 * r + 1]) + p2 * c.rt[4 * r + 2]) + c.rt[4 * r + 3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (cam[0] * c.k[3 * r] + cam[1] * c.k[3 * r + 1]) + cam[2] * c.k[3 * r + 2];
    x = q[0] / q[2];
    y = q[1] / q[2];
    z = q[2];
}

// np.round + the bounds test of z_buffer (:170-171); a non-finite coordinate fails every comparison: out of bounds
__device__ __forceinline__ bool pixel_of(double x, double y, uint32_t H, uint32_t W, uint32_t &pix) {
    const double rx = rint(x), ry = rint(y);
    if (!(rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1))) return false;
    pix = (uint32_t)ry * W + (uint32_t)rx;
    return true;
}

// order-preserving key of a double: a < b  <=>  key(a) < key(b) for all non-NaN a, b (-0.0 sorts just below +0.0)
__device__ __forceinline__ unsigned long long key_of(double z) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(z);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

__device__ __forceinline__ double double_of(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k;
    return __longlong_as_double((long long)b);
}

// F.grid_sample's default (bilinear, zero padding, align_corners=False) at the normalised coordinate (gx, gy) of a
// [H, W] plane, `channels` planes `plane` floats apart: unnormalise ((g + 1) size - 1) / 2, floor, taps nw ne sw se
template <int channels>
__device__ __forceinline__ void bilinear(const float *__restrict__ img, uint32_t H, uint32_t W, float gx, float gy,
                                         float *out) {
    const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
#pragma unroll
    for (int c = 0; c < channels; ++c) out[c] = 0.f;
    // every tap of a coordinate outside (-1, size) lies outside the image (this also catches NaN and what no int holds)
    if (!(ix > -1.f && ix < (float)W && iy > -1.f && iy < (float)H)) return;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx[2] = {(fx + 1.f) - ix, ix - fx}, wy[2] = {(fy + 1.f) - iy, iy - fy};
    const size_t plane = (size_t)H * W;
#pragma unroll
    for (int t = 0; t < 4; ++t) {                       // nw, ne, sw, se
        const int xs = x0 + (t & 1), ys = y0 + (t >> 1);
        if (xs < 0 || xs >= (int)W || ys < 0 || ys >= (int)H) continue;
        const float w = wx[t & 1] * wy[t >> 1];
        const float *px = img + (size_t)ys * W + xs;
#pragma unroll
        for (int c = 0; c < channels; ++c) out[c] = out[c] + px[c * plane] * w;
    }
}

// the reference's `torch.Tensor(xy) / H * 2. - 1.`: BOTH axes divided by H
__device__ __forceinline__ float normalised(float v, uint32_t H) { return v / (float)H * 2.f - 1.f; }

// ------------------------------------------------------------------------------------------------------ unproject

__global__ __launch_bounds__(kBlock) void k_pc_count(const uint8_t *__restrict__ mask, uint32_t n,
                                                     uint32_t *__restrict__ block_sum) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = p < n && mask[p] != 0;
    const unsigned long long vote = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = (uint32_t)__popcll(vote);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += wave_sum[w];
        block_sum[blockIdx.x] = s;
    }
}

// exclusive scan of the workgroup sums in place (at most 2^20 of them), the total -> *count
__global__ __launch_bounds__(kRowThreads) void k_pc_scan(uint32_t *__restrict__ block_sum, uint32_t nb,
                                                         unsigned long long *__restrict__ count) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    const uint32_t total = mi3d_scan::scan_row(block_sum, nb, wave_sum, &base);
    if (threadIdx.x == 0) *count = total;
}

// refine_utils.py:131-139: v = Kinv . (x, y, 1), v *= D[y, x], p = v . R^T + t; consecutive lanes take consecutive x
__global__ __launch_bounds__(kBlock) void k_pc_unproject(const double *__restrict__ depth, const uint8_t *__restrict__ mask,
                                                         uint32_t n, uint32_t W, Unproject u,
                                                         const uint32_t *__restrict__ block_base,
                                                         double *__restrict__ points, unsigned long long cap) {
    __shared__ uint32_t wave_sum[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool keep = p < n && mask[p] != 0;
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(vote);
    __syncthreads();
    if (!keep) return;
    uint32_t rank = (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < kWaves; ++w) rank += w < wave ? wave_sum[w] : 0u;
    const unsigned long long row = (unsigned long long)block_base[blockIdx.x] + rank;
    if (row >= cap) return;                           // the caller reads *count and sees that it passed the cap
    const double x = (double)(p % W), y = (double)(p / W), d = depth[p];
    double v[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = ((u.kinv[3 * r] * x + u.kinv[3 * r + 1] * y) + u.kinv[3 * r + 2] * 1.0) * d;
    double *o = points + row * 3;
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = ((v[0] * u.c2w[4 * r] + v[1] * u.c2w[4 * r + 1]) + v[2] * u.c2w[4 * r + 2]) + u.c2w[4 * r + 3];
}

// ------------------------------------------------------------------------------------------------------- z-buffer

__global__ __launch_bounds__(kBlock) void k_pc_fill(unsigned long long *__restrict__ zkeys, uint32_t n) {
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    if (p < n) zkeys[p] = ~0ull;                      // above the key of every double, +inf included
}

__global__ __launch_bounds__(kBlock) void k_pc_zmin(const double *__restrict__ points, unsigned long long n, Camera c,
                                                    uint32_t H, uint32_t W, unsigned long long *__restrict__ zkeys) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    project(points + i * 3, c, x, y, z);
    uint32_t pix;
    if (!pixel_of(x, y, H, W, pix) || z != z) return;  // (a NaN depth makes x and y NaN: never in bounds)
    atomicMin(&zkeys[pix], key_of(z));
}

__global__ __launch_bounds__(kBlock) void k_pc_visible(const double *__restrict__ points, unsigned long long n, Camera c,
                                                       uint32_t H, uint32_t W,
                                                       const unsigned long long *__restrict__ zkeys,
                                                       uint8_t *__restrict__ visible) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    project(points + i * 3, c, x, y, z);
    uint32_t pix;
    bool vis = false;
    if (pixel_of(x, y, H, W, pix)) vis = z - double_of(zkeys[pix]) <= 1.0 / (double)H;   // NaN compares false
    visible[i] = vis ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------ box morph

// dilate: maximum, erode: minimum; fmaxf / fminf skip a NaN operand, so a NaN pixel counts as outside the image
template <bool dilate>
__device__ __forceinline__ float pick(float a, float b) { return dilate ? fmaxf(a, b) : fminf(a, b); }

template <bool dilate>
__global__ __launch_bounds__(kBlock) void k_box_morph(const float *__restrict__ src, float *__restrict__ dst, uint32_t H,
                                                      uint32_t W, uint32_t kh, uint32_t kw) {
    __shared__ float tile[kMaxTile][kMaxTile + 1];    // the input with its halo
    __shared__ float rows[kMaxTile][kTile];           // after the row pass
    const float pad = dilate ? -INFINITY : INFINITY;  // outside the image: ignored by the window
    const int ry = kh / 2, rx = kw / 2, th = kTile + 2 * ry, tw = kTile + 2 * rx;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    for (int i = threadIdx.x; i < th * tw; i += kBlock) {
        const int ly = i / tw, lx = i - ly * tw, gy = y0 + ly - ry, gx = x0 + lx - rx;
        tile[ly][lx] = (gy >= 0 && gy < (int)H && gx >= 0 && gx < (int)W) ? src[(size_t)gy * W + gx] : pad;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < th * kTile; i += kBlock) {
        const int ly = i / kTile, lx = i % kTile;
        float m = pad;
        for (uint32_t d = 0; d < kw; ++d) m = pick<dilate>(m, tile[ly][lx + d]);
        rows[ly][lx] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTile * kTile; i += kBlock) {
        const int ly = i / kTile, lx = i % kTile, gy = y0 + ly, gx = x0 + lx;
        if (gy >= (int)H || gx >= (int)W) continue;
        float m = pad;
        for (uint32_t d = 0; d < kh; ++d) m = pick<dilate>(m, rows[ly + d][lx]);
        dst[(size_t)gy * W + gx] = m;
    }
}

// ------------------------------------------------------------------------------- canonical filter and colouring

// refine_utils.py:100-107
__global__ __launch_bounds__(kBlock) void k_pc_cano_filter(const double *__restrict__ points, unsigned long long n,
                                                           Camera c, const float *__restrict__ cano_depth, uint32_t H,
                                                           uint32_t W, uint8_t *__restrict__ keep) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    project(points + i * 3, c, x, y, z);
    const double rx = rint(x), ry = rint(y);
    float sampled = 0.f;
    // np.round(..).astype(np.int32) -> torch.Tensor: what is non-finite or fits no int32 is out of bounds: it samples 0
    if (fabs(rx) < 2147483648.0 && fabs(ry) < 2147483648.0)
        bilinear<1>(cano_depth, H, W, normalised((float)rx, H), normalised((float)ry, H), &sampled);
    const double d = z - (double)sampled;
    keep[i] = (d <= 1.0 / (double)H && d >= -0.2) ? 0 : 1;
}

// refine_utils.py:111-114, :147-151: the projected xy is NOT rounded here
__global__ __launch_bounds__(kBlock) void k_pc_colour(const double *__restrict__ points, unsigned long long n, Camera c,
                                                      const float *__restrict__ image, uint32_t H, uint32_t W,
                                                      float *__restrict__ colour) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    project(points + i * 3, c, x, y, z);
    float rgb[3];
    bilinear<3>(image, H, W, normalised((float)x, H), normalised((float)y, H), rgb);
    float *o = colour + i * 3;
    o[0] = rgb[0];
    o[1] = rgb[1];
    o[2] = rgb[2];
}

// `project` itself: what the kernels above evaluate per point, written out
__global__ __launch_bounds__(kBlock) void k_pc_project(const double *__restrict__ points, unsigned long long n, Camera c,
                                                       double *__restrict__ xy, double *__restrict__ zs) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double x, y, z;
    project(points + i * 3, c, x, y, z);
    xy[i * 2] = x;
    xy[i * 2 + 1] = y;
    zs[i] = z;
}

bool pc_image(uint32_t H, uint32_t W) { return H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide; }

bool pc_camera(const double *rt_host, const double *k_host, Camera &c) {
    if (rt_host == nullptr || k_host == nullptr) return false;
    for (int q = 0; q < 12; ++q) c.rt[q] = rt_host[q];
    for (int q = 0; q < 9; ++q) c.k[q] = k_host[q];
    return true;
}

inline size_t unproject_workspace_bytes(uint32_t H, uint32_t W) {
    return (((size_t)pc_blocks((unsigned long long)H * W) * 4 + 7) / 8) * 8;
}

}  // namespace

extern "C" {

size_t mi3d_pc_unproject_workspace(uint32_t H, uint32_t W) { return pc_image(H, W) ? unproject_workspace_bytes(H, W) : 0; }

int mi3d_pc_unproject(const double *depth, const uint8_t *mask, uint32_t H, uint32_t W, const double *kinv_host,
                      const double *c2w_host, void *ws, size_t ws_bytes, double *points, unsigned long long cap,
                      unsigned long long *count, void *stream) {
    if (!pc_image(H, W) || depth == nullptr || mask == nullptr || kinv_host == nullptr || c2w_host == nullptr ||
        ws == nullptr || count == nullptr || (cap > 0 && points == nullptr))
        return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(ws) & 3u) != 0 || (reinterpret_cast<uintptr_t>(count) & 7u) != 0 ||
        ws_bytes < unproject_workspace_bytes(H, W))
        return (int)hipErrorInvalidValue;
    Unproject u;
    for (int q = 0; q < 9; ++q) u.kinv[q] = kinv_host[q];
    for (int q = 0; q < 12; ++q) u.c2w[q] = c2w_host[q];
    const uint32_t n = H * W, nb = pc_blocks(n);
    uint32_t *sums = reinterpret_cast<uint32_t *>(ws);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pc_count, dim3(nb), dim3(kBlock), 0, st, mask, n, sums);
    hipLaunchKernelGGL(k_pc_scan, dim3(1), dim3(kRowThreads), 0, st, sums, nb, count);
    hipLaunchKernelGGL(k_pc_unproject, dim3(nb), dim3(kBlock), 0, st, depth, mask, n, W, u, sums, points, cap);
    return (int)hipGetLastError();
}

int mi3d_pc_project(const double *points, unsigned long long n, const double *rt_host, const double *k_host, double *xy,
                    double *z, void *stream) {
    Camera c;
    if (!pc_camera(rt_host, k_host, c) || n > kMaxPoints || (n > 0 && (points == nullptr || xy == nullptr || z == nullptr)))
        return (int)hipErrorInvalidValue;
    if (n > 0)
        hipLaunchKernelGGL(k_pc_project, dim3(pc_blocks(n)), dim3(kBlock), 0, as_stream(stream), points, n, c, xy, z);
    return (int)hipGetLastError();
}

int mi3d_pc_zmin(const double *points, unsigned long long n, const double *rt_host, const double *k_host, uint32_t H,
                 uint32_t W, unsigned long long *zkeys, void *stream) {
    Camera c;
    if (!pc_image(H, W) || !pc_camera(rt_host, k_host, c) || zkeys == nullptr || (n > 0 && points == nullptr) ||
        n > kMaxPoints || (reinterpret_cast<uintptr_t>(zkeys) & 7u) != 0)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pc_fill, dim3(pc_blocks((unsigned long long)H * W)), dim3(kBlock), 0, st, zkeys, H * W);
    if (n > 0) hipLaunchKernelGGL(k_pc_zmin, dim3(pc_blocks(n)), dim3(kBlock), 0, st, points, n, c, H, W, zkeys);
    return (int)hipGetLastError();
}

int mi3d_pc_visible(const double *points, unsigned long long n, const double *rt_host, const double *k_host, uint32_t H,
                    uint32_t W, const unsigned long long *zkeys, uint8_t *visible, void *stream) {
    Camera c;
    if (!pc_image(H, W) || !pc_camera(rt_host, k_host, c) || zkeys == nullptr || n > kMaxPoints ||
        (n > 0 && (points == nullptr || visible == nullptr)))
        return (int)hipErrorInvalidValue;
    if (n > 0)
        hipLaunchKernelGGL(k_pc_visible, dim3(pc_blocks(n)), dim3(kBlock), 0, as_stream(stream), points, n, c, H, W, zkeys,
                           visible);
    return (int)hipGetLastError();
}

int mi3d_box_morph(const float *src, float *dst, uint32_t H, uint32_t W, uint32_t kh, uint32_t kw, int dilate,
                   void *stream) {
    if (!pc_image(H, W) || src == nullptr || dst == nullptr || src == dst || kh > (uint32_t)kMaxBox ||
        kw > (uint32_t)kMaxBox || (kh & 1u) == 0 || (kw & 1u) == 0 || (dilate != 0 && dilate != 1))
        return (int)hipErrorInvalidValue;
    const dim3 grid((W + kTile - 1) / kTile, (H + kTile - 1) / kTile);
    if (dilate)
        hipLaunchKernelGGL(k_box_morph<true>, grid, dim3(kBlock), 0, as_stream(stream), src, dst, H, W, kh, kw);
    else
        hipLaunchKernelGGL(k_box_morph<false>, grid, dim3(kBlock), 0, as_stream(stream), src, dst, H, W, kh, kw);
    return (int)hipGetLastError();
}

int mi3d_pc_cano_filter(const double *points, unsigned long long n, const double *rt_host, const double *k_host,
                        const float *cano_depth, uint32_t H, uint32_t W, uint8_t *keep, void *stream) {
    Camera c;
    if (!pc_image(H, W) || !pc_camera(rt_host, k_host, c) || cano_depth == nullptr || n > kMaxPoints ||
        (n > 0 && (points == nullptr || keep == nullptr)))
        return (int)hipErrorInvalidValue;
    if (n > 0)
        hipLaunchKernelGGL(k_pc_cano_filter, dim3(pc_blocks(n)), dim3(kBlock), 0, as_stream(stream), points, n, c,
                           cano_depth, H, W, keep);
    return (int)hipGetLastError();
}

int mi3d_pc_colour(const double *points, unsigned long long n, const double *rt_host, const double *k_host,
                   const float *image, uint32_t H, uint32_t W, float *colour, void *stream) {
    Camera c;
    if (!pc_image(H, W) || !pc_camera(rt_host, k_host, c) || image == nullptr || n > kMaxPoints ||
        (n > 0 && (points == nullptr || colour == nullptr)))
        return (int)hipErrorInvalidValue;
    if (n > 0)
        hipLaunchKernelGGL(k_pc_colour, dim3(pc_blocks(n)), dim3(kBlock), 0, as_stream(stream), points, n, c, image, H, W,
                           colour);
    return (int)hipGetLastError();
}

}  // extern "C"
