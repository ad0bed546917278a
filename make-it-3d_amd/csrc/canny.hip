// The Canny depth-edge detector of the refine stage's point cloud, for MI355X (gfx950, wave64): Part 12 of
// include/mi3d.h, which states the contract.  What `cv2.Canny(image, t1, t2)` (apertureSize 3, L1 gradient) computes in
// the reference's load_views (nerf/refine_utils.py:388), restated from memory: the contract is this project's own,
// parity with cv2 UNPINNED.
//
// Integers only: no floating-point flag matters to this unit.  |gx|, |gy| <= 4 * 255, so mag <= 2040 and the direction
// test's largest term, t67 = |gx| * 13573 + (|gx| << 16) <= 1020 * 79109 < 2^27, stays in 32 bits.
//
// Kernels (thread = pixel, consecutive lanes on consecutive x, a 32 x 32 tile per workgroup of 256; no allocation, no
// host synchronisation, no workgroup waits on another):
//   k_canny_classify    the image tile with a 2-pixel halo (borders replicated) -> LDS; Sobel magnitudes of the tile
//                       with a 1-pixel halo (0 outside the image) -> LDS; then per pixel the direction sector,
//                       non-maximum suppression and the double threshold.  Weak / strong counts: wave ballot + popcount,
//                       one 64-bit atomic pair per workgroup.
//   k_canny_hysteresis  one sweep: the class tile with a 1-pixel halo -> LDS; weak pixels with a strong 8-neighbour are
//                       promoted until the tile is stable (read, barrier, write, barrier-or); promoted pixels go back
//                       to memory.  Promotion is monotone (1 -> 2), so a neighbour tile read while it is being written
//                       is merely an earlier or later state of the same ascent: the fixed point is unique.
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_scan.h"

namespace {

constexpr int kBlock = 256, kWaves = kBlock / 64;
constexpr int kTile = 32, kPerThread = kTile * kTile / kBlock;
constexpr int kImg = kTile + 4, kMag = kTile + 2;      // tile sides with the 2- and the 1-pixel halo
constexpr unsigned long long kMaxPixels = 0x7FFFFFFFull;

using mi3d_scan::as_stream;

__host__ __device__ inline uint32_t tiles_of(uint32_t n) { return (n + kTile - 1) / kTile; }

// pixel coordinates are 64-bit: with H * W < 2^31 a side may reach 2^31 - 1, and a tile's halo lies past it
using coord = long long;

__device__ __forceinline__ coord clampc(coord v, coord hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the 3 x 3 Sobel pair about (ly, lx) of the image tile (coordinates of the tile WITH its halo)
__device__ __forceinline__ void sobel(const uint8_t (*img)[kImg + 4], int ly, int lx, int &gx, int &gy) {
    const int a = img[ly - 1][lx - 1], b = img[ly - 1][lx], c = img[ly - 1][lx + 1];
    const int d = img[ly][lx - 1], f = img[ly][lx + 1];
    const int g = img[ly + 1][lx - 1], h = img[ly + 1][lx], i = img[ly + 1][lx + 1];
    gx = (c + 2 * f + i) - (a + 2 * d + g);
    gy = (g + 2 * h + i) - (a + 2 * b + c);
}

__global__ __launch_bounds__(kBlock) void k_canny_classify(const uint8_t *__restrict__ image, uint32_t H, uint32_t W,
                                                           int low, int high, uint8_t *__restrict__ cls,
                                                           unsigned long long *__restrict__ counts) {
    __shared__ uint8_t img[kImg][kImg + 4];            // rows of 40 bytes: whole dwords
    __shared__ uint16_t mag[kMag][kMag + 2];
    __shared__ uint32_t wave_weak[kWaves], wave_strong[kWaves];
    const uint32_t tx = blockIdx.x % tiles_of(W), ty = blockIdx.x / tiles_of(W);
    const coord x0 = (coord)tx * kTile, y0 = (coord)ty * kTile;
    for (int i = threadIdx.x; i < kImg * kImg; i += kBlock) {
        const int ly = i / kImg, lx = i - ly * kImg;
        const coord gy = clampc(y0 + ly - 2, (coord)H - 1), gx = clampc(x0 + lx - 2, (coord)W - 1);
        img[ly][lx] = image[(size_t)gy * W + (size_t)gx];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kMag * kMag; i += kBlock) {
        const int ly = i / kMag, lx = i - ly * kMag;
        const coord py = y0 + ly - 1, px = x0 + lx - 1;
        int m = 0;
        if (py >= 0 && py < (coord)H && px >= 0 && px < (coord)W) {
            int gx, gy;
            sobel(img, ly + 1, lx + 1, gx, gy);
            m = abs(gx) + abs(gy);
        }
        mag[ly][lx] = (uint16_t)m;
    }
    __syncthreads();
    uint32_t weak = 0, strong = 0;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int i = k * kBlock + threadIdx.x, ly = i / kTile, lx = i % kTile;
        const coord py = y0 + ly, px = x0 + lx;
        const bool inside = py < (coord)H && px < (coord)W;
        int c = 0;
        if (inside) {
            const int my = ly + 1, mx = lx + 1, m = mag[my][mx];
            if (m > low) {
                int gx, gy;
                sobel(img, ly + 2, lx + 2, gx, gy);
                const int ax = abs(gx), ay = abs(gy) << 15, t22 = ax * 13573, t67 = t22 + (ax << 16);
                bool keep;
                if (ay < t22)
                    keep = m > mag[my][mx - 1] && m >= mag[my][mx + 1];
                else if (ay > t67)
                    keep = m > mag[my - 1][mx] && m >= mag[my + 1][mx];
                else if ((gx ^ gy) >= 0)
                    keep = m > mag[my - 1][mx - 1] && m > mag[my + 1][mx + 1];
                else
                    keep = m > mag[my - 1][mx + 1] && m > mag[my + 1][mx - 1];
                if (keep) c = m > high ? 2 : 1;
            }
            cls[(size_t)py * W + (size_t)px] = (uint8_t)c;
        }
        weak += (uint32_t)__popcll(__ballot(c == 1));
        strong += (uint32_t)__popcll(__ballot(c == 2));
    }
    if ((threadIdx.x & 63) == 0) {
        wave_weak[threadIdx.x >> 6] = weak;
        wave_strong[threadIdx.x >> 6] = strong;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t w = 0, s = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) {
            w += wave_weak[q];
            s += wave_strong[q];
        }
        if (w) atomicAdd(&counts[0], (unsigned long long)w);
        if (s) atomicAdd(&counts[1], (unsigned long long)s);
    }
}

// one sweep; `changed` is NULL in every sweep of a call but the last
__global__ __launch_bounds__(kBlock) void k_canny_hysteresis(uint8_t *__restrict__ cls, uint32_t H, uint32_t W,
                                                             int *__restrict__ changed) {
    __shared__ uint8_t t[kMag][kMag + 2];              // rows of 36 bytes
    const uint32_t tx = blockIdx.x % tiles_of(W), ty = blockIdx.x / tiles_of(W);
    const coord x0 = (coord)tx * kTile, y0 = (coord)ty * kTile;
    for (int i = threadIdx.x; i < kMag * kMag; i += kBlock) {
        const int ly = i / kMag, lx = i - ly * kMag;
        const coord py = y0 + ly - 1, px = x0 + lx - 1;
        t[ly][lx] = (py >= 0 && py < (coord)H && px >= 0 && px < (coord)W) ? cls[(size_t)py * W + (size_t)px] : (uint8_t)0;
    }
    __syncthreads();
    uint32_t promoted = 0;                             // bit k: this thread's k-th pixel went 1 -> 2
    for (;;) {
        uint32_t now = 0;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            const int i = k * kBlock + threadIdx.x, my = i / kTile + 1, mx = i % kTile + 1;
            if (t[my][mx] != 1) continue;
            const bool strong = t[my - 1][mx - 1] == 2 || t[my - 1][mx] == 2 || t[my - 1][mx + 1] == 2 ||
                                t[my][mx - 1] == 2 || t[my][mx + 1] == 2 || t[my + 1][mx - 1] == 2 ||
                                t[my + 1][mx] == 2 || t[my + 1][mx + 1] == 2;
            if (strong) now |= 1u << k;
        }
        __syncthreads();                               // every read of this round before any write
#pragma unroll
        for (int k = 0; k < kPerThread; ++k)
            if (now >> k & 1u) {
                const int i = k * kBlock + threadIdx.x;
                t[i / kTile + 1][i % kTile + 1] = 2;
            }
        promoted |= now;
        if (!__syncthreads_or((int)now)) break;        // uniform: every thread sees the same vote
    }
    // a weak pixel lies inside the image (outside is 0), so a promoted one does too
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
        if (promoted >> k & 1u) {
            const int i = k * kBlock + threadIdx.x;
            cls[(size_t)(y0 + i / kTile) * W + (size_t)(x0 + i % kTile)] = 2;
        }
    if (changed != nullptr && __syncthreads_or((int)promoted) && threadIdx.x == 0) atomicOr(changed, 1);
}

bool canny_image(uint32_t H, uint32_t W) { return H >= 1 && W >= 1 && (unsigned long long)H * W <= kMaxPixels; }

}  // namespace

extern "C" {

int mi3d_canny_classify(const uint8_t *image, uint32_t H, uint32_t W, int32_t low, int32_t high, uint8_t *cls,
                        unsigned long long *counts, void *stream) {
    if (!canny_image(H, W) || image == nullptr || cls == nullptr || counts == nullptr || image == cls ||
        (reinterpret_cast<uintptr_t>(counts) & 7u) != 0)
        return (int)hipErrorInvalidValue;
    if (low > high) {
        const int32_t s = low;
        low = high;
        high = s;
    }
    const hipStream_t st = as_stream(stream);
    const hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return (int)e;
    // at most 2^31 / 32 tiles (a one-pixel-wide image): a one-dimensional grid holds them
    const uint32_t tiles = tiles_of(W) * tiles_of(H);
    hipLaunchKernelGGL(k_canny_classify, dim3(tiles), dim3(kBlock), 0, st, image, H, W, (int)low, (int)high, cls, counts);
    return (int)hipGetLastError();
}

int mi3d_canny_hysteresis(uint8_t *cls, uint32_t H, uint32_t W, uint32_t sweeps, int32_t *changed, void *stream) {
    if (!canny_image(H, W) || cls == nullptr || changed == nullptr || sweeps < 1 ||
        (reinterpret_cast<uintptr_t>(changed) & 3u) != 0)
        return (int)hipErrorInvalidValue;
    const hipStream_t st = as_stream(stream);
    const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const uint32_t tiles = tiles_of(W) * tiles_of(H);
    for (uint32_t s = 0; s < sweeps; ++s)
        hipLaunchKernelGGL(k_canny_hysteresis, dim3(tiles), dim3(kBlock), 0, st, cls, H, W,
                           s + 1 == sweeps ? reinterpret_cast<int *>(changed) : nullptr);
    return (int)hipGetLastError();
}

}  // extern "C"
