// The integer arithmetic of the area-adaptive atlas (include/mi3d.h Part 20) that the host and the device share: the
// ladder of legs, the class of a bin under a shift, the plan (shelf packing of the class histogram) with its flat
// layout, the position of a class's cell and the ownership rule of a cell's texels.
//
// Plain C++17 without a HIP include: the system compiler builds it alone.  atlasadaptive.hip defines MI3D_HD as
// __host__ __device__ before it includes this file.
#pragma once
#include <cstdint>

#ifndef MI3D_HD
#define MI3D_HD
#endif

namespace mi3d_atlas {

constexpr uint32_t kMinT = 64, kMaxT = 16384;
constexpr int kBins = 64, kClasses = 16;     // bins per leg (64 x 64 histogram), classes per leg (16 x 16 keys)
constexpr int kBinLo = -60, kBinHi = 3;      // the exponents of a squared length that bins 0 and 63 stand for

// plan layout, in 32-bit words (MI3D_ATLAS_PLAN_WORDS of mi3d.h is kPlanWords)
constexpr int kHead = 16, kGroupWords = 8, kClassWords = 12;
constexpr int kGroups = kHead, kRecords = kGroups + kClasses * kGroupWords, kIndex = kRecords + 256 * kClassWords;
constexpr int kPlanWords = kIndex + 256;
enum Head { H_SHIFT, H_T, H_KMAX, H_ROWS, H_GROUPS, H_NCLASS, H_NT, H_OWNED, H_CLAMPED_LO, H_CLAMPED_HI };
enum Group { G_Y0, G_HEIGHT, G_SHELVES, G_FIRST, G_COUNT, G_KB };
enum Class { C_KEY, C_A, C_B, C_X0, C_SHELF0, C_N0, C_PER, C_COUNT, C_START, C_Y0, C_CELLS };

MI3D_HD inline int leg(int k) {  // round(2^(k / 2 + 1)), k = 0 .. 15
    constexpr int kLegs[kClasses] = {2, 3, 4, 6, 8, 11, 16, 23, 32, 45, 64, 91, 128, 181, 256, 362};
    return kLegs[k];
}

// the largest k with leg(k) + 3 <= T; at least 9 for T >= 64
MI3D_HD inline int kmax_of(uint32_t T) {
    int k = 0;
    while (k + 1 < kClasses && (uint32_t)leg(k + 1) + 3u <= T) ++k;
    return k;
}

// the bin of a squared length given as its binary32 bits: biased exponent - 127, clamped to [-60, 3], + 60; zero,
// denormal and non-finite lengths: 0
MI3D_HD inline int bin_of_bits(uint32_t bits) {
    const int e = (int)((bits >> 23) & 0xffu);
    if (e == 0 || e == 255) return 0;
    const int x = e - 127;
    return (x < kBinLo ? kBinLo : x > kBinHi ? kBinHi : x) - kBinLo;
}

MI3D_HD inline int class_of(int bin, int shift, int kmax) {
    const int k = bin - shift;
    return k < 0 ? 0 : k > kmax ? kmax : k;
}

// the shape word of a triangle: rot in bits 0-1, binAB in bits 8-13, binAC in bits 16-21, bit 31: an index out of range
MI3D_HD inline uint32_t shape_word(int rot, int binAB, int binAC, bool bad) {
    return (uint32_t)rot | ((uint32_t)binAB << 8) | ((uint32_t)binAC << 16) | (bad ? 0x80000000u : 0u);
}
MI3D_HD inline int shape_rot(uint32_t w) { return (int)(w & 3u); }
MI3D_HD inline int shape_key(uint32_t w, int shift, int kmax) {  // kb * 16 + ka
    return class_of((int)((w >> 16) & 63u), shift, kmax) * kClasses + class_of((int)((w >> 8) & 63u), shift, kmax);
}

// half 0 of an (a + 3) x (b + 3) cell owns local texel (x, y)
MI3D_HD inline bool owns_half0(int a, int b, int x, int y) {
    if (x < 0 || y < 0 || x > a || y > b) return false;
    const int mx = x > 0 ? x - 1 : 0, my = y > 0 ? y - 1 : 0;
    return b * mx + a * my < a * b;
}

// -1: no one, else the half that owns local texel (x, y), 0 <= x <= a + 2, 0 <= y <= b + 2
MI3D_HD inline int half_of(int a, int b, int x, int y) {
    if (owns_half0(a, b, x, y)) return 0;
    return owns_half0(a, b, a + 2 - x, b + 2 - y) ? 1 : -1;
}

// the top-left texel of cell q of the class record c
MI3D_HD inline void cell_origin(const int32_t *c, uint32_t T, uint32_t q, uint32_t &X0, uint32_t &Y0) {
    const uint32_t w = (uint32_t)c[C_A] + 3u, h = (uint32_t)c[C_B] + 3u, n0 = (uint32_t)c[C_N0];
    (void)T;
    if (q < n0) {
        X0 = (uint32_t)c[C_X0] + q * w;
        Y0 = (uint32_t)c[C_Y0] + (uint32_t)c[C_SHELF0] * h;
    } else {
        const uint32_t r = q - n0, per = (uint32_t)c[C_PER];
        X0 = (r % per) * w;
        Y0 = (uint32_t)c[C_Y0] + ((uint32_t)c[C_SHELF0] + 1u + r / per) * h;
    }
}

// ------------------------------------------------------------------------------------------------ host side

// the 16 x 16 class counts of a 64 x 64 bin histogram (hist[binAC * 64 + binAB]) under a shift, and the clamped legs
inline void classes_of(const uint32_t *hist, int shift, int kmax, unsigned long long *count, unsigned long long *clamped) {
    for (int k = 0; k < 256; ++k) count[k] = 0;
    clamped[0] = clamped[1] = 0;
    for (int bc = 0; bc < kBins; ++bc)
        for (int bb = 0; bb < kBins; ++bb) {
            const unsigned long long n = hist[bc * kBins + bb];
            if (n == 0) continue;
            count[class_of(bc, shift, kmax) * kClasses + class_of(bb, shift, kmax)] += n;
            for (int bin : {bb, bc}) {
                if (bin - shift < 0) clamped[0] += n;        // more texels than its length asks for
                else if (bin - shift > kmax) clamped[1] += n;  // fewer
            }
        }
}

// Shelf packing of the class counts into T columns; writes groups and records if plan is not null.  Returns the rows
// used (they may pass T: the caller compares).
inline unsigned long long pack(const unsigned long long *count, uint32_t T, int32_t *plan) {
    unsigned long long y = 0;
    int g = 0, rec = 0;
    for (int kb = kClasses - 1; kb >= 0; --kb) {
        const uint32_t h = (uint32_t)leg(kb) + 3u;
        unsigned long long shelf = 0;  // the current shelf of the group
        uint32_t x = 0;
        bool any = false;
        const int first = rec;
        for (int ka = kClasses - 1; ka >= 0; --ka) {
            const unsigned long long n = count[kb * kClasses + ka];
            if (n == 0) continue;
            any = true;
            const uint32_t w = (uint32_t)leg(ka) + 3u, per = T / w;
            if (per == 0) return ~0ull;
            const unsigned long long cells = (n + 1) / 2;
            if (T - x < w) { ++shelf; x = 0; }
            const uint32_t n0 = (T - x) / w;
            if (plan != nullptr) {
                int32_t *c = plan + kRecords + rec * kClassWords;
                c[C_KEY] = kb * kClasses + ka; c[C_A] = leg(ka); c[C_B] = leg(kb); c[C_X0] = (int32_t)x;
                c[C_SHELF0] = (int32_t)shelf; c[C_N0] = (int32_t)n0; c[C_PER] = (int32_t)per; c[C_COUNT] = (int32_t)n;
                c[C_START] = 0; c[C_Y0] = (int32_t)y; c[C_CELLS] = (int32_t)cells; c[11] = 0;
                plan[kIndex + kb * kClasses + ka] = rec;
            }
            ++rec;
            if (cells <= n0) {
                x += (uint32_t)cells * w;
            } else {
                const unsigned long long r = cells - n0;       // cells in the shelves below the first
                shelf += (r + per - 1) / per;
                x = (uint32_t)(r - (r - 1) / per * per) * w;   // the last shelf holds 1 .. per of them
            }
        }
        if (!any) continue;
        const unsigned long long shelves = shelf + 1;
        if (plan != nullptr) {
            int32_t *gr = plan + kGroups + g * kGroupWords;
            gr[G_Y0] = (int32_t)y; gr[G_HEIGHT] = (int32_t)h; gr[G_SHELVES] = (int32_t)shelves; gr[G_FIRST] = first;
            gr[G_COUNT] = rec - first; gr[G_KB] = kb; gr[6] = gr[7] = 0;
        }
        ++g;
        y += shelves * h;
        if (y > 0x7fffffffull) return ~0ull;
    }
    if (plan != nullptr) { plan[H_GROUPS] = g; plan[H_NCLASS] = rec; }
    return y;
}

// the texels half 0 of an (a, b) cell owns
inline unsigned long long owned_by_half(int a, int b) {
    unsigned long long n = 0;
    for (int y = 0; y <= b; ++y)
        for (int x = 0; x <= a; ++x) n += owns_half0(a, b, x, y) ? 1u : 0u;
    return n;
}

// The plan of Part 20 for a bin histogram and T: the smallest shift in [0, 63] whose packing uses at most T rows.
// Returns 1 and fills plan[kPlanWords], or returns 0 (T out of range, an empty or oversized histogram, no shift fits)
// and leaves plan unspecified.
inline uint32_t make_plan(const uint32_t *hist, uint32_t T, int32_t *plan) {
    if (hist == nullptr || plan == nullptr || T < kMinT || T > kMaxT) return 0;
    unsigned long long nt = 0;
    for (int i = 0; i < kBins * kBins; ++i) nt += hist[i];
    if (nt == 0 || nt > 0x7fffffffull) return 0;
    const int kmax = kmax_of(T);
    unsigned long long count[256], clamped[2];
    for (int s = 0; s < kBins; ++s) {
        classes_of(hist, s, kmax, count, clamped);
        if (pack(count, T, nullptr) > T) continue;
        for (int i = 0; i < kPlanWords; ++i) plan[i] = i >= kIndex ? -1 : 0;
        const unsigned long long rows = pack(count, T, plan);
        plan[H_SHIFT] = s; plan[H_T] = (int32_t)T; plan[H_KMAX] = kmax; plan[H_ROWS] = (int32_t)rows;
        plan[H_NT] = (int32_t)nt;
        plan[H_CLAMPED_LO] = (int32_t)(clamped[0] > 0x7fffffffull ? 0x7fffffffull : clamped[0]);
        plan[H_CLAMPED_HI] = (int32_t)(clamped[1] > 0x7fffffffull ? 0x7fffffffull : clamped[1]);
        // the sorted order is by key: a class starts where the smaller keys end
        unsigned long long start = 0, owned = 0;
        for (int key = 0; key < 256; ++key) {
            const int rec = plan[kIndex + key];
            if (rec < 0) continue;
            int32_t *c = plan + kRecords + rec * kClassWords;
            c[C_START] = (int32_t)start;
            start += count[key];
            owned += count[key] * owned_by_half(c[C_A], c[C_B]);
        }
        plan[H_OWNED] = (int32_t)owned;  // at most T^2 <= 2^28
        return 1;
    }
    return 0;
}

}  // namespace mi3d_atlas
