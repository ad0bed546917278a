// Host-side planning of the hash-grid kernels (hashgrid.hip): the level table, the structs the kernels take by value, and
// every piece of arithmetic that decides what a launch will do - the gather's per-XCD segments, the binned scatter's
// slices, regions and reduce splits.  No HIP header: this file builds with plain g++ (tests/host_math/host_math.cpp
// compiles the planners for the host), and mi3d_grid.h adds the device-only parts.  The launches AND the plan queries of
// the C ABI (mi3d_grid_encode_plan, mi3d_grid_scatter_plan, mi3d_grid_scatter_binned_workspace) call plan_encode /
// plan_scatter below: "what will this call do" has one answer.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mi3d.h"
#include "mi3d_common.h"
#include "mi3d_dev.h"

namespace mi3d {

constexpr int kWave = 64;
constexpr int kTile = 64;   // samples per workgroup
constexpr int kWaves = 4;   // waves per workgroup

struct GridTable {
    GridLevel level[MI3D_MAX_LEVELS];
    uint32_t n_levels;
    uint32_t n_entries;
};

// Host: the level table exactly as tiny-cuda-nn's GridEncodingTemplated constructor lays it out.
inline uint32_t build_grid_table(GridTable &T, uint32_t n_levels, uint32_t base_resolution, float per_level_scale,
                                 uint32_t log2_hashmap_size) {
    const float l2 = log2f(per_level_scale);
    uint32_t offset = 0;
    T.n_levels = n_levels;
    for (uint32_t i = 0; i < n_levels && i < MI3D_MAX_LEVELS; ++i) {
        GridLevel &L = T.level[i];
        L.scale = exp2f((float)i * l2) * (float)base_resolution - 1.0f;
        L.res = (uint32_t)ceilf(L.scale) + 1u;
        const uint32_t max_params = 0xFFFFFFFFu / 2;
        uint32_t size = (powf((float)L.res, 3.0f) > (float)max_params) ? max_params : L.res * L.res * L.res;
        size = (size + 7u) / 8u * 8u;
        const uint32_t cap = 1u << log2_hashmap_size;
        if (size > cap) size = cap;
        L.size = size;
        L.offset = offset;
        // which dims the dense stride loop covers before the stride exceeds the level size
        uint32_t stride = 1, dims = 0;
        for (; dims < 3 && stride <= size; ++dims) stride *= L.res;
        L.dims = dims;
        L.hashed = size < stride ? 1u : 0u;
        offset += size;
    }
    T.n_entries = offset;
    return offset;
}

// ---------------------------------------------------------------- argument checks of the C entry points
inline bool valid_levels(uint32_t n_levels) { return n_levels != 0 && n_levels <= MI3D_MAX_LEVELS; }
// P stencil points, the first P0 of them around x, the others around x2
inline bool valid_stencil(uint32_t P0, uint32_t P, const float *x2) {
    return !(P == 0 || P > MI3D_MAX_POINTS || P0 > P || (P0 < P && x2 == nullptr));
}
// the marching step in [0, 1] units of a box of half side `bound` (no step known: 1/512)
inline float step01_of(float step, float bound) { return step > 0.f ? step / (2.0f * bound) : 1.0f / 512.0f; }

// Fast index paths.  grid_entry() is the general rule (any dims, any table size, any input): ~30 instructions and four
// uniform branches per corner pair, and with them the gather's coarse levels were INSTRUCTION-bound - ~300 issued
// instructions per (point, level) = the 0.84-1.05 ms those levels cost whether their table sat in the L1 or in LDS.
// Two level shapes cover every level the reference's configurations build, and a stencil point (PointSet mode 1) is
// clamped into [0, 1], so its cell coordinates never exceed res - 1:
//   kDense3    3-D strided index, cy * res and cz * res^2 in 24-bit multiplies.  The index wraps (grid_entry's
//              `index >= size`) only for the +1 corners of the box's last cells: ONE compare on the largest of the
//              four (y, z) bases decides for all eight corners, and a wave with such a lane takes the general path for
//              that point.  Everywhere else entries e and e + 1 are neighbours in memory: one 8-byte-aligned 16-byte
//              load per (y, z) pair, no select.
//   kHashPow2  power-of-two table: (cx ^ cy p1 ^ cz p2) & mask, the +1 bases by adding the prime; the x+1 corner is
//              the other half of the aligned 16-byte slot exactly when cx is even (x enters with prime 1): ONE
//              predicate for the four pairs, the odd lanes fetch their four x+1 corners behind the slots.
// Same entries, same weights, same order of the eight fused multiply-adds: the planes are bit-identical.
enum LevelKind : int { kGeneral = 0, kDense3 = 1, kHashPow2 = 2 };
struct LevelFast {
    int kind;
    uint32_t res2;     // res * res (kDense3)
    uint32_t last;     // size - 1: the mask (kHashPow2), the entry whose x+1 neighbour wraps (kDense3)
};
MI3D_HD LevelFast level_fast(const GridLevel &L, int mode) {
    LevelFast f = {kGeneral, L.res * L.res, L.size - 1u};
    if (mode == 0) return f;  // raw positions may lie outside [0, 1]
    if (L.hashed) {
        if ((L.size & (L.size - 1u)) == 0u && L.size >= 2u) f.kind = kHashPow2;
    } else if (L.dims == 3 && L.res >= 2u && (uint64_t)L.res * L.res * L.res < (1ull << 31) &&
               (uint64_t)L.res * L.res * L.res <= (uint64_t)L.size) {
        f.kind = kDense3;  // the largest corner index, res (1 + res + res^2), is below 2 size: it wraps at most once
    }
    return f;
}

// ---------------------------------------------------------------- the plane gather's plan (k_grid_encode_planes)
constexpr uint32_t kXcds = 8;
constexpr int kMaxSegs = 16;

struct EncodeSeg { uint32_t level, tile0, tile1, wgs; };  // wgs: workgroups of the XCD that walk this segment
struct EncodePlan {
    uint32_t n_seg[kXcds];
    EncodeSeg seg[kXcds][kMaxSegs];
};

// Relative cost of one tile of a level, as a function of x = (marching step) x (level scale) = how many cells of the
// level two consecutive samples of a ray are apart: the measured per-level times above, tabulated against x (C2: step
// 2 sqrt(3) / 1024 in a box of side 2) and interpolated, so other step sizes and grid configurations balance too.
inline double encode_level_cost(double x, bool dense_fast) {
    // ms per level at C2 with 6 workgroups per CU up to x = 0.26 and 3 beyond; a dense level on the short route is
    // instruction-bound and flat.  Round 6's fit, IN SITU: what a tile of each level costs its XCD while the other seven walk
    // theirs, from the per-XCD, per-segment timestamps of the whole gather (tools/encode_xcd_timeline.py,
    // profiles/encode_xcd_timeline_r06*.json).  Round 3's table (per-level launches of the whole chip) was equal within the
    // run-to-run spread: the balance of the XCDs is worth <= 0.9 ms and a static table cannot have it.
    static const double xs[] = {0.0, 0.136, 0.19, 0.26, 0.36, 0.50, 0.69, 0.95, 1.30, 1.80, 2.50, 3.50};
    if (dense_fast) return 0.383;
    static const double cs[] = {0.67, 0.685, 0.80, 0.853, 0.982, 1.416, 1.819, 2.246, 2.656, 2.72, 2.895, 2.78};
    constexpr int N = sizeof(xs) / sizeof(xs[0]);
    if (x <= xs[0]) return cs[0];
    for (int i = 1; i < N; ++i)
        if (x < xs[i]) return cs[i - 1] + (cs[i] - cs[i - 1]) * (x - xs[i - 1]) / (xs[i] - xs[i - 1]);
    return cs[N - 1];
}
// workgroups per CU a level is walked with: measured per level (same file) - 0.84 ms at 6 against 1.06 at 3 for the
// coarse levels, 1.53 at 3 against 1.67 at 6 where a wave's lanes sit in different lines (x = cells per marching step)
inline uint32_t encode_level_wgs_per_cu(double x, uint32_t coarse, uint32_t fine) { return x < 0.30 ? coarse : fine; }

// The (level, tile) list cut into kXcds contiguous segments of equal modelled cost.
inline EncodePlan make_encode_plan(const GridTable &T, uint32_t n_tiles, float step01, int only_level,
                                   uint32_t wgs_coarse_per_xcd, uint32_t wgs_fine_per_xcd, uint32_t first_level = 0,
                                   int point_mode = 1) {
    EncodePlan plan{};
    double cost[MI3D_MAX_LEVELS], total = 0.0;
    for (uint32_t l = 0; l < T.n_levels; ++l) {
        cost[l] = encode_level_cost((double)step01 * (double)T.level[l].scale,
                                    level_fast(T.level[l], point_mode).kind == kDense3);
        if (only_level >= 0) cost[l] = (int)l == only_level ? 1.0 : 0.0;
        if (l < first_level) cost[l] = 0.0;  // served from LDS by k_grid_encode_planes_lds
        total += cost[l];
    }
    const double share = total / kXcds;
    uint32_t x = 0;
    double filled = 0.0;  // cost already given to XCD x
    for (uint32_t l = 0; l < T.n_levels; ++l) {
        if (cost[l] <= 0.0) continue;
        uint32_t t0 = 0;
        while (t0 < n_tiles) {
            // tiles of this level that still fit XCD x's share (the last XCD takes whatever is left)
            const double room = share - filled;
            uint32_t take = (x + 1 == kXcds) ? n_tiles - t0 : (uint32_t)ceil(room / cost[l] * (double)n_tiles - 1e-9);
            if (take > n_tiles - t0) take = n_tiles - t0;
            if (take > 0 && plan.n_seg[x] < (uint32_t)kMaxSegs) {
                const uint32_t wgs = encode_level_wgs_per_cu((double)step01 * (double)T.level[l].scale,
                                                             wgs_coarse_per_xcd, wgs_fine_per_xcd);
                plan.seg[x][plan.n_seg[x]++] = EncodeSeg{l, t0, t0 + take, wgs};
                filled += cost[l] * (double)take / (double)n_tiles;
                t0 += take;
            }
            if (t0 < n_tiles || filled >= share - 1e-12) {
                if (x + 1 < kXcds) { ++x; filled = 0.0; }
                else if (take == 0) break;  // cannot happen: the last XCD takes everything
            }
        }
    }
    return plan;
}

// The longest prefix of levels whose tables fit the LDS of a CU together (150 KB of its 160): served by
// k_grid_encode_planes_lds.  *lds_bytes: the bytes of that prefix.
inline uint32_t lds_levels(const GridTable &T, size_t *lds_bytes) {
    constexpr size_t kEntryBytes = 2 * sizeof(float);
    uint32_t n_lds = 0;
    size_t bytes = 0;
    while (n_lds < T.n_levels && (size_t)(T.level[n_lds].offset + T.level[n_lds].size) * kEntryBytes <= (size_t)150 * 1024) {
        bytes = (size_t)(T.level[n_lds].offset + T.level[n_lds].size) * kEntryBytes;
        ++n_lds;
    }
    if (lds_bytes != nullptr) *lds_bytes = bytes;
    return n_lds;
}

// What one plane gather over n samples does: levels [0, n_lds) from LDS, the others by the XCD plan.  The caller settles
// n_lds (lds_levels, and whatever rule of its own it has); full_machine: the workgroup counts of a launch that fills the
// chip, whatever n is.
struct EncodeLaunchPlan {
    uint32_t n_lds;
    size_t lds_bytes;
    uint32_t wgs_fine, wgs_coarse;  // workgroups per XCD on the fine / the coarse segments
    EncodePlan plan;
};
inline EncodeLaunchPlan plan_encode(const GridTable &T, uint32_t n, float step01, uint32_t n_lds, size_t lds_bytes,
                                    int only_level, bool full_machine) {
    EncodeLaunchPlan e{};
    e.n_lds = n_lds;
    e.lds_bytes = lds_bytes;
    const uint32_t tiles = (n + kTile - 1) / kTile;
    const uint32_t need = full_machine ? 0xFFFFFFFFu : (tiles + kWaves - 1) / kWaves;  // workgroups one XCD needs to give every tile its own wave
    const uint32_t fine_cu = (uint32_t)MI3D_TUNE(MI3D_T_ENCODE_WGS_PER_CU, 3);
    const uint32_t coarse_cu = (uint32_t)MI3D_TUNE(MI3D_T_ENCODE_COARSE_WGS_PER_CU, 6);
    e.wgs_fine = need < 32 * fine_cu ? need : 32 * fine_cu;        // 32 CUs per XCD; persistent beyond
    e.wgs_coarse = need < 32 * coarse_cu ? need : 32 * coarse_cu;
    if (e.wgs_coarse < e.wgs_fine) e.wgs_coarse = e.wgs_fine;
    e.plan = make_encode_plan(T, tiles, step01, only_level, e.wgs_coarse, e.wgs_fine, n_lds);
    return e;
}

// ---------------------------------------------------------------- the binned scatter's plan (k_bin_emit, k_bin_reduce)
// The record path sums a tile in the gather table only where it pays: on levels whose cells are at least this many
// marching steps long (divided by default_merge_levels' own 1.05); the others emit per-point x-pair records.  4 steps =
// levels 0-6 at C2.  The gathered role is bound by its instruction stream and its LDS atomics whatever the gradients
// are, the record role by records, i.e. by how many gradient pairs are not zero.  Round 3 measured the threshold at 16-byte
// records (3 steps: level 7 gathered) - a real field iteration preferred 4.2 (89.5 -> 86.4 ms) but the dense-gradient
// scatter paid 58 -> 66 ms.  With 12-byte binary16 records and the shared-face pass (round 4) level 7 as records wins
// on both: 13-point scatter + deferred point-0 pair, one box, tools/kbench.py --what scatter_ab: dense gradients 62.25 ->
// 61.57 ms, a real step's zero census 40.87 -> 39.77 ms, whole steps -1.9 ms (tools/step_ab.py, anchored A/B); 5.8 steps
// (level 6 as records too): real 39.1, dense 66.2 - not taken (profiles/kbench_r04_scatter_ab.json).
#ifndef MI3D_MERGE_STEPS_X10_DEFAULT
#define MI3D_MERGE_STEPS_X10_DEFAULT 42
#endif
inline float merge_steps() { return (float)MI3D_TUNE(MI3D_T_MERGE_STEPS_X10, MI3D_MERGE_STEPS_X10_DEFAULT) / 10.5f; }

// levels whose cells are longer than one marching step `step01` (in [0,1] units) try to merge neighbours
inline uint32_t default_merge_levels(const GridTable &T, float step01) {
    uint32_t m = 0;
    for (uint32_t l = 0; l < T.n_levels; ++l)
        if (1.0f / (float)T.level[l].res >= 1.05f * step01) m = l + 1;
    return m;
}

constexpr uint32_t kBinShift = 13, kBinEntries = 1u << kBinShift;
#ifndef MI3D_EMIT_FINE_WAVES_DEFAULT
#define MI3D_EMIT_FINE_WAVES_DEFAULT 1536
#endif
constexpr uint32_t kEmitWavesMax = MI3D_EMIT_FINE_WAVES_DEFAULT;
constexpr uint32_t kReduceWavesC = 16;  // waves of a reduce workgroup (= kReduceWaves below)

struct __attribute__((packed, aligned(4))) BinRecord {
    uint32_t entry;  // level-local entry index
    float g0, g1;
};
// One record for the TWO x-neighbours of a (y, z) corner pair on a fine level.  The four values of such a pair have rank
// one - (1 - fx) (a, b) for the corner at x, fx (a, b) for the one at x + 1, with (a, b) = w_y w_z (dfeature0, dfeature1)
// - and the two entries differ in their low bits only (hashed: e1 = e0 ^ (2^t - 1), t = 1 + trailing ones of cx, because x
// enters the hash with prime 1; dense: e1 = e0 + 1), so 16 bytes carry what two 12-byte records did: half the
// lane-stores and LDS counter updates of the emit and two thirds of the bytes.
// hdr = e0 | t << 19 (t = 0: dense "+1").  fx == 0 marks a single (only e0 receives (a, b)): pairs that straddle a bin.
struct __attribute__((aligned(16))) RowRecord {
    uint32_t hdr;
    float a, b, fx;
};
constexpr uint32_t kRowEntryBits = 19;

struct BinPlan {
    uint32_t level_bin0[MI3D_MAX_LEVELS];   // first bin of each level (bins are numbered level by level)
    uint32_t level_cap[MI3D_MAX_LEVELS];    // records one (wave, bin) region of that level holds
    uint32_t level_waves[MI3D_MAX_LEVELS];  // emitting waves of that level (coarse levels: many, fine levels: 2048)
    uint64_t level_base[MI3D_MAX_LEVELS];   // BYTE offset of the level in the arena; inside: [wave][bin][cap] records
    uint32_t level_cnt0[MI3D_MAX_LEVELS];   // first entry of the level in counts[]; inside: [wave][bin]
    uint32_t level_max0[MI3D_MAX_LEVELS];   // first entry of the level in level_max[]; inside: [wave]
    uint64_t total_bytes;
    uint32_t row_mask;                      // fine levels stored as x-pair records (RowRecord, 16 bytes; Row12 with rec12)
    uint32_t rec12;                         // binary16 gradient planes: the pair records are 12 bytes (Row12)
    uint32_t level_split[MI3D_MAX_LEVELS];  // reduce workgroups that share one bin of the level
    uint32_t level_wg0[MI3D_MAX_LEVELS];    // first reduce workgroup of the level; inside: [bin][split]
    uint32_t n_reduce_wgs;
    uint32_t total_counts, total_max;
    uint32_t n_levels, n_bins;
    uint32_t claim0;                        // level_max[claim0 ..+1] as uint32: the two roles' tile-claim counters (k_bin_emit)
};

#ifndef MI3D_EMIT_COARSE_WAVES_DEFAULT
// Emitting waves of the coarse role = regions per coarse bin the reduce has to walk (a fixed cost per slice).  The chip holds
// 3072 emitting waves at a time (256 CUs x 4 SIMDs x 3), 1536 of them the fine role's: 3072 coarse waves are two full rounds
// of the other half.  Round 6, product-grade builds in one process on a placed arena (tools/scatter_ab_libs.py,
// profiles/scatter_ab_libs_r06_coarse_waves_{56,30}GiB.json; dense / real census, ms): 16384 (rounds 3-5) 47.8 / 41.1,
// 4096 48.7 / 43.3, 3072 47.1 / 40.6, 2048 53.9 / 48.3, 1536 47.0 / 40.6, 1024 55.5 / 49.3, 512 81.3 / 75.2 - whole rounds or
// many; with four slices (30 GiB) 16384 54.4 / 44.6, 3072 51.9 / 41.8, 1536 51.7 / 41.9.
#define MI3D_EMIT_COARSE_WAVES_DEFAULT 3072
#endif
#ifndef MI3D_HASHED_SLACK
// a hashed level's region capacity over the uniform share of its records (plan_for)
#define MI3D_HASHED_SLACK 1.25
#endif
MI3D_HD uint32_t level_bins(const GridLevel &L) { return (L.size + kBinEntries - 1) / kBinEntries; }

inline uint32_t round_waves(uint64_t w, uint32_t cap_waves) {
    uint32_t nw = (uint32_t)(w < cap_waves ? w : cap_waves);
    nw = (nw + kWaves - 1) / kWaves * kWaves;
    return nw ? nw : kWaves;
}

// The plan for slices of n_slice samples.  Fine levels are emitted by at most 1536 waves (the lines being appended to
// must fit the L2s); the coarse levels' run merging is latency-bound and emits few records, so it gets up to 3072 (see MI3D_EMIT_COARSE_WAVES_DEFAULT).
// Region capacities - hashed levels: the uniform share of the UNMERGED record count plus 25 % (the hash spreads them
// evenly).  Dense levels: bins are spatial, a wave's samples cluster in few of them, and merging thins the records by
// an unknown factor: the share assumes a quarter of the geometric run length and two-fold imbalance.  A full region is
// not an error - the overflow goes to the table by atomics.
inline BinPlan plan_for(const GridTable &T, uint64_t n_slice, uint32_t P, float step01, uint32_t merge_levels,
                        bool half_planes = false) {
    const uint32_t fine_waves = (uint32_t)MI3D_TUNE(MI3D_T_EMIT_FINE_WAVES, kEmitWavesMax);
    const uint32_t coarse_waves = (uint32_t)MI3D_TUNE(MI3D_T_EMIT_COARSE_WAVES, MI3D_EMIT_COARSE_WAVES_DEFAULT);
    BinPlan p{};
    p.n_levels = T.n_levels;
    p.rec12 = half_planes ? 1u : 0u;
    const uint64_t tiles = (n_slice + kWave - 1) / kWave;
    for (uint32_t l = 0; l < T.n_levels; ++l) {
        const GridLevel &L = T.level[l];
        const uint32_t bins = level_bins(L);
        const bool merged = l < merge_levels;
        p.level_waves[l] = round_waves(tiles, merged ? coarse_waves : fine_waves);
        const double pts_per_wave = (double)n_slice * P / p.level_waves[l];
        double per = pts_per_wave * 8.0 / bins;
        if (L.hashed) {
            per *= MI3D_HASHED_SLACK;
        } else {
            double run = merged ? (1.0 / (double)L.res) / (1.5 * (double)step01) / 4.0 : 1.0;
            run = run < 1.0 ? 1.0 : run;
            per = per / run * 2.0;
        }
        // merged (coarse) levels emit one record per distinct entry a tile touched: measured 3-6 % of the per-contribution
        // count (tools/scatter_fill.py, profiles/scatter_fill_r02.json) - their regions get a fifth of it (round 2 sized
        // them for every contribution: 52 of the arena's 92 GiB at C2).  A full region is not an error (float atomics).
        if (merged) per *= 0.2;
        p.level_cap[l] = (uint32_t)per + 64u;
        // fine fp32 levels whose x-neighbour entries are derivable from each other: one 16-byte record per corner pair
        const bool row = !merged && L.size <= (1u << kRowEntryBits) &&
                         (!L.hashed || (L.size & (L.size - 1u)) == 0u);
        if (row) { p.row_mask |= 1u << l; p.level_cap[l] = p.level_cap[l] / 2u + 64u; }
        p.level_bin0[l] = p.n_bins;
        p.level_base[l] = p.total_bytes;
        p.level_cnt0[l] = p.total_counts;
        p.level_max0[l] = p.total_max;
        p.n_bins += bins;
        p.total_bytes += (uint64_t)p.level_waves[l] * bins * p.level_cap[l] *
                         (row ? (p.rec12 ? sizeof(Row12) : sizeof(RowRecord)) : sizeof(BinRecord));
        p.total_bytes = (p.total_bytes + 255u) / 256u * 256u;
        p.total_counts += p.level_waves[l] * bins;
        p.total_max += p.level_waves[l];
    }
    p.claim0 = p.total_max;
    p.total_max += 4u;
    return p;
}
// How many reduce workgroups share a bin.  A bin's records are spread over the level's emitting waves, so `split`
// workgroups can each take every split-th group of 16 regions.  The bins are NOT equally heavy: a fine level puts ~4.4 M
// x-pair records into each of its 64 bins at C2, but level 0 is ONE bin that receives 80 M run-merged records, level 1
// two bins with 54 M each (tools/scatter_fill.py) - with the same split for every bin the reduce waited 12 ms for those
// few workgroups.  So the split follows the expected work per bin (region capacity x waves x the usual fill - 0.78 for
// per-point records, a few per cent for the gathered records of the coarse levels, whose regions are sized for the worst
// case; an x-pair record costs two single ones), normalised so that the average bin gets `base_split` workgroups.
inline void plan_reduce_splits(BinPlan &p, const GridTable &T, uint32_t base_split, uint32_t merge_levels) {
    double work[MI3D_MAX_LEVELS], total = 0.0;
    uint32_t bins_total = 0;
    for (uint32_t l = 0; l < T.n_levels; ++l) {
        const bool row = (p.row_mask >> l) & 1u;
        work[l] = (double)p.level_waves[l] * p.level_cap[l] * (row ? 0.78 * 2.0 : (l < merge_levels ? 0.05 : 0.78));
        total += work[l] * level_bins(T.level[l]);
        bins_total += level_bins(T.level[l]);
    }
    const double target = total / bins_total / base_split;  // work one reduce workgroup should get
    p.n_reduce_wgs = 0;
    for (uint32_t l = 0; l < T.n_levels; ++l) {
        uint32_t split = (uint32_t)(work[l] / target + 0.5);
        const uint32_t most = p.level_waves[l] / kReduceWavesC ? p.level_waves[l] / kReduceWavesC : 1u;  // >= 1 region per wave
        split = split < 1u ? 1u : (split > most ? most : split);
        p.level_split[l] = split;
        p.level_wg0[l] = p.n_reduce_wgs;
        p.n_reduce_wgs += level_bins(T.level[l]) * split;
    }
}

inline size_t bin_workspace_bytes(const BinPlan &p) {
    return (size_t)p.total_bytes + (size_t)p.total_counts * sizeof(uint32_t) +
           (size_t)p.total_max * sizeof(float);
}

// The slice length of a call over n samples: ceil(n / k) for the smallest k whose plan fits the workspace (k = 1, 2, 3 ...
// up to 64, doubling from there).  Round 2-5 halved the slice (k = 1, 2, 4 ...): at C2 an arena between 31 and 46 GiB then
// ran the four-slice plan of 24.7 GB although three slices (33 GB) fit - and every slice has a fixed cost (the emit's and
// the reduce's tails, the regions the reduce walks).  `plan` receives the slice's plan (which may still not fit: the caller
// checks and takes the atomic path).
inline uint64_t slice_for(const GridTable &T, uint64_t n, uint32_t P, float step01, uint32_t merge_levels, bool half_planes,
                          size_t workspace_bytes, BinPlan &plan) {
    uint64_t n_slice = n;
    plan = plan_for(T, n_slice, P, step01, merge_levels, half_planes);
    for (uint64_t k = 2; n_slice > kWave && bin_workspace_bytes(plan) > workspace_bytes; k = k < 64 ? k + 1 : 2 * k) {
        n_slice = (n + k - 1) / k;
        plan = plan_for(T, n_slice, P, step01, merge_levels, half_planes);
    }
    return n_slice;
}

// slots of the emit's per-wave gather table (hashgrid.hip k_bin_emit, which also stages the fine role's records in it)
constexpr uint32_t kMergeSlots = 512;
MI3D_HD uint32_t emit_wave_words(uint32_t n_bins) {  // 32-bit words of LDS per emitting wave (even)
    return 4u * kMergeSlots + kMergeSlots + ((n_bins + 1u) & ~1u);
}

#ifndef MI3D_REDUCE_BASE_SPLIT
// reduce workgroups per average bin for slices of 30 M evaluations and more (plan_reduce_splits).  Round 6, product-grade builds
// in one process (profiles/scatter_ab_libs_r06_reduce_split.json; dense / synthetic census / captured real step, ms): 3: 44.78 /
// 38.24 / 32.21, 4: 44.85 / 38.25 / 32.28, 6: 44.93 / 38.39 / 32.27, 8: 44.96 / 38.47 / 32.45 - flat: the reduce's tail is not where
// its time goes
#define MI3D_REDUCE_BASE_SPLIT 4
#endif
// reduce workgroups per average bin for a slice of `evals` evaluations: zeroing and flushing the 128 KB tile is most of a
// small pass's work
inline uint32_t reduce_base_split(uint64_t evals) {
    return evals >= 30000000ull ? (uint32_t)MI3D_REDUCE_BASE_SPLIT : (evals >= 8000000ull ? 2u : 1u);
}

// What one binned scatter over n samples does with `workspace_bytes`: P_rec record-carrying points per sample, binary16 or
// fp32 gradient planes.  The plan may still not fit the workspace: the caller checks (bin_workspace_bytes) and takes the
// atomic path; the reduce splits are planned per slice (plan_reduce_splits with reduce_base_split of its evaluations).
struct ScatterPlan {
    BinPlan plan;
    uint64_t n_slice;       // the samples are cut into the FEWEST equal slices whose record arena fits the workspace
    uint32_t merge_levels;  // the record path run-merges only where it pays (cells at least merge_steps() marching steps long)
    uint32_t merge_atomic;  // levels that run-merge on the atomic fallback path
    float step01;
};
inline ScatterPlan plan_scatter(const GridTable &T, uint64_t n, uint32_t P_rec, float bound, float step, bool half_planes,
                                size_t workspace_bytes) {
    ScatterPlan s;
    s.step01 = step01_of(step, bound);
    s.merge_atomic = default_merge_levels(T, s.step01);
    s.merge_levels = default_merge_levels(T, s.step01 * merge_steps());
    s.n_slice = slice_for(T, n, P_rec, s.step01, s.merge_levels, half_planes, workspace_bytes, s.plan);
    return s;
}

}  // namespace mi3d
