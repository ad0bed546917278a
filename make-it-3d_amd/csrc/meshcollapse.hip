// Quadric edge-collapse decimation of an indexed triangle mesh for MI355X (gfx950, wave64); Part 19 of include/mi3d.h,
// which states the contract: usable triangles, the quadrics, the locks, the candidate rules, the placement, the key,
// the independence rule, the quota, the apply, the output, the counts.  Rounds of independent collapses: every round
// rebuilds the vertex -> triangle incidence of the live triangles (as meshsmooth.hip builds its own, through
// mi3d_incidence.h), and every decision of a round reads only what the round before left.
//
// Compiled with -ffp-contract=off: every binary64 operation below is rounded on its own, in the order written.
//
// ORDER.  A triangle claims a slot of each corner's row by an atomic cursor, so the order of a row depends on
// scheduling.  Nothing read from a row does: the border rule and the link condition count equal entries, the flip test
// is a conjunction, the claims are 64-bit atomicMin.  The one ordered sum, the quadric of a vertex, sorts its row first.
//
// WHETHER A ROUND RUNS is decided on the device: k_co_round_begin reads the live count and the winners of the round
// before and sets ctrl->active; every other kernel of the round returns at once without it.
//
// Launches (no host synchronisation, no allocation):
//  begin   k_co_zero        counts = 0, ctrl = 0
//          k_co_vertices    per vertex: position, rep = v, cursor = 0; non-finite vertices -> counts[4]
//          k_co_usable      per triangle: usable -> corners, alive, the degrees; the live count by block sums; the
//                           triangles without a plane -> ctrl
//          k_co_block_sums, k_co_scan, k_co_offsets, k_co_fill: the incidence
//          k_co_quadrics    per vertex: the row sorted, K of every triangle summed in that order
//          k_co_begin_end   one thread: counts[1], counts[2]
//  round   k_co_round_begin one thread: active, quota, the round's counters
//          k_co_clear       per vertex: cursor = 0, claim = none
//          k_co_degree      per live triangle: the degrees
//          k_co_block_sums, k_co_scan, k_co_offsets, k_co_fill
//          k_co_locks       per vertex: degree and border -> locked; counts[6]
//          k_co_candidates  per live triangle and owned edge: the rules, x*, the key; atomicMin on the two claims
//          k_co_winners     per candidate: the claims of the closed neighbourhood; winners per workgroup
//          k_co_rank        one workgroup: scan of the winners per workgroup
//          k_co_apply       per winner below the quota: rep, position, quadric
//          k_co_rename      per live triangle: corners renamed, dead if two coincide; the live count by block sums
//          k_co_rep         per vertex: rep one hop up to date; one thread closes the round's books
//  count   k_co_clear, k_co_cite, k_co_block_sums, k_co_scan, k_co_offsets, k_co_totals
//  emit    k_co_emit_vertices, k_co_emit_triangles
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mi3d.h"
#include "mi3d_incidence.h"

namespace {

using namespace mi3d_scan;

constexpr int kBlock = mi3d_incidence::kBlock, kWaves = mi3d_incidence::kWaves;
constexpr unsigned long long kMaxVertices = 0x7FFFFFFFull;  // indices are int32
constexpr unsigned long long kMaxTriangles = 1ull << 30;    // 3 nt row slots and edge ids are uint32
constexpr uint32_t kMaxDegree = MI3D_COLLAPSE_MAX_DEGREE, kMaxRow = MI3D_COLLAPSE_MAX_ROW;
constexpr uint32_t kMaxRounds = 4096;                       // per call of mi3d_mesh_collapse_rounds
constexpr unsigned long long kNone = ~0ull;                 // a claim nobody made, the key of no candidate

// counts (device uint64[8]): see Part 19
enum { kVertices = 0, kTriangles = 1, kUnusable = 2, kRounds = 3, kNonFinite = 4, kCollapses = 5, kLocked = 6, kErrors = 7 };

// workspace: collapse_layout of mi3d_workspace.h, the one statement of its arrays and its size; Ctrl, its first 64 bytes,
// is what the rounds keep between kernels
using Ctrl = mi3d_workspace::CollapseCtrl;
using Ws = mi3d_workspace::CollapseWorkspace;
using namespace mi3d_workspace;
static_assert(kBlock == kLayoutBlock, "collapse_layout sizes its rows of block sums by this workgroup");

inline size_t ws_bytes_of(unsigned long long nv, unsigned long long nt) {
    return bytes_of(collapse_layout, (uint32_t)nv, (uint32_t)nt);
}

// ------------------------------------------------------------------------------------------------ binary64 geometry

struct D3 {
    double x, y, z;
};

__device__ __forceinline__ D3 widen(const float *__restrict__ row) { return {(double)row[0], (double)row[1], (double)row[2]}; }

__device__ __forceinline__ double dot3(D3 u, D3 v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }

// n = (p1 - p0) x (p2 - p0)
__device__ __forceinline__ D3 normal_of(D3 p0, D3 p1, D3 p2) {
    const D3 u = {p1.x - p0.x, p1.y - p0.y, p1.z - p0.z}, v = {p2.x - p0.x, p2.y - p0.y, p2.z - p0.z};
    return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// K of the plane of a triangle: the ten products of (nx, ny, nz, d), each divided by s; false if s is 0 or not finite
__device__ __forceinline__ bool plane_quadric(D3 p0, D3 p1, D3 p2, double K[10]) {
    const D3 n = normal_of(p0, p1, p2);
    const double s = dot3(n, n);
    if (!(s > 0.0 && s <= 1.7976931348623157e308)) return false;
    const double e[4] = {n.x, n.y, n.z, -dot3(n, p0)};
    int k = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = i; j < 4; ++j) K[k++] = e[i] * e[j] / s;
    return true;
}

// E(x) = x^T A x + 2 b^T x + c; q = (A00, A01, A02, b0, A11, A12, b1, A22, b2, c)
__device__ __forceinline__ double quadric_error(const double q[10], D3 p) {
    const double t0 = (q[0] * p.x + q[1] * p.y) + q[2] * p.z;
    const double t1 = (q[1] * p.x + q[4] * p.y) + q[5] * p.z;
    const double t2 = (q[2] * p.x + q[5] * p.y) + q[7] * p.z;
    const double quad = (p.x * t0 + p.y * t1) + p.z * t2;
    const double lin = (q[3] * p.x + q[6] * p.y) + q[8] * p.z;
    return (quad + 2.0 * lin) + q[9];
}

__device__ __forceinline__ D3 round32(D3 p) { return {(double)(float)p.x, (double)(float)p.y, (double)(float)p.z}; }

// x* and E(x*): p_a, p_b, the midpoint, the optimum where Part 19 admits it - each a binary32 point; the smallest E,
// ties to the earlier.  false if every E is NaN.
__device__ __forceinline__ bool placement(const double q[10], D3 pa, D3 pb, D3 &best, double &best_e) {
    const D3 d = {pb.x - pa.x, pb.y - pa.y, pb.z - pa.z};
    const D3 mid = {(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
    D3 cand[4] = {pa, pb, round32(mid), pa};
    int n = 3;
    const double a00 = q[0], a01 = q[1], a02 = q[2], b0 = q[3], a11 = q[4], a12 = q[5], b1 = q[6], a22 = q[7], b2 = q[8];
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a02 * a12 - a01 * a22;
    const double c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double tr = ((a00 + a11) + a22) / 3.0;
    if (fabs(det) > 1e-3 * ((tr * tr) * tr) && det != 0.0) {
        const D3 o = {-((c00 * b0 + c01 * b1) + c02 * b2) / det, -((c01 * b0 + c11 * b1) + c12 * b2) / det,
                      -((c02 * b0 + c12 * b1) + c22 * b2) / det};
        const D3 w = {o.x - mid.x, o.y - mid.y, o.z - mid.z};
        if (dot3(w, w) <= dot3(d, d)) cand[n++] = round32(o);
    }
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double e = quadric_error(q, cand[i]);
        if (e == e && (!any || e < best_e)) {
            any = true;
            best = cand[i];
            best_e = e;
        }
    }
    return any;
}

__device__ __forceinline__ uint32_t edge_hash(uint32_t a, uint32_t b, uint32_t r) {
    return (((a * 2654435761u) ^ (b * 2246822519u) ^ (r * 3266489917u)) >> 7) & 0xFFFFFu;
}

// ------------------------------------------------------------------------------------------------ begin

__global__ void k_co_zero(Ws w, unsigned long long *__restrict__ counts) {
    if (threadIdx.x < 8) counts[threadIdx.x] = 0;
    if (threadIdx.x < sizeof(Ctrl) / 4) reinterpret_cast<uint32_t *>(w.ctrl)[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kBlock) void k_co_vertices(const float *__restrict__ vertices, uint32_t nv, Ws w,
                                                        unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    const bool in = v < nv;
    bool finite = true;
    if (in) {
        finite = finite3(vertices + (size_t)v * 3);
#pragma unroll
        for (int a = 0; a < 3; ++a) w.P[(size_t)v * 3 + a] = vertices[(size_t)v * 3 + a];
        w.rep[v] = (int32_t)v;
        w.cur[v] = 0;
    }
    wave_count(in && !finite, &counts[kNonFinite]);
}

// usable as in Part 16 (mi3d_incidence.h)
__global__ __launch_bounds__(kBlock) void k_co_usable(const float *__restrict__ vertices, uint32_t nv,
                                                      const int32_t *__restrict__ tri, uint32_t nt, Ws w) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool ok = false, planeless = false;
    if (t < nt) {
        int32_t c[3];
        ok = mi3d_incidence::usable(vertices, nv, tri, t, c);
        if (ok) {
            double K[10];
            planeless = !plane_quadric(widen(vertices + (size_t)c[0] * 3), widen(vertices + (size_t)c[1] * 3),
                                       widen(vertices + (size_t)c[2] * 3), K);
#pragma unroll
            for (int k = 0; k < 3; ++k) atomicAdd(w.cur + c[k], 1);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) w.tri[(size_t)t * 3 + k] = ok ? c[k] : -1;
        w.alive[t] = ok ? 1 : 0;
    }
    uint32_t total;
    block_scan<kWaves>(ok ? 1u : 0u, wave_sum, total);
    if (threadIdx.x == 0 && total != 0) atomicAdd(&w.ctrl->live, total);
    const unsigned long long m = __ballot(planeless);
    if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(&w.ctrl->planeless, (uint32_t)__popcll(m));
}

__global__ void k_co_begin_end(Ws w, uint32_t nt, unsigned long long *__restrict__ counts) {
    if (threadIdx.x != 0) return;
    w.ctrl->last_winners = 1;
    counts[kTriangles] = w.ctrl->live;
    counts[kUnusable] = (unsigned long long)(nt - w.ctrl->live) | ((unsigned long long)w.ctrl->planeless << 32);
}

// ------------------------------------------------------------------------------------------------ the incidence

__global__ __launch_bounds__(kBlock) void k_co_block_sums(uint32_t nv, Ws w, int always) {
    __shared__ uint32_t wave_sum[kWaves];
    if (!always && !w.ctrl->active) return;
    mi3d_incidence::block_sums(w.cur, nv, w.blockv, wave_sum);
}

__global__ __launch_bounds__(kRowThreads) void k_co_scan(Ws w, uint32_t nv, uint32_t nb, int always) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    if (!always && !w.ctrl->active) return;
    mi3d_incidence::scan_blocks(w.blockv, nb, w.offs, nv, wave_sum, &base);
}

__global__ __launch_bounds__(kBlock) void k_co_offsets(uint32_t nv, Ws w, int always) {
    __shared__ uint32_t wave_sum[kWaves];
    if (!always && !w.ctrl->active) return;
    mi3d_incidence::offsets(w.cur, nv, w.blockv, w.offs, wave_sum);
}

__global__ __launch_bounds__(kBlock) void k_co_fill(uint32_t nt, Ws w, int always, unsigned long long *__restrict__ counts) {
    if (!always && !w.ctrl->active) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t lost = 0;
    if (t < nt && w.alive[t]) {
#pragma unroll
        for (int k = 0; k < 3; ++k)  // lost: the state changed since the degrees were counted
            lost += mi3d_incidence::fill(w.cur, w.offs, (uint32_t)w.tri[(size_t)t * 3 + k],
                                         [&](size_t i) { w.rows[i] = 3u * t + (uint32_t)k; });
    }
    if (lost != 0) atomicAdd(&counts[kErrors], (unsigned long long)lost);  // never
}

// Q_v: the K of the usable triangles that cite v, summed in ascending triangle index from zero.  The row is sorted in
// place (insertion sort: the row belongs to this thread, rows are short).  A row longer than kMaxRow is not walked: its
// quadric is NaN, so no edge at v ever has a cost.
__global__ __launch_bounds__(kBlock) void k_co_quadrics(const float *__restrict__ vertices, uint32_t nv, Ws w) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const uint32_t begin = w.offs[v], deg = w.offs[v + 1] - begin;
    double Q[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) Q[k] = 0.0;
    if (deg > kMaxRow) {
#pragma unroll
        for (int k = 0; k < 10; ++k) Q[k] = __longlong_as_double(0x7FF8000000000000ll);
    } else {
        uint32_t *row = w.rows + begin;
        for (uint32_t i = 1; i < deg; ++i) {
            const uint32_t x = row[i];
            uint32_t j = i;
            for (; j > 0 && row[j - 1] > x; --j) row[j] = row[j - 1];
            row[j] = x;
        }
        for (uint32_t i = 0; i < deg; ++i) {
            const uint32_t t = row[i] / 3u;
            const int32_t *c = w.tri + (size_t)t * 3;
            double K[10];
            if (plane_quadric(widen(vertices + (size_t)c[0] * 3), widen(vertices + (size_t)c[1] * 3),
                              widen(vertices + (size_t)c[2] * 3), K)) {
#pragma unroll
                for (int k = 0; k < 10; ++k) Q[k] = Q[k] + K[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) w.Q[(size_t)v * 10 + k] = Q[k];
}

// ------------------------------------------------------------------------------------------------ a round

__global__ void k_co_round_begin(Ws w, unsigned long long target, unsigned long long *__restrict__ counts) {
    if (threadIdx.x != 0) return;
    Ctrl *c = w.ctrl;
    const bool active = (unsigned long long)c->live > target && c->last_winners != 0;
    c->active = active ? 1u : 0u;
    if (!active) return;
    c->quota = (uint32_t)(((unsigned long long)c->live - target + 1) / 2);
    c->winners = 0;
    c->live_next = 0;
    counts[kLocked] = 0;
}

__global__ __launch_bounds__(kBlock) void k_co_clear(uint32_t nv, Ws w, int always) {
    if (!always && !w.ctrl->active) return;
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    w.cur[v] = 0;
    w.claim[v] = kNone;
}

__global__ __launch_bounds__(kBlock) void k_co_degree(uint32_t nt, Ws w) {
    if (!w.ctrl->active) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt || !w.alive[t]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(w.cur + w.tri[(size_t)t * 3 + k], 1);
}

// the other two corners of every triangle in the row of v, which has deg <= kMaxDegree entries: nb[0 .. 2 deg)
__device__ __forceinline__ void gather(const Ws &w, uint32_t v, uint32_t deg, int32_t *nb) {
    const uint32_t *row = w.rows + w.offs[v];
    for (uint32_t r = 0; r < deg; ++r) {
        const uint32_t e = row[r], t = e / 3u, k = e - 3u * t;
        nb[2 * r] = w.tri[(size_t)t * 3 + (k + 1) % 3];
        nb[2 * r + 1] = w.tri[(size_t)t * 3 + (k + 2) % 3];
    }
}

__global__ __launch_bounds__(kBlock) void k_co_locks(uint32_t nv, Ws w, unsigned long long *__restrict__ counts) {
    if (!w.ctrl->active) return;
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    bool locked = false;
    if (v < nv) {
        const uint32_t deg = w.offs[v + 1] - w.offs[v];
        if (deg > kMaxDegree) {
            locked = true;
        } else if (deg != 0) {
            int32_t nb[2 * kMaxDegree];
            gather(w, v, deg, nb);
            const uint32_t n = 2 * deg;
            for (uint32_t i = 0; i < n && !locked; ++i) {
                uint32_t shared = 0;
                for (uint32_t j = 0; j < n; ++j) shared += nb[j] == nb[i] ? 1u : 0u;
                locked = shared == 1;  // one live triangle holds the edge: a border
            }
        }
        w.locked[v] = locked ? 1 : 0;
    }
    wave_count(locked, &counts[kLocked]);
}

__device__ __forceinline__ bool among(const int32_t *nb, uint32_t n, int32_t x) {
    bool found = false;
    for (uint32_t j = 0; j < n; ++j) found = found || nb[j] == x;
    return found;
}

// The triangles at `end` but t and u, with that corner at x: n_old . n_new > 0 and n_new . n_new > 0 for every one.
__device__ __forceinline__ bool keeps_orientation(const Ws &w, uint32_t end, uint32_t deg, uint32_t t, uint32_t u, D3 x) {
    const uint32_t *row = w.rows + w.offs[end];
    bool ok = true;
    for (uint32_t r = 0; r < deg; ++r) {
        const uint32_t e = row[r], f = e / 3u, k = e - 3u * f;
        if (f == t || f == u) continue;
        D3 p[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) p[j] = widen(w.P + (size_t)w.tri[(size_t)f * 3 + j] * 3);
        const D3 n_old = normal_of(p[0], p[1], p[2]);
        if (k == 0) p[0] = x;
        else if (k == 1) p[1] = x;
        else p[2] = x;
        const D3 n_new = normal_of(p[0], p[1], p[2]);
        ok = ok && dot3(n_old, n_new) > 0.0 && dot3(n_new, n_new) > 0.0;
    }
    return ok;
}

__global__ __launch_bounds__(kBlock) void k_co_candidates(uint32_t nt, Ws w, float max_error) {
    if (!w.ctrl->active) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= nt) return;
    const bool alive = w.alive[t] != 0;
    int32_t c[3] = {0, 0, 0};
    if (alive) {
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = w.tri[(size_t)t * 3 + k];
    }
    const uint32_t round = w.ctrl->round;
    for (int i = 0; i < 3; ++i) {
        unsigned long long key = kNone;
        const int32_t a = c[i], b = c[(i + 1) % 3], cc = c[(i + 2) % 3];
        if (alive && a < b && !w.locked[a] && !w.locked[b]) {
            const uint32_t dega = w.offs[a + 1] - w.offs[a], degb = w.offs[b + 1] - w.offs[b];  // both <= kMaxDegree
            int32_t na[2 * kMaxDegree], nb[2 * kMaxDegree];
            gather(w, (uint32_t)a, dega, na);
            gather(w, (uint32_t)b, degb, nb);
            // the live triangles that hold the edge: this one and exactly one more, which runs b -> a
            const uint32_t *row = w.rows + w.offs[a];
            uint32_t holders = 0, u = t;
            int32_t d = -1;
            bool opposite = false;
            for (uint32_t r = 0; r < dega; ++r) {
                if (na[2 * r] != b && na[2 * r + 1] != b) continue;
                ++holders;
                const uint32_t f = row[r] / 3u;
                if (f != t) {
                    u = f;
                    opposite = na[2 * r + 1] == b;
                    d = na[2 * r];
                }
            }
            bool ok = holders == 2 && opposite && d != cc;
            if (ok) {  // the link condition: no common neighbour but c and d
                for (uint32_t j = 0; j < 2 * dega; ++j) {
                    const int32_t y = na[j];
                    if (y != cc && y != d && among(nb, 2 * degb, y)) ok = false;
                }
            }
            ok = ok && dega + degb >= 7 && dega + degb - 4 <= kMaxDegree;
            ok = ok && w.offs[cc + 1] - w.offs[cc] >= 4 && w.offs[d + 1] - w.offs[d] >= 4;
            if (ok) {
                double q[10];
#pragma unroll
                for (int k = 0; k < 10; ++k) q[k] = w.Q[(size_t)a * 10 + k] + w.Q[(size_t)b * 10 + k];
                D3 x = {0.0, 0.0, 0.0};
                double e = 0.0;
                ok = placement(q, widen(w.P + (size_t)a * 3), widen(w.P + (size_t)b * 3), x, e);
                ok = ok && keeps_orientation(w, (uint32_t)a, dega, t, u, x) && keeps_orientation(w, (uint32_t)b, degb, t, u, x);
                const float c32 = (float)(e > 0.0 ? e : 0.0);
                if (ok && c32 <= max_error) {
                    const uint32_t hi = (__float_as_uint(c32) & 0xFFF00000u) | edge_hash((uint32_t)a, (uint32_t)b, round);
                    key = ((unsigned long long)hi << 32) | (unsigned long long)(3u * t + (uint32_t)i);
                    w.xstar[((size_t)t * 3 + i) * 3 + 0] = (float)x.x;
                    w.xstar[((size_t)t * 3 + i) * 3 + 1] = (float)x.y;
                    w.xstar[((size_t)t * 3 + i) * 3 + 2] = (float)x.z;
                    atomicMin(w.claim + a, key);
                    atomicMin(w.claim + b, key);
                }
            }
        }
        w.keys[(size_t)t * 3 + i] = key;
    }
}

// claim[v] >= key for every neighbour v of `end`
__device__ __forceinline__ bool unclaimed_around(const Ws &w, uint32_t end, unsigned long long key) {
    const uint32_t deg = w.offs[end + 1] - w.offs[end];  // <= kMaxDegree: the end is unlocked
    const uint32_t *row = w.rows + w.offs[end];
    bool ok = true;
    for (uint32_t r = 0; r < deg; ++r) {
        const uint32_t e = row[r], f = e / 3u, k = e - 3u * f;
        ok = ok && w.claim[w.tri[(size_t)f * 3 + (k + 1) % 3]] >= key && w.claim[w.tri[(size_t)f * 3 + (k + 2) % 3]] >= key;
    }
    return ok;
}

__global__ __launch_bounds__(kBlock) void k_co_winners(uint32_t nt, Ws w) {
    __shared__ uint32_t wave_sum[kWaves];
    if (!w.ctrl->active) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    uint32_t mask = 0;
    if (t < nt && w.alive[t]) {
        for (int i = 0; i < 3; ++i) {
            const unsigned long long key = w.keys[(size_t)t * 3 + i];
            if (key == kNone) continue;
            const uint32_t a = (uint32_t)w.tri[(size_t)t * 3 + i], b = (uint32_t)w.tri[(size_t)t * 3 + (i + 1) % 3];
            if (w.claim[a] == key && w.claim[b] == key && unclaimed_around(w, a, key) && unclaimed_around(w, b, key))
                mask |= 1u << i;
        }
    }
    if (t < nt) w.wins[t] = (uint8_t)mask;
    uint32_t total;
    block_scan<kWaves>((uint32_t)__popc(mask), wave_sum, total);
    if (threadIdx.x == 0) w.blockt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kRowThreads) void k_co_rank(Ws w, uint32_t nb) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    if (!w.ctrl->active) return;
    const uint32_t total = scan_row(w.blockt, nb, wave_sum, &base);
    if (threadIdx.x == 0) w.ctrl->winners = total;
}

__global__ __launch_bounds__(kBlock) void k_co_apply(uint32_t nt, Ws w) {
    __shared__ uint32_t wave_sum[kWaves];
    if (!w.ctrl->active || w.ctrl->winners == 0) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t mask = t < nt ? w.wins[t] : 0u;
    uint32_t total;
    uint32_t rank = w.blockt[blockIdx.x] + block_scan<kWaves>((uint32_t)__popc(mask), wave_sum, total);
    const uint32_t quota = w.ctrl->quota;
    for (int i = 0; i < 3; ++i) {
        if (!(mask >> i & 1u)) continue;
        if (rank++ >= quota) break;  // winners by ascending edge id 3 t + i
        const int32_t a = w.tri[(size_t)t * 3 + i], b = w.tri[(size_t)t * 3 + (i + 1) % 3];
        w.rep[b] = a;
#pragma unroll
        for (int k = 0; k < 3; ++k) w.P[(size_t)a * 3 + k] = w.xstar[((size_t)t * 3 + i) * 3 + k];
#pragma unroll
        for (int k = 0; k < 10; ++k) w.Q[(size_t)a * 10 + k] = w.Q[(size_t)a * 10 + k] + w.Q[(size_t)b * 10 + k];
    }
}

__global__ __launch_bounds__(kBlock) void k_co_rename(uint32_t nt, Ws w) {
    __shared__ uint32_t wave_sum[kWaves];
    if (!w.ctrl->active || w.ctrl->winners == 0) return;
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    bool alive = t < nt && w.alive[t];
    if (alive) {
        int32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = w.rep[w.tri[(size_t)t * 3 + k]];
            w.tri[(size_t)t * 3 + k] = c[k];
        }
        if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) {
            alive = false;
            w.alive[t] = 0;
        }
    }
    uint32_t total;
    block_scan<kWaves>(alive ? 1u : 0u, wave_sum, total);
    if (threadIdx.x == 0 && total != 0) atomicAdd(&w.ctrl->live_next, total);
}

// rep one hop up to date; thread 0 closes the books of the round (it touches no word another thread of this kernel reads)
__global__ __launch_bounds__(kBlock) void k_co_rep(uint32_t nv, Ws w, unsigned long long *__restrict__ counts) {
    Ctrl *c = w.ctrl;
    if (!c->active) return;
    const uint32_t winners = c->winners;
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (winners != 0 && v < nv) w.rep[v] = w.rep[w.rep[v]];
    if (v != 0) return;
    c->last_winners = winners;
    if (winners == 0) return;
    c->round += 1;
    c->live = c->live_next;
    counts[kTriangles] = c->live_next;
    counts[kRounds] += 1;
    counts[kCollapses] += winners < c->quota ? winners : c->quota;
}

// ------------------------------------------------------------------------------------------------ count and emit

// cur[v] = 1 for every vertex a live triangle cites (plain stores of one value); live triangles per workgroup
__global__ __launch_bounds__(kBlock) void k_co_cite(uint32_t nt, Ws w) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool alive = t < nt && w.alive[t];
    if (alive) {
#pragma unroll
        for (int k = 0; k < 3; ++k) w.cur[w.tri[(size_t)t * 3 + k]] = 1;
    }
    uint32_t total;
    block_scan<kWaves>(alive ? 1u : 0u, wave_sum, total);
    if (threadIdx.x == 0) w.blockt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kRowThreads) void k_co_totals(Ws w, uint32_t nv, uint32_t nbt,
                                                           unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kRowWaves];
    __shared__ uint32_t base;
    const uint32_t total = scan_row(w.blockt, nbt, wave_sum, &base);
    if (threadIdx.x == 0) {
        counts[kTriangles] = total;
        counts[kVertices] = w.offs[nv];
    }
}

__global__ __launch_bounds__(kBlock) void k_co_emit_vertices(uint32_t nv, Ws w, float *__restrict__ out_vertices,
                                                             unsigned long long nv_cap, int32_t *__restrict__ vertex_map,
                                                             unsigned long long *__restrict__ counts) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    bool lost = false;
    if (v < nv) {
        const uint32_t id = w.offs[v];
        if (w.offs[v + 1] != id) {
            if (id < nv_cap) {
#pragma unroll
                for (int a = 0; a < 3; ++a) out_vertices[(size_t)id * 3 + a] = w.P[(size_t)v * 3 + a];
            } else {
                lost = true;
            }
        }
        const uint32_t r = (uint32_t)w.rep[v];
        vertex_map[v] = w.offs[r + 1] != w.offs[r] ? (int32_t)w.offs[r] : -1;
    }
    wave_count(lost, &counts[kErrors]);
}

__global__ __launch_bounds__(kBlock) void k_co_emit_triangles(uint32_t nt, Ws w, int32_t *__restrict__ out_triangles,
                                                              unsigned long long nt_cap,
                                                              unsigned long long *__restrict__ counts) {
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const bool alive = t < nt && w.alive[t];
    uint32_t total;
    const uint32_t rank = w.blockt[blockIdx.x] + block_scan<kWaves>(alive ? 1u : 0u, wave_sum, total);
    const bool lost = alive && rank >= nt_cap;
    if (alive && !lost) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_triangles[(size_t)rank * 3 + k] = (int32_t)w.offs[w.tri[(size_t)t * 3 + k]];
    }
    wave_count(lost, &counts[kErrors]);
}

void launch_incidence(const Ws &w, uint32_t n, uint32_t m, int always, unsigned long long *counts, hipStream_t st) {
    const uint32_t nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    hipLaunchKernelGGL(k_co_block_sums, dim3(nb), dim3(kBlock), 0, st, n, w, always);
    hipLaunchKernelGGL(k_co_scan, dim3(1), dim3(kRowThreads), 0, st, w, n, nb, always);
    hipLaunchKernelGGL(k_co_offsets, dim3(nb), dim3(kBlock), 0, st, n, w, always);
    hipLaunchKernelGGL(k_co_fill, dim3(nbt), dim3(kBlock), 0, st, m, w, always, counts);
}

}  // namespace

extern "C" {

size_t mi3d_mesh_collapse_workspace(unsigned long long nv, unsigned long long nt) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles) || (nv == 0 && nt == 0)) return 0;
    return ws_bytes_of(nv, nt);
}

int mi3d_mesh_collapse_begin(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             void *ws, size_t ws_bytes, unsigned long long *counts, void *stream) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, ws_bytes_of(nv, nt), counts) || (nv > 0 && vertices == nullptr) || (nt > 0 && triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt, nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const Ws w = at(ws, collapse_layout, n, m);
    hipLaunchKernelGGL(k_co_zero, dim3(1), dim3(64), 0, st, w, counts);
    if (n) hipLaunchKernelGGL(k_co_vertices, dim3(nb), dim3(kBlock), 0, st, vertices, n, w, counts);
    if (m) hipLaunchKernelGGL(k_co_usable, dim3(nbt), dim3(kBlock), 0, st, vertices, n, triangles, m, w);
    if (n && m) {
        launch_incidence(w, n, m, 1, counts, st);
        hipLaunchKernelGGL(k_co_quadrics, dim3(nb), dim3(kBlock), 0, st, vertices, n, w);
    }
    hipLaunchKernelGGL(k_co_begin_end, dim3(1), dim3(64), 0, st, w, m, counts);
    return (int)hipGetLastError();
}

int mi3d_mesh_collapse_rounds(unsigned long long nv, unsigned long long nt, unsigned long long target_faces,
                              float max_error, uint32_t n_rounds, void *ws, size_t ws_bytes, unsigned long long *counts,
                              void *stream) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles) || !(max_error >= 0.f) || n_rounds > kMaxRounds) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, ws_bytes_of(nv, nt), counts)) return (int)hipErrorInvalidValue;
    if (nv == 0 || nt == 0) return (int)hipSuccess;  // no live triangle: every round is a no-op
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt, nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const Ws w = at(ws, collapse_layout, n, m);
    for (uint32_t r = 0; r < n_rounds; ++r) {
        hipLaunchKernelGGL(k_co_round_begin, dim3(1), dim3(64), 0, st, w, target_faces, counts);
        hipLaunchKernelGGL(k_co_clear, dim3(nb), dim3(kBlock), 0, st, n, w, 0);
        hipLaunchKernelGGL(k_co_degree, dim3(nbt), dim3(kBlock), 0, st, m, w);
        launch_incidence(w, n, m, 0, counts, st);
        hipLaunchKernelGGL(k_co_locks, dim3(nb), dim3(kBlock), 0, st, n, w, counts);
        hipLaunchKernelGGL(k_co_candidates, dim3(nbt), dim3(kBlock), 0, st, m, w, max_error);
        hipLaunchKernelGGL(k_co_winners, dim3(nbt), dim3(kBlock), 0, st, m, w);
        hipLaunchKernelGGL(k_co_rank, dim3(1), dim3(kRowThreads), 0, st, w, nbt);
        hipLaunchKernelGGL(k_co_apply, dim3(nbt), dim3(kBlock), 0, st, m, w);
        hipLaunchKernelGGL(k_co_rename, dim3(nbt), dim3(kBlock), 0, st, m, w);
        hipLaunchKernelGGL(k_co_rep, dim3(nb), dim3(kBlock), 0, st, n, w, counts);
    }
    return (int)hipGetLastError();
}

int mi3d_mesh_collapse_count(unsigned long long nv, unsigned long long nt, void *ws, size_t ws_bytes,
                             unsigned long long *counts, void *stream) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, ws_bytes_of(nv, nt), counts)) return (int)hipErrorInvalidValue;
    if (nv == 0 || nt == 0) return (int)hipSuccess;  // counts[0] and [1] are the zeros of begin
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt, nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const Ws w = at(ws, collapse_layout, n, m);
    hipLaunchKernelGGL(k_co_clear, dim3(nb), dim3(kBlock), 0, st, n, w, 1);
    hipLaunchKernelGGL(k_co_cite, dim3(nbt), dim3(kBlock), 0, st, m, w);
    hipLaunchKernelGGL(k_co_block_sums, dim3(nb), dim3(kBlock), 0, st, n, w, 1);
    hipLaunchKernelGGL(k_co_scan, dim3(1), dim3(kRowThreads), 0, st, w, n, nb, 1);
    hipLaunchKernelGGL(k_co_offsets, dim3(nb), dim3(kBlock), 0, st, n, w, 1);
    hipLaunchKernelGGL(k_co_totals, dim3(1), dim3(kRowThreads), 0, st, w, n, nbt, counts);
    return (int)hipGetLastError();
}

int mi3d_mesh_collapse_emit(unsigned long long nv, unsigned long long nt, void *ws, size_t ws_bytes, float *out_vertices,
                            unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap,
                            int32_t *vertex_map, unsigned long long *counts, void *stream) {
    if (!sizes_ok(nv, nt, kMaxVertices, kMaxTriangles)) return (int)hipErrorInvalidValue;
    if (nv == 0 && nt == 0) return (int)hipSuccess;
    if (!state_ok(ws, ws_bytes, ws_bytes_of(nv, nt), counts) || (nv > 0 && vertex_map == nullptr) ||
        (nv_cap > 0 && out_vertices == nullptr) || (nt_cap > 0 && out_triangles == nullptr))
        return (int)hipErrorInvalidValue;
    const uint32_t n = (uint32_t)nv, m = (uint32_t)nt, nb = blocks_of(n, kBlock), nbt = blocks_of(m, kBlock);
    const hipStream_t st = as_stream(stream);
    const Ws w = at(ws, collapse_layout, n, m);
    if (n && m) {
        hipLaunchKernelGGL(k_co_emit_vertices, dim3(nb), dim3(kBlock), 0, st, n, w, out_vertices, nv_cap, vertex_map, counts);
        hipLaunchKernelGGL(k_co_emit_triangles, dim3(nbt), dim3(kBlock), 0, st, m, w, out_triangles, nt_cap, counts);
    } else if (n) {
        (void)hipMemsetAsync(vertex_map, 0xFF, (size_t)n * 4, st);  // nt == 0: nothing is cited, every entry -1
    }
    return (int)hipGetLastError();
}

}  // extern "C"
