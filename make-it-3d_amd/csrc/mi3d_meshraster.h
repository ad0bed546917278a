// Device helpers shared by the two rasterisers of the exported mesh: textureviews.hip (include/mi3d.h Part 15: the depth
// maps) and meshrender.hip (Part 17: the visibility buffer and its shading).  The header of Part 15 states the
// arithmetic operation by operation; both translation units are compiled with -ffp-contract=off, so that the one
// definition here gives the same bits in both and a NumPy float32 restatement gives them too.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mi3d_meshraster {

constexpr int kView = 24;  // floats per view record: R[3][3], t[3], K[3][3], centre[3]
constexpr uint32_t kMinSide = 2, kMaxSide = 16384, kMaxViews = 64;

inline bool views_ok(uint32_t V, uint32_t H, uint32_t W) {
    return V >= 1 && V <= kMaxViews && H >= kMinSide && H <= kMaxSide && W >= kMinSide && W <= kMaxSide;
}

struct Projected {
    float x, y, z;
};

// cam = R p + t, q = K cam, sums in index order; x = q0 / q2, y = q1 / q2, z = q2
__device__ __forceinline__ Projected project(const float *__restrict__ view, float p0, float p1, float p2) {
    float cam[3], q[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) cam[r] = ((view[3 * r] * p0 + view[3 * r + 1] * p1) + view[3 * r + 2] * p2) + view[9 + r];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (view[12 + 3 * r] * cam[0] + view[12 + 3 * r + 1] * cam[1]) + view[12 + 3 * r + 2] * cam[2];
    Projected o;
    o.x = q[0] / q[2];
    o.y = q[1] / q[2];
    o.z = q[2];
    return o;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }  // false for NaN

// the edge function of the directed edge a -> b at (px, py), evaluated on the endpoints in ascending vertex-index order
// and negated for the other direction: two triangles that share an edge by index see exactly opposite values
__device__ __forceinline__ float edge_fn(int32_t ia, const Projected &a, int32_t ib, const Projected &b, float px, float py) {
    const bool fwd = ia <= ib;
    const Projected &lo = fwd ? a : b, &hi = fwd ? b : a;
    const float e = (hi.x - lo.x) * (py - lo.y) - (hi.y - lo.y) * (px - lo.x);
    return fwd ? e : -e;
}

// the three indices of triangle i; false (nothing of `vertices` may be read) if one lies outside [0, nv)
__device__ __forceinline__ bool load_triangle(const int32_t *__restrict__ triangles, uint32_t i, uint32_t nv, int32_t id[3]) {
    const int32_t *t = triangles + (size_t)i * 3;
    id[0] = t[0];
    id[1] = t[1];
    id[2] = t[2];
    return (uint32_t)id[0] < nv && (uint32_t)id[1] < nv && (uint32_t)id[2] < nv;
}

// the triangle's corners in one view; false if a corner has z <= 0 or a non-finite x, y or z (not drawn in that view)
__device__ __forceinline__ bool project_triangle(const float *__restrict__ vertices, const int32_t id[3],
                                                 const float *__restrict__ view, Projected P[3]) {
    bool drawn = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *p = vertices + (size_t)id[k] * 3;
        P[k] = project(view, p[0], p[1], p[2]);
        drawn = drawn && P[k].z > 0.0f && finite_f(P[k].z) && finite_f(P[k].x) && finite_f(P[k].y);
    }
    return drawn;
}

// w0, w1, w2 = the edges 1 -> 2, 2 -> 0, 0 -> 1 at the centre (px, py); s = (w0 + w1) + w2
struct Weights {
    float w0, w1, w2, s;
};

__device__ __forceinline__ Weights edge_weights(const int32_t id[3], const Projected P[3], float px, float py) {
    Weights e;
    e.w0 = edge_fn(id[1], P[1], id[2], P[2], px, py);
    e.w1 = edge_fn(id[2], P[2], id[0], P[0], px, py);
    e.w2 = edge_fn(id[0], P[0], id[1], P[1], px, py);
    e.s = (e.w0 + e.w1) + e.w2;
    return e;
}

// covered iff (all w >= 0 or all w <= 0) and s != 0 (s == 0 or NaN: no area)
__device__ __forceinline__ bool covers(const Weights &e) {
    const bool covered = (e.w0 >= 0.0f && e.w1 >= 0.0f && e.w2 >= 0.0f) || (e.w0 <= 0.0f && e.w1 <= 0.0f && e.w2 <= 0.0f);
    return covered && e.s != 0.0f;
}

// r_k = (w_k / s) / z_k, the terms of the perspective-correct depth d = 1 / ((r0 + r1) + r2)
__device__ __forceinline__ float depth_terms(const Weights &e, const Projected P[3], float r[3]) {
    r[0] = (e.w0 / e.s) / P[0].z;
    r[1] = (e.w1 / e.s) / P[1].z;
    r[2] = (e.w2 / e.s) / P[2].z;
    return 1.0f / ((r[0] + r[1]) + r[2]);
}

// What one thread = (triangle i, view v) of a depth-style pass does: the index check and the two counters of
// mi3d_mesh_depth, the projection, the walk over the pixel centres of the clipped bounding box, the coverage test and
// the depth; emit(pixel offset in the view, d) is called for every pixel the depth map writes, with 0 < d < inf.
template <class Emit>
__device__ __forceinline__ void raster_triangle(const float *__restrict__ vertices, uint32_t nv,
                                                const int32_t *__restrict__ triangles, uint32_t i, uint32_t v,
                                                const float *__restrict__ views, uint32_t H, uint32_t W,
                                                unsigned long long *__restrict__ counts, Emit emit) {
    int32_t id[3];
    if (!load_triangle(triangles, i, nv, id)) {
        if (v == 0) atomicAdd(counts, 1ull);  // a bad triangle is counted once, not once per view
        return;
    }
    Projected P[3];
    if (!project_triangle(vertices, id, views + (size_t)v * kView, P)) {
        atomicAdd(counts + 1, 1ull);
        return;
    }
    // pixel (i, j) has its centre at (i + 0.5, j + 0.5): the centres inside the bounding box, clipped to the image
    const float xlo = fmaxf(ceilf(fminf(fminf(P[0].x, P[1].x), P[2].x) - 0.5f), 0.0f);
    const float xhi = fminf(floorf(fmaxf(fmaxf(P[0].x, P[1].x), P[2].x) - 0.5f), (float)(W - 1));
    const float ylo = fmaxf(ceilf(fminf(fminf(P[0].y, P[1].y), P[2].y) - 0.5f), 0.0f);
    const float yhi = fminf(floorf(fmaxf(fmaxf(P[0].y, P[1].y), P[2].y) - 0.5f), (float)(H - 1));
    if (!(xlo <= xhi && ylo <= yhi)) return;
    const uint32_t i0 = (uint32_t)xlo, i1 = (uint32_t)xhi, j0 = (uint32_t)ylo, j1 = (uint32_t)yhi;  // within [0, W) x [0, H)
    for (uint32_t j = j0; j <= j1; ++j) {         // at most H * W iterations in all: the box lies in the image
        const float py = (float)j + 0.5f;
        for (uint32_t ii = i0; ii <= i1; ++ii) {
            const float px = (float)ii + 0.5f;
            const Weights e = edge_weights(id, P, px, py);
            if (!covers(e)) continue;
            float r[3];
            const float d = depth_terms(e, P, r);
            if (!(d > 0.0f) || !finite_f(d)) continue;
            emit((size_t)j * W + ii, d);
        }
    }
}

}  // namespace mi3d_meshraster
