// Multiresolution hash-grid building blocks shared by hashgrid.hip (stand-alone tcnn.Encoding
// replacement) and field.hip (fused field).  Algorithm provenance: oracle/hashgrid_ref.c.
// The level table, the kernels' by-value structs and the host-side planners are in mi3d_grid_plan.h (no HIP header:
// it also builds with plain g++); this file adds the device-only parts.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mi3d.h"
#include "mi3d_common.h"
#include "mi3d_grid_plan.h"

namespace mi3d {

// The 8 lattice corners of one point at one level: entry indices (relative to the level) and weights.
// Corner k: bit0 -> +x, bit1 -> +y, bit2 -> +z (the order tcnn accumulates in).
struct Corners {
    uint32_t idx[8];
    float w[8];
};

__device__ __forceinline__ void grid_corners(const GridLevel &L, float x, float y, float z, Corners &c) {
    uint32_t cx, cy, cz;
    float fx, fy, fz;
    grid_cell(x, L.scale, cx, fx);
    grid_cell(y, L.scale, cy, fy);
    grid_cell(z, L.scale, cz, fz);
    corner_weights(fx, fy, fz, c.w);
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        c.idx[k] = grid_entry(L, cx + (k & 1u), cy + ((k >> 1) & 1u), cz + ((k >> 2) & 1u));
}

// ---------------------------------------------------------------------------------------------
// Run merging in the scatter kernels.
//
// Neighbouring lanes hold neighbouring samples of one ray, so at the coarse and middle levels long runs of lanes
// fall into the SAME lattice cell and would send their corner values to the same addresses (measured: 206 ms for one
// 10.9 M-sample backward without merging).  The kernels in hashgrid.hip group lanes into runs of equal cell key and
// sum each run before it leaves the wave - by a segmented scan across quads (k_scatter) or through an LDS slab
// (k_scatter_runs, k_bin_emit).  Any partition into equal-key runs is valid, so inactive lanes simply break runs.
struct CellKey {
    uint32_t a, b, c;  // lattice cell (cx, cy, cz)
};
__device__ __forceinline__ bool operator==(const CellKey &p, const CellKey &q) {
    return p.a == q.a && p.b == q.b && p.c == q.c;
}

}  // namespace mi3d
