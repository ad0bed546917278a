// Development tunables.  The product library (make-it-3d_amd/build.py) is compiled WITHOUT MI3D_DEV: every
// MI3D_TUNE(i, dflt) is then the literal default and nothing in libmi3d.so reads the environment or carries a
// debug path.  tools/build_dev.py compiles the same sources with -DMI3D_DEV into tools/bin/libmi3d_dev.so, whose
// extra entry point mi3d_dev_set(index, value) lets the kernel micro-benchmarks under tools/ A/B launch
// geometries and kernel variants on the GPU box in one call.
#pragma once

#ifdef MI3D_DEV
extern "C" int mi3d_dev_tunable[32];
#define MI3D_TUNE(i, dflt) (mi3d_dev_tunable[(i)] >= 0 ? mi3d_dev_tunable[(i)] : (int)(dflt))
#else
#define MI3D_TUNE(i, dflt) ((int)(dflt))
#endif

// indices (the tools use the literal numbers: a retired index is not reused)
enum : int {
    MI3D_T_ENCODE_VARIANT = 0,     // gather: bit 0 = 16-byte pair loads, bit 1 (with bit 0) = non-temporal plane stores
    MI3D_T_ENCODE_WGS_PER_CU = 1,  // gather: workgroups per CU on the fine segments
    MI3D_T_ENCODE_ONLY_LEVEL = 2,  // gather: >= 0: the plan holds this level alone (per-level timing)
    MI3D_T_EMIT_FINE_WAVES = 3,    // scatter: emitting waves of the fine (x-pair record) role
    MI3D_T_EMIT_COARSE_WAVES = 4,  // scatter: emitting waves of the coarse (gathered per tile) role
    MI3D_T_SCATTER_LEVEL_MASK = 5, // scatter: bit l = level l is emitted (per-role / per-level timing; the reduce still
                                   //          walks every level's stale counters: a constant)
    // 6: retired (MLP: round 2's kernels)
    MI3D_T_MLP_WGS_PER_CU = 7,     // MLP backward: workgroups per CU
    MI3D_T_SCATTER_MERGE = 8,      // atomic scatter (fallback path): levels that run-merge
    MI3D_T_REPLICAS = 9,           // atomic scatter (fallback path): private table copies
    // 10: retired (scatter emit: order and timing bits)
    MI3D_T_MLP_FWD_WGS_PER_CU = 11,       // MLP forward: workgroups per CU
    MI3D_T_ENCODE_COARSE_WGS_PER_CU = 12, // gather: workgroups per CU on the coarse segments
    MI3D_T_MARCH_RPW_MIN = 13,     // march: smallest rays per wave the launch may choose
    MI3D_T_MARCH_WAVES = 14,       // march: persistent waves
    MI3D_T_MERGE_STEPS_X10 = 15,   // scatter: a level is gathered per tile (coarse role) if its cells are >= this / 10.5
                                   //          marching steps long (product: 42 -> levels 0-6 at C2)
    MI3D_T_ENCODE_LDS_LEVELS = 16, // gather: levels served from LDS (default: as many as fit)
    MI3D_T_ENCODE_STATIC_TILES = 17,  // gather: 1 = tiles dealt statically (round 2's order) instead of claimed
    // 18: retired (gather: the x-group evaluation of the fine hashed levels)
    MI3D_T_SHADE_BACKWARD_LAUNCHES = 19,  // mesh shade backward: bit 0 = the fill and k_grad_amax, bit 1 = k_shade_backward,
                                          //          bit 2 = k_grad_finish (per-launch timing; product: 7, all of them)
};
