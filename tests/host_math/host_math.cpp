// Test helper (NOT product code): compiles make-it-3d_amd/csrc/mi3d_common.h - the exact scalar
// math the HIP kernels use - and csrc/mi3d_grid_plan.h - the hash grid's host-side planners - for the
// HOST, so tests can compare them bit-for-bit with the oracle and with libmi3d.so's own plan queries
// without a GPU.  Built by tests/test_host_math.py with g++ -ffp-contract=off.
#include <cstdint>
#include <cstring>
#include "mi3d_common.h"
#include "mi3d_grid_plan.h"
using namespace mi3d;

extern "C" {

// sequential emulation of k_march_train (slabs in ray order)
void hm_march_train(const float* rays_o, const float* rays_d, const uint8_t* bits, float bound, float dt_gamma,
                    uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M, const float* nears,
                    const float* fars, float* xyzs, float* dirs, float* deltas, int32_t* rays, int32_t* counter,
                    const float* noises) {
    MarchGrid g; march_grid_init(g, bits, bound, dt_gamma, max_steps, C, H);
    uint32_t total = 0;
    for (uint32_t n = 0; n < N; n++) {
        MarchRay r; march_ray_init(r, rays_o + n * 3, rays_d + n * 3);
        const float far = fars[n], t0 = march_t0(nears[n], noises[n], g);
        uint32_t count = 0; float t = t0, x, y, z, dt;
        while (t < far && count < max_steps) if (march_step(r, g, t, x, y, z, dt)) ++count;
        const uint32_t offset = total; total += count;
        rays[n * 3] = n; rays[n * 3 + 1] = offset; rays[n * 3 + 2] = count;
        if (count == 0 || offset + count > M) continue;
        float *px = xyzs + (size_t)offset * 3, *pd = dirs + (size_t)offset * 3, *pl = deltas + (size_t)offset * 2;
        t = t0; float last_t = t0; uint32_t step = 0;
        while (t < far && step < count) {
            if (march_step(r, g, t, x, y, z, dt)) {
                px[0] = x; px[1] = y; px[2] = z; pd[0] = r.dx; pd[1] = r.dy; pd[2] = r.dz;
                pl[0] = dt; pl[1] = t - last_t; last_t = t; px += 3; pd += 3; pl += 2; ++step;
            }
        }
    }
    counter[0] += total; counter[1] += N;
}

void hm_morton(const int32_t* c, uint32_t N, int32_t* out) {
    for (uint32_t n = 0; n < N; n++) out[n] = (int32_t)morton3d(c[n*3], c[n*3+1], c[n*3+2]);
}
void hm_morton_invert(const int32_t* in, uint32_t N, int32_t* c) {
    for (uint32_t n = 0; n < N; n++) { int32_t v = in[n];
        c[n*3] = compact_bits((uint32_t)(v >> 0)); c[n*3+1] = compact_bits((uint32_t)(v >> 1)); c[n*3+2] = compact_bits((uint32_t)(v >> 2)); }
}

// hash-grid corner indices / weights for one level, given the host-built level record
void hm_grid_corners(const float* x, uint32_t n, float scale, uint32_t res, uint32_t offset, uint32_t size,
                     uint32_t hashed, uint32_t dims, uint32_t* idx, float* w) {
    GridLevel L{scale, res, offset, size, hashed, dims};
    for (uint32_t i = 0; i < n; i++) {
        uint32_t c[3]; float f[3];
        for (int d = 0; d < 3; d++) grid_cell(x[i*3+d], scale, c[d], f[d]);
        for (uint32_t k = 0; k < 8; k++) {
            float wk = 1.f; uint32_t q[3];
            for (uint32_t d = 0; d < 3; d++) {
                if (k & (1u << d)) { wk *= f[d]; q[d] = c[d] + 1; } else { wk *= 1 - f[d]; q[d] = c[d]; }
            }
            idx[i*8+k] = grid_entry(L, q[0], q[1], q[2]); w[i*8+k] = wk;
        }
    }
}

// the scatter's 12-byte pair record: pack, unpack, and the x-pair rule on a hashed level of `size` (a power of two) entries
void hm_row12_roundtrip(const uint32_t* e_local, const uint32_t* t, const float* w, const float* fx, const uint32_t* raw,
                        uint32_t n, uint32_t* words, uint32_t* e_out, uint32_t* t_out, float* w_out, float* fx_out) {
    for (uint32_t i = 0; i < n; i++) {
        const Row12 r = pack_row12(e_local[i], t[i], w[i], fx[i], raw[i]);
        words[i*3] = r.w0; words[i*3+1] = r.w1; words[i*3+2] = r.w2;
        unpack_row12_fields(r.w0, r.w2, e_out[i], t_out[i], w_out[i], fx_out[i]);
    }
}
void hm_pair_rule(const uint32_t* cell, uint32_t n, uint32_t size, uint32_t* e0, uint32_t* e1, uint32_t* e1_from_rule) {
    GridLevel L{1.0f, 0u, 0u, size, 1u, 3u};
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cx = cell[i*3], cy = cell[i*3+1], cz = cell[i*3+2];
        e0[i] = grid_entry(L, cx, cy, cz);
        e1[i] = grid_entry(L, cx + 1, cy, cz);
        const uint32_t t = pair_flip_t(cx);
        e1_from_rule[i] = e0[i] ^ (((t >= 32 ? 0xFFFFFFFFu : (1u << t) - 1u)) & (size - 1u));
    }
}
// the scatter emit's pure arithmetic (csrc/mi3d_common.h): the 1.5 * 2^52 rounding, the gather table's power-of-two scale and
// slot hash, the trilinear corner weights, and the face pass's corner maps
void hm_fixed_point(const float* x, uint32_t n, int64_t* out) {
    for (uint32_t i = 0; i < n; i++) out[i] = (int64_t)fixed_point(x[i]);
}
void hm_gather_scale(const float* tmax, uint32_t n, float* scale, double* unscale) {
    for (uint32_t i = 0; i < n; i++) { const GatherScale g = gather_scale(tmax[i]); scale[i] = g.scale; unscale[i] = g.unscale; }
}
void hm_merge_slot(const uint32_t* e, uint32_t n, uint32_t* slot) {
    for (uint32_t i = 0; i < n; i++) slot[i] = merge_slot(e[i]);
}
void hm_corner_weights(const float* f, uint32_t n, float* w) {
    for (uint32_t i = 0; i < n; i++) {
        float wk[8]; corner_weights(f[i*3], f[i*3+1], f[i*3+2], wk);
        for (int k = 0; k < 8; k++) w[i*8+k] = wk[k];
    }
}
// for every axis and far corner j: k1, k0, and the corner's lattice coordinates for the + and the - neighbour of cell `base`
void hm_face_maps(const uint32_t* base, uint32_t* k1, uint32_t* k0, uint32_t* far_plus, uint32_t* far_minus) {
    for (uint32_t axis = 0; axis < 3; axis++)
        for (uint32_t j = 0; j < 4; j++) {
            k1[axis*4+j] = face_k1(axis, j); k0[axis*4+j] = face_k0(axis, j);
            for (uint32_t d = 0; d < 3; d++) {
                far_plus[(axis*4+j)*3+d] = face_far_coord(axis, j, d, base[d], base[axis] + 2u);
                far_minus[(axis*4+j)*3+d] = face_far_coord(axis, j, d, base[d], base[axis] - 1u);
            }
        }
}
// the MLP backward's tile transposition through LDS: the three byte offsets of a lane (csrc/mi3d_common.h)
void hm_tr_offsets(uint32_t* wr_d, uint32_t* wr_x, uint32_t* rd, int32_t* row_bytes) {
    for (int lane = 0; lane < 64; lane++) {
        wr_d[lane] = tr_write_offset_d(lane); wr_x[lane] = tr_write_offset_x(lane); rd[lane] = tr_read_offset(lane);
    }
    *row_bytes = kTrRowBytes;
}

// the hash grid's planners (csrc/mi3d_grid_plan.h) built for the host: the signatures and output layouts of
// mi3d_grid_encode_plan / mi3d_grid_scatter_plan (include/mi3d.h), 1 for an invalid argument
int hm_grid_encode_plan(uint32_t n, float bound, float step, uint32_t n_levels, uint32_t base_resolution,
                        float per_level_scale, uint32_t log2_hashmap_size, uint32_t* n_segments, uint32_t* segments) {
    if (!valid_levels(n_levels) || n_segments == nullptr || segments == nullptr) return 1;
    GridTable T;
    build_grid_table(T, n_levels, base_resolution, per_level_scale, log2_hashmap_size);
    uint32_t n_lds = lds_levels(T, nullptr);
    if (n_lds == T.n_levels) n_lds = 0;   // the query's rule: with every level in LDS it reports them in the XCD plan
    const EncodePlan plan = plan_encode(T, n, step01_of(step, bound), n_lds, 0, -1, true).plan;
    for (uint32_t x = 0; x < kXcds; x++) {
        n_segments[x] = plan.n_seg[x];
        for (uint32_t i = 0; i < (uint32_t)kMaxSegs; i++) {
            const EncodeSeg sg = i < plan.n_seg[x] ? plan.seg[x][i] : EncodeSeg{0u, 0u, 0u, 0u};
            uint32_t* o = segments + (x * kMaxSegs + i) * 3;
            o[0] = sg.level; o[1] = sg.tile0; o[2] = sg.tile1;
        }
    }
    return 0;
}
int hm_grid_scatter_plan(uint32_t n, uint32_t P, float bound, float step, uint32_t n_levels, uint32_t base_resolution,
                         float per_level_scale, uint32_t log2_hashmap_size, size_t workspace_bytes,
                         unsigned long long* out) {
    if (!valid_levels(n_levels) || !valid_stencil(P, P, nullptr) || n == 0 || out == nullptr) return 1;
    GridTable T;
    build_grid_table(T, n_levels, base_resolution, per_level_scale, log2_hashmap_size);
    ScatterPlan sp = plan_scatter(T, n, P, bound, step, false, workspace_bytes);
    BinPlan& p = sp.plan;
    plan_reduce_splits(p, T, reduce_base_split(sp.n_slice * P), sp.merge_levels);
    out[0] = sp.n_slice; out[1] = bin_workspace_bytes(p); out[2] = sp.merge_levels; out[3] = p.n_reduce_wgs;
    out[4] = p.total_bytes; out[5] = p.total_counts;
    for (uint32_t l = 0; l < n_levels; l++) {
        unsigned long long* o = out + 6 + 7 * l;
        o[0] = level_bins(T.level[l]); o[1] = p.level_cap[l]; o[2] = p.level_waves[l]; o[3] = (p.row_mask >> l) & 1u;
        o[4] = p.level_split[l]; o[5] = p.level_wg0[l]; o[6] = p.level_cnt0[l];
    }
    return 0;
}
}
