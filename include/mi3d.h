/*
 * mi3d.h - C ABI of libmi3d.so, the MI355X (gfx950) implementation of Make-It-3D's coarse-stage
 * SDS hot path.  Plain pointers and sizes only; every pointer is a DEVICE pointer unless the
 * parameter name ends in `_host`.  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Every entry point enqueues work on `stream` and returns the hipError_t of the launch
 * as int (0 = hipSuccess); nothing here allocates, frees or synchronises.
 *
 * Part 1 replaces, one for one, the 13 functions of the reference's `_raymarching` backend
 * (/root/reference/raymarching/src/raymarching.h:7-22, bound in bindings.cpp:5-23): same argument
 * order and meaning, `at::Tensor` -> raw pointer, plus the trailing stream.  Caller allocates all
 * outputs (as raymarching/raymarching.py does).
 *
 * Part 2 replaces the tiny-cuda-nn `Encoding` (HashGrid) forward/backward the reference calls at
 * /root/reference/nerf/network_tcnn.py:54-65,107.
 *
 * Part 3 evaluates / back-propagates the encoder for the whole 13-point stencil the reference visits with
 * 13 separate encoder passes per sample (network_tcnn.py:115-128, nerf/renderer.py:521-524).
 *
 * Part 4 replaces the three nn.Linear + two ReLU launches of the reference's `sigma_net`
 * (network_tcnn.py:13-32,67, called at :107) by one matrix-core kernel per direction.
 */
#ifndef MI3D_H
#define MI3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI3D_MAX_LEVELS 16
#define MI3D_MAX_POINTS 16

/* the ABI version: 5 (4 = 3 + the compact-round inference loop of Part 1b; 5: that loop's ctl block is int32[16] with
 * the dropped-row count in [8], and its plan never passes max_steps; every other entry point is unchanged).  Part 8
 * (marching cubes), Part 9 (texture baking), Part 10 (GroupNorm), Part 12 (the Canny detector), Part 1's
 * mi3d_composite_rays_train_backward_depth and mi3d_march_train_plan and the hash grid's input gradients (mi3d_hashgrid_backward_input of Part 2,
 * mi3d_grid_points_backward_input of Part 3) and their second-order passes (mi3d_hashgrid_backward_input_backward,
 * mi3d_grid_points_backward_input_backward) and Parts 11 and 13 to 20 were added under 5: new symbols only, nothing
 * existing changed. */
int mi3d_abi_version(void);
const char *mi3d_last_error_string(int err);

/* ------------------------------------------------------------------ Part 1: raymarching backend */

/* raymarching.h:7  near_far_from_aabb -- rays_o,rays_d [N,3]; aabb [6]; nears,fars [N] */
int mi3d_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N,
                            float min_near, float *nears, float *fars, void *stream);
/* raymarching.h:8  sph_from_ray -- coords [N,2] */
int mi3d_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N, float *coords,
                      void *stream);
/* raymarching.h:9  morton3D -- coords int32 [N,3] -> indices int32 [N] */
int mi3d_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, void *stream);
/* raymarching.h:10 morton3D_invert */
int mi3d_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, void *stream);
/* raymarching.h:11 packbits -- grid float [N*8] -> bitfield uint8 [N] (bit i = grid[8n+i] > thresh) */
int mi3d_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, void *stream);

/* raymarching.h:13 march_rays_train -- xyzs,dirs [M,3]; deltas [M,2]; rays int32 [N,3] = (ray id, offset,
 * count); counter int32 [2] (+= samples, += rays).  Rows are written only for rays whose slab fits in M.
 * Slabs are handed out by one atomic per workgroup after an in-workgroup scan (rays[] rows are in ray
 * order: rays[n] describes ray n). */
int mi3d_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound,
                          float dt_gamma, uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                          const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                          int32_t *rays, int32_t *counter, const float *noises, void *stream);
/* Not in the reference, host only (no GPU, no stream): the launch shape mi3d_march_rays_train takes for N rays, from the
 * very function the launch calls.  out_host [3] = (rays per wave: 64, 32 or 16 - the other lanes of a wave only help to
 * store; batches = ceil(N / rays per wave); workgroups launched = min(batches, 4096), one wave each, a wave walking
 * batches w, w + workgroups, ...).  N == 0: three zeros.  hipErrorInvalidValue for out_host == NULL.  Added under ABI
 * version 5: a new symbol only. */
int mi3d_march_train_plan(uint32_t N, uint32_t *out_host);
/* Not in the reference: zero rows [counter[0], counter[0]+pad) of xyzs/dirs/deltas (pad < align), the rows
 * raymarching.py:237-241 exposes past the last sample; lets the caller skip the 537 MB zero fill of
 * raymarching.py:217-219. */
int mi3d_march_zero_tail(const int32_t *counter, uint32_t align, uint32_t M, float *xyzs, float *dirs,
                         float *deltas, void *stream);

/* raymarching.h:14-15 composite_rays_train_{forward,backward} */
int mi3d_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                      const int32_t *rays, uint32_t M, uint32_t N, float T_thresh,
                                      float *weights_sum, float *depth, float *image, void *stream);
int mi3d_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image,
                                       const float *sigmas, const float *rgbs, const float *deltas,
                                       const int32_t *rays, const float *weights_sum, const float *image,
                                       uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas,
                                       float *grad_rgbs, void *stream);
/* Not in the reference: the density compositor's backward WITH the gradient of `depth` (the reference's op drops
 * grad_depth, raymarching.py:287, so a depth loss reaches the field only through (1 - weights_sum) * max_depth on that
 * path).  grad_depth [N] and depth [N] (the forward's output) are indexed by ray id like grad_weights_sum / weights_sum.
 * grad_sigmas[i] gains, inside its bracket,  grad_depth * (T_incl_i * t_i - (depth - d_i)),  d_i = sum_{j <= i} w_j t_j;
 * grad_rgbs is what composite_rays_train_backward writes.  Same skips: an empty ray, a slab that overflows M, rows past
 * the stop sample.  With grad_depth == 0 the result is bit-identical to composite_rays_train_backward's.  There is no
 * SDF counterpart: that backward stays the reference's formula.  Added under ABI version 5: a new symbol only. */
int mi3d_composite_rays_train_backward_depth(const float *grad_weights_sum, const float *grad_depth,
                                             const float *grad_image, const float *sigmas, const float *rgbs,
                                             const float *deltas, const int32_t *rays, const float *weights_sum,
                                             const float *depth, const float *image, uint32_t M, uint32_t N,
                                             float T_thresh, float *grad_sigmas, float *grad_rgbs, void *stream);
/* raymarching.h:16-17 composite_sdf_rays_train_{forward,backward} (alpha = sigma) */
int mi3d_composite_sdf_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                          const int32_t *rays, uint32_t M, uint32_t N, float T_thresh,
                                          float *weights_sum, float *depth, float *image, void *stream);
int mi3d_composite_sdf_rays_train_backward(const float *grad_weights_sum, const float *grad_image,
                                           const float *sigmas, const float *rgbs, const float *deltas,
                                           const int32_t *rays, const float *weights_sum, const float *image,
                                           uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas,
                                           float *grad_rgbs, void *stream);

/* raymarching.h:20 march_rays (inference) */
int mi3d_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                    const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                    uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars,
                    float *xyzs, float *dirs, float *deltas, const float *noises, void *stream);
/* raymarching.h:21 composite_rays (inference, in place) */
int mi3d_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                        const float *sigmas, const float *rgbs, const float *normals, const float *deltas,
                        float *weights_sum, float *depth, float *image, float *normal, void *stream);
/* raymarching.h:22 composite_sdf_rays */
int mi3d_composite_sdf_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive,
                            float *rays_t, const float *sigmas, const float *rgbs, const float *deltas,
                            float *weights_sum, float *depth, float *image, void *stream);

/* ---- Part 1b: the inference loop driven from the device (replaces the host logic of nerf/renderer.py:526-551).
 * The reference loop reads the number of alive rays back every round (a boolean-mask copy = a synchronisation)
 * because launch sizes and n_step = max(min(N / n_alive, 8), 1) depend on it.  Here that state lives in `ctl`
 * (device int32[8]: [0] n_alive, [1] n_step, [2] rows = n_alive*n_step rounded up PAST a multiple of `align` as
 * raymarching.py:397-400 does, [3] marching steps done, [4] rounds done) and the kernels of a round read it; the host
 * launches each round for an upper bound `n_alive_max` of the alive count and may look at ctl[0] as rarely as it likes.
 *   mi3d_infer_begin        rays_alive = 0..N-1, ctl planned for round 0
 *   mi3d_march_rays_ctl     = mi3d_march_rays for ctl's n_alive / n_step; rows a ray leaves unused and the alignment
 *                             rows are zeroed (buffers of N + align rows are re-used across rounds); `noises` (float[N]
 *                             or NULL) jitters round 0 only (renderer.py:546)
 *   mi3d_composite_rays_ctl = mi3d_composite_rays for ctl's n_alive / n_step
 *   mi3d_compact_alive_ctl  rays_alive_out = the entries >= 0 of rays_alive_in[0 .. n_alive), order kept (the boolean
 *                             mask of renderer.py:550); ctl advanced: steps += n_step, n_alive = 0 once steps >=
 *                             max_steps (`while step < max_steps`), next round planned */
int mi3d_infer_begin(int32_t *ctl, int32_t *rays_alive, uint32_t N, uint32_t align, void *stream);
int mi3d_march_rays_ctl(const int32_t *ctl, uint32_t n_alive_max, const int32_t *rays_alive, const float *rays_t,
                        const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                        uint32_t C, uint32_t H, const uint8_t *grid, const float *fars, float *xyzs, float *dirs,
                        float *deltas, const float *noises, void *stream);
int mi3d_composite_rays_ctl(const int32_t *ctl, uint32_t n_alive_max, float T_thresh, int32_t *rays_alive,
                            float *rays_t, const float *sigmas, const float *rgbs, const float *normals,
                            const float *deltas, float *weights_sum, float *depth, float *image, float *normal,
                            void *stream);
int mi3d_compact_alive_ctl(int32_t *ctl, const int32_t *rays_alive_in, int32_t *rays_alive_out, uint32_t N,
                           uint32_t align, uint32_t max_steps, void *stream);

/* The same loop with the samples of a round COMPACTED and the round size set by a row BUDGET (round 5).  The reference's
 * round takes n_step = clamp(N / n_alive, 1, 8) steps of every alive ray and lays them out at n * n_step, so a 128 x 128
 * render is ~280 rounds of at most 16 384 rows - latency, not work.  A ray's result does not depend on how its samples
 * are cut into rounds (it carries t in rays_t and its transmittance in weights_sum), so here a round takes
 * n_step = clamp(budget / n_alive, step_min, step_max) steps and the march packs what the rays actually emitted into one
 * slab per ray (wave scan + one atomic per wave on ctl[2], as the training march does): a render is a handful of rounds
 * and no row of a finished ray is evaluated.  ctl (int32[16], ABI version 5; version 4: int32[8]): [0] n_alive, [1] n_step,
 * [2] rows of this round (written by the march, zeroed by begin / compact), [3] steps done, [4] rounds done, [5] budget,
 * [6] step_min, [7] step_max, [8] rows DROPPED so far because a ray's slab would have passed rows_cap (sticky; zeroed by
 * begin2; non-zero = the render is incomplete: the caller's rows_cap is below max(budget, N step_min)), [9..15] reserved.
 * The plan never lets steps done + n_step pass max_steps (a ray takes at most max_steps steps whatever the budget).
 *   mi3d_infer_begin2            rays_alive[i] = i, ctl for round 0
 *   mi3d_march_rays_compact_ctl  ray_slab int32[n_alive_max][2] = (first row, rows) per alive slot; t_next f32[n_alive_max] =
 *                                the march's own t behind its last step (what the next round resumes from: the restart is
 *                                exact, so the sample sequence of a ray is the same for every budget); a ray whose slab
 *                                would pass rows_cap emits nothing and its rows are counted in ctl[8] (cannot happen when
 *                                rows_cap >= max(budget, N step_min))
 *   mi3d_composite_rays_compact_ctl  composite_rays over each ray's slab; a ray that used all n_step rows resumes at t_next
 *   mi3d_compact_alive_ctl2      the compaction + the next round's plan                                       */
int mi3d_infer_begin2(int32_t *ctl, int32_t *rays_alive, uint32_t N, uint32_t budget_rows, uint32_t step_min,
                      uint32_t step_max, void *stream);
int mi3d_march_rays_compact_ctl(int32_t *ctl, uint32_t n_alive_max, const int32_t *rays_alive, const float *rays_t,
                                const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                uint32_t C, uint32_t H, const uint8_t *grid, const float *fars, uint32_t rows_cap,
                                float *xyzs, float *dirs, float *deltas, int32_t *ray_slab, float *t_next,
                                const float *noises, void *stream);
int mi3d_composite_rays_compact_ctl(const int32_t *ctl, uint32_t n_alive_max, float T_thresh, int32_t *rays_alive,
                                    float *rays_t, const int32_t *ray_slab, const float *t_next, const float *sigmas,
                                    const float *rgbs, const float *normals, const float *deltas, float *weights_sum,
                                    float *depth, float *image, float *normal, void *stream);
int mi3d_compact_alive_ctl2(int32_t *ctl, const int32_t *rays_alive_in, int32_t *rays_alive_out, uint32_t N,
                            uint32_t max_steps, void *stream);

/* ------------------------------------------------------------------ Part 2: hash-grid encoding */

/* Level table of a tcnn HashGrid (host side; no device work).  offsets_host has n_levels+1 entries in
 * units of grid entries (x n_features=2 floats).  Returns the total number of entries. */
uint32_t mi3d_hashgrid_levels(uint32_t n_levels, uint32_t base_resolution, float per_level_scale,
                              uint32_t log2_hashmap_size, uint32_t *offsets_host, uint32_t *resolutions_host,
                              float *scales_host);

/* tcnn.Encoding.forward: x [n,3] in [0,1]; params fp32 [entries*2]; out [n, n_levels*2] (feature = level*2+f) */
int mi3d_hashgrid_forward(const float *x, uint32_t n, const float *params, uint32_t n_levels,
                          uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size,
                          float *out, void *stream);
/* tcnn.Encoding.backward wrt params: grad_params [entries*2] is ACCUMULATED into (caller zeroes it) */
int mi3d_hashgrid_backward(const float *x, uint32_t n, const float *dout, uint32_t n_levels,
                           uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size,
                           float *grad_params, void *stream);
/* tcnn.Encoding.backward wrt the INPUT: dout [n, n_levels*2] rows -> grad_x [n,3] = dL/dx, WRITTEN (not accumulated).
 * tiny-cuda-nn gives this to any caller whose x requires grad; the reference never asks, so the arithmetic is this
 * project's own contract - PARITY UNPINNED, the standing of this whole Part.  Per level l with scale s_l let (c, f) be
 * cell and fraction of every dimension as the forward computes them (p = fma(s_l, q, 0.5), c = floor(p), f = p - c),
 * w(0) = 1 - f, w(1) = f, and v[.] the eight corner pairs the forward gathers.  For dimension d, with e, e' the other two:
 *     dy[l,feat]/dq_d = s_l * sum over (j,k) in {0,1}^2 of w_e(j) w_e'(k) (v[d=1,j,k].feat - v[d=0,j,k].feat)
 *     dL/dq_d         = sum over l, feat of dout[l,feat] * dy[l,feat]/dq_d
 * - the derivative of the trilinear interpolant INSIDE its cell.  The interpolant is piecewise linear: on a cell face the
 * result is the derivative of the cell floor picked (the one-sided derivative towards +), not a mean of the two.  This call is
 * the first order; its own derivative is mi3d_hashgrid_backward_input_backward below.  fp32 throughout, plain stores,
 * no atomics, one fixed order of additions: two calls give the same bits.
 * n == 0: nothing is launched, success; a null pointer (n > 0) or n_levels > MI3D_MAX_LEVELS: hipErrorInvalidValue.
 * Added under ABI version 5: a new symbol only. */
int mi3d_hashgrid_backward_input(const float *x, uint32_t n, const float *dout, const float *params, uint32_t n_levels,
                                 uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size,
                                 float *grad_x, void *stream);
/* The SECOND-ORDER pass: the backward of mi3d_hashgrid_backward_input, for losses that contain the input gradient (an
 * eikonal term, losses on analytic normals).  tiny-cuda-nn's grid has it as backward_backward_input; the arithmetic is this
 * project's own contract - PARITY UNPINNED.  g = grad_x of the call above is linear in dout and in the table and, inside
 * a cell, bilinear in the fractions.  Given r [n,3] = dL/dg, with the notation above, sigma(0) = -1, sigma(1) = +1, the
 * corners k = bx | by << 1 | bz << 2 and, per level, rho_d = r_d s_l, let
 *     T_{d,c}    = sum_k sigma(b_d) w_e(b_e) w_e'(b_e') v[k].c          (g_d = sum_l sum_c dout[l,c] s_l T_{d,c})
 *     M_{d,d',c} = sum_k sigma(b_d) sigma(b_d') w_e(b_e) v[k].c         (e the remaining dimension)
 * Three outputs, each computed only if its pointer is not NULL:
 *     grad_dout [n, n_levels*2] WRITTEN       grad_dout[l,c] = sum_d rho_d T_{d,c}
 *     grad_x    [n,3]           WRITTEN       grad_q_d' = sum_l s_l sum_c dout[l,c] sum_{d != d'} rho_d M_{d,d',c}
 *     grad_params [entries*2]   ACCUMULATED   grad_params[entry(k), c] += dout[l,c] kappa_k,
 *                                             kappa_k = rho_x sigma(bx) w_y w_z + rho_y w_x sigma(by) w_z + rho_z w_x w_y sigma(bz)
 * grad_x holds the mixed second derivatives of the trilinear interpolant inside its cell; the pure ones are zero.  The
 * two row outputs come from one kernel, launched only if one of them is asked for: plain stores, one fixed order of
 * additions, the same bits from call to call and whichever other outputs are asked for.  grad_params comes from a second
 * kernel, launched only if asked for: the pointwise scatter with the trilinear weight replaced by kappa_k, float atomics
 * (the caller zeroes; the order of the additions is free); a point whose dout pair is zero or whose three rho are zero
 * adds nothing.  It is sized for the <= ~1e7 points a second-order loss is taken on.  n == 0: nothing is launched,
 * success; a null input (n > 0), all three outputs NULL or n_levels > MI3D_MAX_LEVELS: hipErrorInvalidValue.
 * Added under ABI version 5: a new symbol only. */
int mi3d_hashgrid_backward_input_backward(const float *x, uint32_t n, const float *dout, const float *params,
                                          const float *r, uint32_t n_levels, uint32_t base_resolution,
                                          float per_level_scale, uint32_t log2_hashmap_size, float *grad_dout,
                                          float *grad_x, float *grad_params, void *stream);

/* ------------------------------------------------------------------ Part 3: stencil-aware grid ops */

/* The reference evaluates the field at 13 points per sample: x, x +- eps e_i (finite_difference_normal,
 * network_tcnn.py:115-128) and the same six offsets around x2 = x + 0.01 randn (loss_smooth,
 * nerf/renderer.py:521-524), each as a separate encoder pass.  These two entry points take the whole stencil:
 * point p of sample i is clamp(base + offsets[p], -bound, bound) with base = x[i] for p < P0 and x2[i] for
 * P0 <= p < P (x2 may be NULL when P0 == P), mapped to [0,1] as (pt + bound) / (2 bound) (network_tcnn.py:106).
 * Rows are POINT-MAJOR: row (p*n + i) of `out` / `dout` holds the n_levels*2 features of point p of sample i, so the
 * rows of one stencil point are contiguous (a backward pass that only reaches the first P' points - sigma / albedo
 * alone reach point 0, the normal points 0..6 - runs on that prefix of the rows and nothing else).
 * `count` (device int32, may be NULL) caps n at min(n, *count) without a host round trip.
 * `step` (scatter only): the marching step dt_min in world units (0 = unknown); it only selects which levels
 * use run-merging vs lane-quad atomics, never the result. */
int mi3d_grid_encode_points(const float *x, const float *x2, uint32_t n, const int32_t *count,
                            const float *offsets_host, uint32_t P0, uint32_t P, float bound, const float *params,
                            uint32_t n_levels, uint32_t base_resolution, float per_level_scale,
                            uint32_t log2_hashmap_size, float *out, void *stream);
/* dL/dx and dL/dx2 of mi3d_grid_encode_points: dout [P*n, n_levels*2] point-major rows ->
 * grad_x [n,3] = sum over the points p < P0, grad_x2 [n,3] = sum over P0 <= p < P (NULL if and only if x2 is NULL; a buffer
 * passed without x2 is left untouched), both WRITTEN.  Per point the arithmetic is mi3d_hashgrid_backward_input's (Part 2) at q = (pt + bound) / (2 bound), times
 * dq/dpt = 1 / (2 bound) - a multiplication by the reciprocal where 2 bound is a power of two, a division otherwise, as the
 * forward maps the point - and coordinate d of point p reaches its base only where |base_d + offsets[p]_d| <= bound,
 * bounds INCLUDED: the rule of torch.clamp's backward.  No device-side count: the counted rows belong to the inference
 * loop, which never differentiates.  Deterministic like the Part 2 call.  n == 0: nothing is launched, success; a null
 * pointer, a bad stencil (P > MI3D_MAX_POINTS, P0 > P, points around a NULL x2) or x2 without grad_x2:
 * hipErrorInvalidValue.  Added under ABI version 5: a new symbol only. */
int mi3d_grid_points_backward_input(const float *x, const float *x2, uint32_t n, const float *offsets_host, uint32_t P0,
                                    uint32_t P, float bound, const float *dout, const float *params, uint32_t n_levels,
                                    uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size,
                                    float *grad_x, float *grad_x2, void *stream);
/* The second-order pass of mi3d_grid_points_backward_input: r [n,3] = dL/dgrad_x, r2 [n,3] = dL/dgrad_x2 (not NULL
 * exactly when x2 is not NULL).  Per point p the arithmetic is mi3d_hashgrid_backward_input_backward's (Part 2) at
 * q = (pt + bound) / (2 bound) with rho_d = r_d m_d / (2 bound) s_l - r of the point's base, m_d = 1 where
 * |base_d + offsets[p]_d| <= bound (bounds included) and 0 otherwise, the factor 1 / (2 bound) applied as the first-order
 * call applies it - and grad_q_d' is multiplied by m_d' / (2 bound) again on its way to the base.  grad_dout [P*n,
 * n_levels*2] point-major rows, WRITTEN; grad_x [n,3] = the sum over the points p < P0 and grad_x2 [n,3] = the sum over
 * P0 <= p < P, WRITTEN (grad_x2 is passed exactly when both x2 and grad_x are: the two come from one sum); grad_params
 * ACCUMULATED.  Each output is computed only if its pointer is not NULL, by the two kernels of the Part 2 call.  No
 * device-side count.  n == 0: nothing is launched, success; a null input, all outputs NULL, a bad stencil, r2 without x2
 * or x2 without r2, grad_x2 without x2 or without grad_x, x2 and grad_x without grad_x2: hipErrorInvalidValue.
 * Added under ABI version 5: a new symbol only. */
int mi3d_grid_points_backward_input_backward(const float *x, const float *x2, uint32_t n, const float *offsets_host,
                                             uint32_t P0, uint32_t P, float bound, const float *dout, const float *params,
                                             const float *r, const float *r2, uint32_t n_levels, uint32_t base_resolution,
                                             float per_level_scale, uint32_t log2_hashmap_size, float *grad_dout,
                                             float *grad_x, float *grad_x2, float *grad_params, void *stream);
/* mi3d_grid_encode_points with level-major output planes [n_levels][P*n][2] (feature pair of level l, row r = p*n + i
 * at out_planes[(l*P*n + r)*2]) - the layout the MLP kernels take with x_plane_rows = P*n.  The (level, tile) work is
 * tied to XCDs so each XCD's L2 only ever holds the table of the level it is gathering from; `step` (the marching
 * step in world units, 0 = unknown) only balances that split, never the result.  The workgroups of an XCD claim their
 * tiles from per-segment counters: 512 bytes of a 64-slot ring in device memory that belongs to the library, zeroed
 * in `stream` before the launch.  Calls on ONE stream may be queued without limit (a slot coming round again is behind
 * its previous user in stream order); a call that finds its slot last used by ANOTHER stream that has not drained deals
 * its tiles statically instead of claiming them (same planes, slower) - two live launches never share counters.
 * PLANE ELEMENT TYPE: out_half == 0: fp32 pairs (8 bytes per (level, row)); out_half != 0: binary16 pairs (4 bytes) -
 * for use under torch.autocast(float16) only, where the first nn.Linear rounds its input to binary16 anyway
 * (mi3d_mlp_forward / _backward with half_mode != 0 read them with planes_half != 0: same MLP output, bit for bit,
 * half the bytes).  The gradient planes mi3d_mlp_backward writes follow the same flag: the input gradient of that
 * Linear comes out of a binary16 GEMM in the reference, so binary16 planes hold exactly what autocast would hand the
 * encoder's backward. */
int mi3d_grid_encode_points_planes(const float *x, const float *x2, uint32_t n, const float *offsets_host, uint32_t P0,
                                   uint32_t P, float bound, const float *params, uint32_t n_levels,
                                   uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size, float step,
                                   void *out_planes, int out_half, void *stream);
/* ... with a DEVICE-side sample count (count == NULL: all n): samples s >= *count are not evaluated, their rows are not
 * written; the plane strides stay n.  Used by the inference loop, whose row count lives in its control block. */
int mi3d_grid_encode_points_planes_counted(const float *x, const float *x2, uint32_t n, const int32_t *count,
                                           const float *offsets_host, uint32_t P0, uint32_t P, float bound,
                                           const float *params, uint32_t n_levels, uint32_t base_resolution,
                                           float per_level_scale, uint32_t log2_hashmap_size, float step, void *out_planes,
                                           int out_half, void *stream);
int mi3d_grid_scatter_points(const float *x, const float *x2, uint32_t n, const int32_t *count,
                             const float *offsets_host, uint32_t P0, uint32_t P, float bound, const float *dout,
                             uint32_t n_levels, uint32_t base_resolution, float per_level_scale,
                             uint32_t log2_hashmap_size, float step, float *grad_params, void *stream);

/* The same scatter without global atomics: every corner contribution (on the coarse levels: what a wave's 64 samples
 * x P points contribute to one entry, summed in LDS first; on the fine levels: the two x-neighbours of a corner pair as
 * ONE 16-byte record) is appended to the region of its 64-KB gradient bin, then each bin is accumulated in LDS in 64-bit fixed point and
 * added to the table (see hashgrid.hip).  fp32 contributions throughout; a non-finite contribution bypasses the
 * records and is added to the table with float atomics, so the inf / NaN lands on exactly the entries the reference's
 * atomicAdd would have put it on (and nowhere else).
 * `dout_planes` is level-major [n_levels][P*n][2], rows point-major (what mi3d_mlp_backward writes with
 * dx_plane_rows = P*n); dout_half != 0: binary16 pairs (see mi3d_grid_encode_points_planes).
 * `workspace` is caller-provided device scratch (never allocated here); samples are processed in the FEWEST equal
 * slices whose record arena fits it (ceil(n / k), k = 1, 2, 3 ...; the emit's tile-claim counters live in it too); with workspace == NULL or too small for even 64 samples the atomic kernels of mi3d_grid_scatter_points run
 * instead.  mi3d_grid_scatter_binned_workspace() returns the size that lets n samples go in ONE slice. */
size_t mi3d_grid_scatter_binned_workspace(uint32_t n, uint32_t P, float bound, float step, uint32_t n_levels,
                                          uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size);
int mi3d_grid_scatter_binned(const float *x, const float *x2, uint32_t n, const float *offsets_host, uint32_t P0,
                             uint32_t P, float bound, const void *dout_planes, int dout_half, uint32_t n_levels,
                             uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size, float step,
                             void *workspace, size_t workspace_bytes, float *grad_params, void *stream);
/* ... plus a SECOND gradient pair for stencil point 0: `extra_point0_planes` [n_levels][n][2] (same element type as
 * dout_planes; NULL = none).  The reference back-propagates twice through one forward (nerf/sd.py:171 latents.backward,
 * then nerf/utils.py:983 scaler.scale(loss).backward()); the first pass reaches sigma / albedo of point 0 only.  Its
 * point-0 gradient planes can be handed to the second pass's scatter here, which adds the two pairs of point 0 in fp32
 * and scatters the sum - the same table gradient as two scatters (tcnn's atomics add the two products separately: equal
 * up to fp32 rounding of w (a + b) against w a + w b), for one pass over the table instead of two. */
int mi3d_grid_scatter_binned_plus(const float *x, const float *x2, uint32_t n, const float *offsets_host, uint32_t P0,
                                  uint32_t P, float bound, const void *dout_planes, const void *extra_point0_planes,
                                  int dout_half, uint32_t n_levels, uint32_t base_resolution, float per_level_scale,
                                  uint32_t log2_hashmap_size, float step, void *workspace, size_t workspace_bytes,
                                  float *grad_params, void *stream);

/* Host-side planning queries: no device work, callable without a GPU (tests/test_plan_cpu.py).
 * mi3d_grid_encode_plan: how mi3d_grid_encode_points_planes cuts the (level, tile-of-64-samples) list into one run of
 *   segments per XCD: n_segments[8], segments[8][16][3] = (level, first tile, end tile).
 * mi3d_grid_scatter_plan: how mi3d_grid_scatter_binned lays out its workspace for n samples and `workspace_bytes`:
 *   out[0] samples per slice, out[1] workspace bytes one slice uses, out[2] coarse levels (gathered per tile),
 *   out[3] reduce workgroups, out[4] record-arena bytes, out[5] region counters, then 7 values per level: bins, region
 *   capacity (records), emitting waves, 1 = 16-byte x-pair records, reduce workgroups per bin, first reduce workgroup,
 *   first region counter.  out must hold 6 + 7 * n_levels values.  (The layout for fp32 gradient planes, 16-byte pair
 *   records - what mi3d_grid_scatter_binned_workspace sizes; with binary16 planes the pair records take 12 bytes, so the
 *   same workspace holds more samples per slice than this query says.)
 * mi3d_grid_level_routes: which index route the plane gather and the scatter's emit take on each level (kinds[n_levels]):
 *   0 the general rule (any dims, any table size, any input - tcnn's grid_index as the oracle restates it), 1 dense 3-D
 *   strided (24-bit multiplies, at most one wrap), 2 power-of-two hash (mask).  `stencil_points` != 0: the positions are
 *   clamped stencil points (mi3d_grid_encode_points*), 0: raw positions (mi3d_hashgrid_*), which always take route 0. */
int mi3d_grid_encode_plan(uint32_t n, float bound, float step, uint32_t n_levels, uint32_t base_resolution,
                          float per_level_scale, uint32_t log2_hashmap_size, uint32_t *n_segments, uint32_t *segments);
int mi3d_grid_scatter_plan(uint32_t n, uint32_t P, float bound, float step, uint32_t n_levels, uint32_t base_resolution,
                           float per_level_scale, uint32_t log2_hashmap_size, size_t workspace_bytes,
                           unsigned long long *out);
int mi3d_grid_level_routes(uint32_t n_levels, uint32_t base_resolution, float per_level_scale, uint32_t log2_hashmap_size,
                           int stencil_points, int32_t *kinds);

/* ------------------------------------------------------------------ Part 4: the field's MLP (sigma_net) */

/* network_tcnn.py:13-32: y = W3 relu(W2 relu(W1 x + b1) + b2) + b3, torch nn.Linear layout (W_l is [out_l, in_l]
 * row-major fp32, the master weights).  x [n, dim_in] fp32 rows (x_plane_rows == 0), or level-major planes
 * [dim_in/2][x_plane_rows][2] of which the first n rows are processed (x_plane_rows >= n; planes_half != 0: the planes
 * hold binary16 pairs, half_mode only - applies to x and, in the backward, to dx alike); out [n, dim_out] fp32.
 * half_mode != 0 reproduces torch.autocast(float16) around the stack (nerf/utils.py:979): inputs, weights, biases
 * and every layer output are rounded to binary16, products accumulate in fp32 (v_mfma_f32_32x32x16_f16);
 * half_mode == 0 is exact fp32 (v_mfma_f32_32x32x2_f32).  Supported shapes - every one the reference's MLP class can
 * build around this field (network_tcnn.py:37-45,67 takes num_layers and hidden_dim; BASELINE config 1 is 8 -> 32 -> 4):
 * dim_in even, 2..32 (= 2 x grid levels), dim_hidden 32 or 64, dim_out 4, two or three layers.  TWO layers are
 * requested by passing W2 == b2 == NULL (and dW2 == db2 == NULL in the backward): y = W3 relu(W1 x + b1) + b3.
 * Anything else returns hipErrorInvalidValue - ask mi3d_mlp_supported() first. */
int mi3d_mlp_supported(uint32_t dim_in, uint32_t dim_hidden, uint32_t dim_out, uint32_t num_layers);
int mi3d_mlp_forward(const void *x, uint32_t x_plane_rows, int planes_half, uint32_t n, const float *W1,
                     const float *b1, const float *W2, const float *b2,
                     const float *W3, const float *b3, uint32_t dim_in, uint32_t dim_hidden, uint32_t dim_out,
                     int half_mode, float *out, void *stream);
/* Backward of the above for upstream gradient dout [n, dim_out]: writes dx and ACCUMULATES the weight and bias
 * gradients (fp32, same layouts as the weights; caller zeroes them).  Activations are recomputed.
 * dx_plane_rows == 0: dx is [n, dim_in] rows; otherwise dx is level-major planes [dim_in/2][dx_plane_rows][2]
 * (feature pair (2l, 2l+1) of row r at dx[(l*dx_plane_rows + r)*2]), the layout mi3d_grid_scatter_binned consumes.
 * ALIASING: dx may be x itself (dx == x) when both have the same layout - dx_plane_rows == x_plane_rows (0 = rows for both)
 * - and therefore the same element type (planes_half covers both): the gradient of a row replaces the row.  Any n is
 * allowed, a partial last tile (n % 32 != 0) and plane rows past n included; those rows keep their contents.  A wave reads
 * the 32 rows of its tile before it stores their gradients and no other wave reads them (rows past n are read as row n - 1
 * by the wave that owns row n - 1).  dx == x in different layouts returns hipErrorInvalidValue; buffers that overlap in any
 * other way, and dout or a weight overlapping an output, are undefined.  In the forward, `out` must not overlap x. */
/* The same with a DEVICE-side row count (the inference loop's control block, Part 1b): rows are point-major with
 * `n_stride` rows per stencil point, and only samples s < *count carry data; tiles wholly beyond it are skipped and
 * their outputs left untouched, and so is every row s >= *count of a tile that straddles it.  count == NULL: every row.  (The gather and the head have the same variant.) */
int mi3d_mlp_forward_counted(const void *x, uint32_t x_plane_rows, int planes_half, uint32_t n, const int32_t *count,
                             uint32_t n_stride, const float *W1, const float *b1, const float *W2, const float *b2,
                             const float *W3, const float *b3, uint32_t dim_in, uint32_t dim_hidden, uint32_t dim_out,
                             int half_mode, float *out, void *stream);
int mi3d_mlp_backward(const void *x, uint32_t x_plane_rows, int planes_half, const float *dout, uint32_t n,
                      const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                      const float *b3, uint32_t dim_in, uint32_t dim_hidden, uint32_t dim_out, int half_mode, void *dx,
                      uint32_t dx_plane_rows, float *dW1, float *db1, float *dW2, float *db2, float *dW3, float *db3,
                      void *stream);
/* SECOND ORDER: the backward of mi3d_mlp_backward's dx, for losses on the input gradient.  Exact fp32, rows
 * only: x, dout and r = dL/d(dx) are [n, dim_in], [n, dim_out] and [n, dim_in] rows.  With a1 = W1 x + b1, M1 = [a1 > 0],
 * a2 = W2 relu(a1) + b2, M2 = [a2 > 0] (open iff not (activation <= 0), the first-order kernel's masks bit for bit: the
 * forward is recomputed with the same product sequence) and the first-order chain
 *   d2 = M2 (W3^T dy),  d1 = M1 (W2^T d2),  dx = W1^T d1
 * one tangent chain through the same masks,
 *   u1 = M1 (W1 r),  u2 = M2 (W2 u1),  u3 = W3 u2          (so that <dx, r> = dy^T u3),
 * gives every output:
 *   grad_dout [n, dim_out] = u3                                            plain stores
 *   gW3 += sum_rows dy u2^T,  gW2 += sum_rows d2 u1^T,  gW1 += sum_rows d1 r^T     ACCUMULATED, caller zeroes
 * Two layers (W2 == b2 == NULL; gW2 is ignored): u1 = M1 (W1 r), u3 = W3 u1, gW3 += dy u1^T, gW1 += d1 r^T.
 * The gradients with respect to x and to the biases are exact zeros - dx depends on them through the piecewise constant
 * masks only - and are not written.  grad_dout == NULL skips it; gW1 == gW2 == gW3 == NULL skips the weight gradients,
 * which otherwise come together (gW1, gW3 and, with three layers, gW2); grad_dout has the same bits either way.  Rows at or
 * past n are neither read nor written.  hipErrorInvalidValue: unsupported dims, a null x / dout / r / weight / bias, some but
 * not all weight outputs, every output null.  (dout must be given even when grad_dout alone is asked for, although u3 does
 * not depend on it and that launch never reads it: one rule for every call.)  n == 0 returns 0.  Never allocates, never synchronises.  No output may
 * overlap an input. */
int mi3d_mlp_backward_backward(const float *x, const float *dout, const float *r, uint32_t n, const float *W1,
                               const float *b1, const float *W2, const float *b2, const float *W3, const float *b3,
                               uint32_t dim_in, uint32_t dim_hidden, uint32_t dim_out, float *grad_dout, float *gW1,
                               float *gW2, float *gW3, void *stream);

/* ------------------------------------------------------------------ Part 5: the field head */

/* From the MLP output h [P, n, 4] (point-major rows p*n + i) of the stencil points (P = 7: sample + its six +-epsilon neighbours in the order
 * +x,-x,+y,-y,+z,-z; P = 13: plus the six neighbours of x2) to what the renderer consumes, in one elementwise pass:
 *   sigma [n]     = exp(h_0[0] + blob(x))                         network_tcnn.py:94-100,109, activation.py:5-18
 *   albedo [n,3]  = sigmoid(h_0[1..3])                            network_tcnn.py:110
 *   normal [n,3]  = nan_to_num(safe_normalize(-(sigma+ - sigma-) / (2 epsilon)))   network_tcnn.py:115-138, utils.py:47-48
 *   normal2 [n,3] = the same around x2 (P = 13 only)              nerf/renderer.py:521-524
 * The stencil positions are clamp(base + offsets_host[p], -bound, bound), as in mi3d_grid_encode_points. */
int mi3d_field_head_forward(const float *h, const float *x, const float *x2, uint32_t n, const float *offsets_host,
                            uint32_t P, float bound, float blob_density, float blob_radius, float epsilon, float *sigma,
                            float *albedo, float *normal, float *normal2, void *stream);
int mi3d_field_head_forward_counted(const float *h, const float *x, const float *x2, uint32_t n, const int32_t *count,
                                    const float *offsets_host, uint32_t P, float bound, float blob_density,
                                    float blob_radius, float epsilon, float *sigma, float *albedo, float *normal,
                                    float *normal2, void *stream);
/* Backward: upstream gradients (any may be NULL = zero) -> dh [P_active, n, 4], the rows of the first P_active
 * points only: 1 (sigma / albedo alone carry a gradient: the SDS pass), 7 (+ normal) or 13 (+ normal2); the caller
 * runs the MLP backward and the scatter over that prefix.  trunc_exp's clamped derivative (activation.py:15-18),
 * clamp and nan_to_num pass gradients exactly where torch's do. */
int mi3d_field_head_backward(const float *h, const float *x, const float *x2, uint32_t n, const float *offsets_host,
                             uint32_t P, uint32_t P_active, float bound, float blob_density, float blob_radius,
                             float epsilon, const float *dsigma, const float *dalbedo, const float *dnormal,
                             const float *dnormal2, float *dh, void *stream);

/* ------------------------------------------------------------------ Part 6: the optimizer step */

/* Adan as the reference configures it (main.py:132; optimizer.py:100-249 `Adan.step` + `_single_tensor_adan`), one
 * fused elementwise pass per parameter tensor, in the reference's operation order.  All pointers are device fp32
 * arrays of `count` elements, 16-byte aligned; grad is scaled by the clip factor in place (as the reference does),
 * the four state arrays are updated in place (the caller zero-initialises exp_avg / exp_avg_sq / exp_avg_diff once;
 * neg_pre_grad is initialised here when first_step != 0).
 * The global-norm clip stays on the device: call mi3d_sumsq_accumulate on every gradient tensor into ONE zeroed device
 * double (8-byte aligned; the sum and the factor are formed in binary64, the factor rounded once), pass it as grad_sumsq; clip = min(max_grad_norm / (sqrt(sum) + clip_eps), 1) (optimizer.py:107-127, without
 * its `.item()` host sync).  grad_sumsq == NULL or max_grad_norm <= 0: no clipping.
 * The betas are binary64: the kernel uses (float)beta and (float)(1 - beta), each rounded once from the caller's value,
 * as the reference's `mul_(beta)` / `alpha=1 - beta` do (1.0f - (float)beta is off 1 - beta by up to 2^-25 / (1 - beta)). */
int mi3d_sumsq_accumulate(const float *x, size_t n, double *acc, void *stream);
int mi3d_adan_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, float *exp_avg_diff,
                   float *neg_pre_grad, size_t count, const double *grad_sumsq, float max_grad_norm, float clip_eps,
                   int first_step, double beta1, double beta2, double beta3, float bias_correction1,
                   float bias_correction2, float bias_correction3_sqrt, float lr, float weight_decay, float eps,
                   int no_prox, void *stream);

/* ------------------------------------------------------------------ Part 7: refine-stage point renderer */

/* The two pytorch3d calls of the reference's `render_point` (nerf/refine_utils.py:306-333).
 * mi3d_points_rasterize = pytorch3d.renderer.points.rasterize_points on ONE point cloud: points_ndc [P,3] = (x, y in
 * pytorch3d NDC: +X left, +Y up; z = depth, points with z < 0 are skipped), image H x W, `radius` in NDC units,
 * K = points_per_pixel <= 8.  Outputs [H,W,K]: idx (point index, -1 = unused), zbuf (may be NULL), dists (squared NDC
 * distance to the pixel centre, -1 = unused), the K nearest covering points in ascending z (ties: lower index first).
 * `workspace` holds the per-tile point lists (mi3d_points_rasterize_workspace bytes cover the worst case; P = 0 is
 * legal, needs the tile table alone and gives -1 everywhere).
 * mi3d_points_composite_forward = alphas = 1 - sqrt(clamp(0.1 dists / radius^2, 1e-3, 1)) (refine_utils.py:321-326)
 * followed by compositing.alpha_composite: out [C,H,W] from features [P,C] (C <= 32), front to back.
 * mi3d_points_composite_backward ACCUMULATES d out / d features into grad_features [P,C] (caller zeroes it).
 *
 * Gradient for the point positions (and, through the caller's projection, the camera) - this project's own contract:
 * pytorch3d differentiates rasterize_points through `dists` and alpha_composite through `alphas`, but it is absent and
 * unpinned, the standing of the rest of this Part.  For one pixel let its used slots be k = 0 .. n-1, front to back as
 * idx stores them (slots with idx < 0 are skipped, exactly as in the forward), and
 *     u_k = 0.1 dist_k / radius^2,   a_k = 1 - sqrt(clamp(u_k, 1e-3, 1)),   T_k = prod_{j<k} (1 - a_j),
 *     s_k = sum_c grad_out[c, pixel] * features[idx_k, c].
 * Back to front, R_{n-1} = 0 and R_{k-1} = a_k s_k + (1 - a_k) R_k.  Then
 *     dL/da_k    = T_k (s_k - R_k)                      (no division by 1 - a; pytorch3d divides by 1 - a + eps, we do not)
 *     dL/ddist_k = dL/da_k * (-0.05 / (radius^2 sqrt(u_k)))   where 1e-3 <= u_k <= 1, and 0 outside
 *                  (the closed interval is torch.clamp's gradient; since dist < radius^2 only the lower clamp ever binds,
 *                  for points within a tenth of the radius of the pixel centre)
 *     dL/dx_p   += 2 (x_p - xf) dL/ddist_k, y likewise, with (xf, yf) the pixel centre mi3d_points_rasterize measures
 *                  dist from (pix_to_ndc of the mirrored pixel index);   dL/dz_p = 0: depth decides only the order.
 * This is the exact derivative of the forward for FIXED idx, i.e. almost everywhere.  The jump at the edge of a point's
 * disc - alpha drops from 1 - sqrt(0.1) = 0.68 to nothing - and the changes of the depth order are NOT differentiated.
 * mi3d_points_composite_backward_dists writes grad_dists [H,W,K] with plain stores (0 in unused slots and where the
 * clamp binds): reproducible run to run.  K <= 8, C <= 32; argument checks otherwise those of
 * mi3d_points_composite_backward.
 * mi3d_points_rasterize_backward ACCUMULATES into the x and y columns of grad_points [P,3] (caller zeroes it; the z
 * column is never touched) with float atomics, for every slot idx names - no test against the disc; an index outside
 * [0, P) is skipped.  The sum's last bits depend on the arrival order. */
size_t mi3d_points_rasterize_workspace(uint32_t P, uint32_t H, uint32_t W, float radius);
int mi3d_points_rasterize(const float *points_ndc, uint32_t P, uint32_t H, uint32_t W, float radius,
                          uint32_t points_per_pixel, void *workspace, size_t workspace_bytes, int32_t *idx, float *zbuf,
                          float *dists, void *stream);
int mi3d_points_composite_forward(const int32_t *idx, const float *dists, uint32_t H, uint32_t W, uint32_t points_per_pixel,
                                  const float *features, uint32_t C, double radius, float *out, void *stream);
int mi3d_points_composite_backward(const int32_t *idx, const float *dists, uint32_t H, uint32_t W,
                                   uint32_t points_per_pixel, const float *grad_out, uint32_t C, double radius,
                                   float *grad_features, void *stream);
int mi3d_points_composite_backward_dists(const int32_t *idx, const float *dists, uint32_t H, uint32_t W,
                                         uint32_t points_per_pixel, const float *grad_out, const float *features,
                                         uint32_t C, double radius, float *grad_dists, void *stream);
int mi3d_points_rasterize_backward(const float *points_ndc, uint32_t P, const int32_t *idx, const float *grad_dists,
                                   uint32_t H, uint32_t W, uint32_t points_per_pixel, float *grad_points, void *stream);

/* ------------------------------------------------------------------ Part 8: marching cubes (mesh export) */

/* A dense scalar volume -> a WELDED, INDEXED triangle mesh in a deterministic order: what `mcubes.marching_cubes` does
 * for the reference's export_mesh (nerf/renderer.py:182).  PyMCubes is on no machine this project builds on and its
 * conventions can only be quoted from memory, so the semantics below are this project's own contract - PARITY UNPINNED,
 * the standing tiny-cuda-nn's (Part 2) and pytorch3d's (Part 7) restatements have.
 *
 * vol float[Rx*Ry*Rz], x slowest: grid point (i, j, k) at (i*Ry + j)*Rz + k; each of Rx, Ry, Rz in [2, 1024].
 *   - A grid point is INSIDE iff vol >= iso (NaN is outside).  iso must not be NaN.
 *   - Cube corners 0..7 sit at the min corner + (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1), cube
 *     edges 0..11 join corners 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7 (the numbering of Bourke's
 *     "Polygonising a scalar field"); bit c of the case index is set iff corner c is inside.
 *   - The 256-case table (csrc/mi3d_mc_tables.h, constructed by tools/gen_mc_tables.py, read back through mi3d_mc_case)
 *     cuts off the INSIDE corners separately on every ambiguous face, so the segments a cube leaves on a face depend on
 *     that face's four corners alone and the neighbour has the same segments reversed: meshes have no cracks.  At most
 *     five triangles per cube.  tests/test_mc_tables_cpu.py states and checks the properties.
 *   - Every grid edge whose ends differ in side owns exactly ONE vertex.  On the edge from point a to b = a + e_axis it
 *     sits, in index units, at a_axis + t, t = (iso - va) / (vb - va) in binary32, each operation rounded once; t outside
 *     [0, 1] (NaN included: a non-finite va or vb) becomes 0.5.  Written: origin_host[c] + spacing_host[c] * (a_c + t_c)
 *     per coordinate c (t_c = t on the edge's axis, 0 elsewhere) as three separately rounded binary32 operations - the add
 *     in the parentheses, the multiply, the add; no fused multiply-add.
 *   - Triangles are wound so that normals point from inside to outside (towards decreasing values) for positive
 *     spacings: the mesh of a density blob has positive signed volume.  Degenerate triangles (a corner value exactly
 *     iso) are kept.
 *   - ORDER (part of the contract; two runs give byte-identical buffers): vertices by owning grid point a (linear index),
 *     then axis x, y, z; triangles by cell (linear index of its min corner), then table order.
 *
 *   mi3d_mc_workspace  bytes of device scratch for a volume of this size (0 for sizes out of range); host only
 *   mi3d_mc_case       host only: copies table row `case_index` (cube edges, three per triangle, -1 terminated) into
 *                      edges_host[16] and returns its triangle count; -1 for case_index > 255 or a NULL pointer
 *   mi3d_mc_count      per-workgroup vertex and triangle counts -> workspace
 *   mi3d_mc_scan       their exclusive scan; counts (device uint64[4], 8-byte aligned) = {vertices, triangles, 0, 0}.
 *                      The caller reads counts once to size the outputs - the only host read of an extraction.
 *   mi3d_mc_emit       vertices float[nv_cap][3], triangles int32[nt_cap][3].  Nothing is written past the caps (vertex
 *                      ids are int32: at most 2^31 - 1 vertices); what could not be placed is COUNTED in counts[2]
 *                      (vertices + triangles) instead of being dropped silently, the convention ctl[8] of Part 1b set.
 * count, scan and emit of one extraction go to the same stream, in this order, with the same vol / sizes / iso / ws. */
size_t mi3d_mc_workspace(uint32_t Rx, uint32_t Ry, uint32_t Rz);
int mi3d_mc_case(uint32_t case_index, int8_t *edges_host);
int mi3d_mc_count(const float *vol, uint32_t Rx, uint32_t Ry, uint32_t Rz, float iso, void *ws, size_t ws_bytes,
                  unsigned long long *counts, void *stream);
int mi3d_mc_scan(uint32_t Rx, uint32_t Ry, uint32_t Rz, void *ws, size_t ws_bytes, unsigned long long *counts,
                 void *stream);
int mi3d_mc_emit(const float *vol, uint32_t Rx, uint32_t Ry, uint32_t Rz, float iso, const float *origin_host,
                 const float *spacing_host, void *ws, size_t ws_bytes, unsigned long long *counts, float *vertices,
                 unsigned long long nv_cap, int32_t *triangles, unsigned long long nt_cap, void *stream);

/* ------------------------------------------------------------------ Part 9: texture baking (mesh export) */

/* An indexed triangle mesh (Part 8's output) -> a UV atlas, the surface point of every texel, and the 8-bit RGB image of
 * the albedo evaluated there: what xatlas (unwrap), nvdiffrast (UV-space rasterisation) and the kd-tree inpainting do for
 * the reference's export_mesh (nerf/renderer.py:193-299).  None of them exists for this hardware; the layout below is this
 * project's own contract - PARITY UNPINNED, the standing of Part 8.  Added under ABI version 5: new symbols only.
 *
 * Marching-cubes triangles are all at most one grid cell large, so every triangle gets the SAME right-triangle patch of
 * texels and two patches share a rectangular cell (the trivial per-triangle parametrisation): O(1) per triangle,
 * deterministic, and it needs no inpainting - the gutter texels are evaluated at the affinely extrapolated surface point.
 *
 *   - TEXTURE: T x T texels, T in [64, 16384]; image row 0 is the TOP row; texel (X, Y) = column X of row Y.
 *   - CELL: c + 1 texels wide, c high, c >= 4.  Cells tile the image from the top-left, row by row: cols = T / (c + 1),
 *     rows = T / c (integer divisions).  Triangle i lies in cell q = i / 2, at cell column q % cols and cell row q / cols,
 *     as half i & 1.  c is the LARGEST value with 2 * cols * rows >= nt (the product is non-increasing in c);
 *     mi3d_atlas_cell returns it, 0 if T is out of range or even c = 4 does not hold nt triangles.
 *   - OWNERSHIP: local texel (x, y) of a cell, 0 <= x <= c, 0 <= y <= c - 1.  Half 0 owns x <= c - 1 and x + y <= c - 1,
 *     half 1 the rest: c (c + 1) / 2 texels each; half 1 is half 0 under the point reflection (x, y) -> (c - x, c - 1 - y),
 *     which keeps the winding.  Texels outside every cell (right and bottom margins), in cells past the last triangle and
 *     in the missing second half of an odd last triangle are owned by no one: owner -1, colour 0.
 *   - UV CORNERS: vertices 0, 1, 2 of half 0 sit at the CENTRES of local texels (0, 0), (c - 2, 0), (0, c - 2); half 1 at
 *     their reflections.  Global texel (X, Y) -> vt = ((X + 0.5) / T, 1 - (Y + 0.5) / T) in binary32, each operation
 *     rounded once (the reference's `1 - v` flip).  Three vt per triangle, unshared: vt index 3 i + k.  Every texel that
 *     bilinear filtering touches with non-zero weight at a point of the UV triangle lies in the triangle's own half.
 *   - TEXEL -> SURFACE POINT: (u, v) = the local coordinates, reflected for half 1; s = u / (c - 2), t = v / (c - 2);
 *     p = (A + s * (B - A)) + t * (C - A) per coordinate with A, B, C the triangle's vertices 0, 1, 2 - every operation a
 *     separately rounded binary32 one in this order, no fused multiply-add - then clamped to [-1, 1] (the extraction's
 *     box).  s, t and s + t pass 1 by up to one texel in the gutter: the intended extrapolation.
 *   - SUPERSAMPLING: ssaa in {1, 2, 4}.  Sub-sample (i, j) of a texel uses u + ((i + 0.5) / ssaa - 0.5) and likewise v with
 *     j (exact in binary32) in place of u and v; the texel's ssaa^2 samples are stored consecutively, index j * ssaa + i.
 *     The texel's colour is the binary32 sum of its samples' albedos in that order, times 1 / ssaa^2.
 *   - QUANTISATION: min(255, floor(a * 255)) in binary32 (the reference's `(feats * 255).astype(np.uint8)`); a negative
 *     or NaN value gives 0.
 *
 *   mi3d_atlas_cell       host only: c for nt triangles in a T x T texture, or 0
 *   mi3d_atlas_uv         vt float[3 nt][2]
 *   mi3d_atlas_positions  the band of image rows [row0, row0 + rows), rows >= 1, row0 + rows <= T:
 *                         xyz float[rows * T * ssaa^2][3] (zeros for a texel no one owns) and, unless NULL,
 *                         owner int32[rows * T] (triangle index or -1).  vertices float[nv][3], triangles int32[nt][3].
 *                         A triangle with an index outside [0, nv) is never dereferenced: it owns nothing and is COUNTED
 *                         in *bad (device uint64, 8-byte aligned, zeroed by the caller, added to by the band that holds
 *                         the texel of its vertex 0) - the convention counts[2] of Part 8 set.
 *   mi3d_texture_pack     albedo float[rows * T * ssaa^2][3] in the sample order above, owner int32[rows * T] ->
 *                         image uint8[rows][T][3] (RGB, 4-byte aligned): the mean, the quantisation, 0 where owner < 0.
 *                         Written as whole 32-bit words, four texels to three words; only the last one to three texels
 *                         of a band whose texel count is no multiple of four are written as bytes.
 * nt in [1, 2^31 - 1] and a (nt, T) pair with c = 0 are refused (hipErrorInvalidValue), as is every NULL pointer other
 * than `owner` of mi3d_atlas_positions. */
uint32_t mi3d_atlas_cell(unsigned long long nt, uint32_t T);
int mi3d_atlas_uv(unsigned long long nt, uint32_t T, float *vt, void *stream);
int mi3d_atlas_positions(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         uint32_t T, uint32_t ssaa, uint32_t row0, uint32_t rows, float *xyz, int32_t *owner,
                         unsigned long long *bad, void *stream);
int mi3d_texture_pack(const float *albedo, const int32_t *owner, uint32_t T, uint32_t ssaa, uint32_t rows, uint8_t *image,
                      void *stream);

/* ------------------------------------------------------------------ Part 10: GroupNorm (+ SiLU) of the diffusion half */

/* group_norm, optionally followed by SiLU, on binary16 tensors with fp32 arithmetic in registers: what the guidance
 * networks (mi3d/sd_standin.py) compute around every convolution, where stock PyTorch under autocast runs a chain of
 * fp32 kernels (cast, statistics, multiply-add, silu, cast back).  Added under ABI version 5: new symbols only.
 *
 *   - LAYOUT: x, y, dy, dx are binary16 [B][C][HW], contiguous; G divides C; group g of a sample is its channels
 *     [g C/G, (g + 1) C/G), a contiguous span of C/G * HW elements, at most 2^24.  weight, bias float[C];
 *     mean, rstd float[B][G].
 *   - CHUNKS: every (sample, channel) row of HW elements is cut into Sc = mi3d_groupnorm_chunks(HW) chunks; one workgroup
 *     owns one (row, chunk), index (b * C + c) * Sc + k.  The caller allocates the per-chunk workspaces:
 *     ws float[B * C * Sc][3] = (count, mean, M2) and partial float[B * C * Sc][2] = (sum dz, sum dz * x).
 *   - FORWARD, two launches: mi3d_groupnorm_stats fills ws (Chan's merge throughout, never sum-of-squares minus
 *     square-of-sum); mi3d_groupnorm_act_forward merges each group's triples itself, stores mean and
 *     rstd = 1 / sqrt(M2 / n + eps), and writes y = act(x a_c + b_c), a_c = rstd weight_c, b_c = bias_c - mean a_c,
 *     rounded once to binary16.  act 0 = identity, 1 = silu(z) = z / (1 + exp(-z)).
 *   - BACKWARD, input gradient only, two launches: with z recomputed and dz = dy act'(z),
 *     mi3d_groupnorm_act_backward_sums fills partial; mi3d_groupnorm_act_backward merges each group's sums into
 *     ds = sum_c weight_c sum dz x, db = sum_c weight_c sum dz and writes dx = rstd weight_c dz + c2 x + c3 with
 *     c2 = (db mean - ds) rstd^3 / n, c3 = -c2 mean - db rstd / n (n = C/G * HW): ATen's formula.
 *   - No atomics, fixed reduction orders: bit-reproducible.  No entry point synchronises, allocates or queries the device,
 *     so all of them can be captured into a hipGraph.  16-byte vector access where the pointers are 16-byte aligned, with
 *     a scalar head and tail per chunk; any alignment of at least 2 bytes is accepted.
 * A zero dimension, G not dividing C, a group of more than 2^24 elements, act outside {0, 1} and every NULL pointer are
 * refused (hipErrorInvalidValue). */
uint32_t mi3d_groupnorm_chunks(uint32_t HW);
int mi3d_groupnorm_stats(const void *x, uint32_t B, uint32_t C, uint32_t HW, uint32_t G, float *ws, void *stream);
int mi3d_groupnorm_act_forward(const void *x, const float *ws, const float *weight, const float *bias, uint32_t B,
                               uint32_t C, uint32_t HW, uint32_t G, float eps, int act, void *y, float *mean, float *rstd,
                               void *stream);
int mi3d_groupnorm_act_backward_sums(const void *x, const void *dy, const float *mean, const float *rstd,
                                     const float *weight, const float *bias, uint32_t B, uint32_t C, uint32_t HW,
                                     uint32_t G, int act, float *partial, void *stream);
int mi3d_groupnorm_act_backward(const void *x, const void *dy, const float *mean, const float *rstd, const float *weight,
                                const float *bias, const float *partial, uint32_t B, uint32_t C, uint32_t HW, uint32_t G,
                                int act, void *dx, void *stream);

/* The same four steps for CHANNELS-LAST tensors: x, y, dy, dx binary16 [B][HW][C] with C contiguous (what PyTorch calls
 * torch.channels_last), so that the convolutions around a GroupNorm can run in NHWC without a transpose.  Added under
 * ABI version 5: new symbols only.  The contract is that of the entry points above - binary16 in and out, fp32 in
 * registers, one rounding, Chan's merge (a thread adds one element at a time to its 8 channels' sets; sets are then united
 * by mean = sum n_i mean_i / n, M2 = sum M2_i + sum n_i (mean_i - mean)^2, or pairwise), ATen's dx formula, no atomics,
 * fixed orders, nothing that cannot be captured - with these differences:
 *   - C % 8 == 0 and lcm(C / G, 8) <= 2048; every tensor pointer 16-byte aligned: all access is by 16-byte vectors of 8
 *     channels of one pixel.  Anything else is refused.
 *   - SPANS: a sample's pixels are cut into Sc = mi3d_groupnorm_nhwc_spans(C, HW, G) spans of
 *     P = mi3d_groupnorm_nhwc_span(C, HW, G) whole pixels (the last one shorter); both return 0 for a shape that is
 *     refused.  One workgroup owns one (sample, span, slab of whole groups, at least 64 channels wide).  The workspaces
 *     hold one entry per (sample, span, group), index (b * Sc + k) * G + g: ws float[B * Sc * G][3] = (count, mean, M2),
 *     partial float[B * Sc * G][2] = (sum_c weight_c sum dz, sum_c weight_c sum dz (x - mean)) - weighted and centred,
 *     unlike above: dx = rstd weight_c dz + c2 (x - mean) - db rstd / n with c2 = -(ds - db mean) rstd^3 / n is ATen's
 *     dx = rstd weight_c dz + c2 x + c3 without its two large cancelling terms. */
uint32_t mi3d_groupnorm_nhwc_span(uint32_t C, uint32_t HW, uint32_t G);
uint32_t mi3d_groupnorm_nhwc_spans(uint32_t C, uint32_t HW, uint32_t G);
int mi3d_groupnorm_nhwc_stats(const void *x, uint32_t B, uint32_t C, uint32_t HW, uint32_t G, float *ws, void *stream);
int mi3d_groupnorm_nhwc_act_forward(const void *x, const float *ws, const float *weight, const float *bias, uint32_t B,
                                    uint32_t C, uint32_t HW, uint32_t G, float eps, int act, void *y, float *mean,
                                    float *rstd, void *stream);
int mi3d_groupnorm_nhwc_act_backward_sums(const void *x, const void *dy, const float *mean, const float *rstd,
                                          const float *weight, const float *bias, uint32_t B, uint32_t C, uint32_t HW,
                                          uint32_t G, int act, float *partial, void *stream);
int mi3d_groupnorm_nhwc_act_backward(const void *x, const void *dy, const float *mean, const float *rstd,
                                     const float *weight, const float *bias, const float *partial, uint32_t B, uint32_t C,
                                     uint32_t HW, uint32_t G, int act, void *dx, void *stream);

/* ------------------------------------------------------------------ Part 12: the Canny depth-edge detector */

/* The edge detector of the reference's load_views (nerf/refine_utils.py:386-393: `cv2.Canny(uint8 depth, 10, 10)`, dilated
 * and removed from a novel view's mask, so that the "flying" pixels of a depth discontinuity never become points).  Added
 * under ABI version 5: new symbols only.  (Declared ahead of the point-cloud part it serves: tests/test_pointcloud_cpu.py
 * reads that part as the tail of this header.)
 *
 * STANDING.  The arithmetic below is OpenCV's `Canny(image, t1, t2)` with apertureSize = 3 and L2gradient = False,
 * RESTATED FROM MEMORY: cv2 is on no machine this project builds or runs on.  The contract is therefore this project's
 * own and parity with cv2 is UNPINNED - the standing of mi3d_box_morph's border, of mcubes and of xatlas.
 *
 *   - SIZE: H, W >= 1 and H * W < 2^31.  image and cls are uint8[H][W], row-major.
 *   - THRESHOLDS: low = floor(t1), high = floor(t2) as int32 (the caller's floor); swapped here if low > high.
 *   - SOBEL, image borders replicated, all in integers:
 *       gx = (I[y-1][x+1] + 2 I[y][x+1] + I[y+1][x+1]) - (the same at x-1)
 *       gy = (I[y+1][x-1] + 2 I[y+1][x] + I[y+1][x+1]) - (the same at y-1)
 *       mag = |gx| + |gy| (at most 2040).  The magnitude of a position outside the image is 0.
 *   - DIRECTION: a pixel is a candidate iff mag > low.  ax = |gx|, ay = |gy| << 15, t22 = ax * 13573 (tan 22.5 deg in
 *     15 fractional bits), t67 = t22 + (ax << 16); with ax, |gy| <= 1020 every term is below 2^27: 32-bit arithmetic.
 *   - NON-MAXIMUM SUPPRESSION by sector:
 *       ay < t22 (horizontal gradient)  keep iff mag > mag[y][x-1] and mag >= mag[y][x+1]
 *       ay > t67 (vertical gradient)    keep iff mag > mag[y-1][x] and mag >= mag[y+1][x]
 *       otherwise (diagonal)            (gx ^ gy) >= 0: keep iff mag > mag[y-1][x-1] and mag > mag[y+1][x+1]
 *                                       else:           keep iff mag > mag[y-1][x+1] and mag > mag[y+1][x-1]
 *   - CLASSES: a kept pixel is strong (2) if mag > high, else weak (1); everything else is 0.
 *   - HYSTERESIS: a weak pixel with a strong 8-neighbour becomes strong, to the fixed point.  Promotion is monotone
 *     (1 -> 2 only), so the fixed point is unique: the weak pixels 8-connected to a strong one through weak pixels.
 *   - FINAL EDGE MAP (the caller's): 255 where cls == 2 after hysteresis, else 0.
 *
 *   mi3d_canny_classify    one launch: Sobel, magnitude, non-maximum suppression and the double threshold, from a
 *                          32 x 32 image tile with its 2-pixel halo in LDS (a decision needs the magnitudes of the 8
 *                          neighbours).  counts (device uint64[2], 8-byte aligned) is zeroed in-stream and receives
 *                          {weak, strong}.  image != cls.
 *   mi3d_canny_hysteresis  `sweeps` >= 1 sweeps over cls, in place, in-stream.  In a sweep every workgroup loads its tile
 *                          of cls with a 1-pixel halo, promotes until the tile is stable and writes its promoted pixels
 *                          back.  No workgroup waits on another (no grid barrier, no cooperative launch); a tile reads
 *                          its neighbours' pixels in whatever state of the ascent they are in, which changes how many
 *                          sweeps are needed and never the fixed point.  After the call changed[0] (device int32) != 0
 *                          iff the call's FINAL sweep promoted at least one pixel; the host repeats the call until it
 *                          is 0.  H * W sweeps always suffice.
 * No entry point allocates or synchronises.  A NULL pointer, a size out of range and sweeps = 0 are refused
 * (hipErrorInvalidValue). */
int mi3d_canny_classify(const uint8_t *image, uint32_t H, uint32_t W, int32_t low, int32_t high, uint8_t *cls,
                        unsigned long long *counts, void *stream);
int mi3d_canny_hysteresis(uint8_t *cls, uint32_t H, uint32_t W, uint32_t sweeps, int32_t *changed, void *stream);

/* ------------------------------------------------------------------ Part 13: mesh components (mesh export) */

/* The connected components of an indexed triangle mesh (Part 8's output, or any other) and a filter that drops the small
 * ones - the islands a density field leaves above the threshold - with the bit-exact, order-preserving standing of
 * Part 8.  What the `clean_mesh` step (min_f / min_d, through pymeshlab) of projects of this family does on the CPU;
 * pymeshlab is on no machine this project builds on, so the semantics below are this project's own contract - PARITY
 * UNPINNED.  Added under ABI version 5: new symbols only.  (Declared ahead of the point-cloud part, like Part 12.)
 *
 * vertices float[nv][3], triangles int32[nt][3]; nv, nt <= 2^31 - 1.
 *   - CONNECTIVITY: two vertices are connected iff some triangle cites both; components are the transitive closure.  By
 *     shared vertex INDEX - not by position, not by shared edge: two surfaces that touch in one welded vertex are one
 *     component.  Duplicate and degenerate (a == b) triangles are legal: they count as faces and connect what they cite.
 *   - BAD INDICES: a triangle with an index outside [0, nv) connects nothing, is no face, is never emitted and never
 *     dereferenced; it is COUNTED in counts[2] - the convention counts[2] of Part 8 and `bad` of Part 9 set.
 *   - LABELS: label[v] (int32[nv]) = the smallest vertex index of v's component.  A vertex no triangle cites is its own
 *     component with zero faces.  The label does not depend on scheduling: two runs give byte-identical buffers.
 *   - PER COMPONENT, at the row of its label vertex L (label[L] == L); the rows of all other vertices hold 0:
 *       faces[L]   (uint32[nv]) the number of valid triangles whose FIRST index lies in the component;
 *       box_min[L], box_max[L] (float[nv][3]) per axis the smallest and largest coordinate of the component's vertices in
 *                  the order of the order-preserving integer image of binary32 (-0 below +0, infinities at the ends).  A
 *                  NaN coordinate is ignored; an axis on which the component has no other coordinate gets [0, 0].
 *   - DIAGONAL: d_c = box_max[c] - box_min[c] in binary32, a NaN d_c (both ends the same infinity) taken as 0;
 *     diag2 = dx*dx + dy*dy + dz*dz in binary32, each operation rounded once, left to right, no fused multiply-add.  A
 *     component without a finite coordinate has diag2 = 0; one that reaches an infinity from elsewhere has diag2 = +inf.
 *   - KEEP RULE (min_faces >= 0, min_diagonal >= 0 and not NaN, largest): a component is kept iff faces >= 1 and
 *     faces >= min_faces and diag2 >= min_diagonal * min_diagonal (that product one binary32 multiply).  Equality
 *     keeps.  With `largest` it must ALSO be the component with the most faces, ties going to the smaller label: if the
 *     thresholds exclude that one, nothing is kept.
 *   - OUTPUT: the kept vertices and the kept triangles in their ORIGINAL RELATIVE ORDER (stable compaction: per-workgroup
 *     counts, an exclusive scan, an emit - no atomic appends), vertex rows copied bit for bit, triangle indices renumbered;
 *     vertex_map int32[nv] = the new index of every old vertex, -1 for a dropped one.
 *   - counts (device uint64[8], 8-byte aligned): [0] kept vertices, [1] kept triangles, [2] bad triangles, [3] threads
 *     that GAVE UP, [4] (faces << 32) | ~label of the largest component (0: no component has a face), [5] components
 *     with at least one face, [6] elements mi3d_mesh_clean_emit could not place, [7] 0.
 *   - GIVING UP: the labelling is a lock-free union-find whose parents only ever decrease (parent[v] <= v), so every
 *     loop walks a strictly decreasing chain and no correct execution takes more than nv + 1 steps per chain.  No wave
 *     waits for another.  A thread that exceeds the bound adds to counts[3] and leaves: a non-zero counts[3] means the
 *     result is invalid - an error for the caller to raise, never a hang.
 *
 *   mi3d_mesh_components_workspace  host only: bytes of device scratch mi3d_mesh_clean_count / _emit need for a mesh of
 *                          this size (0 for nv = nt = 0 and for sizes out of range).  mi3d_mesh_components needs none:
 *                          it works inside its outputs.
 *   mi3d_mesh_components   label, faces, box_min, box_max as above; counts zeroed in-stream, then [2] .. [5] filled.
 *   mi3d_mesh_clean_count  the keep rule, per-workgroup counts and their scan -> ws; counts[0], counts[1] (and [6] = 0).
 *                          label .. counts as mi3d_mesh_components left them.  The caller reads counts ONCE here to size
 *                          the outputs and to see [2] and [3] - the only host read of a clean.
 *   mi3d_mesh_clean_emit   out_vertices float[nv_cap][3], out_triangles int32[nt_cap][3], vertex_map int32[nv].  Nothing
 *                          is written past the caps; what could not be placed is counted in counts[6].
 * components, count and emit of one clean go to the same stream, in this order, with the same mesh and ws.  No entry
 * point allocates or synchronises.  nv = nt = 0 launches nothing and succeeds (counts is not touched); nt = 0 or nv = 0
 * alone is served (every vertex its own faceless component; every triangle bad).  Sizes out of range, a negative or NaN
 * min_diagonal, a workspace that is too small or not 8-byte aligned and every NULL pointer that would be dereferenced
 * are refused (hipErrorInvalidValue) and launch nothing. */
size_t mi3d_mesh_components_workspace(unsigned long long nv, unsigned long long nt);
int mi3d_mesh_components(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         int32_t *label, uint32_t *faces, float *box_min, float *box_max, unsigned long long *counts,
                         void *stream);
int mi3d_mesh_clean_count(const int32_t *triangles, unsigned long long nv, unsigned long long nt, const int32_t *label,
                          const uint32_t *faces, const float *box_min, const float *box_max, uint32_t min_faces,
                          float min_diagonal, int largest, void *ws, size_t ws_bytes, unsigned long long *counts,
                          void *stream);
int mi3d_mesh_clean_emit(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         const int32_t *label, void *ws, size_t ws_bytes, unsigned long long *counts, float *out_vertices,
                         unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap, int32_t *vertex_map,
                         void *stream);

/* ------------------------------------------------------------------ Part 14: mesh simplification (mesh export) */

/* Vertex clustering (Rossignac-Borrel) of an indexed triangle mesh: every vertex falls into a cell of a uniform lattice,
 * the vertices of a cell become one vertex at their mean position, triangles that lose a corner or repeat another are
 * dropped.  One pass over the vertices and one over the triangles; integer atomics only, so the result does not depend on
 * scheduling: two runs give byte-identical buffers, and a NumPy restatement gives the same bytes.  Projects of this
 * family expose decimation as a target face count through pymeshlab's edge collapse, which is on no machine this project
 * builds on: the semantics below are this project's own contract - PARITY UNPINNED.  Added under ABI version 5: new
 * symbols only.  (Declared ahead of the point-cloud part, like Parts 12 and 13.)
 *
 * vertices float[nv][3], triangles int32[nt][3]; nv, nt <= 2^31 - 1.  The lattice: origin_host = 3 floats o (a HOST
 * pointer read during the call, all finite) and cell (finite, > 0).
 *   - CLUSTER of a vertex, per axis: g = (v - o) / cell, a binary32 subtraction and a binary32 division, each rounded on
 *     its own; c = floorf(g) clamped to [-2^30, 2^30 - 1], an int32.  The cluster is the triple c.  A vertex with a
 *     non-finite coordinate joins NO cluster and is counted in counts[4].
 *   - LEADER of a cluster: the smallest vertex index in it.  Found with an open-addressing table whose slots hold a
 *     vertex index (-1: empty): atomicCAS claims an empty slot; a thread that meets an occupied slot recomputes the
 *     cluster of the vertex stored there from the read-only input and, if it equals its own, lowers the slot by atomicMin
 *     and is done, else probes the next slot.  A slot is only ever replaced by a vertex of the same cluster: its key
 *     never changes.  No key is packed; the clamp is the only limit on c.  The hash function is not part of the contract.
 *   - POSITION of a cluster: per member and axis f = g - (float)c in binary32, taken into [0, 1] (this moves nothing
 *     unless c was clamped), q = (int64)floorf(f * 2^20).  S = sum of q and n = the member count are accumulated in the
 *     leader's row by 64-bit integer atomics.  The new coordinate is (float)(o + cell * (c + (S / n) * 2^-20)) with o,
 *     cell, c, S, n converted to binary64, every operation a separately rounded binary64 one (no fused multiply-add) and
 *     ONE final rounding to binary32.  It does not depend on the order in which the atomics land.  It lies in the
 *     cluster's cell (up to that final rounding), not on the original surface.
 *   - TRIANGLES: every corner is replaced by its cluster.  A triangle with an index outside [0, nv) is never
 *     dereferenced; it and a triangle that cites a vertex without a cluster are COUNTED in counts[2] and dropped.  A
 *     triangle with two corners in one cluster is DEGENERATE: dropped, counts[6].  Two triangles are DUPLICATES iff their
 *     three clusters are the same SET, whatever the orientation: of each such set the smallest triangle index survives,
 *     with its own corner order; the others are dropped, counts[7].  Found with a second table of the same kind: a slot
 *     holds a triangle index, its key is re-derived from the leaders of the stored triangle's corners, atomicMin on
 *     equal keys.
 *   - OUTPUT: a cluster is emitted iff a surviving triangle cites it; the emitted clusters in ascending order of their
 *     LEADER index, the surviving triangles in ascending original index, renumbered (stable compaction: per-workgroup
 *     counts, an exclusive scan, an emit - no atomic appends).  vertex_map int32[nv] = the new index of every old
 *     vertex's cluster, -1 if the cluster was not emitted or the vertex has none.
 *   - counts (device uint64[8], 8-byte aligned): [0] emitted vertices kv, [1] surviving triangles kt, [2] bad triangles,
 *     [3] threads that GAVE UP, [4] non-finite vertices, [5] clusters (before the uncited ones are dropped),
 *     [6] degenerate triangles, [7] duplicate triangles.  kt + counts[6] + counts[7] + counts[2] == nt always.
 *   - GIVING UP: every probe sequence ends after at most `capacity` steps; no thread waits for another.  A thread that
 *     runs out adds to counts[3] and leaves: a non-zero counts[3] means the result is invalid - an error for the caller
 *     to raise, never a hang.
 *   - NON-MANIFOLD OUTPUT: clustering can join sheets that did not touch: edges with more than two triangles and
 *     vertices whose triangles form more than one fan are legal output.  Nothing repairs them.
 *
 *   mi3d_mesh_simplify_workspace  host only: bytes of device scratch for a mesh of this size (0 for nv = nt = 0 and for
 *                          sizes out of range).  tight = 0: the recommended size, table capacities = twice the smallest
 *                          power of two above the element count (at most 2^31), a load below one half; tight != 0: the
 *                          minimum, capacities = the smallest power of two above the element count.  A call uses the
 *                          recommended capacities if ws_bytes holds them, else the tight ones: the largest powers of two
 *                          that fit.  The result does not depend on the capacity.
 *   mi3d_mesh_simplify_count   everything above but the output buffers: tables and accumulators initialised in-stream,
 *                          counts zeroed in-stream and filled.  The caller reads counts ONCE here to size the outputs and
 *                          to see [2], [3] and [4] - the only host read of a simplification.  Called alone it answers
 *                          "how many faces would this cell leave".
 *   mi3d_mesh_simplify_emit    out_vertices float[nv_cap][3], out_triangles int32[nt_cap][3], vertex_map int32[nv].
 *                          Nothing is written past the caps; what could not be placed is counted in *lost (device
 *                          uint64, 8-byte aligned, zeroed in-stream).
 * count and emit of one simplification go to the same stream, in this order, with the same mesh, lattice, ws and
 * ws_bytes.  No entry point allocates or synchronises.  nv = nt = 0 launches nothing and succeeds; nt = 0 or nv = 0 alone
 * is served (nothing is emitted; every triangle is bad).  Sizes out of range, a cell that is not finite and > 0, a
 * non-finite origin, a workspace below the tight size or not 8-byte aligned and every NULL pointer that would be
 * dereferenced are refused (hipErrorInvalidValue) and launch nothing. */
size_t mi3d_mesh_simplify_workspace(unsigned long long nv, unsigned long long nt, int tight);
int mi3d_mesh_simplify_count(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             const float *origin_host, float cell, void *ws, size_t ws_bytes, unsigned long long *counts,
                             void *stream);
int mi3d_mesh_simplify_emit(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                            const float *origin_host, float cell, void *ws, size_t ws_bytes, float *out_vertices,
                            unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap,
                            int32_t *vertex_map, unsigned long long *lost, void *stream);

/* ------------------------------------------------------------------ Part 15: texturing from views (mesh export) */

/* Projective texturing of Part 9's atlas: a depth map of the mesh per view, and per atlas sample a visibility-tested,
 * angle-weighted mean of the views' colours.  The reference bakes the field only (nerf/renderer.py:193-299); this
 * contract is this project's own - PARITY UNPINNED, the standing of Parts 8, 9, 13 and 14.  Added under ABI version 5:
 * new symbols only.  (Declared ahead of the point-cloud part, like Parts 12 to 14.)
 *
 * ARITHMETIC.  Everything is binary32, every operation rounded separately (no fused multiply-add), three-term sums in
 * index order k = 0, 1, 2 as ((t0 + t1) + t2), a translation added last.  No sqrt, no transcendental function: cosines
 * enter as squares.  A NumPy float32 restatement gives the same bits.
 *   - VIEWS: V in [1, 64] views of one size H x W, each in [2, 16384].  views float[V][24], one record per view:
 *     [0..8] R row-major and [9..11] t of the world-to-camera matrix [R | t]; [12..20] K row-major (last row 0 0 1);
 *     [21..23] the camera centre (the translation column of c2w).  The caller inverts c2w in binary64 and rounds once.
 *   - PROJECTION of a point p: cam_r = ((R_r0 p0 + R_r1 p1) + R_r2 p2) + t_r; q_r = (K_r0 cam0 + K_r1 cam1) + K_r2 cam2;
 *     x = q0 / q2, y = q1 / q2, z = q2.  Pixel (i, j) - column i of row j - has its centre at (i + 0.5, j + 0.5).
 *
 * DEPTH MAP (mi3d_mesh_depth): depth float[V][H][W], +inf where nothing is drawn; counts uint64[2], 8-byte aligned,
 * zeroed in-stream.  One fill launch, then one launch with thread = (triangle, view).
 *   - A triangle with an index outside [0, nv) is never dereferenced; it is COUNTED in counts[0], once (not per view).
 *   - A triangle with a vertex whose z <= 0, or whose x, y or z is not finite, is not drawn in that view and COUNTED in
 *     counts[1], once per view.  Nothing is clipped at a near plane.
 *   - The thread walks the pixel centres of the bounding box: columns max(ceil(min x - 0.5), 0) .. min(floor(max x -
 *     0.5), W - 1), rows likewise; at most H W iterations.
 *   - EDGE FUNCTION of the directed edge a -> b at a centre P, for vertex indices ia <= ib:
 *     E = (xb - xa) (Py - ya) - (yb - ya) (Px - xa); for ia > ib the endpoints swap and E is negated (the WATERTIGHT
 *     rule: two triangles sharing an edge by index see exactly opposite values).  w0, w1, w2 = the edges 1 -> 2, 2 -> 0,
 *     0 -> 1.  s = (w0 + w1) + w2.  The pixel is covered iff (all w >= 0 or all w <= 0) and s != 0.  No back-face
 *     culling.
 *   - DEPTH: d = 1 / (((w0 / s) / z0 + (w1 / s) / z1) + (w2 / s) / z2); written iff 0 < d < inf, by atomicMin on its
 *     uint32 bits (positive floats order like their bits): order-independent, two runs give identical bytes.
 *
 * PROJECTION OF THE VIEWS (mi3d_texture_project): thread = texel of a band of `rows` image rows, the mapping of
 * mi3d_atlas_positions, whose xyz float[rows T ssaa^2][3] and owner int32[rows T] it reads.  N = (B - A) x (C - A) of
 * the owner triangle: e1 = B - A, e2 = C - A, N = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x),
 * nn = (Nx Nx + Ny Ny) + Nz Nz.  For each sample p and v = 0 .. V - 1 in order, view v CONTRIBUTES iff
 *   (a) z > 0;
 *   (b) 0.5 <= x <= W - 0.5 and 0.5 <= y <= H - 0.5; gx = x - 0.5, i0 = min(floor(gx), W - 2), fx = gx - i0; the
 *       same in y (gy, j0, fy); the four taps are (i0 + a, j0 + b), a, b in {0, 1};
 *   (c) all four depth taps are finite and z <= min(min(d00, d10), min(d01, d11)) + depth_tol  (d_ab at (i0+a, j0+b));
 *   (d) with masks uint8[V][H][W]: all four mask taps are non-zero;
 *   (e) with d = centre - p: nd = (Nx dx + Ny dy) + Nz dz > 0, dd = (dx dx + dy dy) + dz dz,
 *       cos2 = (nd nd) / (nn dd) >= min_cos2.
 * Its weight is w = weights[v] * cos2^(power / 2), power in {2, 4, 8, 16}, by power / 2 = 1, 2, 4, 8 -> 0 .. 3
 * squarings of cos2.  Its colour per channel, images float[V][H][W][3]: hx = 1 - fx, hy = 1 - fy,
 * top = c00 hx + c10 fx, bot = c01 hx + c11 fx, c = top hy + bot fy.  sw = sw + w and sc = sc + w c in view order from 0.
 * Output per sample: colour = sc / sw if sw > 0 else base[sample] (base float[rows T ssaa^2][3], the layout
 * mi3d_texture_pack reads); hits uint8 = the number of contributing views (a view of weight 0 counts).  nn == 0 (a
 * degenerate triangle), a non-finite nn and owner < 0 contribute nothing: base, hits 0.  An owner or a vertex index out
 * of range is never dereferenced (treated like owner < 0).  No atomics: two runs give identical bytes.
 *
 * ERROR AGAINST EXACT ARITHMETIC (what tests/test_texture_views_cpu.py counts; u = 2^-24): a component of cam passes 4
 * roundings, one of q 4 more, x and y one more each; an edge function 2 subtractions per factor, 2 products and a
 * subtraction on top of its inputs' errors; N 3 per component on top of the 1 of each edge vector; nd and dd 3 more.
 * The test propagates these as first-order running bounds and leaves a sample out whose comparison in (b), (c) or (e)
 * lies within twice the bound.
 *
 * No entry point allocates or synchronises.  A NULL pointer other than `masks`, V outside [1, 64], H or W outside
 * [2, 16384], T or ssaa outside Part 9's ranges, rows outside [1, T], a power outside the set, a min_cos2 outside
 * [0, 1] and a depth_tol that is negative or not finite are refused (hipErrorInvalidValue) and launch nothing.
 * mi3d_mesh_depth accepts nt = 0 (the fill alone). */
int mi3d_mesh_depth(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                    const float *views, uint32_t V, uint32_t H, uint32_t W, float *depth, unsigned long long *counts,
                    void *stream);
int mi3d_texture_project(const float *xyz, const int32_t *owner, const float *vertices, unsigned long long nv,
                         const int32_t *triangles, unsigned long long nt, uint32_t T, uint32_t ssaa, uint32_t rows,
                         const float *views, uint32_t V, uint32_t H, uint32_t W, const float *depth, const float *images,
                         const uint8_t *masks, const float *weights, uint32_t power, float min_cos2, float depth_tol,
                         const float *base, float *colour, uint8_t *hits, void *stream);

/* ------------------------------------------------------------------ Part 16: Taubin smoothing (mesh export) */

/* Taubin's lambda | mu smoothing of the vertices of an indexed triangle mesh: every iteration moves each vertex towards
 * the mean of its umbrella by the factor lambda, then by the factor mu (negative: back out), which removes the
 * voxel-scale bumps of a marching-cubes surface and the stair steps of Part 14 without the shrinkage of plain Laplacian
 * smoothing.  The neighbour sums are fixed-point integers, so the result does not depend on the order in which a row
 * of neighbours is stored or walked: two runs give byte-identical buffers, and a NumPy restatement gives the same
 * bytes.  Projects of this family smooth through pymeshlab, which is on no machine this project builds on: the
 * semantics below are this project's own contract - PARITY UNPINNED, the standing of Parts 13 and 14.  Added under
 * ABI version 5: new symbols only.  (Declared ahead of the point-cloud part, like Parts 12 to 15.)
 *
 * vertices float[nv][3], triangles int32[nt][3]; nv <= 2^31 - 1, nt <= 2^30 (a row offset is a uint32 below 3 nt).
 * iterations in [1, 1000]; lambda and mu binary64, finite, in [-1, 1]; pin_border a flag; max_move binary32, >= 0,
 * +infinity for "no clamp"; e = fraction_bits in [0, 40].
 *   - USABLE TRIANGLES: a triangle is usable iff its three indices lie in [0, nv), are pairwise distinct and name
 *     vertices whose three coordinates are finite IN THE INPUT.  The others are never dereferenced past the index check;
 *     they are COUNTED in counts[0] and take no part in anything below.
 *   - UMBRELLA of vertex i: for every usable triangle that cites i, the positions of its two other corners, each with
 *     weight 1 - a neighbour across an interior edge of a manifold enters twice, once per triangle, which on a closed
 *     manifold is the uniform umbrella.  deg(i) = the number of usable triangles that cite i; w = 2 deg(i).  No edge
 *     table is built.
 *   - EXACT SUMS: a neighbour's coordinate p enters as the integer q: with x = (double)p * 2^e (exact), q = 2^40 if
 *     x >= 2^40, -2^40 if x <= -2^40, 0 if x is NaN, else llrint(x) (to nearest, ties to even).  S (per axis) = the sum
 *     of q over the umbrella and w are 64-bit integers.  |S| <= 2 deg 2^40, so neither can overflow for any degree
 *     below 2^22.  The limit that applies is lower, MI3D_SMOOTH_MAX_DEGREE = 1024, because the border rule below costs
 *     deg^2 comparisons: a vertex with deg > 1024 is PINNED whatever pin_border says, its row is never walked, and it
 *     is COUNTED in counts[4].  (Marching cubes gives degrees up to about 12, clustering a few dozen; one thread took about
 *     2.8 s for the border rule of a vertex of degree 4096 on an MI355X, hence 1024: a sixteenth of that.)
 *   - ONE PASS with factor k, per vertex and axis: m = ((double)S / (double)w) * 2^-e, then
 *     p' = (float)((double)p + k * (m - (double)p)): a division, a multiplication by a power of two, a subtraction, a
 *     multiplication and an addition, every one a separately rounded binary64 operation (no fused multiply-add), and
 *     ONE final rounding to binary32.  Every vertex of a pass reads the positions from BEFORE the pass (Jacobi: two
 *     buffers, plain stores).  A vertex with w = 0 stays where it is, bit for bit, and so does a pinned one and one
 *     that is not finite in the input.  A pass with k == 0 is not launched.
 *   - ONE ITERATION: a pass with lambda, then a pass with mu.  lambda = mu = 0 copies the input.
 *   - BORDER: with pin_border != 0 a vertex is pinned iff it shares exactly ONE usable triangle with some neighbour -
 *     it lies on an open edge.  An edge with three or more triangles (clustering produces them) pins nothing.  The
 *     flags are computed once, from the connectivity alone.
 *   - MAX_MOVE: after every pass each coordinate p' of a vertex that moved is clamped to [lo, hi], lo = p0 - max_move
 *     and hi = p0 + max_move, p0 the INPUT coordinate, both binary32 operations: lo if p' < lo, else hi if p' > hi,
 *     else p'.  A box: no sqrt.  It keeps the smoothed surface within a stated distance of the isosurface.
 *   - OUTPUT: out_vertices float[nv][3]; the triangles are not touched.  out_vertices must not alias vertices.
 *   - counts (device uint64[8], 8-byte aligned, zeroed in-stream): [0] unusable triangles, [1] non-finite vertices,
 *     [2] vertices no usable triangle cites (w = 0; every non-finite vertex is one), [3] vertices pinned as border (0
 *     without pin_border), [4] vertices above the degree limit, [5] vertices of which the clamp changed a coordinate
 *     in the LAST pass launched, [6] row slots that could not be placed - an inconsistency: non-zero means the result
 *     is invalid, an error for the caller to raise - [7] 0.
 *   - HOW: the vertex -> triangle incidence is built ONCE: the degree of every vertex by int32 atomics (thread =
 *     triangle), an exclusive scan (per-workgroup sums, one workgroup scans them, an offsets pass), and a fill in which
 *     a triangle claims a slot of each corner's row by an atomic cursor and stores the pair of its other corners.  The
 *     order inside a row depends on scheduling; nothing above does.  Then the border flags (thread = vertex: for each
 *     entry of the row, the number of entries that name the same neighbour) and 2 x iterations passes (thread =
 *     vertex) without any atomic.  Every loop is bounded by a row length; no thread waits for another.
 *
 *   mi3d_mesh_smooth_workspace  host only: bytes of device scratch for a mesh of this size (0 for nv = 0 and for sizes
 *                          out of range): the cursors, the row offsets, the scan's block sums, the flags, the second
 *                          vertex buffer and 3 nt rows of two int32.
 *   mi3d_mesh_smooth       everything above on `stream`.  The caller MAY read counts afterwards; nothing needs to be read.
 * No entry point allocates or synchronises.  nv = 0 launches nothing and succeeds (counts is not touched).  Sizes,
 * iterations or fraction_bits out of range, a lambda or mu that is not finite or outside [-1, 1], a max_move that is
 * negative or NaN, out_vertices == vertices, a workspace that is too small or not 8-byte aligned, a counts that is not
 * 8-byte aligned and every NULL pointer that would be dereferenced are refused (hipErrorInvalidValue) and launch
 * nothing. */
#define MI3D_SMOOTH_MAX_DEGREE 1024
size_t mi3d_mesh_smooth_workspace(unsigned long long nv, unsigned long long nt);
int mi3d_mesh_smooth(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                     uint32_t iterations, double lambda, double mu, int pin_border, float max_move,
                     uint32_t fraction_bits, void *ws, size_t ws_bytes, float *out_vertices, unsigned long long *counts,
                     void *stream);

/* ------------------------------------------------------------------ Part 17: rendering the mesh (mesh export) */

/* A rasteriser for the exported mesh: per view the nearest triangle at every pixel centre (a visibility buffer), and a
 * shading pass that turns it into an image from vertex colours or from Part 9's atlas and its 8-bit texture - the
 * forward half of what nvdiffrast does for the reference's export, there in UV space only (nerf/renderer.py:193-299);
 * what an external viewer shows of mesh.obj, mesh.mtl and albedo.png.  This contract is this project's own - PARITY
 * UNPINNED, the standing of Parts 8, 9 and 13 to 16.  Added under ABI version 5: new symbols only.  (Declared ahead of
 * the point-cloud part, like Parts 12 to 16.)
 *
 * ARITHMETIC: Part 15's rules - binary32, every operation rounded separately, three-term sums ((t0 + t1) + t2), no
 * sqrt, no transcendental function; a NumPy float32 restatement gives the same bits.  Part 15's VIEWS records,
 * PROJECTION, pixel centres, bounding-box walk, EDGE FUNCTION, coverage test and DEPTH d are used as they stand there
 * (one definition in the source, shared with mi3d_mesh_depth).
 *
 * VISIBILITY (mi3d_mesh_visibility): vis uint64[V][H][W], 8-byte aligned; counts uint64[2] as mi3d_mesh_depth's ([0]
 * triangles with an index outside [0, nv), once; [1] (triangle, view) pairs left out for a z <= 0 or a non-finite
 * value), zeroed in-stream.  One fill launch writes all-ones; one launch with thread = (triangle, view) does, for
 * exactly the pixels and the d that mi3d_mesh_depth would write, an unsigned 64-bit atomicMin with the key
 * (bits(d) << 32) | triangle_index, its result unused.  0 < d < inf, so the upper word orders like the depth and never
 * is all-ones; EQUAL DEPTHS RESOLVE TO THE SMALLER TRIANGLE INDEX - a rule, not an accident.  Order-independent: two
 * runs give identical bytes.  The upper word of a key equals the bits mi3d_mesh_depth writes at that pixel.  nt <=
 * 2^31 - 1 (the index is also an int32 output below).
 *
 * SHADING (mi3d_mesh_shade): thread = pixel of [V][H][W]; no atomics: two runs give identical bytes.
 *   - A pixel whose key is all-ones gets image = background (HOST float[3], read when the call is made), alpha 0,
 *     depth +inf, tri -1, bary 0 0 0, normal 0 0 0.  So does a key whose triangle index is not below nt or whose
 *     triangle has a vertex index outside [0, nv): no pass above writes one, and it is never dereferenced.
 *   - Otherwise the triangle's three vertices are projected again and w0, w1, w2, s recomputed at the pixel centre - the
 *     operations of the visibility pass, so s != 0.  b_k = w_k / s, r_k = b_k / z_k, S = (r0 + r1) + r2, d = 1 / S (the
 *     bits of the key's upper word), lambda_k = r_k d: the perspective-correct weights.  An attribute a with the values
 *     a0, a1, a2 at the corners is ((lambda0 a0 + lambda1 a1) + lambda2 a2).
 *   - COLOUR, exactly one source: (a) colors float[nv][3], interpolated; (b) vt float[3 nt][2] (Part 9's unshared
 *     corners, vt index 3 i + k) with texture uint8[T][T][3] (row 0 the top row), T in [64, 16384]: (u, v) interpolated,
 *     gx = u T - 0.5, gy = (1 - v) T - 0.5 (the inverse of Part 9's vt = ((X + 0.5) / T, 1 - (Y + 0.5) / T)),
 *     i0 = min(max(floor(gx), 0), T - 2), fx = min(max(gx - i0, 0), 1) (a NaN gives 0 in both), the same in y (j0, fy);
 *     the taps c_ab at texel (i0 + a, j0 + b) converted to float; hx = 1 - fx, hy = 1 - fy, top = c00 hx + c10 fx,
 *     bot = c01 hx + c11 fx, c = top hy + bot fy (Part 15's blend); colour = c / 255.  No mip-mapping.
 *   - OUTPUTS: image float[V][H][W][3]; and, each written only if its pointer is not NULL, normal float[V][H][W][3] (vn
 *     float[nv][3] interpolated, NOT normalised; needs vn), depth float[V][H][W] (d), tri int32[V][H][W], bary
 *     float[V][H][W][3] (lambda), alpha uint8[V][H][W] (1 where a triangle is drawn).
 *
 * ERROR AGAINST EXACT ARITHMETIC (what tests/test_mesh_render_cpu.py counts; u = 2^-24), by Part 15's method: on top of
 * the bounds of w_k, s and d there, b_k has the relative error of w_k and s plus one rounding, r_k that of z_k plus one
 * more, lambda_k that of d plus one more; an interpolated attribute adds 3 u sum |lambda_k a_k| to
 * sum |a_k| E(lambda_k).  Out of scope: clipping at a near plane (Part 15's rule stands: a triangle with a corner at
 * z <= 0 is left out of the view), splitting a large triangle across threads, mip-mapping, gradients of positions and
 * cameras (Part 18 has those of the two colour sources).
 *
 * Neither entry point allocates or synchronises.  V, H, W outside Part 15's ranges, a T outside Part 9's with a texture,
 * nv or nt above 2^31 - 1, a vis or counts that is NULL or not 8-byte aligned, a NULL views, background or image, both
 * colour sources or neither, one of vt and texture without the other, a normal without vn, and NULL triangles (with
 * nt > 0) or vertices (with nt > 0 and nv > 0) are refused (hipErrorInvalidValue) and launch nothing.  nt = 0 is
 * accepted: the fill alone, and the background everywhere. */
int mi3d_mesh_visibility(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                         const float *views, uint32_t V, uint32_t H, uint32_t W, unsigned long long *vis,
                         unsigned long long *counts, void *stream);
int mi3d_mesh_shade(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                    const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                    const float *colors, const float *vt, const uint8_t *texture, uint32_t T, const float *vn,
                    const float *background, float *image, float *normal, float *depth, int32_t *tri, float *bary,
                    uint8_t *alpha, void *stream);

/* ------------------------------------------------------------------ Part 18: gradients of the mesh render's colours */

/* The shading pass of Part 17 with a float texture, and the adjoint of the shading pass in its colour source: what a
 * texture or a set of vertex colours needs to be fitted to views through the renderer that will show them.  VISIBILITY
 * AND GEOMETRY STAY FIXED: the keys of mi3d_mesh_visibility are an input, and nothing here differentiates the weights,
 * the projection or the coverage.  This contract is this project's own - PARITY UNPINNED.  Added under ABI version 5: new
 * symbols only.  (Declared ahead of the point-cloud part, like Parts 12 to 17.)
 *
 * FLOAT TEXTURE (mi3d_mesh_shade_f32): mi3d_mesh_shade with texture float[T][T][3]: the same kernel template, the same
 * operations in the same order up to c = top hy + bot fy, and colour = c itself (no / 255).  Every other argument, output
 * and refusal is Part 17's.
 *
 * THE PASS IS LINEAR IN ITS COLOUR SOURCE: image[p][ch] = sum_k w_k(p) source[a_k(p)][ch] for a drawn pixel p, with
 *   (a) by vertex: a_k = the triangle's vertex k, w_k = lambda_k, k = 0, 1, 2;
 *   (b) textured: the four taps (i0 + a, j0 + b), w00 = hx hy, w10 = fx hy, w01 = hx fy, w11 = fx fy, each product ONE
 *       binary32 operation; lambda, i0, j0, fx, fy, hx = 1 - fx, hy = 1 - fy exactly the values of Part 17 (one
 *       definition in the source, shared with the forward).  (The forward rounds top and bot before the last blend; the
 *       adjoint is that of the weights above - what exact arithmetic makes of the forward.)
 * So the adjoint needs no texture values, and one backward serves both texel types.
 *
 * BACKWARD (mi3d_mesh_shade_backward): dimage float[V][H][W][3] -> exactly one of grad_colors float[nv][3] and
 * grad_texture float[T][T][3] (the latter with vt and T as Part 17 takes them), every element written.  N = V H W.  A
 * fill (it zeroes the sums and the amax word) and three launches on `stream`:
 *   1. amax = the largest bits(|g|) over the 3 N entries of dimage, one unsigned atomicMax per workgroup.  Positive
 *      floats order like their bits, and a NaN's bits exceed infinity's: a non-finite entry wins by construction.
 *   2. thread = pixel.  Part 17's key test: an all-ones key, a triangle index not below nt and a triangle with a vertex
 *      index outside [0, nv) contribute nothing and are never dereferenced.  Otherwise, per weight w and channel ch:
 *      t = w * g[ch] (one binary32 operation), x = (double)t * 2^-e (exact), saturated to [-2^(61 - L), 2^(61 - L)] and
 *      0 for a NaN, q = llrint(x) (to nearest, ties to even); q is added to the int64 sum of element (a, ch) by a
 *      no-return 64-bit integer atomicAdd (a zero q is not sent).  Integer sums are exact: arrival order cannot change a
 *      bit, two runs give identical bytes, and a NumPy restatement gives the same bytes.
 *   3. thread = element: grad = (float)((double)sum * 2^e): one rounding to binary64 (a sum can exceed 2^53), one to
 *      binary32.
 *   - THE EXPONENT e is the same for every thread: E = (bits(amax) >> 23) - 127, so that 2^(E + 1) > amax (denormals
 *     included); L = the smallest integer with 2^L >= N; e = (E + 1) + L - 60.  HEADROOM: a weight is at most 1 plus a few
 *     ulp, so |x| < 2^(60 - L) (1 + 2^-20), far inside the saturation bound, which therefore never acts on keys a
 *     visibility pass of this mesh wrote; a pixel adds to one sum at most 3 times (a triangle that names a vertex
 *     thrice), so |sum| <= 3 N 2^(61 - L) <= 3 x 2^61 < 2^63 whatever the keys hold.  RESOLUTION: one unit is
 *     2^e = 2^(E + 1) 2^(L - 60), so a contribution is off by at most 2^(e - 1) <= amax 2^(L - 60): 26 bits below amax at
 *     the largest N = 2^34, 40 and more at the sizes tests run at.
 *   - amax == 0 (dimage is all zeros): launch 2 leaves at once by a device-side test and every element is +0.
 *   - amax NOT FINITE (an infinity or a NaN anywhere in dimage): launch 2 leaves at once and EVERY element is a quiet
 *     NaN (bits 0x7FC00000).  A stated rule: a poisoned upstream gradient poisons the whole result.
 *   - An element no pixel contributes to is exactly +0.
 *
 *   mi3d_mesh_shade_backward_workspace  host only: bytes of device scratch for a gradient of `elements` floats (3 nv or
 *                          3 T^2): 8 (elements + 1) - the int64 sums and the amax word; 0 above 3 (2^31 - 1).
 * ERROR AGAINST EXACT ARITHMETIC (what tests/test_mesh_shade_grad_cpu.py counts; u = 2^-24), given the binary32 weights'
 * own error E(w) (Part 17's E(lambda); for a tap weight 2 u on top of the fractions'): a sum of n contributions is off by
 * at most sum (|g| E(w) + u |w g|) + n 2^(e - 1), and the result adds u |grad| (2^-53 for the binary64 step is below it).
 *
 * No entry point allocates or synchronises.  Refused (hipErrorInvalidValue), launching nothing: everything Part 17
 * refuses of the arguments the two share; a NULL dimage; both gradients or neither; vt without T or T without vt; vt
 * with grad_colors; grad_texture with a T outside Part 9's range; a workspace that is NULL, too small or not 8-byte
 * aligned.  nt = 0 is accepted (every element +0) and so is nv = 0 with grad_colors (nothing to write). */
int mi3d_mesh_shade_f32(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                        const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                        const float *colors, const float *vt, const float *texture, uint32_t T, const float *vn,
                        const float *background, float *image, float *normal, float *depth, int32_t *tri, float *bary,
                        uint8_t *alpha, void *stream);
size_t mi3d_mesh_shade_backward_workspace(unsigned long long elements);
int mi3d_mesh_shade_backward(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             const float *views, uint32_t V, uint32_t H, uint32_t W, const unsigned long long *vis,
                             const float *dimage, const float *vt, uint32_t T, float *grad_colors, float *grad_texture,
                             void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ Part 19: edge-collapse decimation (mesh export) */

/* Decimation of an indexed triangle mesh to a face count by quadric edge collapse (Garland and Heckbert, "Surface
 * simplification using quadric error metrics", SIGGRAPH 1997), in rounds of INDEPENDENT collapses.  Where Part 14
 * rounds every corner to a cluster mean, joins sheets closer than a cell and leaves a non-manifold mesh, a collapse
 * keeps a closed manifold closed and manifold, places the new vertex where the planes around it meet, and stops on the
 * face count asked for.  Integer atomics only; every binary64 operation is rounded separately (no fused multiply-add),
 * no sqrt: two runs give byte-identical buffers, and a restatement in Python floats (tests/mesh_collapse_model.py)
 * gives the same bytes.  Projects of this family decimate through pymeshlab, which is on no machine this project builds
 * on: the semantics below are this project's own contract - PARITY UNPINNED, the standing of Parts 13 to 16.  Added
 * under ABI version 5: new symbols only.  (Declared ahead of the point-cloud part, like Parts 12 to 18.)
 *
 * vertices float[nv][3], triangles int32[nt][3]; nv <= 2^31 - 1, nt <= 2^30 (a row slot and an edge id are uint32 below
 * 3 nt).  target_faces >= 0 (uint64); max_error binary32, >= 0, +infinity for none.
 *   - USABLE TRIANGLES: Part 16's rule (indices in [0, nv), pairwise distinct, three vertices finite in the input).
 *     The others are never dereferenced past the index check, are counted, and take no part.  The usable triangles are
 *     LIVE at the start.  A triangle keeps its input index t0 and its three corner slots for the whole run; a corner
 *     changes only by being renamed to the vertex its vertex was collapsed into.
 *   - QUADRICS, once: for a usable triangle with corners widened to binary64, n = (p1 - p0) x (p2 - p0) (u = p1 - p0,
 *     v = p2 - p0, n = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx)), s = n.n, d = -(n.p0), every dot product
 *     (x x' + y y') + z z'.  K = the ten products e_i e_j (i <= j) of e = (nx, ny, nz, d), each divided by s, in the
 *     order q = (A00, A01, A02, b0, A11, A12, b1, A22, b2, c).  s == 0 or a non-finite s: K contributes nothing, counted.
 *     Q_v = the sum of K_t over the usable triangles that cite v in ASCENDING triangle index, from +0.  A vertex cited
 *     by more than MI3D_COLLAPSE_MAX_ROW = 1024 usable triangles gets a quadric of NaNs instead (its row is not sorted;
 *     Part 16's reason): no edge at it ever has a cost.  A collapse sets Q_a <- Q_a + Q_b, entry by entry.
 *   - E(x) = x^T A x + 2 b^T x + c, evaluated as: t0 = (A00 x + A01 y) + A02 z, t1 = (A01 x + A11 y) + A12 z,
 *     t2 = (A02 x + A12 y) + A22 z, quad = (x t0 + y t1) + z t2, lin = (b0 x + b1 y) + b2 z, E = (quad + 2 lin) + c.
 *   - ROUNDS.  Everything below is recomputed every round from the live triangles.  deg v = the live triangles that
 *     cite v; N(v) = the other corners of those triangles.
 *   - LOCKS: a vertex is locked iff it lies on an edge that exactly ONE live triangle holds, or deg v >
 *     MI3D_COLLAPSE_MAX_DEGREE = 64.  A locked vertex neither moves nor disappears.
 *   - CANDIDATES: the directed edge a -> b with a < b, in live triangle t0 from corner slot i to slot (i + 1) mod 3, with
 *     c at the third slot, is a candidate iff all of: both ends are unlocked; exactly two live triangles hold the edge
 *     and the other one runs b -> a (d = its third corner); c != d and N(a) and N(b) share no vertex but c and d (the
 *     link condition); 3 <= deg a + deg b - 4 <= 64; deg c >= 4 and deg d >= 4; the placement below yields an x*; for
 *     every other live triangle at a or b, with that corner at x*, n_old . n_new > 0 and n_new . n_new > 0 (normals as
 *     above, in the triangle's own corner order, the other corners where they are); c32 = (float)max(E(x*), 0) <=
 *     max_error.
 *   - PLACEMENT with Q = Q_a + Q_b: the points p_a, p_b, m = (p_a + p_b) * 0.5 and - iff |det A| > 1e-3 ((tr tr) tr),
 *     tr = ((A00 + A11) + A22) / 3, det A != 0 and |o - m|^2 <= |p_b - p_a|^2 - the optimum o = -A^-1 b by the adjugate:
 *     c00 = A11 A22 - A12 A12, c01 = A02 A12 - A01 A22, c02 = A01 A12 - A02 A11, c11 = A00 A22 - A02 A02,
 *     c12 = A01 A02 - A00 A12, c22 = A00 A11 - A01 A01, det = (A00 c00 + A01 c01) + A02 c02,
 *     o = (-((c00 b0 + c01 b1) + c02 b2) / det, -((c01 b0 + c11 b1) + c12 b2) / det, -((c02 b0 + c12 b1) + c22 b2) / det).
 *     Each point is rounded ONCE to binary32 (m and o; the distance test uses them unrounded) and E is evaluated at the
 *     rounded point, so the cost is that of the vertex as stored.  The smallest E that is not NaN wins, ties to the
 *     earlier point in this order; no such E: no candidate.
 *   - KEY of a candidate in round r (r = the rounds that had a winner so far): upper word (bits(c32) & 0xFFF00000) | h,
 *     h = ((a 2654435761 ^ b 2246822519 ^ r 3266489917) >> 7) & 0xFFFFF in uint32 arithmetic; lower word the edge id
 *     3 t0 + i.  A cost bucket, a per-round hash, a unique id.
 *   - INDEPENDENCE: every candidate does a 64-bit atomicMin of its key on claim[a] and claim[b].  It WINS iff
 *     claim[a] == claim[b] == key and claim[v] >= key for every v in N(a) and N(b).  No end of one winner lies in the
 *     closed neighbourhood of another's ends: their triangles are disjoint, and nothing one's tests read is changed by
 *     the other.
 *   - QUOTA: with L live triangles at the start of the round, quota = ceil((L - target_faces) / 2); the winners are
 *     ranked by ascending edge id and the ranks below the quota are APPLIED: rep[b] = a, P[a] = x*, Q_a += Q_b; then
 *     every live triangle renames its corners through rep and dies if two coincide, and rep[v] <- rep[rep[v]].
 *   - A round is a NO-OP once L <= target_faces or once the round before it had no winner; both are read on the device.
 *   - OUTPUT: the live triangles by ascending t0 in their own corner order; the vertices they cite by ascending index,
 *     at their current positions; vertex_map int32[nv] = the output index of rep[v], -1 if it is not emitted.
 *   - counts (device uint64[8], 8-byte aligned, zeroed by begin): [0] output vertices and [1] output triangles ([1] is
 *     the live count after begin and after every round, [0] is filled by count), [2] unusable triangles in the low
 *     word, usable triangles without a plane (s == 0) << 32, [3] rounds that had a winner, [4] non-finite vertices,
 *     [5] collapses applied, [6] vertices locked in the last round that ran, [7] row slots or output rows that could
 *     not be placed - non-zero means the result is invalid.
 *
 *   mi3d_mesh_collapse_workspace  host only: bytes of device scratch for a mesh of this size (0 for nv = nt = 0 and for
 *                          sizes out of range).  ALL state of a run lives there.
 *   mi3d_mesh_collapse_begin    usable flags, quadrics, state; counts zeroed and [1], [2], [4] filled.
 *   mi3d_mesh_collapse_rounds   n_rounds <= 4096 rounds.  After k rounds in all, counts[3] < k tells that the run is
 *                          over: counts[1] <= target_faces, or stalled above it.
 *   mi3d_mesh_collapse_count    counts[0], counts[1] and the output numbering; the caller reads counts here to size
 *   mi3d_mesh_collapse_emit     out_vertices float[nv_cap][3], out_triangles int32[nt_cap][3], vertex_map int32[nv];
 *                          nothing is written past the caps, what could not be placed is counted in counts[7].
 * All calls of one run go to the same stream with the same nv, nt, ws, ws_bytes and counts; count directly before
 * emit.  No entry point allocates or synchronises.  nv = nt = 0 launches nothing and succeeds; nv = 0 or nt = 0 alone
 * is served.  Sizes out of range, a max_error that is negative or NaN, n_rounds > 4096, a workspace that is NULL, too
 * small or not 8-byte aligned, a counts that is NULL or not 8-byte aligned and every other NULL pointer that would be
 * dereferenced are refused (hipErrorInvalidValue) and launch nothing. */
#define MI3D_COLLAPSE_MAX_DEGREE 64
#define MI3D_COLLAPSE_MAX_ROW 1024
size_t mi3d_mesh_collapse_workspace(unsigned long long nv, unsigned long long nt);
int mi3d_mesh_collapse_begin(const float *vertices, unsigned long long nv, const int32_t *triangles, unsigned long long nt,
                             void *ws, size_t ws_bytes, unsigned long long *counts, void *stream);
int mi3d_mesh_collapse_rounds(unsigned long long nv, unsigned long long nt, unsigned long long target_faces,
                              float max_error, uint32_t n_rounds, void *ws, size_t ws_bytes, unsigned long long *counts,
                              void *stream);
int mi3d_mesh_collapse_count(unsigned long long nv, unsigned long long nt, void *ws, size_t ws_bytes,
                             unsigned long long *counts, void *stream);
int mi3d_mesh_collapse_emit(unsigned long long nv, unsigned long long nt, void *ws, size_t ws_bytes, float *out_vertices,
                            unsigned long long nv_cap, int32_t *out_triangles, unsigned long long nt_cap,
                            int32_t *vertex_map, unsigned long long *counts, void *stream);

/* ------------------------------------------------------------------ Part 20: the area-adaptive atlas (mesh export) */

/* Part 9's atlas with patch sizes that follow the triangle's edge lengths, for meshes whose triangles differ in size by
 * orders of magnitude (after Part 14 or Part 19).  Still one patch per triangle with unshared vt, still no inpainting
 * (the gutter is evaluated at the extrapolated point); vt, xyz and owner keep Part 9's formats, so mi3d_texture_pack,
 * mi3d_texture_project and mi3d_mesh_shade* consume them unchanged.  This project's own contract - PARITY UNPINNED.
 * Added under ABI version 5: new symbols only.  (Declared ahead of the point-cloud part, like Part 12.)
 *
 * ARITHMETIC: binary32, every operation rounded separately (the unit is built with -ffp-contract=off), no sqrt, no
 * transcendental function: a NumPy float32 restatement gives the same bits (tests/atlas_adaptive_model.py).  All
 * counters are integers, no float atomics: two runs give the same bytes.
 *
 *   1. MEASURE, thread = triangle.  Squared edge lengths l = (dx dx + dy dy) + dz dz; edge k is the one opposite corner
 *      k.  rot = the corner opposite the longest edge: rot = 0; if l1 > l0 then 1; if l2 > the larger then 2 (ties go to
 *      the smallest index; a NaN never wins).  Patch corners A' = corner rot, B' = corner (rot + 1) % 3, C' = corner
 *      (rot + 2) % 3: a cyclic rotation, the winding stays.  A squared length's BIN is its binary32 biased exponent
 *      - 127, clamped to [-60, 3], + 60, so in [0, 63]; a biased exponent of 0 or 255 (zero, denormal, infinite, NaN)
 *      gives bin 0.  One bin step is a factor sqrt 2 in length.  Outputs: shape uint32[nt], the SHAPE WORD rot |
 *      binAB << 8 | binAC << 16 | bad << 31 with AB = A'B' and AC = A'C'; hist uint32[64][64], hist[binAC][binAB] ADDED
 *      to (zeroed by the caller), built in LDS per workgroup and merged with integer atomics.  A triangle with a vertex
 *      index outside [0, nv) is never dereferenced: rot 0, bins (0, 0), bit 31 set; it is sorted and placed like any
 *      class-(0, 0) triangle but owns nothing, and is COUNTED once in *bad (device uint64, 8-byte aligned, zeroed by the
 *      caller) - Part 9's convention.
 *   2. PLAN, host only, a pure function of hist and T in [64, 16384].  LEGS = 2 3 4 6 8 11 16 23 32 45 64 91 128 181 256
 *      362 (round(2^(k / 2 + 1)), k = 0 .. 15); kmax = the largest k with LEGS[k] + 3 <= T.  Under a SHIFT s in [0, 63] a
 *      leg's class is clamp(bin - s, 0, kmax); a triangle of class (ka, kb) = (class of binAB, class of binAC) has
 *      a = LEGS[ka] texel intervals along A'B' and b = LEGS[kb] along A'C', KEY kb * 16 + ka, and a CELL of (a + 3) x
 *      (b + 3) texels that two triangles of the class share as halves 0 and 1: ceil(count / 2) cells per class.
 *      SHELVES: height classes kb in descending order, each starting a new shelf at x = 0; inside one, width classes ka
 *      in descending order; a class goes on in the current shelf at the current x while a cell still fits
 *      (T - x >= a + 3), else in the next shelf at x = 0; empty classes take nothing.  Rows used = the sum over the
 *      height classes of shelves * (b + 3).  The plan takes the SMALLEST s whose rows used are <= T, scanning upward
 *      from 0; if none fits (or hist is empty or sums to more than 2^31 - 1) mi3d_atlas_adaptive_plan returns 0, else 1.
 *      plan_host int32[MI3D_ATLAS_PLAN_WORDS]:
 *        [0 .. 16)       s, T, kmax, rows used, height groups G, classes NC, nt, owned texels, legs with bin - s < 0
 *                        (clamped at the smallest class), legs with bin - s > kmax (clamped at the largest), 0 ...
 *        [16 .. 144)     G groups of 8 words, in placement order: y0 (first image row), b + 3, shelves, first class
 *                        record, class records, kb, 0, 0
 *        [144 .. 3216)   NC class records of 12 words, in placement order: key, a, b, x0 and shelf (within the group) of
 *                        cell 0, n0 = cells in that first shelf's rest ((T - x0) / (a + 3)), per = cells in a whole
 *                        shelf (T / (a + 3)), count, start, y0 of the group, cells, 0
 *        [3216 .. 3472)  key -> class record index, -1 for an empty class
 *      Cell q of a class: q < n0 at (x0 + q (a + 3), y0 + shelf (b + 3)); else with r = q - n0 at ((r % per) (a + 3),
 *      y0 + (shelf + 1 + r / per) (b + 3)).  The caller uploads the plan (too large for kernel arguments).
 *   3. SORT: a stable counting sort of the triangles by key (one 8-bit pass; csrc/mi3d_scan.h's scan).  `start` of a class
 *      is the number of triangles with a smaller key.  slot uint32[nt]: slot[i] = start + the number of triangles
 *      j < i of the same key; triangle_of uint32[nt] its inverse.  Triangle i lies in cell (slot[i] - start) / 2 of its
 *      class as half (slot[i] - start) & 1; the missing partner of an odd count owns nothing.
 *   4. OWNERSHIP AND UVS: local texel (x, y) of a cell, 0 <= x <= a + 2, 0 <= y <= b + 2.  Half 0 owns it iff x <= a,
 *      y <= b and b max(x - 1, 0) + a max(y - 1, 0) < a b (integers); half 1 owns the image of that set under
 *      (x, y) -> (a + 2 - x, b + 2 - y); every other texel of the cell, like margins and unused cells, is owned by no
 *      one: owner -1, colour 0.  Half 0's set is exactly what a bilinear lookup touches with non-zero weight somewhere
 *      in the UV triangle, and the halves never meet (tests/test_atlas_adaptive_cpu.py checks all pairs with legs up to
 *      91).  Half 0 puts A', B', C' at the CENTRES of local texels (0, 0), (a, 0), (0, b), half 1 at their reflections;
 *      vt = ((X + 0.5) / T, 1 - (Y + 0.5) / T) as in Part 9.  vt float[3 nt][2], row 3 i + k for ORIGINAL corner k:
 *      faces and everything downstream are unchanged.
 *   5. TEXEL -> SURFACE POINT: Part 9's formula on the rotated corners: (u, v) = the local coordinates, reflected for
 *      half 1; s = u / a, t = v / b; p = (A' + s (B' - A')) + t (C' - A'), clamped to [-1, 1] with fmax then fmin (a NaN
 *      becomes -1).  Part 9's SUPERSAMPLING offsets and storage order.  Per texel: the height group by row, then the
 *      class by position in the group's strip of shelves (the last class that starts at or before shelf * T + X), at
 *      most 16 steps each.
 *
 *   mi3d_atlas_adaptive_workspace  bytes of device scratch for the sort of nt triangles (0 for nt outside
 *                                  [1, 2^31 - 1]); host only
 *   mi3d_atlas_adaptive_measure    step 1
 *   mi3d_atlas_adaptive_plan       step 2; host only, both pointers host memory
 *   mi3d_atlas_adaptive_owner      host only: -1, 0 or 1, the half that owns local texel (x, y) of a class-(ka, kb)
 *                                  cell; -2 for a class above 15 or a texel outside the cell
 *   mi3d_atlas_adaptive_sort       step 3: shape and the uploaded plan -> slot, triangle_of
 *   mi3d_atlas_adaptive_uv         step 4: vt
 *   mi3d_atlas_adaptive_positions  step 5 for the band of image rows [row0, row0 + rows): xyz and owner (may be NULL) as
 *                                  mi3d_atlas_positions writes them
 * measure, sort, uv and positions of one atlas go to the same stream in this order, with the plan made from the
 * histogram measure wrote.  A plan that does not belong to the mesh gives a wrong atlas but no access outside the
 * arrays: every index taken from it is compared with its bound.  No entry point allocates or synchronises; a bake
 * reads the host twice (hist before the plan, bad at the end).  Refused (hipErrorInvalidValue), launching nothing: nt
 * or nv outside [1, 2^31 - 1], T or ssaa or a band outside Part 9's ranges, a workspace that is NULL, too small or not
 * 8-byte aligned, a bad that is not 8-byte aligned, and every NULL pointer other than `owner`. */
#define MI3D_ATLAS_PLAN_WORDS 3472
size_t mi3d_atlas_adaptive_workspace(unsigned long long nt);
int mi3d_atlas_adaptive_measure(const float *vertices, unsigned long long nv, const int32_t *triangles,
                                unsigned long long nt, uint32_t *shape, uint32_t *hist, unsigned long long *bad,
                                void *stream);
uint32_t mi3d_atlas_adaptive_plan(const uint32_t *hist_host, uint32_t T, int32_t *plan_host);
int mi3d_atlas_adaptive_owner(uint32_t ka, uint32_t kb, uint32_t x, uint32_t y);
int mi3d_atlas_adaptive_sort(const uint32_t *shape, unsigned long long nt, const int32_t *plan, void *ws, size_t ws_bytes,
                             uint32_t *slot, uint32_t *triangle_of, void *stream);
int mi3d_atlas_adaptive_uv(const uint32_t *shape, const uint32_t *slot, unsigned long long nt, const int32_t *plan,
                           uint32_t T, float *vt, void *stream);
int mi3d_atlas_adaptive_positions(const float *vertices, unsigned long long nv, const int32_t *triangles,
                                  unsigned long long nt, const uint32_t *shape, const uint32_t *triangle_of,
                                  const int32_t *plan, uint32_t T, uint32_t ssaa, uint32_t row0, uint32_t rows, float *xyz,
                                  int32_t *owner, void *stream);

/* ------------------------------------------------------------------ Part 11: the refine stage's point cloud */

/* Depth / mask / rgb views -> the coloured point cloud the refine stage starts from: what `depth2point`,
 * `multidepth2point_mask`, `z_buffer` and `project` of the reference's nerf/refine_utils.py (:61-208) compute, there in
 * NumPy, two Python loops over every point, and cv2.erode.  Added under ABI version 5: new symbols only.
 *
 * ARITHMETIC.  The reference computes positions, projections and depths in binary64 (NumPy) and the sampled colours and
 * the canonical-depth lookup in binary32 (torch.Tensor, F.grid_sample); so do these kernels.
 *   - Geometry is `double`, every operation rounded separately (no fused multiply-add), three-term sums in index order
 *     k = 0, 1, 2, a translation added last.
 *   - CAMERA: rt_host = 12 doubles, the rows of the 3 x 4 world-to-camera matrix [R | t]; k_host = 9 doubles, the 3 x 3
 *     intrinsics, row-major.  Both are HOST pointers read during the call (inverses are the caller's, in NumPy float64).
 *   - PROJECTION (`project`): cam = p . R^T + t, q = cam . K^T, xy = q[:2] / q[2], z = q[2].  z <= 0 is not rejected.
 *   - PIXEL: rint (round half to even, `np.round`) of x and y; in bounds iff 0 <= x <= W - 1 and 0 <= y <= H - 1.  The
 *     reference is undefined for a coordinate that is non-finite or fits no int32; here such a point is OUT OF BOUNDS.
 *   - SAMPLING (F.grid_sample's defaults: bilinear, zero padding, align_corners=False), binary32: a pixel coordinate v
 *     becomes g = v / H * 2 - 1 - BOTH axes divided by H, as the reference has it - then i = ((g + 1) * size - 1) / 2
 *     with size = W for x and H for y, floor, and the four taps nw, ne, sw, se added in this order to 0, each
 *     value * (x weight * y weight); a tap outside the image adds nothing.
 * Points are double[n][3]; images are row-major [H][W], 1 <= H, W <= 16384; n <= (2^31 - 1) * 256.
 *
 *   mi3d_pc_unproject_workspace  host only: bytes of device scratch for an H x W view (0 for sizes out of range)
 *   mi3d_pc_unproject  depth double[H][W], mask uint8[H][W] -> the world points of the pixels with mask != 0, in
 *                      ROW-MAJOR PIXEL ORDER: v = Kinv . (x, y, 1), v *= depth[y][x], p = v . R^T + t with kinv_host
 *                      (9 doubles) and c2w_host (12 doubles: rows [R | t] of the camera-to-world matrix).  Compaction is
 *                      order-preserving and deterministic (wave ballot, workgroup sums, a scan across workgroups - no
 *                      atomic appends): two runs give identical bytes.  *count (device uint64, 8-byte aligned) = the
 *                      number of kept pixels; rows at or past `cap` are not written, so count > cap tells the caller.
 *   mi3d_pc_project    the PROJECTION written out: xy double[n][2], z double[n]
 *   mi3d_pc_zmin       zkeys uint64[H][W] (8-byte aligned), initialised in-stream, then one 64-bit atomicMin per in-bounds
 *                      point of an order-preserving key of its depth z (negative depths order correctly).
 *   mi3d_pc_visible    the reference's `z_buffer`, which depends on the per-pixel minimum alone:
 *                      visible[i] = in_bounds(i) and z_i - zmin[pixel(i)] <= 1.0 / H, uint8 0 / 1.  A NaN compares false.
 *                      Same points and camera as the mi3d_pc_zmin call before it on the same stream.
 *   mi3d_box_morph     erosion (dilate = 0: minimum) or dilation (dilate = 1: maximum) of float[H][W] by a kh x kw box of
 *                      ones, kh and kw odd and <= 31, anchor at the centre; separable, rows then columns through an LDS
 *                      tile with its halo, one launch.  src != dst.  BORDER: pixels outside the image are ignored - a
 *                      window's minimum / maximum is taken over its in-image part (cv2.erode / cv2.dilate with their
 *                      default border).  cv2 is on no machine this project builds on: the border rule is this project's
 *                      contract, PARITY UNPINNED.  A NaN pixel is ignored like one outside (all-NaN window: +-inf).
 *   mi3d_pc_cano_filter  refine_utils.py:100-107 against the canonical camera: xy rounded (rint), converted to float, the
 *                      SAMPLING rule on cano_depth float[H][W], then in double d = z - sampled and
 *                      keep[i] = not (d <= 1.0 / H and d >= -0.2), uint8 0 / 1.  A coordinate that is non-finite or fits
 *                      no int32 samples 0.  The reference's arithmetic assumes H == W; this entry point does not check.
 *   mi3d_pc_colour     refine_utils.py:111-114: xy NOT rounded, converted to float, the SAMPLING rule on image
 *                      float[3][H][W] -> colour float[n][3].
 * No entry point allocates or synchronises.  A NULL pointer, a size out of range and an even or oversized box are refused
 * (hipErrorInvalidValue); n = 0 is accepted. */
size_t mi3d_pc_unproject_workspace(uint32_t H, uint32_t W);
int mi3d_pc_unproject(const double *depth, const uint8_t *mask, uint32_t H, uint32_t W, const double *kinv_host,
                      const double *c2w_host, void *ws, size_t ws_bytes, double *points, unsigned long long cap,
                      unsigned long long *count, void *stream);
int mi3d_pc_project(const double *points, unsigned long long n, const double *rt_host, const double *k_host, double *xy,
                    double *z, void *stream);
int mi3d_pc_zmin(const double *points, unsigned long long n, const double *rt_host, const double *k_host, uint32_t H,
                 uint32_t W, unsigned long long *zkeys, void *stream);
int mi3d_pc_visible(const double *points, unsigned long long n, const double *rt_host, const double *k_host, uint32_t H,
                    uint32_t W, const unsigned long long *zkeys, uint8_t *visible, void *stream);
int mi3d_box_morph(const float *src, float *dst, uint32_t H, uint32_t W, uint32_t kh, uint32_t kw, int dilate,
                   void *stream);
int mi3d_pc_cano_filter(const double *points, unsigned long long n, const double *rt_host, const double *k_host,
                        const float *cano_depth, uint32_t H, uint32_t W, uint8_t *keep, void *stream);
int mi3d_pc_colour(const double *points, unsigned long long n, const double *rt_host, const double *k_host,
                   const float *image, uint32_t H, uint32_t W, float *colour, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MI3D_H */
