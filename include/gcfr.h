/*
 * gcfr.h -- C ABI of libgcfr_hip.so: the MI355X (gfx950) implementation of GeomConsistentFR's
 * render block (ray-marched soft shadow + Lambertian shading + compositing).
 *
 * The reference (andrewhou1/GeomConsistentFR) has NO operator/plugin/FFI interface for this path:
 * the block is ~170 inline lines of torch ops at the end of RelightNet.forward
 * (train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:352-524, "T8"; inference variants
 * test_relight_single_image.py:326-505 "S1", test_relight_single_image_lighting_transfer.py:325-514
 * "SLT").  The entry points below are therefore the seams a maintainer would cut at T8:352; each one
 * cites the reference lines it replaces.  INTEGRATION.md shows the ctypes binding and the edit to
 * RelightNet.forward.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (hipMalloc / torch tensor storage),
 *     contiguous, planes in NCHW order; nothing is allocated, freed or synchronised inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue work;
 *   - re-entrant and thread-safe: the library keeps NO process-wide mutable state -- every knob and hook is
 *     an argument (`gcfr_options`), so two host threads may launch on two streams with different options;
 *     return value: GCFR_OK or a negative gcfr_status;
 *   - shapes: B images, L lights per image, H rows, W columns, N samples per ray.
 *     Pixel (r,c) has image-plane coordinates x = c - W/2, y = H/2 - r           (T8:51-55).
 */
#ifndef GCFR_H
#define GCFR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gcfr_status {
    GCFR_OK = 0,
    GCFR_ERR_INVALID_ARGUMENT = -1, /* null pointer / non-positive or unsupported dimension */
    GCFR_ERR_LAUNCH = -2            /* hipGetLastError() != hipSuccess after the launch       */
} gcfr_status;

/* Library / build identification: "gcfr-hip <version> gfx950". */
const char *gcfr_version(void);

/*
 * ABI revision of THIS header.  It changes whenever an entry point's argument list or a struct layout changes
 * (every symbol keeps its name, so a stale library would otherwise be called with shifted arguments).  A binding
 * compares gcfr_abi_version() of the library it loaded with the GCFR_ABI_VERSION it was written against and refuses
 * to proceed on a mismatch (geomconsistentfr_amd/_lib.py does).
 *   3: round 3 -- gcfr_inference_images_u8 gained `mask_f32`; gcfr_abi_version itself; the metrics entry points.
 *   4: round 4 -- gcfr_options gained `pixels`.
 *   5: round 5 -- gcfr_options gained `phase` (the prepass as its own enqueue); gcfr_copy_probe.
 *   6: round 6 -- gcfr_options lost the dead `schedule` / `tile_order` fields (sizeof 64 -> 56: `phase` had gone into what
 *      was tail padding, so revision 5's struct_size could not tell a revision-4 caller from a revision-5 one -- this one
 *      can); gcfr_inference_images_u8 gained `L` (relit images per photograph: many lights per face).
 *      Still 6: gcfr_options.lds_stage is accepted for compatibility and ignored -- the LDS-staged march it selected (built,
 *      bit-identical, not faster: profiles/r03_lds_stage_ab.md) builds from commit 0b22e41; gcfr_shadow_workspace_bytes()
 *      returns what it did (that variant's region is an unused tail now).
 * struct_size guards the struct's SIZE only: a field added into padding does not change it.  The revision check is
 * therefore mandatory for every binding, and every entry point validates struct_size before it reads any other field.
 */
#define GCFR_ABI_VERSION 6
int32_t gcfr_abi_version(void);

/*
 * Per-call options of the forward entry points (HOST struct, read during the call only; NULL = defaults).
 * With ONE exception (`pixels`, off by default) nothing here changes a result bit: the knobs select among kernels /
 * schedules that are bit-identical (tests/test_gpu_parity.py asserts it for every combination), the hooks only observe.
 */
#define GCFR_N_COUNTERS 28
typedef struct gcfr_options {
    uint32_t struct_size;      /* sizeof(gcfr_options) of the caller's build; a mismatch is GCFR_ERR_INVALID_ARGUMENT */
    int32_t tile_w;            /* pixels per tile row: 8, 16, 32 or 64 (a wave marches a tile_w x 64/tile_w tile); 0 = auto */
    int32_t group;             /* samples per skip group: 1, 2 or 4; 0 = auto (4) */
    int32_t ksplit;            /* split each tile's sample range over the 4 waves of a workgroup: 0, 1, -1 = auto by launch size */
    int32_t depth_bound_skip;  /* exact depth-bound group skip: 0, 1, -1 = auto (on) */
    int32_t lds_stage;         /* selects nothing: accepted for compatibility (-1, 0 or 1; anything else is rejected) and
                                  ignored.  It chose the LDS-staged march, which was removed (see the revision history) */
    void *event_start;         /* hipEvent_t recorded on `stream` immediately before the march kernel, or NULL */
    void *event_stop;          /* hipEvent_t recorded immediately after it, or NULL */
    uint64_t *counters;        /* DEVICE array of GCFR_N_COUNTERS + 4 * (number of tiles) u64: the march kernel adds its work
                                  counts (executed groups, bound tests, ...; tools/count_work.py) to the first
                                  GCFR_N_COUNTERS and writes a 4-word timeline record per tile behind them
                                  (tools/trace_timeline.py); only a library built with -DGCFR_COUNTERS touches it
                                  (gcfr_version() then ends in "+counters"), else ignored.  With -DGCFR_AUDIT as well ("+audit")
                                  the last eight tallies count the claims the march makes about samples it does not evaluate and
                                  the ones a plain evaluation of those samples contradicts (tools/audit.py) */
    int32_t pixels;            /* WHICH PIXELS are marched.  0 (default; also -1): every pixel, as the reference does
                                  (T8:371-515 computes minimum_distance for all H x W pixels).
                                  1 ("mask"; DEVIATES from the reference's returned tensors, opt-in): pixels whose OWN mask cell
                                  is zero are not marched -- they get the masked value the reference assigns to a ray without
                                  an unmasked sample (minimum_distance 1e6, T8:512; argmin -1), hence shadow_mask_weights 1,
                                  final_shading = full_shading, rendered_images = albedo x full_shading there -- and a tile
                                  without an unmasked pixel does no march at all.  Every other pixel is bit-identical to
                                  pixels = 0.  Why it is safe for the training script: each consumer of the block's outputs
                                  multiplies them by that same mask (T8:619, 633, 641, 643: `rendered_images * masks` in the
                                  reconstruction, adversarial and DSSIM terms), so the losses are bit-equal and the masked-out
                                  pixels receive a zero upstream gradient either way; `shadow_mask_weights` / `full_shading` /
                                  `ambient_light` are returned by T8:524 but used by no loss.  Not for callers that
                                  look at the shadow OUTSIDE the mask (the inference scripts write the un-masked shadow image
                                  only after multiplying by the mask as well, S8:603-608).  Honoured by the workspace path when
                                  `argmin` is requested (the training forward; halves its march on face-shaped masks);
                                  GCFR_ERR_INVALID_ARGUMENT without a workspace or without `argmin`. */
    int32_t phase;             /* WHICH HALF of a workspace call is enqueued (gcfr_shadow_fwd, gcfr_render_fwd,
                                  gcfr_render_from_depth_fwd).  0 (default; also -1): both -- the prepass launch (depth repack, mask
                                  statistics, depth bounds, horizon tables, light preparation, sample-table check: everything that
                                  depends on depth, mask, light_raw and t_table only) and the march launch behind it on `stream`.
                                  1: the prepass only.  2: the march only, on a workspace that a phase-1 call WITH THE SAME ARGUMENTS
                                  AND OPTIONS filled (the caller orders the two: same stream, or an event between two streams).
                                  Bit-identical to phase 0 by construction: the same two launches with the same arguments, enqueued by
                                  two calls.  Why: in RelightNet.forward the depth head, the light and the mask exist before the albedo
                                  decoder has run (T8:226-350), so the prepass can run on a side stream under the decoder's
                                  convolutions and the march then starts without a dependent launch in front of it.  A phase-1 call
                                  reads only: depth, mask_u8, light_raw (where the entry point has it), t_table; writes: workspace,
                                  unit_out / light_pt_out (where the entry point has them).  The remaining pointers are not touched
                                  and may be NULL (the albedo does not exist yet).  GCFR_ERR_INVALID_ARGUMENT without a workspace. */
} gcfr_options;

/* Fills `opt` with the defaults (struct_size set, every knob "auto", no hooks). */
void gcfr_options_default(gcfr_options *opt);

/*
 * Sample fractions t_k along the pixel->light segment, HOST side helper.
 * Replaces np.arange(t0, ., dt) at T8:468 (S1:445, SLT:451) with numpy's value rule
 * t_k = t0 + k*((t0+dt)-t0), all f64.  Writes n doubles to `out_host`; upload it and pass the
 * device copy as `t_table`.
 */
int gcfr_sample_table(double t0, double dt, int32_t n, double *out_host);

/*
 * Light preparation.  Replaces T8:357-363 (clamp_z = 1, clamp_min = 0; SLT:332 uses 0.16) and
 * S1:332-336 (clamp_z = 0).
 *   light_raw     (n,3) f32   SL_lin2[...,1:4] or target_lighting
 *   unit_out      (n,3) f32   unit_light_direction
 *   light_pt_out  (n,3) f32   incident_light_points = light_distance * unit (T8:362)
 */
int gcfr_light_prep(const float *light_raw, int32_t n, int32_t clamp_z, float clamp_min,
                    float light_distance, float *unit_out, float *light_pt_out, void *stream);

/*
 * Ray march: minimum point-to-line distance over the sample table.  Replaces T8:371-515
 * (S1:349-496, SLT:355-504): slopes/intercepts, the nine-way end-point branch, clamp, the
 * (N,2,H,W) f64 sample grids, five gathers, bilinear depth, cross product distance, mask, min.
 *   depth       (B,H,W) f32      c2_o_depth, already x100 (T8:350)
 *   mask_u8     (MB,H,W) u8      1 where the reference's mask != 0; MB = mask_batch = B (T8:510)
 *                                or 1 (one mask shared by all images, S1:488)
 *   light_pt    (B,L,3) f32      from gcfr_light_prep
 *   t_table     (N) f64          from gcfr_sample_table (device copy).  Any table gives the reference's
 *                                results; the workspace path's pruning / skipping only engages on a table its
 *                                prepass finds increasing, inside [0, 1] and uniform to 0.1 %
 *   bonus       added to the minimum when the light's (x,y) lies inside bonus_box
 *               = {x_lo, x_hi, y_lo, y_hi} (S1:495-496: box = image, bonus = 5; SLT:503-504);
 *               training form: bonus = 0 (bonus_box may be NULL).  bonus_box is a HOST pointer.
 *   min_dist    (B,L,H,W) f32 out   minimum_distance (T8:515)
 *   argmin      (B,L,H,W) i32 out   index of the minimising sample (saved for backward); may be NULL
 *   opt         per-call options (host pointer) or NULL for the defaults; see gcfr_options
 *   workspace   device scratch of >= gcfr_shadow_workspace_bytes(B,H,W) bytes, 16-byte aligned, or NULL.
 *               With a workspace the depth maps are first repacked into 2x2-neighbourhood texels
 *               (one 16-byte gather per ray-step instead of four 4-byte gathers) and a coarse grid of
 *               depth bounds lets the march skip sample groups that provably cannot lower a
 *               pixel's running minimum; since round 3 the prepass also leaves, per image, running column / row
 *               maxima of the depth an unmasked sample can read ("horizon tables", shapes with W % 4 == 0 and
 *               H, W <= 1024), against which a ray that has passed its last candidate stops marching; results are
 *               bit-identical to the NULL-workspace path, only faster.  Contents are scratch: rewritten by every
 *               call, nothing in it needs initialising.  Images with H < 6 or W < 6 are marched WITHOUT the depth
 *               bounds by the grid kernels (the same bits; at most four rows or columns of work): the bounds variant
 *               takes its bilinear weights from v_fract_f64, which is the reference's arithmetic only where no sample
 *               position can fall inside 0 < |u| <= 2^-54 -- every image of six or more rows and columns.
 * Supported: 2 <= H,W <= 4096, even; 1 <= N <= 4096.
 */
size_t gcfr_shadow_workspace_bytes(int32_t B, int32_t H, int32_t W);

int gcfr_shadow_fwd(const float *depth, const uint8_t *mask_u8, int32_t mask_batch,
                    const float *light_pt, int32_t B, int32_t L, int32_t H, int32_t W, int32_t N,
                    const double *t_table, float bonus, const float *bonus_box, float *min_dist,
                    int32_t *argmin, void *workspace, size_t workspace_bytes, void *stream,
                    const gcfr_options *opt);

/*
 * Soft-shadow transfer + Lambert shading + composite.  Replaces T8:364-369 and T8:517-522.
 *   normals     (B,3,H,W) f32    depth_to_normals(depth+offset, K) with y negated (T8:353-354);
 *                                 re-normalised inside (T8:365)
 *   depth       (B,H,W) f32;  albedo (B,3,H,W) f32;  light_pt (B,L,3) f32;  ambient (B,L) f32
 *   min_dist    (B,L,H,W) f32    from gcfr_shadow_fwd
 *   intensity   directional_intensity (T8:46: 0.5; SLT:20: 0.41)
 * outputs (any may be NULL except rendered):
 *   shadow_w    (B,L,H,W) f32    shadow_mask_weights = 1 - 4e^-d/(1+e^-d)^2        (T8:517)
 *   full        (B,L,H,W) f32    full_shading = ambient + I*max(n.l, 0)            (T8:366-369)
 *   final       (B,L,H,W) f32    final_shading = w*full + (1-w)*ambient            (T8:518)
 *   rendered    (B,L,3,H,W) f32  rendered_images = albedo * final                  (T8:519-522)
 */
int gcfr_shade_fwd(const float *normals, const float *depth, const float *albedo,
                   const float *light_pt, const float *ambient, const float *min_dist, int32_t B,
                   int32_t L, int32_t H, int32_t W, float intensity, float *shadow_w, float *full,
                   float *final_shading, float *rendered, void *stream);

/*
 * Surface normals from depth.  Replaces the kornia call + sign flip at T8:353-354 (SLT:325: offset 1410,
 * focal 700).  kornia 0.4.1 is un-vendored: this restates its published algorithm (unproject with the
 * camera matrix, normalised 3x3 Sobel with replicate padding, cross, normalise) -- parity UNPINNED.
 *   depth (B,H,W) f32;  fx, fy, cx, cy from intrinsic_matrix (T8:571-577);  z_offset added in f32
 *   negate_y: 1 = apply T8:354;  normals (B,3,H,W) f32 out, unit length
 * 1 <= B <= 65535, H >= 2 and W >= 2 (any parity), fx and fy non-zero; anything else, or a NULL buffer, is
 * GCFR_ERR_INVALID_ARGUMENT before a launch, for gcfr_normals_fwd and gcfr_normals_bwd alike.  A one-pixel-wide image is refused
 * because replicate padding then makes both neighbours of a pixel the pixel itself: dP/du (W = 1) or dP/dv (H = 1) is the zero
 * vector, the cross product vanishes and the restated algorithm returns 0 / 1e-12, not a unit normal.
 * Numerical contract (also of the normals the fused epilogue of gcfr_render_from_depth_fwd computes and of `normals_out`):
 * NOT bit-reproducible against another evaluation order -- the reference's chain is f64 with an unspecified conv2d
 * summation order, and the kernels use reciprocals / v_rsq + Newton steps instead of IEEE divisions -- but within 4 f32
 * ulp of the f64 restatement (oracle/normals_restatement.py) after rounding to f32; a non-finite depth cell makes
 * exactly the normals non-finite whose clamped 3 x 3 neighbourhood contains it (tests/test_gpu_normals.py).
 */
int gcfr_normals_fwd(const float *depth, int32_t B, int32_t H, int32_t W, double fx, double fy, double cx,
                     double cy, float z_offset, int32_t negate_y, float *normals, void *stream);
/* Backward of gcfr_normals_fwd: grad_normals (B,3,H,W) f32 -> grad_depth (B,H,W) f32 += (atomics). */
int gcfr_normals_bwd(const float *grad_normals, const float *depth, int32_t B, int32_t H, int32_t W,
                     double fx, double fy, double cx, double cy, float z_offset, int32_t negate_y,
                     float *grad_depth, void *stream);

/*
 * One-call forward for a batch: gcfr_light_prep + depth repack + ray march with the shading fused
 * into the march kernel's epilogue (each lane shades the pixel it just marched; min_dist never
 * makes a round trip through HBM).  Replaces T8:356-522 in one enqueue.  Arguments as in the three
 * entry points above; workspace is mandatory; argmin / shadow_w / full / final_shading may be NULL.
 * Results are bit-identical to calling gcfr_light_prep, gcfr_shadow_fwd and gcfr_shade_fwd in turn.
 */
int gcfr_render_fwd(const float *light_raw, int32_t clamp_z, float clamp_min, float light_distance,
                    const float *depth, const uint8_t *mask_u8, int32_t mask_batch,
                    const float *normals, const float *albedo, const float *ambient, int32_t B,
                    int32_t L, int32_t H, int32_t W, int32_t N, const double *t_table, float bonus,
                    const float *bonus_box, float intensity, float *unit_out, float *light_pt_out,
                    float *min_dist, int32_t *argmin, float *shadow_w, float *full,
                    float *final_shading, float *rendered, void *workspace, size_t workspace_bytes,
                    void *stream, const gcfr_options *opt);

/*
 * gcfr_render_fwd with the normals stage fused in: the march epilogue evaluates the 3x3 depth stencil of
 * gcfr_normals_fwd itself (same device function, same bits), so T8:353-522 is two launches and the
 * (B,3,H,W) normals tensor makes no HBM round trip.  normals_out (B,3,H,W) may be NULL.
 */
int gcfr_render_from_depth_fwd(const float *light_raw, int32_t clamp_z, float clamp_min,
                               float light_distance, const float *depth, const uint8_t *mask_u8,
                               int32_t mask_batch, double fx, double fy, double cx, double cy,
                               float z_offset, int32_t negate_y, const float *albedo, const float *ambient,
                               int32_t B, int32_t L, int32_t H, int32_t W, int32_t N, const double *t_table,
                               float bonus, const float *bonus_box, float intensity, float *unit_out,
                               float *light_pt_out, float *min_dist, int32_t *argmin, float *normals_out,
                               float *shadow_w, float *full, float *final_shading, float *rendered,
                               void *workspace, size_t workspace_bytes, void *stream,
                               const gcfr_options *opt);

/* ---------------------------------------------------------------------------------------------
 * Backward.  The reference has no explicit backward: torch autograd replays T8:352-524
 * (loss.backward() at T8:655).  These entry points compute the same vector-Jacobian products.
 * Buffers marked "+=" are ACCUMULATED into (zero them first); "=" are overwritten.
 * ------------------------------------------------------------------------------------------- */

/*
 * Backward of gcfr_shadow_fwd (T8:371-515 under autograd): only the argmin sample of each pixel
 * carries gradient (torch.min, T8:514); round/floor/ceil, the end-point branch and the clamp are
 * piecewise constant.
 *   grad_min_dist (B,L,H,W) f32   dLoss/d minimum_distance
 *   argmin        (B,L,H,W) i32   from gcfr_shadow_fwd (-1 = masked minimum: no gradient)
 *   grad_depth    (B,H,W) f32 +=  to the four bilinear corners and the pixel's own depth (atomics)
 *   grad_light_pt (B,L,3) f64 +=  to incident_light_points (reduced over pixels in f64)
 */
int gcfr_shadow_bwd(const float *grad_min_dist, const float *depth, const float *light_pt,
                    const int32_t *argmin, int32_t B, int32_t L, int32_t H, int32_t W, int32_t N,
                    const double *t_table, float *grad_depth, double *grad_light_pt, void *stream);

/*
 * Backward of gcfr_shade_fwd (T8:364-369, 517-522 under autograd).
 *   g_shadow_w, g_full, g_final (B,L,H,W) f32, g_rendered (B,L,3,H,W) f32: upstream grads, any may be NULL
 *   grad_normals (B,3,H,W) f32 =   (w.r.t. the un-normalised normals passed to the forward)
 *   grad_albedo  (B,3,H,W) f32 =
 *   grad_depth   (B,H,W) f32 +=    through the incident-light direction only
 *   grad_light_pt (B,L,3) f64 +=,  grad_ambient (B,L) f64 +=
 *   grad_min_dist (B,L,H,W) f32 =  feed to gcfr_shadow_bwd
 */
int gcfr_shade_bwd(const float *normals, const float *depth, const float *albedo,
                   const float *light_pt, const float *ambient, const float *min_dist, int32_t B,
                   int32_t L, int32_t H, int32_t W, float intensity, const float *g_shadow_w,
                   const float *g_full, const float *g_final, const float *g_rendered,
                   float *grad_normals, float *grad_albedo, float *grad_depth, double *grad_light_pt,
                   double *grad_ambient, float *grad_min_dist, void *stream);

/*
 * Backward of gcfr_render_from_depth_fwd in ONE launch: per (image, pixel) the shading backward of every light,
 * the ray-march backward through each light's argmin sample and the normals-stencil backward, with no
 * intermediate grad_min_dist / grad_normals tensors (same per-pixel device functions as the three kernels
 * above, so the same numbers up to atomic ordering).  Follow with gcfr_light_prep_bwd.
 *   normals_fwd (B,3,H,W) f32 or NULL: the unit normals the forward wrote (gcfr_render_from_depth_fwd's normals_out);
 *                 given them the backward evaluates the depth stencil once instead of twice
 *   g_normals_out (B,3,H,W) f32 or NULL: upstream gradient on the returned unit normals
 *   grad_albedo (B,3,H,W) f32 =;  grad_depth (B,H,W) f32 +=;  grad_light_pt (B,L,3) f64 +=;  grad_ambient (B,L) f64 +=
 */
int gcfr_render_bwd(const float *depth, const float *albedo, const float *light_pt, const float *ambient,
                    const float *min_dist, const int32_t *argmin, const float *normals_fwd, int32_t B, int32_t L,
                    int32_t H, int32_t W,
                    int32_t N, const double *t_table, double fx, double fy, double cx, double cy,
                    float z_offset, int32_t negate_y, float intensity, const float *g_shadow_w,
                    const float *g_full, const float *g_final, const float *g_rendered,
                    const float *g_normals_out, float *grad_albedo, float *grad_depth,
                    double *grad_light_pt, double *grad_ambient, void *stream);

/*
 * Backward of gcfr_light_prep (T8:357-363 under autograd).
 *   grad_unit (n,3) f32 or NULL: dLoss/d unit_light_direction (T8:636 uses it in the cosine loss)
 *   grad_light_pt (n,3) f64 or NULL: accumulated by the two kernels above
 *   grad_light_raw (n,3) f32 =
 */
int gcfr_light_prep_bwd(const float *light_raw, int32_t n, int32_t clamp_z, float clamp_min,
                        float light_distance, const float *grad_unit, const double *grad_light_pt,
                        float *grad_light_raw, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Inference-side consumers of the block's outputs: what the test scripts do between the forward
 * and cv2.imwrite, and the MATLAB border fix -- on the device, so a relit batch leaves it as bytes.
 * ------------------------------------------------------------------------------------------- */

/*
 * The images the inference scripts write per face, quantised as cv2.imwrite quantises a float image
 * (round half to even, clip to [0, 255]); RGB, HWC -- the bytes that end up in the PNG.
 * Replaces test_relight_single_image.py:601-620 (rendered image only) and
 * test_raytracing_relighting_CelebAHQ_DSSIM_8x.py:583-608 / ..._lighting_transfer.py:560-579 (all six).
 * B photographs, L relit images per photograph (L = 1: the scripts' one target light per forward, S1:582-588; L > 1: the
 * many-lights forward, all L composites of a face from ONE network pass -- the scripts re-run the model per light):
 *   input_hwc     (B,H,W,3) f32 in [0,1]   the photograph, as the scripts hold it (training_images)
 *   rendered      (B,L,3,H,W) f32          rendered_images                   -> out_rendered (B,L,H,W,3): the relit face
 *                                          pasted into the photograph where mask > 0
 *   (albedo, depth, normals and their outputs are per photograph, (B,...); shadow_w / final_shading and theirs (B,L,H,W))
 *   albedo        (B,3,H,W) f32 or NULL    -> out_albedo  (B,H,W,3) = 255 albedo mask
 *   depth         (B,H,W) f32 or NULL      -> out_depth   (B,H,W)   = 255 (-depth - lo)/(hi - lo) mask, with
 *   depth_range   DEVICE {lo, hi} f32      = min / max of -depth over the whole batch (S8:589-590)
 *   shadow_w, final_shading (B,H,W) f32 or NULL -> out_shadow, out_shading (B,H,W) = 255 x mask
 *   normals       (B,3,H,W) f32 or NULL    -> out_normals (B,H,W,3) = 255 (n + 1)/2 mask
 *   mask          (MB,H,W) u8               the skin mask as read from disk; the kernel forms the scripts' mask/255.0
 *                                          itself; MB = 1 or B
 *   mask_f32      0: the mask is f64 as in test_relight_single_image.py:580 / S8:569-578 (numpy f64 array / 255.0);
 *                 1: f32 as in test_relight_single_image_lighting_transfer.py:540 (torch uint8 tensor / 255.0), which
 *                    keeps the shadow-mask and depth images' products in f32 (SLT:575, 577)
 * final_shading and normals are f64 in the reference; they are widened to f64 before the arithmetic.
 * Pinned to the reference's own main() (tests/golden/slt_main_*.npz).  Any out_* except out_rendered may be NULL.
 */
int gcfr_inference_images_u8(const float *input_hwc, const float *rendered, const float *albedo, const float *depth,
                             const float *depth_range, const float *shadow_w, const float *final_shading,
                             const float *normals, const uint8_t *mask, int32_t mask_batch, int32_t B, int32_t L,
                             int32_t H, int32_t W, uint8_t *out_rendered, uint8_t *out_shadow, uint8_t *out_albedo,
                             uint8_t *out_depth, uint8_t *out_shading, uint8_t *out_normals, int32_t mask_f32,
                             void *stream);

/*
 * fix_border_artifacts_CVPR2022.m:1-18: pixels on the border of the face mask (0 < 7x7 box sum of the rounded
 * mask < 30, zero padding) take the 3x3 median (zero padding) of their channel.
 *   img_hwc (B,H,W,3) u8;  face_mask_u8 (MB,H,W) u8 skin mask as stored on disk (0 ... 255);  out_hwc (B,H,W,3) u8,
 *   must not alias img_hwc.
 */
int gcfr_fix_border_u8(const uint8_t *img_hwc, const uint8_t *face_mask_u8, int32_t mask_batch, int32_t B, int32_t H,
                       int32_t W, uint8_t *out_hwc, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Data formats either side of the block: batch assembly from the bytes load_data() reads, and the
 * MATLAB evaluation scripts' two metrics as device reductions.
 * ------------------------------------------------------------------------------------------- */

/*
 * One training batch from the uint8 arrays as stored on disk -- what
 * train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:545-556 (load_data) and :607-615 (batch slicing) do in float64 on
 * the host for the whole dataset, here per batch on the device:
 *   images_u8     (B,H,W,3) u8  imread(jpg)                      -> images     (B,H,W,3) f32 = f32(u8 / 255.0)      T8:550, 618
 *   depth_mask_u8 (B,H,W)   u8  imread(depth mask)               -> masks      (B,H,W)   f32 = u8 / 255.0           T8:546, 610
 *   face_mask_u8  (B,H,W)   u8  imread(face mask)                -> masks_fill (B,H,W)   f32 = (max(face, depth) > 128) ? 1 : 0   T8:552-556, 612
 *   albedo_u8     (B,H,W)   u8  imread(grey albedo)              -> albedo     (B,H,W)   f32 = u8 / 255.0           T8:551, 615
 * masks / masks_fill (with face_mask_u8) / albedo (with albedo_u8) may be NULL.
 */
int gcfr_assemble_batch_u8(const uint8_t *images_u8, const uint8_t *depth_mask_u8, const uint8_t *face_mask_u8,
                           const uint8_t *albedo_u8, int32_t B, int32_t H, int32_t W, float *images, float *masks,
                           float *masks_fill, float *albedo, void *stream);

/*
 * Masked MSE (MSE_MP.m:24) and masked DSSIM (DSSIM_MP_RGB.m:24-26) of B image pairs, f64:
 *   recon_u8, gt_u8 (B,H,W,3) u8 RGB;  mask_u8 (MB,H,W) u8 (MB = 1 or B), all scaled by 1/255.0 as the scripts do;
 *   mse_out, dssim_out (B) f64, either may be NULL;
 *   workspace: gcfr_masked_metrics_workspace_bytes(B,H,W) bytes of device scratch, 8-byte aligned.
 * DSSIM follows MATLAB ssim()'s documented defaults on an M x N x 3 volume (Gaussian sigma 1.5, radius 5, replicate padding
 * on all three axes, K = (0.01, 0.03), dynamic range 1).  PARITY UNPINNED: MATLAB is not available to the builder.
 */
size_t gcfr_masked_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gcfr_masked_metrics_u8(const uint8_t *recon_u8, const uint8_t *gt_u8, const uint8_t *mask_u8, int32_t mask_batch,
                           int32_t B, int32_t H, int32_t W, double *mse_out, double *dssim_out, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The training step's image-loss head: everything the step computes from `rendered_images` and the photograph
 * between the render block and loss.backward() -- the mask paste, the masked reconstruction L2's sums and the SSIM of
 * the DSSIM term -- as one fused forward and one fused backward (csrc/gcfr_losses.hip).
 * ------------------------------------------------------------------------------------------- */

/* layout of the photograph argument below */
#define GCFR_IMAGES_NHWC 0 /* (B,H,W,3), as the training batch holds it (T8:618) */
#define GCFR_IMAGES_NCHW 1 /* (B,3,H,W) */

/*
 * Forward.  Replaces train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:619 and :641 (the paste, evaluated twice there),
 * :633 (the two sums of the masked L2) and :643 (pytorch_msssim.ssim up to its per-channel mean):
 *   rendered   (B,3,H,W) f32        rendered_images
 *   images     (B,H,W,3) or (B,3,H,W) f32, by `images_layout`      the photograph
 *   mask       (B,H,W) f32, any values, or NULL (no mask: m = 1)  mask_fill_nose_and_mouth
 *   window     HOST, 11 f32         the normalised Gaussian window (sigma 1.5 in the reference); read during the call
 *   data_range                      pytorch_msssim's data_range (1.0 at T8:643): C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2
 *   composite  (B,3,H,W) f32        = rendered * m + (1 - m) * images, each operation separately rounded
 *   ssim       (B,3) f32            the mean of the SSIM map over its (H-10) x (W-10) 'valid' positions, per image and
 *                                   channel, BEFORE the relu (nonnegative_ssim) and the means over channels and images
 *   sums       (2) f64              { sum (rendered m - images m)^2, sum m }, both over (B,3,H,W) as T8:633's mse_loss(...,
 *                                   'sum') and mask.sum() on the mask repeated over the three channels
 *   workspace  gcfr_image_losses_workspace_bytes(B,H,W) = 8 * (5 * B * ceil(H/16) * ceil(W/32) + 2 * B) bytes of device
 *              scratch, 8-byte aligned (0 is returned for an unsupported shape); it need not be cleared
 * C = 3 and the window of 11 are fixed; 11 <= H, W <= 4096 (any parity), 1 <= B <= 65535; anything else is
 * GCFR_ERR_INVALID_ARGUMENT before a launch.
 * Numerical contract: the results are the stated operation order, exactly.  Every product, sum and quotient is one IEEE f32
 * operation (no contraction, IEEE division, denormals kept): paste t1 = rendered m, t3 = (1 - m) images, composite = t1 + t3;
 * d = t1 - images m; the five maps X, Y, X X, Y Y, X Y filtered along H, then along W, each as acc = 0, acc += w[t] v[t] for
 * t = 0..10; s1 = xx - mu1 mu1, s2 = yy - mu2 mu2, s12 = xy - mu1 mu2, cs = (2 s12 + C2) / (s1 + s2 + C2),
 * lum = (2 mu1 mu2 + C1) / (mu1 mu1 + mu2 mu2 + C1), map = lum cs, with C1, C2 rounded to f32 from the f64 products.  The map
 * values, d d and m are added in f64 (lanes, waves, tiles, images in a fixed order, no floating-point atomics) and
 * ssim = (float)(sum / n_valid): two calls return the same bits, `composite` is bit-equal to the torch f32 expression, and a
 * restatement of this order in f32 (tests/image_losses_emulation.py) reproduces `composite` bit for bit and `ssim` / `sums`
 * (as f32) to one ulp, the association of the f64 sums being the only freedom.
 * The DISTANCE from the same formulas evaluated in f64 on the f32 inputs is not a constant: s1, s2, s12 cancel, so it grows as
 * the windows' variance falls towards C2.  `sums` stay within 2e-6 relative.  `ssim`, absolute error, measured on an MI355X,
 * largest over {face, fractional, no mask} x {NHWC, NCHW} at 2 x 3 x 128 x 128: this head | train.ssim in f32 on the CPU, on the
 * GPU with MIOpen's blur, on the GPU with ATen's blur:
 *     uniform random + 8 % noise (window variance 1/12)    4.3e-8 | 1.0e-7, 1.2e-7, 1.2e-7
 *     smooth sinusoid + 1e-2 noise                          9.3e-7 | 9.4e-7, 1.2e-6, 9.4e-7
 *     the same pasted under a face mask                     6.4e-7 | 5.8e-7, 5.8e-7, 5.8e-7
 *     a synthetic_batch face                                6.1e-7 | 9.6e-7, 1.6e-6, 1.1e-6
 *     constant 0.9 + 1e-2 noise                             1.9e-5 | 6.3e-5, 7.0e-5, 6.1e-5
 *     constant 0.9 + 1e-3 noise                             3.3e-5 | 3.9e-5, 7.7e-5, 3.7e-5
 *     smooth, images of 11..27 x 11..43 (a few hundred valid positions or fewer: no averaging)   up to 1.6e-4 | 1.6e-4, 7e-5, 1.6e-4
 *     rendered == images under a {0,1} mask or none, and all-zero inputs: exactly 1.0f
 * i.e. the former "2e-6 relative" holds on white noise only; on the smooth images the training step feeds, f32 SSIM in ANY order
 * is 1e-6 .. 1e-4 from f64, and this order is as good as torch's (tests/test_gpu_image_losses_regimes.py compares it with twice
 * the worst of the three torch forms, per input).
 * The window must be symmetric (w[t] == w[10 - t]): the backward reuses it unflipped.
 */
size_t gcfr_image_losses_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gcfr_image_losses_fwd(const float *rendered, const float *images, const float *mask, int32_t images_layout,
                          int32_t B, int32_t H, int32_t W, const float *window, double data_range, float *composite,
                          float *ssim, double *sums, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of the above with respect to `rendered` (what autograd replays for T8:619 / 633 / 641 / 643), gather form:
 *   g_composite (B,3,H,W) f32 or NULL   dLoss/d composite (PatchGAN's gradient)
 *   g_ssim      (B,3) f32 or NULL       dLoss/d ssim
 *   g_recon     DEVICE (1) f32 or NULL  dLoss/d sums[0]
 *   grad_rendered (B,3,H,W) f32 = m (g_composite + gX) + g_recon 2 m (rendered m - images m), with
 *       gX = blurT(a) + 2 X blurT(b) + Y blurT(c);  X = composite, Y = images;  a, b, c = the adjoints of the SSIM map with
 *       respect to blur(X), blur(X X), blur(X Y), scaled by g_ssim / ((H-10)(W-10)) and recomputed from the inputs;  blurT = the
 *       same symmetric window applied to the zero-extended valid map.
 * The other arguments as in the forward.  Contract: the stated operation order, exactly -- u = g_ssim / (float)((H-10)(W-10));
 * B1 = mu1 mu1 + mu2 mu2 + C1, B2 = s1 + s2 + C2; d_mu1 = 2 cs (mu2 - lum mu1) / B1 + 2 lum (cs mu1 - mu2) / B2,
 * d_xx = -(lum cs) / B2, d_xy = 2 lum / B2; a, b, c = u d_mu1, u d_xx, u d_xy at the valid positions, zero elsewhere; blurT along
 * H, then along W, taps 0..10 with the window UNFLIPPED (hence: symmetric windows only); gX = ta + 2 X tb + Y tc;
 * out = m (g_composite + gX), then out += g_recon (2 m (rendered m - images m)), each operation one IEEE f32 operation, left to
 * right.  Every element is written once by one lane (no atomics): bit-reproducible, and bit-equal to the f32 restatement of this
 * order (tests/image_losses_emulation.py).  Distance from the f64 evaluation, as a fraction of the gradient's largest entry, with
 * the SSIM's upstream gradient alone, inputs and forms as above (torch differentiates op by op), measured on an MI355X:
 *     uniform random + 8 % noise                            1.5e-6 | 1.3e-6, 1.9e-6, 1.2e-6
 *     smooth sinusoid + 1e-2 noise                          1.3e-4 | 1.1e-4, 1.5e-4, 1.1e-4
 *     the same pasted under a face mask                     1.2e-4 | 1.1e-4, 1.5e-4, 1.0e-4
 *     a synthetic_batch face                                7.8e-5 | 7.2e-5, 1.1e-4, 7.3e-5
 *     constant 0.9 + 1e-2 noise                             3.6e-4 | 2.6e-4, 3.4e-4, 2.7e-4
 *     constant 0.9 + 1e-3 noise                             5.1e-4 | 3.9e-4, 4.1e-4, 3.5e-4
 * (the closed forms mu2 - lum mu1 and cs mu1 - mu2 cancel on flat windows as torch's op-by-op adjoints do: up to 1.4x the best
 * torch form's error, not an order of magnitude).  With PatchGAN's and the L2's upstream gradients of order 1 beside it: 3.9e-7 or
 * less in all of these.  The former "2e-5" holds for the three together, and for the SSIM's part alone on white noise only.
 * grad_rendered must not alias an input.
 */
int gcfr_image_losses_bwd(const float *rendered, const float *images, const float *mask, int32_t images_layout,
                          int32_t B, int32_t H, int32_t W, const float *window, double data_range,
                          const float *g_composite, const float *g_ssim, const float *g_recon, float *grad_rendered,
                          void *stream);

/* ---------------------------------------------------------------------------------------------
 * The training step's supervised-loss head: the five generator-side terms that do NOT read `rendered_images` -- the masked
 * depth L1, the ambient L1, the 1 - cos lighting term, the masked grey-albedo L1 and the generator's BCE -- as one fused forward
 * (plus one finishing launch) and one fused backward (csrc/gcfr_supervised_losses.hip).
 * ------------------------------------------------------------------------------------------- */

/*
 * Forward.  Replaces train_raytracing_relighting_CelebAHQ_DSSIM_8x.py:634 (depth), :635 (ambient), :636 (lighting), :638-639
 * (grey albedo) and :642 (BCE of PatchGAN's logits against ones).  All planes contiguous f32:
 *   depth          (B,1,H,W)          the network's depth
 *   gt_depth, mask (B,H,W,1)          batch depths and skin masks (the same memory order as depth)
 *   albedo         (B,3,H,W)          the network's albedo
 *   gt_albedo, mask_fill (B,H,W,1)    batch grey albedo and mask_fill_nose_and_mouth
 *   unit_light     (B,3)              unit_light_direction (B,3,1,1)
 *   ambient_values (B)                (B,1,1)
 *   lightings      (B,4)              batch lightings: [ambient, light direction]
 *   logits         (n_logits) or NULL PatchGAN's output for the composite; NULL: terms[4] is exactly 0 (n_logits is ignored)
 *   terms          (5) f32            depth, ambient, lighting, albedo, generator -- `generator_losses`' order:
 *                                     S_d / M,  2.5 (A / B),  L / B,  5 (S_a / M_f),  0.01 (G / n_logits), f32 operations on the
 *                                     f64 sums rounded to f32; an all-zero mask gives 0 / 0 = NaN, as torch does
 *   sums           (4) f64            { S_d = sum |depth m - gt_depth m|, M = sum m, S_a = sum |grey mf - gt_albedo mf|,
 *                                     M_f = sum mf }; the backward reads M and M_f from here
 *   workspace      gcfr_supervised_losses_workspace_bytes(B,H,W) = 8 * 5 * ceil(B H W / 1024) bytes of device scratch, 8-byte
 *                  aligned (0 is returned for an unsupported shape); it need not be cleared
 * 1 <= B <= 65535, 1 <= H, W <= 4096, B H W < 2^31, 1 <= n_logits < 2^31; anything else is GCFR_ERR_INVALID_ARGUMENT before a
 * launch.
 * Numerical contract: the stated operation order, exactly.  Per pixel, each one IEEE f32 operation (no contraction):
 * |depth m - gt_depth m|;  grey = ((a0 + a1) + a2) * (1.0f / 3.0f), |grey mf - gt_albedo mf|.  Per image:
 * |ambient_b - lightings[b,0]|;  1 - ((u0 l1 + u1 l2) + u2 l3).  Per logit, in f64: max(-x, 0) + log1p(exp(-|x|)).  The addends
 * are summed in f64 in a fixed order (lanes, waves, workgroups; no floating-point atomics): two calls return the same bits, and
 * the f32 restatement of this order (tests/supervised_losses_emulation.py) reproduces the terms to one ulp, the association of
 * the f64 sums being the only freedom.  Planes are read with 16-byte loads when H W is a multiple of 4 and every plane pointer is
 * 16-byte aligned, with 4-byte loads otherwise (same results).
 */
size_t gcfr_supervised_losses_workspace_bytes(int32_t B, int32_t H, int32_t W);
int gcfr_supervised_losses_fwd(const float *depth, const float *gt_depth, const float *mask, const float *albedo,
                               const float *gt_albedo, const float *mask_fill, const float *unit_light,
                               const float *ambient_values, const float *lightings, const float *logits, int64_t n_logits,
                               int32_t B, int32_t H, int32_t W, float *terms, double *sums, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * Backward of the above (what autograd replays for T8:634-639 and :642), one launch, every element written once:
 *   sums                       the forward's (M and M_f are read from it on the device)
 *   g_depth ... g_generator    DEVICE (1) f32 each or NULL: dLoss/d terms[0..4]; NULL writes zeros for that term's gradient
 *   grad_depth (B,1,H,W)       = ((g_depth / M) sgn(depth m - gt_depth m)) m
 *   grad_albedo (B,3,H,W)      = ((((g_albedo 5) / M_f) sgn(grey mf - gt_albedo mf)) mf) * (1.0f / 3.0f), the same in the three channels
 *   grad_ambient_values (B)    = ((g_ambient 2.5) / B) sgn(ambient_b - lightings[b,0])
 *   grad_unit_light (B,3)      = (-(g_lighting / B)) lightings[b,1+c]
 *   grad_logits (n_logits)     = ((g_generator 0.01) / n_logits) (-(1 / (1 + e^x))); required when logits is given, untouched otherwise
 * sgn(0) = 0 (and sgn(NaN) = 0), M and M_f rounded to f32, each operation one IEEE f32 operation, left to right; e^x is
 * evaluated from plain f32 operations (clamp to [-87, 88], Cody-Waite reduction, a degree-5 polynomial, ldexp), within ~2 ulp.
 * Bit-reproducible, and bit-equal to the f32 restatement of this order (tests/supervised_losses_emulation.py).  No output may
 * alias an input.
 */
int gcfr_supervised_losses_bwd(const float *depth, const float *gt_depth, const float *mask, const float *albedo,
                               const float *gt_albedo, const float *mask_fill, const float *ambient_values,
                               const float *lightings, const float *logits, int64_t n_logits, int32_t B, int32_t H, int32_t W,
                               const double *sums, const float *g_depth, const float *g_ambient, const float *g_lighting,
                               const float *g_albedo, const float *g_generator, float *grad_depth, float *grad_albedo,
                               float *grad_unit_light, float *grad_ambient_values, float *grad_logits, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The light-rig stage: the L per-light shadings of the many-lights path combined, with a colour x weight per light, into ONE relit
 * image per face (an area light as a cone of directions, a coloured key / fill / rim set, a sampled environment), as one forward
 * and one backward launch (csrc/gcfr_light_rig.hip).  No existing entry point changes: the stage reads the `final` plane that
 * gcfr_render_fwd / gcfr_render_from_depth_fwd write, and its g_final is what gcfr_render_bwd accepts as `g_final`.
 * ------------------------------------------------------------------------------------------- */

/*
 * Forward, one launch.  All planes contiguous f32:
 *   final_shading (B,L,H,W)            the many-lights `final` (T8:518 per light)
 *   albedo        (B,3,H,W)
 *   rgb           (rgb_batch,L,3)      colour x weight of every light; rgb_batch = B (a rig per face) or 1 (one rig for all faces)
 *   rendered      (B,3,H,W) out  =     albedo[b,c,p] * shading_rgb[b,c,p]
 *   shading_rgb   (B,3,H,W) out  =     sum_l rgb[b,l,c] * final_shading[b,l,p];  may be NULL (then it is not written)
 * The colour weights the whole per-light shading, its ambient term included: weights that sum to 1 count the ambient once.
 * B >= 1, 1 <= L <= 4096, H, W >= 1 (any parity) with H W < 2^31 and B ceil(H W / 1024) < 2^31, rgb_batch = 1 or B; anything else,
 * or a NULL among final_shading / albedo / rgb / rendered, is GCFR_ERR_INVALID_ARGUMENT before a launch.
 * Numerical contract: the stated operation order, exactly.  Every product and sum is one IEEE f32 operation (no contraction):
 * acc = rgb[0,c] final[0]; acc = acc + rgb[l,c] final[l] for l = 1 .. L-1 in ascending order (no add to zero); rendered = albedo acc.
 * Nothing is clamped (negative and zero weights are legal) and non-finite values propagate as IEEE arithmetic propagates them.
 * Bit-reproducible, and bit-equal to the f32 restatement of this order (tests/light_rig_emulation.py); at L = 1 and rgb = 1 it is
 * gcfr_shade_fwd's composite.  Planes are read and written with 16-byte accesses when H W is a multiple of 4 and every plane pointer
 * is 16-byte aligned, with 4-byte accesses otherwise (same results).  The uint8 composite is not written here: pass `rendered` to
 * gcfr_inference_images_u8 with L = 1.  No output may alias an input.
 */
int gcfr_light_rig_fwd(const float *final_shading, const float *albedo, const float *rgb, int32_t rgb_batch, int32_t B, int32_t L,
                       int32_t H, int32_t W, float *rendered, float *shading_rgb, void *stream);

/*
 * Backward of the above, one launch.  final_shading, albedo, rgb and the shape as in the forward (shading_rgb is recomputed, the
 * forward's copy is not read):
 *   g_rendered    (B,3,H,W) f32 or NULL   dLoss/d rendered
 *   g_shading_rgb (B,3,H,W) f32 or NULL   dLoss/d shading_rgb; at least one of the two must be given.  With
 *                                         u[c] = g_shading_rgb[c] + g_rendered[c] * albedo[c] (an absent term is not formed):
 *   g_final  (B,L,H,W) f32 or NULL    =   (rgb[b,l,0] u[0] + rgb[b,l,1] u[1]) + rgb[b,l,2] u[2]
 *   g_albedo (B,3,H,W) f32 or NULL    =   g_rendered[c] * shading_rgb[c]  (zeros without g_rendered)
 *   g_rgb    (rgb_batch,L,3) F64 or NULL  +=  sum_p final_shading[b,l,p] u[c,p], for rgb_batch = 1 also summed over b.  ACCUMULATED:
 *                                         the caller clears it (as grad_light_pt / grad_ambient of gcfr_render_bwd) and rounds to f32
 * At least one output must be given; a NULL output is skipped.  Each f32 product and sum is one IEEE operation in the stated order,
 * channels 0, 1, 2, the first product initialising: g_final and g_albedo are bit-reproducible and bit-equal to the f32 restatement.
 * g_rgb: a lane adds the (exact) f64 products of its four pixels, a wave reduces them through a shuffle tree, the workgroup adds
 * the waves' sums in LDS and adds its totals to g_rgb with one f64 atomic per entry (wave reduction + f64 atomics, no finishing
 * pass): the order of these f64 additions is free, so two calls may differ in the last bits of the f64 sum -- after the rounding to
 * f32, by one ulp of sum_p |final_shading u| at the most.
 */
int gcfr_light_rig_bwd(const float *final_shading, const float *albedo, const float *rgb, int32_t rgb_batch, int32_t B, int32_t L,
                       int32_t H, int32_t W, const float *g_rendered, const float *g_shading_rgb, float *g_final, float *g_albedo,
                       double *g_rgb, void *stream);

/*
 * Rig frames, one launch (csrc/gcfr_rig_frames.hip): F rigs per face combined with the per-light shadings of ONE many-lights pass
 * and pasted into the photograph, straight to uint8 frames -- an animated rig or a turntable of an environment map.  It replaces,
 * per frame, gcfr_light_rig_fwd above followed by gcfr_inference_images_u8 at L = 1 (the scripts' S1:601-620 / SLT:567-572 on
 * T8:519-522's composite); the f32 `rendered` is not written.  All planes contiguous:
 *   final_shading (B,L,H,W) f32            the many-lights `final` (T8:518 per light)
 *   albedo        (B,3,H,W) f32
 *   input_hwc     (B,H,W,3) f32            the photographs, as gcfr_inference_images_u8 takes them
 *   mask          (mask_batch,H,W) u8      the compositing mask as stored on disk; mask_batch = B or 1
 *   mask_f32      0 / 1                    the mask's quotient in f64 (S1:580) or in f32, widened (SLT:540), as gcfr_inference_images_u8
 *   rgb           (rgb_batch,F,L,3) f32    colour x weight of every light of every frame; rgb_batch = B (rigs per face) or 1
 *   frames        (B,F,H,W,3) u8 out       RGB, HWC
 * B >= 1, 1 <= L <= 4096, 1 <= F <= 4096, H, W >= 1 (any parity) with H W < 2^31 and B ceil(H W / 1024) < 2^31; anything else, a
 * NULL pointer, mask_batch / rgb_batch other than 1 / B or mask_f32 other than 0 / 1 is GCFR_ERR_INVALID_ARGUMENT before the
 * launch.  Allocates nothing, never synchronises, may be captured into a graph.  No output may alias an input.
 * Numerical contract: frames[b,f] equals, BYTE FOR BYTE, gcfr_light_rig_fwd with rgb[.,f] followed by gcfr_inference_images_u8 with
 * L = 1 on its `rendered`, by construction: per pixel and channel the rig stage's chain, every product and sum one IEEE f32
 * operation -- acc = rgb[f,0,c] final[0]; acc = acc + rgb[f,l,c] final[l] for l = 1 .. L-1 ascending; rendered = albedo[c] acc --
 * and then the image kernel's own composite (one shared device function, csrc/gcfr_composite.hpp):
 *   m = mask_f32 ? (double)((float)mk / 255.0f) : (double)mk / 255.0
 *   byte = saturate(rint(m > 0 ? (double)(255.0f * rendered) * m : (double)input * 255.0))      round half to even; NaN -> 0
 * Nothing is clamped before the quantisation.  Bit-equal to the composition of the two restatements
 * (tests/rig_frames_emulation.py).  Planes move in 16-byte accesses and a frame's 12 bytes per four pixels in three dword stores
 * when H W is a multiple of 4, final_shading / albedo / input_hwc are 16-byte aligned and mask / frames 4-byte aligned; one
 * element at a time otherwise (same results).  A plane of final_shading is read ceil(F / 4) times, not F times.
 */
int gcfr_light_rig_frames_u8(const float *final_shading, const float *albedo, const float *input_hwc, const uint8_t *mask,
                             int32_t mask_batch, int32_t mask_f32, const float *rgb, int32_t rgb_batch, int32_t B, int32_t L,
                             int32_t F, int32_t H, int32_t W, uint8_t *frames, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Full-resolution relighting (csrc/gcfr_fullres.hip): the two ends of the inference path around the network's resolution (h, w).
 * The photograph is (s h, s w) with s = 1, 2, 4 or 8 (H = s h, W = s w; every bilinear weight is then a multiple of 1 / (2 s),
 * exact in f32).  All arrays contiguous:
 *   photo_u8   (B,H,W,3) u8                 the photographs, RGB, HWC
 *   x_lo       (B,h,w,3) f32                the network's input: what gcfr_ingest_photographs_u8 writes
 *   rendered   (B,L,3,h,w) f32              the relit images of ONE many-lights pass
 *   mask_u8    (mask_batch,h,w) u8          the compositing mask AT THE NETWORK'S RESOLUTION, as stored on disk; mask_batch = B or 1
 *   out_u8     (B,L,H,W,3) u8 out
 * Every operation is one separately rounded IEEE f32 operation unless marked f64; max / min are fmaxf / fminf.
 *   Ingest:  x_lo[b,i,j,c] = (float)((double)S / (255.0 s s)), S the integer sum of the s x s block of bytes; at s = 1 the bits of
 *            np.float32(img / 255.0) (S1:515/580).
 *   Up(a), bilinear with half-pixel centres, per axis and hi-res index y: fy = max((y + 0.5) / s - 0.5, 0), y0 = floor(fy),
 *            t = fy - y0, y1 = min(y0 + 1, n - 1) (all exact); horizontal first on both rows as a0 + tx (a1 - a0), then
 *            top + ty (bot - top).  A constant field is returned exactly.  Both taps are always read (a tap of weight 0 still
 *            carries a NaN into its pixel).
 *   Composite, per hi-res pixel, light l and channel c:
 *            p = (float)photo_u8;  xl = Up(x_lo[..., c]) 255.0f;  d = min(max(p / max(xl, floor), 1.0f / detail_clamp), detail_clamp)
 *            m = Up((float)mask_u8 / 255.0f);  r = Up(rendered[b,l,c]) 255.0f;  v = p + m (r d - p)
 *            byte = m > 0 ? saturate(rint((double)v)) : photo_u8       the image kernel's quantisation (round half to even, NaN -> 0)
 *   `floor` (in grey levels) keeps the quotient finite in the dark; `detail_clamp` bounds it to [1 / detail_clamp, detail_clamp].
 *   Outside the mask (m = 0) the photograph's byte is copied: nothing in `rendered` can reach it.  The mask BLENDS here (the
 *   low-resolution composite pastes rendered * mask).
 * B, h, w >= 1 (any parity), 1 <= L <= 4096, H W < 2^31 and B ceil(H W / 1024) < 2^31; anything else, a NULL pointer, s not in
 * {1,2,4,8}, mask_batch other than 1 / B, out_u8 == photo_u8, detail_clamp < 1 or floor <= 0 (or either a NaN) is
 * GCFR_ERR_INVALID_ARGUMENT before the launch.  One launch each; allocates nothing, never synchronises, may be captured into a
 * graph.  No output may alias an input.  Bit-equal to the numpy restatement (tests/fullres_emulation.py).  The composite moves the
 * photograph's and each light's 12 bytes per four pixels as three dwords when W is a multiple of 4 and photo_u8 / out_u8 are 4-byte
 * aligned (the ingest: w a multiple of 4, photo_u8 4-byte and x_lo_out 16-byte aligned); one element at a time otherwise (same
 * results).  The photograph, x_lo and the mask are read once per pixel, not once per light.
 */
int gcfr_ingest_photographs_u8(const uint8_t *photo_u8, int32_t B, int32_t h, int32_t w, int32_t s, float *x_lo_out, void *stream);
int gcfr_fullres_composites_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                               int32_t mask_batch, int32_t B, int32_t L, int32_t h, int32_t w, int32_t s, float floor,
                               float detail_clamp, uint8_t *out_u8, void *stream);

/*
 * The same composite with an EDGE-AWARE (joint-bilateral) upsample Up_J, guided by the photograph, in place of the bilinear Up
 * (csrc/gcfr_fullres_guided.hip): the relighting gain no longer mixes the two sides of an edge the network's resolution does not
 * see, and the mask no longer leaks across it.  Operands, layouts and limits are gcfr_fullres_composites_u8's; `range_sigma` is in
 * grey levels.  Every operation is one separately rounded IEEE f32 operation; the divisions are correctly rounded.
 *   Taps, per axis and hi-res index y of a low-resolution axis of n, in integers: u = max(2 y + 1 - s, 0), y0 = u div 2 s,
 *            r = u mod 2 s (Up's u and y0).  The four taps are clamp(y0 - 1 + j, 0, n - 1), j = 0..3, with the integer weights
 *            (2 s - r, 4 s - r, 2 s + r, r) over 4 s: a tent of radius two low-resolution pixels.  The four sum to 2, each is exact
 *            in f32 (sy[j], sx[i]) and so is sy[j] sx[i].  A tap replicated at a border keeps its own weight.
 *   Weights, once per hi-res pixel P, the same for every light.  p[c] = (float)photo_u8[P, c]; for tap (j, i) at low-resolution
 *            pixel q, g[c] = x_lo[q, c] 255.0f:
 *              e[c] = p[c] - g[c];  d2 = (e[0] e[0] + e[1] e[1]) + e[2] e[2];  k = 1.0f / (1.0f + d2 inv)
 *              wt = (sy[j] sx[i]) k;  den = the sum of the 16 wt, row-major (j outer, i inner), starting from wt[0][0]
 *              rcp = 1.0f / den;  wn = wt rcp
 *            with inv = 1.0f / (range_sigma range_sigma) formed once on the host in f32.  k is a Lorentzian range kernel: no
 *            transcendental.  range_sigma = +inf gives inv = 0 and k = 1: the spatial tent alone, den == 4 exactly.
 *   Up_J(a)(P) = the sum over the 16 taps, row-major, of wn[j][i] a[tap]: the first product starts the sum and every product and
 *            sum is rounded.  All 16 taps are always read (a tap of weight 0 still carries a NaN into its pixel).
 *   Composite: the one above with Up_J in all three places and the SAME wn for each:
 *            xl = Up_J(x_lo[..., c]) 255.0f;  d = min(max(p / max(xl, floor), 1.0f / detail_clamp), detail_clamp)
 *            m = Up_J((float)mask_u8 / 255.0f);  r = Up_J(rendered[b,l,c]) 255.0f;  v = p + m (r d - p)
 *            byte = m > 0 ? saturate(rint((double)v)) : photo_u8
 *   Consequences: rendered == x_lo with no pixel clamped (d strictly inside its bounds, xl >= floor) returns the photograph in
 *   every byte.  A NaN in x_lo makes m a NaN at the pixels it reaches (it is in their wn), so they keep the photograph's byte.  A
 *   NaN in `rendered` alone gives byte 0 where m > 0.
 * Refusals: gcfr_fullres_composites_u8's, and range_sigma <= 0 or a NaN; GCFR_ERR_INVALID_ARGUMENT before the launch.  One launch;
 * allocates nothing, never synchronises, may be captured into a graph.  Bit-equal to the numpy restatement
 * (tests/fullres_guided_emulation.py).  The weights, d and m are formed once per pixel; per light a pixel costs 3 x 16 products and
 * sums, the blend and the quantisation.  Three dwords per four pixels on the same conditions as above; one element at a time
 * otherwise (same results).
 */
int gcfr_fullres_composites_guided_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                      int32_t mask_batch, int32_t B, int32_t L, int32_t h, int32_t w, int32_t s, float floor,
                                      float detail_clamp, float range_sigma, uint8_t *out_u8, void *stream);

/*
 * The same two ends for a FACE BOX inside a larger photograph (csrc/gcfr_fullres_box.hip): a box of any integer size and position
 * in a photograph of any size goes in; the photograph, relit inside the box and untouched outside it, comes out.  A strict
 * generalisation of the two entries at the top of this section: with the box the whole photograph and bh = s h, bw = s w,
 * s in {1, 2, 4, 8}, both return those entries' bits.  All arrays contiguous:
 *   photo_u8   (B,Hp,Wp,3) u8               the photographs, RGB, HWC
 *   boxes      (B,4) int32, HOST            one box (x0, y0, bw, bh) per face, in photograph pixels
 *   x_lo       (B,h,w,3) f32                the network's input: what gcfr_ingest_box_u8 writes
 *   rendered   (B,L,3,h,w) f32              the relit images of ONE many-lights pass
 *   mask_u8    (mask_batch,h,w) u8          the compositing mask at the network's resolution, IN THE BOX'S FRAME; mask_batch = B or 1
 *   out_u8     paste = 1: (B,L,Hp,Wp,3) u8 out, the photograph with the box relit
 *              paste = 0: (B,L,bh,bw,3) u8 out, the box alone; all faces of the call then share one (bw, bh)
 * `boxes` IS A HOST POINTER -- the one place this ABI takes a host array.  The entry reads it during the call, validates every box
 * on the host and hands the boxes to the kernels BY VALUE in their argument blocks, 32 faces per launch (a larger B is a short
 * loop of launches): the array may be freed or changed as soon as the call returns, nothing is uploaded, no device scratch is
 * needed, and the values are baked into the launches, so the call may be captured into a graph.
 * Box rules, each GCFR_ERR_INVALID_ARGUMENT before any launch: 0 <= x0, x0 + bw <= Wp, 0 <= y0, y0 + bh <= Hp; bw >= w and
 * bh >= h (the box is never smaller than the network's input); 2 bh h and 2 bw w fit 31 bits; Hp Wp < 2^31 and
 * B ceil(Hp Wp / 1024) < 2^31.  The two axes are independent: bh / h need not equal bw / w, and neither needs to be an integer.
 * Every operation is one separately rounded IEEE f32 operation unless marked otherwise.
 *   Box ingest, an exact area mean in integers.  On the row axis photograph row y of the box and low-resolution row i overlap by
 *            the integer wy(i,y) = max(0, min((y+1) h, (i+1) bh) - max(y h, i bh)), which lies in [0, h]; columns use the same
 *            formula.  S[i,j,c] = sum of wy wx byte, an exact integer of at most 255 bh bw (64-bit).
 *            x_lo = (float)((double)S / (255.0 bh bw)): the denominator is exact in f64, the quotient is rounded once to f32.
 *   Up over the box, per axis and box-relative index y: N = max((2y+1) h - bh, 0), y0 = N div (2 bh), rem = N - y0 2 bh,
 *            t = (float)((double)rem / (double)(2 bh)), y1 = min(y0 + 1, h - 1): exact integer work but for the one rounding of
 *            t.  The lerps and their order are Up's above: horizontal a0 + tx (a1 - a0) on both rows, then top + ty (bot - top).
 *            Both taps are always read.
 *   Composite: inside the box the p, xl, d, m, r, v above, then byte = m > 0 ? saturate(rint((double)v)) : photo_u8 (the same
 *            device functions as gcfr_fullres_composites_u8).  A pixel of the output window outside the box is the photograph's
 *            byte, for every light.
 * Refusals: everything gcfr_fullres_composites_u8 refuses (but there is no `s`), the box rules, a NULL `boxes`, `paste` outside
 * {0, 1}, boxes of different sizes with paste = 0, and an out_u8 whose bytes overlap photo_u8's.  Allocates nothing, never
 * synchronises.  Bit-equal to the numpy restatement (tests/fullres_box_emulation.py).  The composite moves each light's 12 bytes
 * per four pixels as three dwords when the output window's width (Wp, or bw with paste = 0) is a multiple of 4 and out_u8 is
 * 4-byte aligned; one element at a time otherwise (same results).  The photograph, x_lo, the mask, the taps and both weights are
 * formed once per pixel, not once per light.
 */
int gcfr_ingest_box_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int32_t *boxes, int32_t h, int32_t w,
                       float *x_lo_out, void *stream);
int gcfr_fullres_composites_box_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                   int32_t mask_batch, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int32_t *boxes, int32_t h,
                                   int32_t w, int32_t paste, float floor, float detail_clamp, uint8_t *out_u8, void *stream);

/*
 * The box composite with the EDGE-AWARE upsample Up_J of gcfr_fullres_composites_guided_u8 in place of the bilinear Up
 * (csrc/gcfr_fullres_box_guided.hip): the guided upsample over a face box of any integer size and position.  Operands, layouts, box
 * rules and `paste` are exactly gcfr_fullres_composites_box_u8's, plus `range_sigma` (grey levels, > 0, +inf allowed).  Every
 * operation is one separately rounded IEEE f32 operation unless marked otherwise; the divisions are correctly rounded.
 *   Taps, per axis with box-relative index y, box extent b and low-resolution extent n.  The integers are Up-over-the-box's:
 *            N = max((2y+1) n - b, 0), y0 = N div 2b, rem = N - y0 2b.  The four taps are clamp(y0 - 1 + j, 0, n - 1), j = 0..3.
 *            Their weights are the integers (2b - rem, 4b - rem, 2b + rem, rem) over 4b, each formed as
 *            (float)((double)k / (double)(4b)) with one rounding (sy[j], sx[i]): a tent of radius two low-resolution pixels about
 *            the pixel's half-pixel centre.  The four integers sum to 8b.  A tap replicated at a border keeps its own weight.
 *            4b < 2^32 follows from the box rule 2 b n < 2^31.  At b = s n the weights are the exact k / (4s) of
 *            gcfr_fullres_composites_guided_u8.
 *   Weights, Up_J and the composite are gcfr_fullres_composites_guided_u8's, unchanged in formula and order.  p is the
 *            photograph's pixel inside the box; for tap (j, i) at low-resolution pixel q, g[c] = x_lo[q, c] 255.0f:
 *              e[c] = p[c] - g[c];  d2 = (e[0] e[0] + e[1] e[1]) + e[2] e[2];  k = 1.0f / (1.0f + d2 inv)
 *              wt = (sy[j] sx[i]) k;  den = the sum of the 16 wt, row-major (j outer, i inner), starting from wt[0][0]
 *              rcp = 1.0f / den;  wn = wt rcp
 *            with inv = 1.0f / (range_sigma range_sigma) formed once on the host in f32.  The product sy[j] sx[i] is a ROUNDED f32
 *            product here (it is exact only where both weights are: at b = s n); with range_sigma = +inf, |den - 4| <= 72 x 2^-24.
 *            Up_J(a) = the sum over the 16 taps, row-major, of wn[j][i] a[tap], the first product starting the sum; all 16 taps
 *            are always read.  Inside the box:
 *              xl = Up_J(x_lo[..., c]) 255.0f;  d = min(max(p / max(xl, floor), 1.0f / detail_clamp), detail_clamp)
 *              m = Up_J((float)mask_u8 / 255.0f);  r = Up_J(rendered[b,l,c]) 255.0f;  v = p + m (r d - p)
 *              byte = m > 0 ? saturate(rint((double)v)) : photo_u8
 *            through the same device functions as the three entries above.  A pixel of the output window outside the box is the
 *            photograph's byte, for every light.  mask_u8 stays low-resolution, in the box's frame.
 *   Anchor, with no tolerance: with the box the whole photograph and bh = s h, bw = s w, s in {1, 2, 4, 8}, the bytes are those of
 *            gcfr_fullres_composites_guided_u8.  The consequences stated there (identity, NaNs) hold here over the box.
 * Refusals: gcfr_fullres_composites_box_u8's, and range_sigma <= 0 or a NaN; GCFR_ERR_INVALID_ARGUMENT before any launch.  32 faces
 * per launch with the boxes by value; allocates nothing, never synchronises, may be captured into a graph.  Bit-equal to the numpy
 * restatement (tests/fullres_box_guided_emulation.py).  Three dwords per four pixels on gcfr_fullres_composites_box_u8's
 * conditions; one element at a time otherwise (same results).  The taps, the weights, d and m are formed once per pixel; per light a
 * pixel costs 3 x 16 loads, products and sums, the blend and the quantisation.
 */
int gcfr_fullres_composites_box_guided_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                          int32_t mask_batch, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int32_t *boxes,
                                          int32_t h, int32_t w, int32_t paste, float floor, float detail_clamp, float range_sigma,
                                          uint8_t *out_u8, void *stream);

/*
 * The box entries WITHOUT the rule bw >= w, bh >= h (csrc/gcfr_fullres_anybox.hip): a face smaller than the network's input on
 * either axis, or on both.  Operands, layouts, the host `boxes`, `paste` and the parameter lists are exactly gcfr_ingest_box_u8's
 * and gcfr_fullres_composites_box_u8's; the two entries above keep refusing small boxes.  Each axis is treated on its own; below,
 * an axis has the box's length nb (bh or bw) and the network's length n (h or w).
 * Box rules, each GCFR_ERR_INVALID_ARGUMENT before any launch: 0 <= x0, x0 + bw <= Wp, 0 <= y0, y0 + bh <= Hp; nb >= 1 and
 * 8 nb >= n on both axes (the cap bounds every loop below at nine taps per axis); 2 bh h and 2 bw w fit 31 bits; Hp Wp < 2^31 and
 * B ceil(Hp Wp / 1024) < 2^31; with paste = 0 all boxes share one size.
 *   Ingest, one exact integer and one rounding for all four axis combinations:
 *            x_lo[i,j,c] = (float)((double)S / (255.0 Dy Dx)), S = sum_y sum_x wy wx byte in 64 bits.
 *            Axis with nb >= n (gcfr_ingest_box_u8's area mean): wy(i,y) = max(0, min((y+1) n, (i+1) nb) - max(y n, i nb)), D = nb.
 *            Axis with nb < n (magnify; half-pixel-centre bilinear in integers): N = max((2i+1) nb - n, 0), i0 = N div 2n,
 *            rem = N - i0 2n, i1 = min(i0 + 1, nb - 1); tap i0 weighs 2n - rem and tap i1 weighs rem (where i1 = i0 the pixel
 *            receives both weights), D = 2n.  255 Dy Dx is exact in f64.
 *   Carry to the box: the operator that the box entries call Up, applied to x_lo, to the mask quotient (float)mask_u8 / 255.0f
 *            and to every plane of `rendered`.  Separable: horizontal first on every tap row, each result rounded to f32, then
 *            vertical.
 *            Axis with nb >= n: Up-over-the-box's two taps and t, and one lerp a0 + t (a1 - a0) in f32.
 *            Axis with nb < n (minify; exact-footprint area mean): box index y overlaps network index i by
 *            wt(y,i) = max(0, min((i+1) nb, (y+1) n) - max(i nb, y n)); i runs from (y n) div nb to ceil((y+1) n / nb) - 1, at
 *            most nine taps, whose weights sum to n.  The value is (float)(acc / (double)n), acc the f64 sum, starting from +0.0,
 *            of (double)wt (double)v in ascending i.  wt <= nb < 2^15, so every product is exact; every f64 addition is separate.
 *   Composite: inside the box the p, xl, d, m, r, v and the byte of gcfr_fullres_composites_u8 through the same device functions,
 *            with the carrying operator in the place of Up.  A pixel of the output window outside the box is the photograph's
 *            byte, for every light.  mask_u8 stays at the network's resolution, in the box's frame.
 *   Anchor, with no tolerance: with bw >= w and bh >= h every formula is the box entries' own and the bits and bytes are theirs.
 * Refusals: gcfr_ingest_box_u8's and gcfr_fullres_composites_box_u8's with the box rules above.  32 faces per launch with the boxes
 * by value; allocates nothing, never synchronises, may be captured into a graph.  Bit-equal to the numpy restatement
 * (tests/fullres_anybox_emulation.py).  Three dwords per four pixels on gcfr_fullres_composites_box_u8's conditions, the copy outside
 * the box included; one element at a time otherwise (same results).
 */
int gcfr_ingest_anybox_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int32_t *boxes, int32_t h, int32_t w,
                          float *x_lo_out, void *stream);
int gcfr_fullres_composites_anybox_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                      int32_t mask_batch, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int32_t *boxes,
                                      int32_t h, int32_t w, int32_t paste, float floor, float detail_clamp, uint8_t *out_u8,
                                      void *stream);

/*
 * GROUP PHOTOGRAPHS (csrc/gcfr_fullres_group.hip): every face of a photograph relit in one pass over the photograph's bytes.  The
 * any-size entries above take one box per photograph and return one photograph per face; here B >= 1 faces are spread over P
 * photographs and ONE photograph per photograph comes back.
 *   photo_u8     (P,Hp,Wp,3) u8
 *   boxes        (B,4) i32 HOST (x0, y0, bw, bh) under gcfr_ingest_anybox_u8's box rules (inside the photograph, bw, bh >= 1,
 *                8 bw >= w, 8 bh >= h, 2 bh h and 2 bw w in 31 bits)
 *   photo_index  (B,) i32 HOST, 0 <= photo_index[b] < P: the photograph of face b.  Any order; a photograph may have no face, one
 *                face or many, more than 32 included.  Read during the call like `boxes`, and handed to the kernels by value.
 *   x_lo         (B,h,w,3) f32;  rendered (B,L,3,h,w) f32;  mask_u8 (mask_batch,h,w) u8, mask_batch in {1, B}: per FACE, in the
 *                box's frame, exactly as gcfr_fullres_composites_anybox_u8 takes them
 *   out_u8       (P,L,Hp,Wp,3) u8 out
 * Ingest: x_lo_out[b] is gcfr_ingest_anybox_u8's ingest of box b of photograph photo_index[b] -- the bits that entry returns for
 * the gathered photographs photo_u8[photo_index] -- and the photographs are neither gathered nor copied.
 * Composite: for every photograph q and every light l the result is the CHAIN of gcfr_fullres_composites_anybox_u8's pasted
 * composite over the faces of q (photo_index[b] = q) in ascending face index b.  The running image starts as the photograph.  Face b
 * applies that entry's composite (the carrying operator, p, xl, d, m, r, v and the byte, through the same device functions) inside
 * its box, with the RUNNING bytes wherever that entry reads the photograph's: p in the blend v = p + m (r d - p) and p in the
 * quotient d.  x_lo, rendered and the mask are face b's own.  Where face b's carried mask m is 0, and outside its box, the running
 * byte is kept.  Every step rounds to a byte, as a call of that entry does.
 *   Consequences.  Where at most one face relights a pixel (m > 0 inside its box), the byte is
 *            gcfr_fullres_composites_anybox_u8's.  Where two carried masks are positive, the second face's relighting gain
 *            multiplies the first face's result, up to the clamps and the intermediate byte: order matters there and nowhere else.
 *            A photograph without faces is returned as it is, for every light.  All faces of a photograph share the light index l.
 *   Anchor, with no tolerance anywhere, overlaps included: the result equals gcfr_fullres_composites_anybox_u8 (paste = 1) called
 *            once per face with the L lights as its batch -- photo_u8 the running (L,Hp,Wp,3), the box and x_lo[b] repeated L
 *            times, rendered[b] passed as (L,1,3,h,w) -- and its output taken as the next running image.  With
 *            photo_index[b] = b and P = B the bytes are those of ONE call of that entry.
 * Refusals, each GCFR_ERR_INVALID_ARGUMENT before any launch: a NULL pointer (`boxes` and `photo_index` included); B < 1, P < 1; the
 * box rules; a photo_index outside [0, P); everything gcfr_fullres_composites_u8 refuses of L, mask_batch, detail_clamp and floor;
 * Hp Wp >= 2^31 or P ceil(Hp Wp / 1024) >= 2^31; an out_u8 whose bytes overlap photo_u8's (the ingest: x_lo_out == photo_u8).
 * There is no paste = 0, no guided carrying and no gradient.
 * Launches: a workgroup owns 1024 consecutive pixels of ONE photograph and walks that photograph's faces in order; a launch covers
 * whole photographs with at most 32 face slots in all (boxes, face indices and each photograph's slot range by value: nothing is
 * uploaded, no device scratch, capture-safe).  The running bytes live in out_u8: the first face that relights a pixel starts from
 * the photograph's bytes, a later one reads back what the same thread stored for that light.  A photograph with more than 32 faces
 * gets continuation launches on the same stream, which start from out_u8 and write only what their faces relight.  A pixel no face
 * relights is copied once per light.  Three dwords per four pixels when Wp is a multiple of 4 and out_u8 is 4-byte aligned; one
 * element at a time otherwise (same results).  Allocates nothing on the device, never synchronises.  Bit-equal to the numpy
 * restatement (tests/fullres_group_emulation.py).
 */
int gcfr_ingest_group_u8(const uint8_t *photo_u8, int32_t P, int32_t Hp, int32_t Wp, const int32_t *boxes, const int32_t *photo_index,
                         int32_t B, int32_t h, int32_t w, float *x_lo_out, void *stream);
int gcfr_fullres_composites_group_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                     int32_t mask_batch, int32_t P, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int32_t *boxes,
                                     const int32_t *photo_index, int32_t h, int32_t w, float floor, float detail_clamp,
                                     uint8_t *out_u8, void *stream);

/*
 * ROTATED FACES (csrc/gcfr_fullres_affine.hip): the two ends for a face under a 2 x 3 AFFINE MAP -- the similarity a face aligner
 * reports -- in the place of an axis-aligned box.  The ingest samples the photograph through the map into the network's input; the
 * composite carries the L relit images back through the inverse map onto the photograph's own pixels, one launch for all lights.
 *   photo_u8   (B,Hp,Wp,3) u8               the photographs, RGB, HWC
 *   F, I       (B,2,3) int64, HOST          one map per face, row-major (M00, M01, M02, M10, M11, M12), in units of 2^-14
 *                                           F: network -> photograph, (X, Y) = F (u, v, 1); I: photograph -> network
 *   x_lo       (B,h,w,3) f32                the network's input: what gcfr_ingest_affine_u8 writes
 *   rendered   (B,L,3,h,w) f32;  mask_u8 (mask_batch,h,w) u8 in the NETWORK'S frame, mask_batch = B or 1
 *   out_u8     (B,L,Hp,Wp,3) u8 out         the photograph with the face relit; there is no "box alone"
 * The entries take the matrices as GIVEN integers: the ingest reads only F, the composite reads only I; that the two are inverse
 * to each other is the caller's business (postprocess.quantise_affine derives both from one f64 matrix).  F and I are HOST pointers
 * like `boxes` above: read during the call, validated on the host and handed to the kernels by value, 32 faces per launch.
 * All geometry is in INTEGERS, fixed point with 14 fractional bits, ONE = 2^14: no float decides a tap or a weight, and every value
 * is rounded once.  Coordinates are continuous: pixel k covers [k, k+1) and its centre is k + 1/2, on both sides.
 *   Sub-sampling.  For a matrix M, K(M) is the smallest of 1, 2, 4, 8 with K^2 ONE^2 >= max(M00^2 + M10^2, M01^2 + M11^2), an
 *            integer comparison: how many sub-samples per axis a destination pixel takes when a step of one destination pixel
 *            crosses more than one source pixel (the scales 1, 2, 4, 8 and the rule 8 nb >= n above).  Let den = 2 K ONE.
 *            Destination pixel (x, y) has sub-samples (a, b) in [0, K)^2; sub-sample (a, b) has the source tap coordinate, already
 *            shifted by the half pixel,
 *              P0 = M00 (2Kx + 2a + 1) + M01 (2Ky + 2b + 1) + 2K M02 - K ONE,    P1 the same with row 1 of M,
 *            exact in 64 bits, in units of 1 / den.
 *   Ingest, K = K(F), per network pixel (column x = j, row y = i) and channel: S = the sum over the K^2 sub-samples (b outer, a
 *            inner) and the four taps of each of wy wx byte, where x0 = floor(P0 / den), fx = P0 - x0 den, the taps are x0 and
 *            x0 + 1 with weights den - fx and fx, and rows likewise with P1.  Tap indices are CLAMPED into the photograph
 *            (replicate): a face may hang over the photograph's edge.  S < 255 x 64 x 2^36 = 2^50, so (double)S is exact;
 *            x_lo = (float)((double)S / (255.0 K K (double)den (double)den)): one exact integer, one rounding.
 *            For F = (s ONE, 0, x0 ONE; 0, s ONE, y0 ONE), s in {1, 2, 4, 8}, the bits are gcfr_ingest_box_u8's on the box
 *            (x0, y0, s w, s h).
 *   Inside test.  Photograph pixel (x, y) belongs to the face iff its centre lands in the network square:
 *              c0 = I00 (2x+1) + I01 (2y+1) + 2 I02 lies in [0, 2 ONE w)  and  c1, with row 1, lies in [0, 2 ONE h).
 *            Every other pixel is the photograph's byte for every light.
 *   Carrier, K = K(I): applied to every channel of x_lo, to (float)mask_u8 / 255.0f and to every plane of `rendered`.  Per
 *            sub-sample: U = max(P0, 0), j0 = min(U div den, w - 1), fu = U - (U div den) den, j1 = min(j0 + 1, w - 1),
 *            tx = (float)((double)fu / (double)den), which is exact (den is a power of two, fu < 2^18); rows likewise with P1, h,
 *            i0, i1, ty.  The sub-sample's value is Up's lerps in Up's order: a00 + tx (a01 - a00) on both rows, then
 *            top + ty (bot - top).  With K = 1 that value is the carried value.  With K > 1 it is (float)(acc / (double)(K K)), acc
 *            the f64 sum, starting from +0.0, with b outer and a inner, of (double)value.
 *   Composite: inside, the p, xl, d, m, r, v above with the carrier in the place of Up, then byte = m > 0 ? saturate(rint((double)v))
 *            : photo_u8 (the same device functions as gcfr_fullres_composites_u8).
 *   Anchor, with no tolerance: with I the exact inverse of an axis-aligned F at s in {1, 2, 4} and integer x0, y0, every byte is
 *            gcfr_fullres_composites_box_u8's (paste = 1) on that box: the taps, t and the clamps coincide.
 * Refusals, each GCFR_ERR_INVALID_ARGUMENT before any launch: a NULL pointer (the matrix included); the pixel and chunk counts of
 * the box entries (Hp Wp, h w < 2^31, B ceil(Hp Wp / 1024) < 2^31); for the matrix the entry reads: det = M00 M11 - M01 M10 <= 0 (no
 * mirror image: a mirrored face would need a mirrored light), a column longer than 8 ONE, |M02| or |M12| > 2^40; everything
 * gcfr_fullres_composites_u8 refuses of L, mask_batch, detail_clamp and floor; an out_u8 whose bytes overlap photo_u8's (the
 * ingest: x_lo_out == photo_u8).  No gradient, no guided carrying, no perspective maps.
 * Allocates nothing, never synchronises, may be captured into a graph.  Bit-equal to the numpy restatement
 * (tests/fullres_affine_emulation.py).  Three dwords per four pixels when Wp is a multiple of 4 and out_u8 is 4-byte aligned, the
 * copy outside the face included; one element at a time otherwise (same results).  The inside test, the taps, d and m are formed
 * once per pixel, not once per light; with K > 1 the sub-samples' taps are recomputed per light.
 */
int gcfr_ingest_affine_u8(const uint8_t *photo_u8, int32_t B, int32_t Hp, int32_t Wp, const int64_t *F, int32_t h, int32_t w,
                          float *x_lo_out, void *stream);
int gcfr_fullres_composites_affine_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                      int32_t mask_batch, int32_t B, int32_t L, int32_t Hp, int32_t Wp, const int64_t *I, int32_t h,
                                      int32_t w, float floor, float detail_clamp, uint8_t *out_u8, void *stream);

/*
 * ROTATED FACES IN GROUP PHOTOGRAPHS (csrc/gcfr_fullres_group_affine.hip): every tilted face of a photograph relit in one pass over
 * the photograph's bytes.  The group entries above take only axis-aligned boxes; the affine entries above take one face per
 * photograph and return one photograph per face.  Here B >= 1 faces, each under its own pair of maps, are spread over P photographs
 * and ONE photograph per photograph comes back.
 *   photo_u8     (P,Hp,Wp,3) u8
 *   F, I         (B,2,3) int64 HOST, one pair per face under gcfr_ingest_affine_u8's rules: row-major, in units of 2^-14 (ONE =
 *                2^14); det > 0; no column longer than 8 ONE; |M02|, |M12| <= 2^40.  The ingest reads only F, the composite only I.
 *   photo_index  (B,) i32 HOST, 0 <= photo_index[b] < P: the photograph of face b.  Any order; a photograph may have no face, one
 *                face or many, more than 32 included.  Read during the call like the maps, and handed to the kernels by value.
 *   x_lo         (B,h,w,3) f32;  rendered (B,L,3,h,w) f32;  mask_u8 (mask_batch,h,w) u8, mask_batch in {1, B}: per FACE, in the
 *                network's frame, exactly as gcfr_fullres_composites_affine_u8 takes them
 *   out_u8       (P,L,Hp,Wp,3) u8 out
 * Ingest: x_lo_out[b] is gcfr_ingest_affine_u8's ingest of photograph photo_index[b] through F[b] (K(F[b]), P0, P1, the clamped
 * taps, S and the one division, as stated there) -- the bits that entry returns for the gathered photographs
 * photo_u8[photo_index] -- and the photographs are neither gathered nor copied.
 * Composite: for every photograph q and every light l the result is the CHAIN of gcfr_fullres_composites_affine_u8's composite over
 * the faces of q (photo_index[b] = q) in ascending face index b.  The running image starts as the photograph.  Face b applies that
 * entry's inside test (c0, c1 under I[b]), its carrier with K = K(I[b]), and its p, xl, d, m, r, v and byte through the same device
 * functions, with the RUNNING byte wherever that entry reads the photograph's: p in the blend v = p + m (r d - p) and p in the
 * quotient d.  x_lo, rendered and the mask are face b's own.  Outside face b's quad, and where its carried mask m is not positive,
 * the running byte is kept.  Every step rounds to a byte, as a call of that entry does.
 *   Consequences.  Where at most one face relights a pixel (inside its quad with m > 0), the byte is
 *            gcfr_fullres_composites_affine_u8's.  Where two faces relight a pixel, the second face's relighting gain multiplies the
 *            first face's result, up to the clamps and the intermediate byte: order matters there and nowhere else.  A photograph
 *            without faces is returned as it is, for every light.  All faces of a photograph share the light index l.
 *   Anchors, with no tolerance anywhere, overlaps included.
 *            1. The result equals gcfr_fullres_composites_affine_u8 called once per face with the L lights as its batch -- photo_u8
 *               the running (L,Hp,Wp,3), I[b] and x_lo[b] repeated L times, rendered[b] passed as (L,1,3,h,w) -- and its output
 *               taken as the next running image.
 *            2. With photo_index[b] = b and P = B the bytes are those of ONE call of that entry, and the ingest's bits those of ONE
 *               call of gcfr_ingest_affine_u8.
 *            3. With every I the exact inverse of an axis-aligned F at s in {1, 2, 4} and integer x0, y0, every byte is
 *               gcfr_fullres_composites_group_u8's on the boxes (x0, y0, s w, s h), overlapping boxes included: each link of this
 *               chain is that entry's link, by the affine entries' anchor and the any-size entries' anchor.
 * Refusals, each GCFR_ERR_INVALID_ARGUMENT before any launch: a NULL pointer (the maps and `photo_index` included); B < 1, P < 1;
 * the map rules, for every face; a photo_index outside [0, P); everything gcfr_fullres_composites_u8 refuses of L, mask_batch,
 * detail_clamp and floor; Hp Wp or h w >= 2^31 or P ceil(Hp Wp / 1024) >= 2^31; an out_u8 whose bytes overlap photo_u8's (the
 * ingest: x_lo_out == photo_u8).  No gradient, no guided carrying, no perspective maps, no boxes mixed with maps.
 * Launches: a workgroup owns 1024 consecutive pixels of ONE photograph and walks that photograph's faces in order; a face whose
 * reachable rows miss the workgroup's rows costs it no 64-bit work.  A launch covers whole photographs, at most 32 of them, with at
 * most 32 face slots in all (the I maps, K, the reachable rows, face indices and each photograph's slot range by value, about
 * 2.2 KB: nothing is uploaded, no device scratch, capture-safe).  The running bytes live in out_u8: the first face that relights a
 * pixel starts from the photograph's bytes, a later one reads back what the same thread stored for that light.  A photograph with
 * more than 32 faces is launched alone, 32 faces at a time; its continuation launches run on the same stream, start from out_u8
 * and write only what their faces relight.  A pixel no face relights is copied once per light.  Three dwords per four pixels when
 * Wp is a multiple of 4 and out_u8 is 4-byte aligned; one element at a time otherwise (same results).  The ingest takes 32 faces
 * per launch.  Allocates nothing on the device, never synchronises.  Bit-equal to the numpy restatement
 * (tests/fullres_group_affine_emulation.py).
 */
int gcfr_ingest_group_affine_u8(const uint8_t *photo_u8, int32_t P, int32_t Hp, int32_t Wp, const int64_t *F,
                                const int32_t *photo_index, int32_t B, int32_t h, int32_t w, float *x_lo_out, void *stream);
int gcfr_fullres_composites_group_affine_u8(const uint8_t *photo_u8, const float *x_lo, const float *rendered, const uint8_t *mask_u8,
                                            int32_t mask_batch, int32_t P, int32_t B, int32_t L, int32_t Hp, int32_t Wp,
                                            const int64_t *I, const int32_t *photo_index, int32_t h, int32_t w, float floor,
                                            float detail_clamp, uint8_t *out_u8, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Environment-map lighting: a lat-long radiance map integrated into the `rgb` (colour x weight per light) of the light-rig stage
 * above (csrc/gcfr_environment.hip).  Every texel belongs to the light direction nearest to it; a light's rgb is the
 * solid-angle-weighted sum of its texels.  No kernel evaluates a transcendental function: the trigonometry arrives in host-built
 * tables (lighting.environment_tables), all contiguous:
 *   rows     (He,2) f32   sin, cos of row r's polar angle theta_r = pi (r + 1/2) / He, measured from +y
 *   cols     (We,2) f32   sin, cos of column c's azimuth phi_c = 2 pi (c + 1/2) / We - pi (the centre column faces +z)
 *   row_w    (He,)  F64   the row's solid angle per texel over 4 pi: (cos theta_top - cos theta_bottom) / (2 We); 8-byte aligned
 *   dirs_map (L,3)  f32   the light directions IN THE MAP'S FRAME (a rotation is the caller's matmul; nothing is rotated here)
 *   cell     (He,We) i32  the index of the texel's light, or -1
 * 1 <= L <= 4096, He, We >= 1 with He We <= 2^24, 1 <= E <= 65535; anything else, a NULL pointer or a misaligned row_w is
 * GCFR_ERR_INVALID_ARGUMENT before a launch.  The entries allocate nothing and never synchronise.
 * ------------------------------------------------------------------------------------------- */

/*
 * The cell map, one launch.  Per texel (row r, column c): omega = (sin_t sin_p, cos_t, sin_t cos_p), each product one f32 operation;
 * best = -inf, cell = -1; for l = 0 .. L-1 ascending: s = (omega_x d_x + omega_y d_y) + omega_z d_z, every product and sum one
 * IEEE f32 operation (no contraction); if (s > best) { best = s; cell = l; } -- a tie keeps the lowest index, a NaN score never
 * wins (nor does -inf); afterwards if (!(best >= min_cos)) cell = -1.  min_cos <= -1 drops nothing but texels without any finite
 * score; min_cos > 1 drops every texel.  Bit-equal to the numpy restatement (tests/environment_emulation.py).
 */
int gcfr_environment_cells(const float *rows, const float *cols, const float *dirs_map, int32_t He, int32_t We, int32_t L,
                           float min_cos, int32_t *cell_out, void *stream);

/*
 * The integration, one launch:   env (E,He,We,3) f32 radiance   ->   rgb_out (E,L,3) f32,
 *   rgb_out[e,l,c] = (float) sum_{t : cell[t] == l} (double)env[e,t,c] * row_w[row(t)]          t = r We + c, row(t) = t / We
 * The products and the sum are f64 operations (unfused), in a FIXED order: one workgroup of 256 lanes per (e, l); lane i adds the
 * texels i, i + 256, i + 512, ... of the cell in ascending order to a sum that starts at +0; the 256 sums are added as each
 * wave's xor-shuffle tree (offsets 32, 16, ..., 1), then the four waves as (w0 + w1) + (w2 + w3); one rounding to f32.  No
 * floating-point atomic: every element of rgb_out is written exactly once, an empty cell gives +0, two calls on the same inputs
 * return the same bits, and the result equals the restatement of this order bit for bit.  Nothing is clamped (negative radiance
 * is legal); a non-finite texel propagates into its own cell's entry of that channel and map, and nowhere else.  The weights of
 * all texels sum to 1: a constant map of radiance 1 whose every texel has a cell gives sum_l rgb = 1.  cell values outside
 * [0, L) belong to no light.
 */
int gcfr_environment_fwd(const float *env, int32_t E, int32_t He, int32_t We, const double *row_w, const int32_t *cell, int32_t L,
                         float *rgb_out, void *stream);

/*
 * Backward of the integration with respect to the radiance, one launch, a gather:   g_rgb (E,L,3) f32   ->   g_env (E,He,We,3) f32,
 *   g_env[e,t,c] = (float)row_w[row(t)] * g_rgb[e,cell[t],c]      one f32 product;   +0 where cell[t] is -1 (or outside [0, L))
 * Every element is written once (no accumulation: the caller clears nothing).  There is NO gradient with respect to the
 * directions: the cell assignment is piecewise constant in them (its derivative is zero almost everywhere and undefined on the
 * cell borders), so gcfr_environment_cells has no backward.
 */
int gcfr_environment_bwd(const float *g_rgb, const double *row_w, const int32_t *cell, int32_t E, int32_t He, int32_t We, int32_t L,
                         float *g_env, void *stream);

/*
 * The two forward stages with a FRAME axis, one launch each (a turntable: F rotations of the rig's directions against one map).
 *   dirs_map (F,L,3) f32   ->   cell_out (F,He,We) i32             gcfr_environment_cells_frames
 *   cell (F,He,We) i32, env (E,He,We,3) f32   ->   rgb_out (E,F,L,3) f32, the layout gcfr_light_rig_frames_u8 takes
 * 1 <= F <= 4096 and L E F < 2^31 besides the ranges above.  Frame f is gcfr_environment_cells / gcfr_environment_fwd on
 * dirs_map[f] / cell[f] BIT FOR BIT: the kernels call the same device functions for the per-texel score loop and for the lane walk
 * and its fixed-order f64 sum; only the frame's offset into dirs_map, cell and rgb_out is added.  No backward in this form.
 */
int gcfr_environment_cells_frames(const float *rows, const float *cols, const float *dirs_map, int32_t F, int32_t He, int32_t We,
                                  int32_t L, float min_cos, int32_t *cell_out, void *stream);
int gcfr_environment_fwd_frames(const float *env, int32_t E, int32_t He, int32_t We, const double *row_w, const int32_t *cell,
                                int32_t F, int32_t L, float *rgb_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rig capture: the `rgb` (colour x weight per light) of the light-rig stage above FITTED to a photograph, by weighted least squares
 * over the per-light shadings of the many-lights path (csrc/gcfr_light_fit.hip).  Per face b and channel c, over the pixels p:
 *   minimise  sum_p w[b,p] (image[b,c,p] - albedo[b,c,p] sum_l x[b,l,c] final_shading[b,l,p])^2  +  lambda_c |x[b,:,c]|^2
 * whose normal equations are A_c x_c = r_c with
 *   G_c[l,l'] = sum_p w a_c^2 f_l f_l'     r_c[l] = sum_p w a_c I_c f_l     A_c = G_c + ridge (trace(G_c) / L) I
 * gcfr_light_fit_normal forms G and r, gcfr_light_fit_solve solves.  1 <= L <= 64, 1 <= B <= 65535, H, W >= 1 with H W < 2^31 - 64.
 * The entries allocate nothing, never synchronise, use no floating-point atomic and no cross-lane reduction, and may be captured
 * into a graph.  Every sum is an f64 sum in a FIXED order, stated below: two calls return the same bits, and the numpy restatement of
 * that order (tests/light_fit_emulation.py) returns them too.  The library is built with -ffp-contract=off: every product and sum
 * below is one IEEE f64 operation.
 * ------------------------------------------------------------------------------------------- */

/*
 * Bytes of caller-owned scratch gcfr_light_fit_normal needs for its per-workgroup partials: 8 B groups 3 L (L + 3) / 2 with
 * groups = min(ceil(H W / 64), max(1, 512 / B)), the workgroups per face (a chunk is 64 pixels; 512 workgroups per launch at the
 * most).  0 for a shape outside the ranges above.
 */
size_t gcfr_light_fit_workspace_bytes(int32_t B, int32_t L, int32_t H, int32_t W);

/*
 * The normal equations, two launches.  All planes contiguous:
 *   final_shading (B,L,H,W) f32      the many-lights `final`
 *   albedo        (B,3,H,W) f32
 *   image         f32                the photograph: (B,H,W,3) when image_nhwc = 1, (B,3,H,W) when image_nhwc = 0
 *   weight        f32 or NULL        (weight_batch,H,W) with weight_batch = B (per face) or 1 (shared); NULL: all ones
 *   workspace     gcfr_light_fit_workspace_bytes(B, L, H, W) bytes, 8-byte aligned; its contents afterwards are unspecified
 *   gram (B,3,L,L) F64 out, rhs (B,3,L) F64 out      8-byte aligned; every element is written once (the caller clears nothing)
 * A NULL among the required pointers, a misaligned f64 pointer, image_nhwc other than 0 / 1, weight_batch other than 1 / B with a
 * weight, or a shape out of range is GCFR_ERR_INVALID_ARGUMENT before any launch.
 * Order of operations, per pixel p and channel c, in f64:
 *   s = (double)w * (double)a_c          (exact)
 *   q = s * (double)a_c                  u = s * (double)I_c
 *   G_c[l,l'] += (q * (double)f_l) * (double)f_l'     for l' <= l
 *   r_c[l]    += u * (double)f_l
 * Who sums what: the face's pixels are cut into chunks of 64 consecutive pixels; workgroup g of the face's `groups` takes the chunks
 * g, g + groups, g + 2 groups, ...  Each entry of a workgroup's partial is summed by ONE lane, sequentially over that workgroup's
 * pixels in ascending pixel order, starting from +0.  An entry of the face's total is the sum of its workgroups' partials in
 * ascending workgroup order, starting from partial 0 (no add to zero).  gram is written full and symmetric: the upper triangle is a
 * copy of the lower one, not a second sum.  Nothing is clamped: non-finite values propagate to the entries they enter, also under
 * a weight of 0 (0 * NaN is NaN).
 */
int gcfr_light_fit_normal(const float *final_shading, const float *albedo, const float *image, int32_t image_nhwc,
                          const float *weight, int32_t weight_batch, int32_t B, int32_t L, int32_t H, int32_t W, void *workspace,
                          double *gram, double *rhs, void *stream);

/*
 * The solve, one launch, one workgroup per (rig, channel):   gram (B,3,L,L) F64, rhs (B,3,L) F64   ->   rgb (rgb_batch,L,3) f32,
 * the layout gcfr_light_rig_fwd takes, and info (rgb_batch,3) i32.  rgb_batch = B fits a rig per face; rgb_batch = 1 fits ONE rig
 * to all faces: the B matrices and right-hand sides are added first, entry by entry, in ascending b starting from face 0's.
 * Only gram's lower triangle is read.  ridge >= 0 and finite, rgb_batch = 1 or B, 1 <= L <= 64, 1 <= B <= 65535, no NULL, f64
 * pointers 8-byte aligned: anything else is GCFR_ERR_INVALID_ARGUMENT before the launch.  Order, all f64, one lane per sum:
 *   trace = 0; trace += G[l,l] for l ascending;   A[l,l] = G[l,l] + ridge * (trace / (double)L)       (ridge = 0 adds an exact 0)
 *   Cholesky, column k ascending:  s_i = A[i,k]; s_i = s_i - C[i,m] * C[k,m] for m = 0 .. k-1 ascending   (every row i >= k);
 *       the pivot s_k must be a positive finite number; C[k,k] = sqrt(s_k), C[i,k] = s_i / C[k,k]         (IEEE sqrt and division)
 *   forward, k ascending:   z_k = y_k / C[k,k];  y_i = y_i - C[i,k] * z_k for i > k                    (y starts as the right-hand side)
 *   back, k descending:     x_k = z_k / C[k,k];  z_i = z_i - C[k,i] * x_k for i < k
 *   rgb[., l, c] = (float)x_l, one rounding.
 * info[., c] = 0 on success.  When pivot k is not a positive finite number, info[., c] = k + 1 and that channel's L entries of rgb
 * are NaN; nothing else is written.  A non-finite right-hand side under a good matrix gives non-finite rgb with info = 0.
 */
int gcfr_light_fit_solve(const double *gram, const double *rhs, int32_t B, int32_t L, double ridge, int32_t rgb_batch, float *rgb,
                         int32_t *info, void *stream);

/*
 * The NON-NEGATIVE solve, one launch, one workgroup per (rig, channel), on the same gram / rhs:
 *   minimise  1/2 x^T A x - r^T x   subject to  x >= 0        A = G + ridge (trace(G) / L) I, r: exactly those of gcfr_light_fit_solve
 * by Lawson and Hanson's active-set method on the normal equations.  Arguments, ranges, alignment and refusals as for
 * gcfr_light_fit_solve; in addition max_solves >= 0 caps the factorisations per (rig, channel), 0 meaning the default cap 3 L, and
 * solves (rgb_batch,3) i32 receives their number (NULL: not wanted).  Allocates nothing, never synchronises, may be captured.
 * Order, all f64, one lane per sum, every product, sum, division and sqrt one IEEE operation:
 *   1. x = 0; the passive set P empty; n = 0; tol = 2^-40 * max_l |r_l|  (an exact product; the maximum starts at 0 and takes |r_l|
 *      where |r_l| > maximum, so a NaN never enters it).
 *   2. for every l outside P:  w_l = r_l;  w_l = w_l - A[l,j] * x_j for j in P ascending.  j = the FIRST index with the largest w_l
 *      among those with w_l > tol (comparisons are `>`: a NaN never wins).  None: finish, info 0.  Else j enters P.
 *   3. if n == cap: finish, info -1.  Else n += 1 and solve A_PP s_P = r_P by the factorisation and substitutions of
 *      gcfr_light_fit_solve restricted to the rows and columns in P, in ascending light index: column k in P gets
 *      s_i = A[i,k]; s_i = s_i - C[i,m] * C[k,m] for m in P, m < k, ascending (rows i in P, i >= k); forward over k in P ascending,
 *      back descending.  A pivot that is not a positive finite number: info = k + 1 (k the LIGHT's index), that channel's L entries
 *      of rgb NaN, solves = n, finish.
 *      If s_l > 0 for every l in P:  x_P = s_P, go to 2.
 *      Else alpha and l* start as the quotient x_l / (x_l - s_l) and index of the first l in P with !(s_l > 0); a later such l
 *      replaces them where its quotient `<` alpha (the first index wins a tie; a NaN quotient -- 0 / 0 -- never replaces, a first
 *      one stays).  Then for l in P:  d = s_l - x_l;  m = alpha * d;  x_l = x_l + m  (three operations);  x_l* = 0;  every l in P
 *      with !(x_l > 0) gets x_l = 0 and leaves P.  Repeat 3.
 *   4. finishing with info 0 or -1:  rgb[., l, c] = (float)x_l, one rounding, a zero exactly +0;  solves[., c] = n.  Under info -1
 *      x is the current iterate, feasible by construction.
 * Consequences: every entry written is >= 0 or NaN.  Where the final passive set is all L lights, the last factorisation is
 * operation for operation that of gcfr_light_fit_solve: wherever the unconstrained solution is positive in every entry the two
 * entries return the same bits.  In exact arithmetic a newly admitted light has s_j > 0; where rounding makes it otherwise step 3
 * removes it again with alpha = 0 and the cap ends the fit -- there is no extra rule.  Every loop is bounded by L, by the lights in
 * P or by the cap, none by a floating-point condition: non-finite input ends within `cap` factorisations too (a NaN in r is never
 * admitted: that light stays 0).
 */
int gcfr_light_fit_solve_nonneg(const double *gram, const double *rhs, int32_t B, int32_t L, double ridge, int32_t rgb_batch,
                                int32_t max_solves, float *rgb, int32_t *info, int32_t *solves, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement aid (bench.py `roofline.hbm_measured_copy_GBs`): a float4 grid-stride device-to-device copy of `bytes` bytes
 * (multiple of 16, both pointers 16-byte aligned), one workgroup of 256 lanes per CU, four loads in flight per lane, non-temporal --
 * the achievable-HBM probe (6.3 TB/s, read + write) the roofline's 8 TB/s spec peak is reported beside.  Not part of the render path.
 * ------------------------------------------------------------------------------------------- */
int gcfr_copy_probe(const void *src, void *dst, size_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GCFR_H */
