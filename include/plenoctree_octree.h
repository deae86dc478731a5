/*
 * plenoctree_octree.h -- C ABI of the PlenOctree side of the path on MI355X (gfx950): building the
 * N3Tree from the dense-grid evaluation, the training-view weight mask, and the octree volume
 * renderer with its gradient.  Same library (libplenoctree_hip.so) and conventions as
 * plenoctree_hip.h: extern "C", plain pointers, caller-owned device memory, asynchronous on
 * `void* stream` unless a host-side result is returned, 0 = ok / negative = error.
 *
 * In the reference these operations are calls into the third-party package svox
 * (svox>=0.2.28, not part of the reference tree); each entry point cites the reference call
 * site (file:line) whose svox call it replaces.
 *
 * N3Tree storage (N = 2), identical to svox's and to the npz keys of octree/compression.py:76-86:
 *   child        int32 [n, 2,2,2]        index(child node) - n, 0 = leaf
 *   parent_depth int32 [n, 2]            (packed parent cell index ((p*2+i)*2+j)*2+k, depth)
 *   data         float [n, 2,2,2, D]     D = 3*basis_dim + 1, rgb SH coefficients channel-major,
 *                                        last channel sigma
 *   offset[3], invradius[3]              x_tree = offset + invradius * x_world
 * Nodes are stored breadth-first: all nodes of depth d before depth d+1, each level ordered by
 * packed parent cell index (the order svox's refine() produces when whole levels are refined).
 */
#ifndef PLENOCTREE_OCTREE_H_
#define PLENOCTREE_OCTREE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXO_TREE_MAX_DEPTH 10   /* depth_limit <= 10: grid of at most 2048^3 */

/* svox RenderOptions (VolumeRenderer._get_options; octree/extraction.py:184-195). */
typedef struct PxoRenderOpts {
  float step_size;              /* --renderer_step_size, octree/nerf/utils.py:211-215 */
  float background_brightness;  /* 1.0 */
  float sigma_thresh;           /* 0 exact / 1e-2 fast (eval_octree: fast = not no_early_stop) */
  float stop_thresh;            /* 0 exact / 1e-2 fast */
} PxoRenderOpts;

/* Read-only view of a tree for the renderers. */
typedef struct PxoTree {
  const int32_t* child;
  const float* data;
  int64_t n_internal;
  int32_t data_dim;             /* 3*basis_dim + 1 */
  int32_t basis_dim;            /* 1, 4, 9, 16 or 25 (data_format SH<k>) */
  float offset[3];
  float invradius[3];
} PxoTree;

/* Pinhole camera (svox CameraSpec; octree/extraction.py:197-201, octree/nerf/utils.py:473-474).
 * c2w: device pointer to the first 3 rows of the camera-to-world matrix, 12 floats row-major. */
typedef struct PxoCamera {
  const float* c2w;
  float fx, fy;
  int32_t width, height;
} PxoCamera;

/* ---- step 1: mask -> tree  (octree/extraction.py:322-352: mask, `tree[grid].refine()` x depth) ---- */

/* mask[i] = value[i] >= thresh (sigma or grid-weight masking, octree/extraction.py:322-331). */
int pxo_threshold_mask(const float* value, int64_t n, float thresh, uint8_t* mask, void* stream);

/* Workspace for the occupancy pyramid of a 2^(depth+1) grid. */
int pxo_tree_workspace_bytes(int depth, size_t* bytes);
/* Builds the occupancy pyramid of `mask` ([reso^3] bytes, reso = 2^(depth+1), x slowest) in `ws` and
 * returns on the HOST the number of nodes per depth, level_nodes[0..depth] (level_nodes[0] = 1, the
 * root).  Synchronises `stream`.  The tree will have sum(level_nodes) nodes. */
int pxo_tree_count_nodes(const uint8_t* mask, int depth, void* ws, size_t ws_bytes, int64_t* level_nodes,
                         void* stream);
/* Writes child [n,8] and parent_depth [n,2] of the tree whose pyramid is in `ws` (after
 * pxo_tree_count_nodes on the same ws); n = sum(level_nodes). */
int pxo_tree_build(const void* ws, size_t ws_bytes, int depth, const int64_t* level_nodes, int32_t* child,
                   int32_t* parent_depth, void* stream);

/* ---- step 2: leaf samples and assignment  (octree/extraction.py:355-394, :503) ---- */

/* tree[inds].sample(S) for the 8 cells of each node in [node0, node0+n_nodes): point (cell c, sample s)
 * = corner + u * side in tree coordinates, returned in world coordinates ((p - offset) / invradius).
 * u: [n_nodes*8*S, 3] uniforms in [0,1) (pxo_uniform).  points: [n_nodes*8*S, 3], cells in packed order. */
int pxo_tree_sample_cells(const int32_t* parent_depth, int64_t node0, int64_t n_nodes, int S, const float* u,
                          const float offset[3], const float invradius[3], float* points, void* stream);
/* The same for arbitrary leaves given by packed cell index node*8 + cell (`tree[leaf_inds].sample(S)` with any index
 * set, octree/extraction.py:358-369): u [n_cells*S, 3], points [n_cells*S, 3]. */
int pxo_tree_sample_leaves(const int32_t* parent_depth, const int64_t* packed, int64_t n_cells, int S, const float* u,
                           const float offset[3], const float invradius[3], float* points, void* stream);
/* tree[points] (the indexing behind `tree[grid].refine()`, octree/extraction.py:341-350): packed index
 * node*8 + cell of the leaf that contains each world-space point [n,3] (tree coordinates clamped to
 * [0, 1 - 1e-6] as svox does). */
int pxo_tree_query(const int32_t* child, const float* points, int64_t n, const float offset[3],
                   const float invradius[3], int64_t* packed, void* stream);
/* tree[:, -1:].relu_()  (octree/extraction.py:503): clamps the sigma channel of n_cells cells at 0. */
int pxo_tree_relu_sigma(float* data, int64_t n_cells, int data_dim, void* stream);

/* ---- weight mask  (_C.grid_weight_render, octree/extraction.py:181-214) ---- */

/* For each of the n_cams cameras (c2w_all: [n_cams,12] device) and every pixel, marches the ray through
 * the dense sigma grid [reso^3] and keeps, per voxel, the maximum compositing weight
 * light * (1 - exp(-dt * sigma)).  grid_weight [reso^3] must be zero-initialised by the caller for the
 * first call; successive calls accumulate the maximum (torch.max over cameras, :206-212).
 * ws: pxo_grid_weight_workspace_bytes(reso) bytes (brick-ordered copies of the grid and the weights, and the count of
 * voxels above sigma_thresh by which the launch picks its marcher on the device: slab-staged for dense grids, per-sample
 * for sparse ones - same samples, same arithmetic, bit-identical weights either way; the call stays asynchronous). */
int pxo_grid_weight_workspace_bytes(int reso, size_t* bytes);
int pxo_grid_weight_render(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx,
                           float fy, int width, int height, const PxoRenderOpts* opts, const float offset[3],
                           const float invradius[3], float* grid_weight, void* ws, size_t ws_bytes, void* stream);

/* ---- octree volume renderer  (VolumeRenderer.render_persp / render; octree/nerf/utils.py:456-474,
 *      octree/optimization.py:174-216) ---- */

/* Lanes of a wave that cooperate on one ray in the forward / backward renderer launches: 4, 8 or 16, or 0 for
 * the measured default (4 both ways; backward at 4 = 4-lane march with a 16-lane cooperative gradient scatter).  A tuning knob (results are identical up to the SH summation
 * order); process-wide. */
int pxo_octree_set_lanes_per_ray(int forward, int backward);

/* The other two launch-time choices between kernels that compute the SAME result (A/B sessions, the bit-equality test of
 * the two weight-mask marchers); process-wide, validated, no environment variables are read anywhere in the library.
 *   PXO_TUNE_GW_MARCHER      -1 chosen on the device by the occupied fraction of the grid (default), 0 per-sample, 1 slab-staged
 *   PXO_TUNE_BWD_CACHE_ROWS  rows of the backward renderer's per-wave write-combining cache: 16 (default), 0 (direct
 *                            scatter), 4, 8, 32, 64
 *   PXO_TUNE_BWD_UPDATE      how a sample's gradient row reaches that cache: 0 the whole wave on one sample's row at a time,
 *                            1 every ray's own 4 lanes on its row, all 16 rays of the wave at once (LDS float atomics; misses
 *                            elect one winner per slot).  Same sums in a different order (float32 round-off apart). */
#define PXO_TUNE_GW_MARCHER 0
#define PXO_TUNE_BWD_CACHE_ROWS 1
#define PXO_TUNE_BWD_UPDATE 2
#define PXO_TUNE_GW_TILE_ORDER 3   /* weight mask on power-of-two grids: 0 workgroups take tiles in row-major order (default), 1 the tiles of
                                      a 4x4-tile square all go to one XCD (one L2); same weights either way (max is order-free) */
int pxo_octree_set_tuning(int knob, int value);
int pxo_octree_get_tuning(int knob, int* value);

/* Forward.  Rays come either from `cam` (cam != NULL: B must be width*height, ray r = pixel
 * (r % width, r / width), out [H,W,3]) or from explicit arrays origins/dirs/viewdirs [B,3] in world
 * space with unit dirs (cam == NULL).  out_rgb [B,3]. */
int pxo_octree_render_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                          const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb,
                          void* stream);
/* pxo_octree_render_fwd with three more outputs per ray, taken from the same march (same rays, same options, same sample
 * sequence; out_rgb is bit for bit that of pxo_octree_render_fwd).  The march visits samples i = 0, 1, .. at parameters t_i
 * (tree units, t_0 = tmin) with steps delta_i.  A sample is shaded when sigma_i > sigma_thresh; then, with light = 1 before
 * the first sample,
 *   dtw_i = delta_i * delta_scale,  att_i = exp(-dtw_i * sigma_i),  w_i = light * (1 - att_i),  light *= att_i,
 *   s_i   = (t_i + 0.5 * delta_i) * delta_scale
 * s_i is the Euclidean world distance from the ray ORIGIN along the unit direction to the middle of the step (not from the
 * point where the ray enters the volume, and not z-depth).  out_aux [B,3] (camera mode: [H,W,3]) holds per ray
 *   [0] alpha    sum of w_i over the shaded samples (= 1 - final light up to round-off)
 *   [1] depth    sum of w_i * s_i: the expected termination distance, NOT divided by alpha, no background term
 *   [2] surface  s_i of the first shaded sample after which light <= surface_thresh; +inf if that never happens
 * With stop_thresh > 0 a ray that stops early has rgb, alpha and depth multiplied by 1 / (1 - light); surface is never
 * scaled.  A ray that misses the volume gets (0, 0, +inf) and the background as its rgb.  Requires
 * stop_thresh < surface_thresh < 1 (PXO_ERR_ARG otherwise: an early stop could come before the crossing) and a non-null
 * out_aux.  Not differentiable: there is no gradient entry point for these outputs. */
int pxo_octree_render_aux_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                              float* out_rgb, float* out_aux, void* stream);
/* Gradient of sum(out_rgb * grad_out) w.r.t. tree->data, ACCUMULATED (atomic adds) into grad_data
 * [n_internal,2,2,2,D] -- zero it first (optimizer.zero_grad(), octree/optimization.py:221-224).
 * Training semantics: exact marching (stop_thresh is ignored: no early-stop rescale).
 * out_rgb: the [B,3] result of pxo_octree_render_fwd for the same rays with the same exact options, or NULL
 * (the kernel then re-marches once more to recover it).  Passing out_rgb together with opts->stop_thresh > 0
 * is rejected (PXO_ERR_ARG): an early-stopped image is not the image this gradient belongs to. */
int pxo_octree_render_bwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                          const float* viewdirs, int64_t B, const PxoRenderOpts* opts, const float* out_rgb,
                          const float* grad_out, float* grad_data, void* stream);

/* ---- spherical-Gaussian trees  (svox data_format "SG<K>" with extra_data; octree/extraction.py:436-442, :481-499;
 *      rendered at octree/nerf/utils.py:456-474, fine-tuned at octree/optimization.py:174-216) ----
 * lobes: device float32 [tree->basis_dim, 4], row i = (lambda_i, mu_i.x, mu_i.y, mu_i.z) with lambda_i > 0 and mu_i a unit
 * vector (the tree's extra_data).  The per-ray basis is
 *   basis_i(d) = exp(lambda_i * (dot(mu_i, d) - 1)) / K      (eval_sg, nerf_sh/nerf/sg.py:35-66)
 * in float32, evaluated as written (dot, minus 1, times lambda, expf, times 1/K), in place of the SH basis.  Everything
 * else -- rays, march, sample sequence, early stop and its rescale, the out_rgb contract of the backward, the accumulation
 * into grad_data, pxo_octree_set_lanes_per_ray and the tuning knobs -- is that of pxo_octree_render_fwd /
 * pxo_octree_render_bwd; tree->data is laid out as for SH (channel-major, sigma last).  There is no gradient with respect
 * to the lobes (svox does not optimise extra_data).  PXO_ERR_ARG if basis_dim is not 1, 4, 9, 16 or 25, data_dim != 3
 * basis_dim + 1 or lobes is NULL. */
int pxo_octree_render_sg_fwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                             const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb,
                             void* stream);
int pxo_octree_render_sg_bwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                             const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts,
                             const float* out_rgb, const float* grad_out, float* grad_data, void* stream);

/* ---- forward-facing (LLFF) scenes in normalised device coordinates  (svox.NDCConfig / RenderOptions.ndc_*;
 *      octree/extraction.py:184-195, octree/nerf/utils.py:456-474, octree/optimization.py:170-216) ----
 * The tree of such a scene lives in the NDC cube (--radius 1 1 1 --center 0 0 0); rays arrive in WORLD space, exactly as
 * for the world-space entry points (from `cam`, or as origins / dirs / viewdirs), and are converted per ray, in float32,
 * one rounding per operation, IEEE divisions, in this order (o, d: world origin and direction):
 *   1. View direction.  vdir is the WORLD-space unit direction, taken before the conversion: what the camera produces in
 *      camera mode, the `viewdirs` argument in explicit-ray mode.  The SH basis is evaluated on vdir, never on the NDC
 *      direction (the NeRF was trained with world viewdirs, so the baked coefficients expect them).
 *   2. Conversion (convert_to_ndc, octree/nerf/datasets.py:37-57).  t = -(near + o_z) / d_z;  o = o + t d;  then
 *        cw = (2 focal) / width,  ch = (2 focal) / height,  ox = o_x / o_z,  oy = o_y / o_z,
 *        o' = (-cw ox, -ch oy, 1 + (2 near) / o_z),   d' = (-cw (d_x / d_z - ox), -ch (d_y / d_z - oy), (-2 near) / o_z).
 *      The result does not depend on the length of d.
 *   3. Normalisation.  n = sqrtf((d'_x^2 + d'_y^2) + d'_z^2),  d' = d' / n.
 *   4. The world-space code from here: o', d' go through the tree transform, the march, shading, early stop, its rescale
 *      and the background exactly as o, d do in the world-space twin.  delta_scale is therefore a length in NDC space,
 *      the quantity a NeRF trained in NDC integrates sigma over.
 *   5. Misses.  A ray is a miss unless d_z < 0, the six components of o', d' of step 2 are finite and 0 < n < inf.  A
 *      miss gets the background colour, a zero gradient and no weight; it is decided before the march.
 * svox's own NDC kernel was not available to compare against: this arithmetic is fixed by the reference's convert_to_ndc and
 * by the NeRF side of this library (pxo_generate_rays_ndc), which the tree has to reproduce.
 * Each entry point takes the arguments of its world-space twin plus `ndc` and keeps the twin's contracts (camera or
 * explicit rays, the out_rgb rule of the backward, accumulation, workspace, asynchrony, pxo_octree_set_lanes_per_ray and
 * every PXO_TUNE_* knob: all of their choices run the NDC set-up).  SH trees only.  PXO_ERR_ARG on a null ndc, width < 1,
 * height < 1, focal <= 0, near <= 0, or tree->basis_dim outside {1, 4, 9, 16, 25}.  In camera mode ndc->width / height /
 * focal describe the projection the scene was trained with; they are independent of cam (callers normally pass equal
 * values). */
typedef struct PxoNdc {
  int32_t width, height;
  float focal, near;
} PxoNdc;
int pxo_octree_render_ndc_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream,
                              const PxoNdc* ndc);
int pxo_octree_render_ndc_bwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                              const float* viewdirs, int64_t B, const PxoRenderOpts* opts, const float* out_rgb,
                              const float* grad_out, float* grad_data, void* stream, const PxoNdc* ndc);
int pxo_grid_weight_render_ndc(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                               int width, int height, const PxoRenderOpts* opts, const float offset[3],
                               const float invradius[3], float* grid_weight, void* ws, size_t ws_bytes, void* stream,
                               const PxoNdc* ndc);

/* ---- compressed trees rendered in place  (the palette form octree/compression.py:88-139 writes) ----
 *
 * File arrays (K = basis_dim, r = n_retained, Kq = K - r, C = n_internal * 8 cells, P = 2^bits palette entries):
 *   quant_colors  float16 [Kq, P, 3]     quant_map  uint16 [Kq, C]     sigma  float16 or float32 [C]
 *   data_retained float16 [r, C, 3]      (only with --retain r)
 * Device layout made by pxo_octree_quant_pack, one buffer of four 256-byte aligned sections (PxoQuantLayout):
 *   idx       uint16  [C, idx_stride]    idx_stride = Kq rounded up to a multiple of 4: a leaf's indices are contiguous
 *                                        and every 8-byte group of four is 8-byte aligned whatever Kq is (odd for SH9,
 *                                        SH25 or an odd remainder after `retain`); the padding holds index 0
 *   palette   float16 [Kq, P, 4]         (r, g, b, 0): one 8-byte load per lookup
 *   sigma     float32 [C]                widened (exactly) from the file's type
 *   retained  float16 [C, r, 4]          (r, g, b, 0) per retained basis function; ret_stride = 4 r
 * Bytes per leaf: 2 idx_stride + 4 + 8 r (SH16, retain 0: 36; float form 4 (3K+1) = 196), plus 8 Kq P for the palettes. */
typedef struct PxoQuantLayout {
  int64_t idx_offset, palette_offset, sigma_offset, retained_offset;   /* bytes into the packed buffer */
  int64_t total_bytes;
  int32_t idx_stride;           /* uint16 elements per leaf */
  int32_t ret_stride;           /* float16 elements per leaf */
} PxoQuantLayout;

/* Read-only view of a packed compressed tree for pxo_octree_render_quant_fwd. */
typedef struct PxoQuantTree {
  const int32_t* child;
  const uint16_t* idx;          /* packed indices [C, idx_stride], 8-byte aligned */
  const void* palette;          /* float16 [Kq, 2^bits, 4], 8-byte aligned */
  const float* sigma;           /* [C] */
  const void* retained;         /* float16 [C, n_retained, 4], 8-byte aligned; ignored when n_retained == 0 */
  int64_t n_internal;
  int32_t basis_dim;            /* 1, 4, 9, 16 or 25 */
  int32_t n_retained;           /* 0 .. basis_dim - 1 */
  int32_t bits;                 /* 1 .. 16 */
  int32_t idx_stride;
  int32_t ret_stride;
  float offset[3];
  float invradius[3];
} PxoQuantTree;

/* Section offsets, strides and size of the packed form of a tree in the format of octree/compression.py:88-139
 * (host only). */
int pxo_octree_quant_pack_bytes(int64_t n_internal, int basis_dim, int n_retained, int bits, PxoQuantLayout* layout);
/* Packs the arrays of a file written by octree/compression.py:88-139, uploaded as they are (device pointers), into
 * `packed` (layout->total_bytes bytes, 256-byte aligned): transposes quant_map, pads the palette entries and the retained
 * planes to 8 bytes and widens sigma (sigma_elem_bytes: 2 = float16, 4 = float32).  data_retained may be NULL when
 * n_retained == 0.  Indices are NOT range-checked here: the caller validates them against 2^bits on the host (the
 * renderer masks them to `bits` bits, so a bad index can give a wrong colour but never an out-of-range read). */
int pxo_octree_quant_pack(const uint16_t* quant_map, const void* quant_colors, const void* sigma, int sigma_elem_bytes,
                          const void* data_retained, int64_t n_internal, int basis_dim, int n_retained, int bits,
                          void* packed, size_t packed_bytes, void* stream);
/* pxo_octree_render_fwd on a tree in the palette form of octree/compression.py:88-139, read in place: same rays, same
 * options, same sample sequence; per shaded sample and channel c, p_c = sum_b Y_b(viewdir) coef[c][b] with coef from
 * `retained` for b < n_retained and from palette[b - n_retained][idx[leaf][b - n_retained]] otherwise, each float16
 * widened to float32.  Lanes per ray: the forward value of pxo_octree_set_lanes_per_ray (4, 8, 16; default 4); the
 * summation order over b is fixed by (lanes per ray, basis_dim, n_retained).  Forward only: a compressed tree is
 * read-only. */
int pxo_octree_render_quant_fwd(const PxoQuantTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb,
                                void* stream);
/* pxo_octree_render_aux_fwd on a tree in the palette form: out_rgb is that of pxo_octree_render_quant_fwd, out_aux as defined
 * at pxo_octree_render_aux_fwd (it depends on sigma and the geometry only, so it equals the float tree's bit for bit when
 * that tree carries the same float32 sigma).  Same argument checks as pxo_octree_render_quant_fwd, plus those on
 * surface_thresh and out_aux. */
int pxo_octree_render_quant_aux_fwd(const PxoQuantTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                    const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                                    float* out_rgb, float* out_aux, void* stream);

/* ---- float16 trees rendered in place  (the `data` array of the files N3Tree.save writes; svox writes the same) ----
 *
 * File array (D = data_dim = 3 basis_dim + 1, C = n_internal * 8 cells):
 *   data  float16 [C, D]      rgb coefficients channel-major, last channel sigma, as in the float form
 * Device layout made by pxo_octree_half_pack, one buffer:
 *   data  float16 [C, row_stride]   logical index i of leaf r at half r * row_stride + i; row_stride = D rounded up to a
 *                                   multiple of 4 (4, 16, 28, 52, 76 for basis_dim 1, 4, 9, 16, 25), so that a row starts 8-byte
 *                                   aligned and every group of four logical indices that starts at a multiple of 4 is one
 *                                   aligned 8-byte load; the padding (basis_dim 4 and 16: 3 halves) holds zeros
 * Bytes per leaf: 2 row_stride (SH16: 104; float form 4 D = 196).  No load of the renderers leaves a row's row_stride halves. */

/* Read-only view of a packed float16 tree for pxo_octree_render_half_fwd. */
typedef struct PxoHalfTree {
  const int32_t* child;
  const void* data;             /* float16 [C, row_stride], 8-byte aligned */
  int64_t n_internal;
  int32_t data_dim;             /* 3*basis_dim + 1 */
  int32_t basis_dim;            /* 1, 4, 9, 16 or 25 (SH<k> or SG<k>) */
  int32_t row_stride;           /* halves per leaf: pxo_octree_half_pack_bytes */
  float offset[3];
  float invradius[3];
} PxoHalfTree;

/* Row stride (halves) and size (bytes) of the packed form of a tree of n_internal nodes with data_dim values per leaf
 * (host only).  PXO_ERR_ARG unless data_dim is 3 k + 1 with k in {1, 4, 9, 16, 25}. */
int pxo_octree_half_pack_bytes(int64_t n_internal, int data_dim, int32_t* row_stride, int64_t* bytes);
/* Packs `src`, the file's data[:n_internal] uploaded as it is (device float16 [C, D]), into `packed` (`bytes` bytes, 8-byte
 * aligned): the same halves at the row stride above, zeros in the padding. */
int pxo_octree_half_pack(const void* src, int64_t n_internal, int data_dim, void* packed, size_t packed_bytes, void* stream);
/* pxo_octree_render_fwd (lobes == NULL, ndc == NULL), pxo_octree_render_sg_fwd (lobes: the [basis_dim,4] lobes) or
 * pxo_octree_render_ndc_fwd (ndc) on a float16 tree read in place: the same kernel with another load.  Rays, march, sample
 * sequence, early stop, its rescale and the background are those of the float entry point, and so are, per lanes-per-ray
 * setting (the forward value of pxo_octree_set_lanes_per_ray), the lane that owns a logical coefficient and the order of the
 * multiply-adds; a coefficient is its half widened to float32 at the load, sigma the half at logical index data_dim - 1.
 * Widening is exact, so out_rgb equals, bit for bit, what the float entry point returns for the tree whose data is the
 * widened halves.  Argument checks of the float entry points, plus: row_stride must be that of pxo_octree_half_pack_bytes,
 * data 8-byte aligned, and lobes together with ndc is PXO_ERR_ARG (SG trees have no NDC form).  Forward only. */
int pxo_octree_render_half_fwd(const PxoHalfTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                               const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts,
                               float* out_rgb, void* stream, const PxoNdc* ndc);
/* pxo_octree_render_aux_fwd on a float16 tree (SH, world space): out_rgb and out_aux equal the float entry point's bit for
 * bit.  Same argument checks as pxo_octree_render_half_fwd, plus those on surface_thresh and out_aux. */
int pxo_octree_render_half_aux_fwd(const PxoHalfTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                   const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float surface_thresh,
                                   float* out_rgb, float* out_aux, void* stream);

/* ---- work counters of the marchers (roofline pass: scripts/octree_bench.py states each kernel's algorithmic bytes from
 *      these; nothing on the product path calls them) ----
 * One thread per ray repeats the renderer's / the weight mask's march -- same ray set-up, leaf lookup, step rule and early
 * stop, hence the same sample sequence -- and counts:
 *   counts[0] rays that enter the volume        counts[2] samples with sigma > sigma_thresh (one leaf row read / one
 *   counts[1] samples (one sigma read each)               weight update each)
 *   counts[3] child-pointer loads of the leaf lookups (tree marcher only)
 * counts: 4 device uint64, ACCUMULATED (zero them first).  leaf_seen [n_internal*8] / voxel_seen [reso^3] (uint8, may be
 * NULL): set to 1 where a sample above the threshold fell, so that the distinct rows a launch must fetch from HBM at
 * least once can be counted.  pxo_grid_weight_count_work takes power-of-two grids only (reso >= 4: every grid the extraction
 * makes): it repeats the march of the power-of-two weight-mask kernels, whose division by reso is an exact multiplication. */
int pxo_octree_count_work(const PxoTree* tree, const PxoCamera* cam, const PxoRenderOpts* opts,
                          unsigned long long* counts, uint8_t* leaf_seen, void* stream);
int pxo_grid_weight_count_work(const float* sigma_grid, int reso, const float* c2w_all, int n_cams, float fx, float fy,
                               int width, int height, const PxoRenderOpts* opts, const float offset[3],
                               const float invradius[3], unsigned long long* counts, uint8_t* voxel_seen,
                               void* stream);

/* ---- per-leaf compositing weights  (svox N3Tree.accumulate_weights; no call site in the reference: the published svox
 *      interface, parity unpinned) ----
 * For every ray, the march of pxo_octree_render_fwd without shading, operation for operation: the ray from camera_ray
 * (cameras) or the explicit loads, the NDC conversion above when `ndc` is given (NULL: world space), the tree transform, the
 * clamp of the position to [0, 1 - 1e-6], the leaf lookup, the step  delta = cell_exit(local) * 2^-(depth+1) + step_size,
 * the test sigma > sigma_thresh, light *= att with a stop once light <= stop_thresh, and the end of the march when
 * !(t + delta > t).  For every shaded sample in leaf l,
 *   w = light * (1 - expf(-(delta * delta_scale) * sigma))
 * which is the forward kernel's compositing weight of that sample, taken before any early-stop rescale.
 *   op == 0 (max)  weights[l] = max(weights[l], w)      op == 1 (sum)  weights[l] += w   (atomic, any order)
 * weights: float32 [n_internal*8], indexed by the flat cell index node*8 + cell that addresses the rows of `data`; the caller
 * zeroes it and it ACCUMULATES across calls (max: the result does not depend on the order of rays or calls, bit for bit).
 * Cells that are not leaves are never written.  Rays that miss the volume and NDC misses contribute nothing.
 * sigma is read at data[l * data_dim + data_dim - 1]: SH and SG float trees alike; no basis is evaluated, no lobes needed,
 * basis_dim is not looked at.
 * _cams: c2w_all [n_cams,12] device, as pxo_grid_weight_render takes it; one launch covers all n_cams * width * height rays
 * (ray = (camera * height + py) * width + px).  _rays: origins / dirs [B,3] in world space, unit dirs.
 * PXO_ERR_ARG: op outside {0, 1}, n_cams < 0, B < 0, width / height < 1, a focal length <= 0, and with non-empty work a null
 * tree / options / ray or camera array / weights, step_size <= 0 or a bad ndc.  n_cams == 0 and B == 0 return 0 without
 * a launch. */
int pxo_octree_weight_accum_cams(const PxoTree* tree, const float* c2w_all, int n_cams, float fx, float fy,
                                 int width, int height, const PxoRenderOpts* opts, int op,
                                 float* weights, void* stream, const PxoNdc* ndc /* NULL: world space */);
int pxo_octree_weight_accum_rays(const PxoTree* tree, const float* origins, const float* dirs, int64_t B,
                                 const PxoRenderOpts* opts, int op, float* weights, void* stream,
                                 const PxoNdc* ndc);

/* ---- structural collapse of a tree under a keep mask over its cells  (no svox counterpart) ----
 * keep: uint8 [n*8] over cells.  A leaf cell is dead when keep == 0; a node is dead when each of its 8 cells is a dead leaf
 * or points to a dead node; the root is never removed.  A dead node disappears and the parent cell that pointed to it
 * becomes a dead leaf.  Three steps:
 *   pxo_tree_collapse_mark   node_dead uint8 [n]: bottom-up, one pass per depth max_depth .. 1, nodes selected by
 *                            parent_depth[:,1] (so node order does not matter); max_depth = the deepest node's depth
 *   the caller               new_index int64 [n] = exclusive scan of (node_dead == 0); n_new = number of survivors
 *   pxo_tree_collapse_emit   new_child [n_new,8]: index(new child) - index(new node), 0 where the cell is a leaf or its
 *                            child died; new_parent_depth [n_new,2]; new_data [n_new,8,data_dim]: a survivor's rows copied,
 *                            every dead leaf cell (old, or made by a node's removal) an all-zero row; old2new int64 [n]
 *                            (-1 for removed nodes)
 * Survivors keep their relative storage order: a breadth-first tree stays breadth-first. */
int pxo_tree_collapse_mark(const int32_t* child, const int32_t* parent_depth, const uint8_t* keep, int64_t n, int max_depth,
                           uint8_t* node_dead, void* stream);
int pxo_tree_collapse_emit(const int32_t* child, const int32_t* parent_depth, const float* data, int data_dim,
                           const uint8_t* keep, const uint8_t* node_dead, const int64_t* new_index, int64_t n, int64_t n_new,
                           int32_t* new_child, int32_t* new_parent_depth, float* new_data, int64_t* old2new, void* stream);

/* ---- level of detail: a mean pyramid in the rows of the cells that have a child  (no svox counterpart; the reduction is
 *      this project's definition, not svox's) ----
 * `data` holds a row for every cell, also for the cells that have a child; no renderer reads those (a marcher stops where
 * child == 0) and the extraction leaves them zero.  pxo_tree_lod_fill writes into each of them the VALUE of the child node,
 * deepest level first.  The value of node n, from the rows (c_j[0..D-2], s_j) of its cells j = 0..7 in storage order (the row
 * of a cell that has a child is that child's value, already written), D = data_dim, all in float32, one rounding per
 * operation, no contraction:
 *   w_j = max(s_j, 0)                                           (negative sigma left by fine-tuning must not cancel density)
 *   S = ((((((w_0 + w_1) + w_2) + w_3) + w_4) + w_5) + w_6) + w_7           sigma = S * 0.125
 *   c[k] = (((w_0 c_0[k] + w_1 c_1[k]) + ...) + w_7 c_7[k]) / S   if S > 0 (IEEE division), else 0
 * The colour coefficients are weighted by density, so empty octants do not wash them out; SH and SG trees alike (the lobes
 * are not touched).  Every node of depth d >= 1 (parent_depth[n, 1]) writes its value into the row of its parent cell
 * (parent_depth[n, 0]), one pass per depth max_depth .. 1 in stream order; nodes are picked by their stored depth, so node
 * order does not matter (a tree that is not breadth-first, or a collapsed one).  Rows of leaves are never written: a row is
 * written only where child[parent cell] points back at the node.  A level reads only rows of its own depth and writes only
 * rows one level up, and a parent cell has one child: no atomics, the result does not depend on scheduling.
 * A copy of `child` with the pointers of all nodes of depth >= L zeroed then renders level L (2^(L+1) cells per axis) in place
 * through every entry point above, from the same `data`.
 * data: float32 [n_internal, 8, data_dim], updated in place.  max_depth: the deepest node's depth.  PXO_ERR_ARG: a null
 * pointer, n_internal outside [1, 2^28), data_dim not 3 k + 1 with k in {1, 4, 9, 16, 25}, max_depth outside
 * [0, PXO_TREE_MAX_DEPTH].  n_internal == 1 or max_depth == 0 (a root-only tree) returns 0 without a launch.  Asynchronous. */
int pxo_tree_lod_fill(const int32_t* child, const int32_t* parent_depth, float* data, int64_t n_internal, int data_dim,
                      int max_depth, void* stream);

/* ---- footprint: a depth chosen per sample by the width of the pixel there  (no svox counterpart; this project's definition) ----
 * pxo_octree_render_fwd / pxo_octree_render_sg_fwd (lobes != NULL) / pxo_octree_render_aux_fwd on a tree whose `data`
 * pxo_tree_lod_fill has filled, with every sample's descent stopped where the pixel is at least as wide as the cell.  Forward
 * only, float rows, world space.  Per launch:
 *   cone >= 0   world-space width of a pixel per unit of world distance along the ray (the caller has multiplied in how many
 *               pixels a cell may span); one cone per launch
 *   min_depth   in [0, PXO_TREE_MAX_DEPTH]: no sample stops above this depth on account of the footprint
 * All in float32, one rounding per operation, no contraction:
 *   g = fl(cone * m),  m = min(invradius[0..2])      once per launch, on the host.  The smallest invradius: a cell is folded
 *                                                    only if its LONGEST world side is at most the footprint (on an
 *                                                    anisotropic volume this errs towards detail)
 *   k = fl(delta_scale * g)                          per ray; delta_scale: the world length of a unit tree-space step
 *   f = fl(tt * k)                                   per sample, at the ray parameter tt the descent is made for: the
 *                                                    footprint in tree units
 *   cap = clamp(126 - (bits(f) >> 23), min_depth, PXO_TREE_MAX_DEPTH)
 * bits(f) >> 23 is the biased exponent of f (f >= 0), so cap is the smallest depth d whose cell side 2^-(d+1) is <= f,
 * integer-exact, no log2.  f = 0 or a denormal gives 126: no cap.  f >= 0.5 (also +inf) gives <= 0: min_depth.
 * The descent stops at the first cell where child == 0 or depth >= cap (which subsumes the depth bound of the other marchers);
 * the sample reads data[node * 8 + cell] of that cell -- the filled row where the cell has a child -- and steps to the exit of
 * THAT cell: cell_exit(local) * 2^-(depth+1) + step_size with the depth the descent stopped at.  The descent resumes from the
 * previous sample's path at min(common, last_depth, cap): without the clamp by cap, a ray whose cap falls between two samples
 * inside one deep cell would read the fine cell.  Compositing, the early stop, its rescale and the aux distances are those
 * of the entry points named above; there is no blending between levels (level changes along a ray are hard steps).
 * Consequences: cone so small that f stays below 2^-(PXO_TREE_MAX_DEPTH+1), or min_depth >= the tree's depth, renders the
 * uncapped image bit for bit; a huge cone renders the level-min_depth view of pxo_tree_lod_fill's closing paragraph bit for bit.
 * The caller answers for `data` being filled; a stale pyramid renders without a word.
 * lobes: NULL for an SH tree, else the [basis_dim,4] lobes of an SG tree (checked as pxo_octree_render_sg_fwd checks them).
 * The aux entry is SH only, as pxo_octree_render_aux_fwd.  PXO_ERR_ARG before any launch: a null tree, cone negative or not
 * finite, min_depth outside its range, and whatever the uncapped entry points refuse.  Asynchronous. */
int pxo_octree_render_foot_fwd(const PxoTree* tree, const float* lobes, const PxoCamera* cam, const float* origins,
                               const float* dirs, const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float cone,
                               int min_depth, float* out_rgb, void* stream);
int pxo_octree_render_foot_aux_fwd(const PxoTree* tree, const PxoCamera* cam, const float* origins, const float* dirs,
                                   const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float cone, int min_depth,
                                   float surface_thresh, float* out_rgb, float* out_aux, void* stream);

/* ---- scene: several trees in one world, each under its own similarity transform  (no svox counterpart; this project's
 *      definition -- the "object insertion" of the PlenOctree paper) ----
 * A scene is n instances, 1 <= n <= PXO_SCENE_MAX_INSTANCES.  Instance i is a float SH tree (PxoTree, any of SH1/4/9/16/25,
 * formats may differ between instances) and a transform world <- object, x_w = s R x_o + t, R a rotation, s > 0.  A ray is
 * carried into every object's frame -- the view direction rotates with it, so no coefficient is touched -- and all trees are
 * marched together, one compositing sample per round.  Forward only.  All in float32, one rounding per operation, no
 * contraction, in this order (o, d, vdir: the world ray of camera_ray or the explicit arrays; M = rot_t, row-major R^T;
 * M v means ((M[a][0] v_0 + M[a][1] v_1) + M[a][2] v_2) per row a):
 *   Set-up, per instance:  o_i = (M (o - t)) * inv_scale,  d_i = M d,  v_i = M vdir;  the tree transform and slab test of the
 *     single-tree renderer on (o_i, d_i) give o, d, invdir, delta_scale_i, tmin_i, tmax_i.  The instance is hit unless
 *     tmax_i < 0 or tmin_i > tmax_i or !(tmin_i < tmax_i); a hit instance WAITS.  c_i = scale * delta_scale_i (tree parameter
 *     -> world length),  enter_i = tmin_i * c_i.  The SH basis of instance i is evaluated on v_i.
 *   State:  a world parameter w, starting at the smallest enter_i of the waiting instances (none: the ray gets the
 *     background), light = 1, and per instance a tree parameter tt_i.
 *   Round:  (1) every waiting instance with enter_i <= w becomes INSIDE at tt_i = tmin_i.  (2) Every inside instance is located
 *     exactly as the single-tree marchers do it (position o + tt d clamped to [0, 1 - 1e-6], descent, delta_i =
 *     cell_exit * 2^-(depth+1) + step_size) and offers step_i = delta_i * c_i; every waiting instance offers the gap
 *     enter_i - w.  D = the minimum of all offers.  With nothing inside, w jumps to the smallest enter_i of the waiting
 *     instances and the round starts over; with nothing waiting either, the ray ends.
 *   Sample:  for every inside instance with sigma_i > sigma_thresh (a LIVE instance), tau_i = (D * inv_scale_i) * sigma_i --
 *     a scaled object keeps its opacity.  tau = ((0 + tau_a) + tau_b) + .. over the live instances in instance order.  If
 *     tau > 0:  att = expf(-tau),  weight = light * (1 - att),  every live instance in instance order adds
 *     (weight * (tau_i / tau)) * sigmoid(logit_i,c) to channel c (logit: the 4-lane channel-aligned sum of
 *     pxo_octree_render_fwd at its default lanes per ray),  light = light * att;  once light <= stop_thresh the colour is
 *     multiplied by 1 / (1 - light) and the ray ends without a background term.  tau == 0 adds nothing.
 *   Advance:  an inside instance whose own step_i == D goes to tt_i + delta_i (its exact cell exit: instances of identical
 *     structure stay in lockstep); every other inside instance goes to tt_i + D / c_i.  An instance leaves when the new
 *     parameter is >= tmax_i or is not greater than the old one (the no-progress guard of the single-tree marchers).  If the
 *     gap of a waiting instance was D, w becomes the largest enter_i among those instances, exactly; otherwise w = w + D.
 *   End:  a ray that did not stop early adds light * background_brightness.
 * Consequences, all bit for bit: one instance under the identity renders the image of pxo_octree_render_fwd; a tree cut into
 * two trees of the same structure with complementary sigma renders the whole tree (x / x = 1); an instance under a signed
 * permutation R and a power-of-two scale seen from the camera carried along renders the plain image.
 * Out of scope, refused where a caller can reach them: gradients, alpha / depth / surface outputs, float16 / palette / SG
 * instances, NDC, a depth cap or footprint, non-uniform scale or shear, more than PXO_SCENE_MAX_INSTANCES instances.  There is
 * no acceleration structure over instances: the per-ray slab tests are the cull. */
#define PXO_SCENE_MAX_INSTANCES 8
typedef struct PxoInstance {
  PxoTree tree;
  float rot_t[9];               /* R^T, row-major */
  float trans[3];               /* t */
  float scale, inv_scale;       /* s and fl(1 / s) */
} PxoInstance;
/* Checks n HOST records before the caller uploads them (host only, no launch).  The renderer reads trees, formats and scales
 * from the device array, which the host cannot inspect at launch: this is where they are refused.  PXO_ERR_ARG: n outside
 * [1, PXO_SCENE_MAX_INSTANCES], a null pointer, a tree the single-tree renderer would refuse (check_tree: null arrays,
 * basis_dim outside {1, 4, 9, 16, 25}, data_dim != 3 basis_dim + 1, n_internal out of range), a scale that is not finite or
 * not > 0, an inv_scale that is not fl(1 / scale), a non-finite rot_t or trans.  Orthonormality of rot_t is the caller's to
 * ensure. */
int pxo_scene_check(const PxoInstance* instances, int n);
/* out_rgb [B,3] (camera mode: [H,W,3]) of the scene in d_instances, the device copy of n records pxo_scene_check has passed;
 * rays and options as pxo_octree_render_fwd takes them.  Always the scene kernel: a one-instance scene is not forwarded to the single-tree
 * renderer.  4 lanes per ray whatever pxo_octree_set_lanes_per_ray says; LDS is sized by n (bytes per workgroup:
 * pxo_scene_lds_bytes).  PXO_ERR_ARG: n outside [1, PXO_SCENE_MAX_INSTANCES], null d_instances, and the option / camera / ray
 * checks of pxo_octree_render_fwd.  Asynchronous; B == 0 launches nothing. */
int pxo_scene_render_fwd(const PxoInstance* d_instances, int n, const PxoCamera* cam, const float* origins, const float* dirs,
                         const float* viewdirs, int64_t B, const PxoRenderOpts* opts, float* out_rgb, void* stream);
/* Dynamic LDS of one workgroup (64 rays) of pxo_scene_render_fwd at n instances (host only). */
int pxo_scene_lds_bytes(int n, size_t* bytes);

/* ---- isosurface meshing  (marching cubes on the device; the reference meshes on the host: nerf_sh/gen_mesh.py:88-130) ----
 * Definition and output order are those of plenoctree_amd/nerf_sh/isosurface.py:marching_cubes, so the arrays compare with ==:
 *   inside(p) = vol[p] >= (float)iso                      vol: float32 [nx, ny, nz], x slowest, finite values
 *   one vertex per grid edge whose two end points differ in `inside`; vertices are numbered axis by axis (all x-edges, then
 *   y, then z), within an axis in C order of the edge's lower grid point p; position = p + (iso - v0) / (v1 - v0) along the
 *   axis, evaluated in float64 from the float32 values and the double iso (index units)
 *   triangles come cell by cell in C order of the cell's lower corner, each cell's in the order of its case-table row
 * The case table is the caller's (uploaded from isosurface.TRI_TABLE / TRI_COUNT; the library holds none):
 *   tri_count  uint8 [256]        triangles of case c = sum over corners (dx + 2 dy + 4 dz) of inside << corner; at most 5
 *   tri_table  int8  [256, 5, 3]  per triangle corner the cell edge it lies on, as  axis << 3 | offset,  offset = dx + 2 dy +
 *                                 4 dz of the edge's lower end point relative to the cell's lower corner
 * Workspace for an N = nx ny nz point grid, with nb = ceil(N / 256) workgroups, nt = ceil(nb / 1024) scan tiles and r(b) = b
 * rounded up to a multiple of 256:
 *   bytes = 3 r(4 N) + 2 r(N) + r(16 nb) + r(32 nt) + 256
 * (three dense int32 vertex-id arrays, a case and a flag byte per point, the scanned block and tile sums of the four
 * counters, the four totals); 0 when min(nx, ny, nz) < 2.  PXO_ERR_ARG when N >= 2^31: the crossing edges of one axis alone
 * could then leave the int32 id range (1024^3 is allowed, 2048 x 2048 x 512 is not). */
int pxo_mc_workspace_bytes(int nx, int ny, int nz, size_t* bytes);
/* Classifies every grid point and cell, scans the per-workgroup counts in `ws` and returns on the HOST counts[0..2] = crossing
 * edges along x, y, z and counts[3] = triangles.  Synchronises `stream`.  min(nx, ny, nz) < 2: all zero, nothing launched,
 * vol / ws may be NULL.  Counts of 2^31 or more are returned as they are; pxo_mc_emit refuses them. */
int pxo_mc_count(const float* vol, int nx, int ny, int nz, double iso, const uint8_t* tri_count, void* ws, size_t ws_bytes,
                 int64_t* counts, void* stream);
/* Writes the mesh counted by pxo_mc_count on the same vol / iso / ws (counts: its host result): vertices float64 [V, 3] with
 * V = counts[0] + counts[1] + counts[2], triangles int64 [T, 3] with T = counts[3] (vertex ids), and, unless NULL, inside_idx
 * int64 [V]: the linear grid index of that end point of each vertex's edge whose value is >= iso.  The per-cell triangle
 * counts are those pxo_mc_count left in `ws` (so tri_count is not passed again).  Asynchronous.  PXO_ERR_ARG if V or T
 * reaches 2^31; V == T == 0 launches nothing. */
int pxo_mc_emit(const float* vol, int nx, int ny, int nz, double iso, const int8_t* tri_table, const void* ws, size_t ws_bytes,
                const int64_t* counts, double* vertices, int64_t* triangles, int64_t* inside_idx, void* stream);
/* Sigma of the tree at the centres of the 2^depth cells per axis, written into sigma float32 [(2^depth + 2 pad)^3] (x
 * slowest) with `pad` layers of 0 around it; packed (int64, same shape, may be NULL) receives the packed index node*8 + cell
 * of the leaf each sample fell in, -1 in the pad.  The centre of cell i is (i + 1/2) / 2^depth, whose binary digits are the
 * bits of i followed by a one: the descent reads its child from those bits, no float coordinate is formed, so it is exact
 * for 1 <= depth <= PXO_TREE_MAX_DEPTH + 1, finer or coarser than the tree's own cells alike.  0 <= pad <= 64.  offset /
 * invradius of the tree are not used: the grid spans the tree's unit cube. */
int pxo_tree_sigma_grid(const PxoTree* tree, int depth, int pad, float* sigma, int64_t* packed, void* stream);
/* ---- per-vertex normals and colour  (the reference's gen_mesh.py:77-82 defines no colour flag and its save_obj, :133-158,
 * is never given a vert_rgb: "# TODO: implement color") ----
 * Sigma gradient at every vertex of the mesh pxo_mc_count / pxo_mc_emit made on the same vol / iso / ws / counts, in the
 * vertices' order: gradients float64 [V, 3], index units, equal to plenoctree_amd/nerf_sh/isosurface.py:vertex_gradients
 * element for element.  Grid-point gradient g(p)[a] in float64 from the float32 samples, one rounding per operation:
 *   (vol[p + e_a] - vol[p - e_a]) * 0.5  where both neighbours exist,  vol[p + e_a] - vol[p]  at the lower border,
 *   vol[p] - vol[p - e_a]  at the upper border;
 * vertex on the edge (lo, hi = lo + e_a), with the f = (iso - v0) / (v1 - v0) that places it:  (1 - f) g(lo) + f g(hi).
 * inside_idx is pxo_mc_emit's output (it names one end of each vertex's edge; the id arrays emit left in `ws` tell which
 * edge).  One vertex per lane.  Asynchronous.  Preconditions and refusals are pxo_mc_emit's; V == 0 launches nothing. */
int pxo_mc_vertex_gradients(const float* vol, int nx, int ny, int nz, double iso, const void* ws, size_t ws_bytes,
                            const int64_t* counts, const int64_t* inside_idx, double* gradients, void* stream);
/* out_rgb[i, c] = sigmoid(sum_k Y_k(dirs[i]) * coef[r * row_stride + c * K + k]),  r = rows ? rows[i] : i,  K = basis_dim,
 * float32, one point per lane, the sum in the order of k.  Y is the SH basis for lobes == NULL, else the SG basis
 * exp(lambda_k (mu_k . d - 1)) / K of lobes float32 [K, 4] rows (lambda, mu) -- the functions the octree renderers call.
 * dirs float32 [n, 3] (unit vectors; not normalised here), rows int64 [n] or NULL, out_rgb float32 [n, 3].  A negative row
 * gives colour 0; rows are not checked against the length of coef (the caller's to bound).  row_stride = 3 K + 1 with rows reads
 * a tree's leaves in place; row_stride = 3 K without rows reads a NeRF's raw_rgb.  basis_dim outside {1, 4, 9, 16, 25},
 * row_stride < 3 K or n outside [0, 2^31): PXO_ERR_ARG.  Asynchronous; n == 0 launches nothing. */
int pxo_shade_points(const float* coef, int64_t row_stride, const int64_t* rows, const float* dirs, int64_t n, int basis_dim,
                     const float* lobes, float* out_rgb, void* stream);

/* mse = mean((clamp(im,0,1) - gt)^2) and its gradient w.r.t. im  (octree/optimization.py:217-219);
 * n = number of floats.  sse_out: device scalar receiving sum of squares (mse = sse/n); grad may be NULL.
 * The clamp is torch.clamp's: a NaN in im stays NaN and makes sse NaN (its own gradient is 0), +-inf clamp to 1 / 0. */
int pxo_image_mse(const float* im, const float* gt, int64_t n, float* grad, float* sse_out, void* stream);

/* torch.optim.SGD step on the tree data (octree/optimization.py:176-181): with momentum mu > 0,
 * buf = mu*buf + g (buf = g on the first step), g' = g + mu*buf if nesterov else buf; p -= lr * g'. */
int pxo_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float mu,
                 int nesterov, int first_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PLENOCTREE_OCTREE_H_ */
