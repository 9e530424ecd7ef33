/*
 * relu_field.h -- C ABI of the MI355X (gfx950) ReLU-Fields render hot path.
 *
 * Shared library: thr3ed_atom_amd/csrc/librelu_field_hip.so (built by __graft_entry__.build()).
 *
 * The reference (akanimax/thr3ed_atom) is pure Python on PyTorch and has no FFI; its plug-in point for
 * this path is the Python callable type
 *     RenderProcedure = Callable[[Module, Rays, RenderConfig, Optional[int]], RenderOut]
 *     (thre3d_atom/thre3d_reprs/renderers.py:22-25), invoked only at
 *     thre3d_atom/modules/volumetric_model.py:112-114.
 * The entry points below are what a binding for that path binds to (INTEGRATION.md shows the ctypes stub);
 * each one names the reference code it replaces.
 *
 * Conventions
 *  - All pointers named *_dev are DEVICE pointers owned by the caller (PyTorch allocations); the library
 *    never allocates, frees or retains them.  All tensors are contiguous float32 unless a stride is given.
 *  - Every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); no implicit synchronisation.
 *  - Re-entrant: no mutable state is shared between calls.  What the library keeps per process is read-only after its first
 *    use: tuning knobs read from the environment ($RF_FRAME_TILES, $RF_FWD_PAIR, $RF_EMIT_PAIR, $RF_BRICK_STAGGER, $RF_FAR_ADDRESSING, $RF_STEP_SPECIALISED -- A/B switches,
 *    unset in production) and the cached result of one-time hipFuncSetAttribute calls (dynamic LDS size of the brick kernels).
 *    Return value: RF_OK (0) or a negative RF_ERR_* code; nothing is thrown across the ABI.  rf_error_string() maps a code to text.
 *  - Gradient buffers are ACCUMULATED into (+=) with float32 hardware atomics; the caller zero-fills them
 *    (or keeps accumulating across several renders, which is autograd's semantics).
 */
#ifndef RELU_FIELD_H_
#define RELU_FIELD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RF_ABI_VERSION 4
/* brick_size value for bricks of 4 x 8 x 8 nodes (see the binned backward below) */
#define RF_BRICK_4X8X8 488

enum {
  RF_OK = 0,
  RF_ERR_NULL_POINTER = -1,
  RF_ERR_BAD_SHAPE = -2,
  RF_ERR_UNSUPPORTED = -3,
  RF_ERR_LAUNCH = -4
};

/* density activation variants of VoxelGrid (thre3d_reprs/voxels.py:292-309; the three configurations the
 * reference's trainer script builds: train_sh_based_voxel_grid_with_posed_images.py:169-192) */
enum {
  RF_DENSITY_RELU = 0,     /* pre = identity, post = ReLU      (the ReLU field)       */
  RF_DENSITY_SOFTPLUS = 1, /* pre = identity, post = softplus(beta=1, threshold=20)   */
  RF_DENSITY_ABS = 2,      /* pre = |.|,      post = identity  (traditional grid)     */
  RF_DENSITY_IDENTITY = 3  /* pre = identity, post = identity                         */
};

/* storage layout of the grid tensors handed to the kernels */
enum {
  RF_LAYOUT_REFERENCE = 0, /* the reference's two tensors: densities [X,Y,Z,1], features [X,Y,Z,F]
                              (feature index = colour*K + k, thre3d_reprs/voxels.py:70-71)                 */
  RF_LAYOUT_SPLIT = 1,     /* MI355X-native: densities_dev -> base [X,Y,Z,4] = (density, sh0 r, sh0 g, sh0 b),
                              features_dev -> rest [X,Y,Z,F-3] with index = colour*(K-1) + (k-1), k >= 1
                              (NULL when F == 3).  The diffuse pass and the density gather touch only the
                              16-byte base records; gradient buffers use the same layout.                 */
  RF_LAYOUT_BRICKED = 2    /* the split channel arrangement with BRICK-MAJOR node order: the grid is cut into
                              8x8x8-node bricks stored contiguously, base [NBX,NBY,NBZ,8,8,8,4] and rest
                              [NBX,NBY,NBZ,8,8,8,F-3] with NB* = ceil(dim/8) (nodes beyond dims are padding the
                              kernels never touch).  The 8 corners of a cell lie within ~1 KB (base) instead of
                              megabytes apart, and a brick of the binned backward is one contiguous write.    */
};

/* render flags (SHVoxGridRenderConfig fields, thre3d_reprs/renderers.py:28-45) */
enum {
  RF_FLAG_WHITE_BKGD = 1,     /* white_bkgd                                                        */
  RF_FLAG_RENDER_DIFFUSE = 2, /* render_diffuse: only the degree-0 SH coefficient of each colour   */
  RF_FLAG_AABB_SAMPLING = 4,  /* optimized_sampling: per-ray [t_enter, t_exit] from the slab test  */
  RF_FLAG_OCCUPANCY_SKIP = 8, /* use RFGrid.occupancy_dev to skip provably-empty cells (exact)     */
  RF_FLAG_JITTER_KEYED = 16   /* perturb_sampled_points without a [N,S] tensor: when RFRayBatch.t_rand_dev is NULL the jitter
                                 of (ray, sample) is a counter-based hash of (jitter_key, first_ray + ray, sample) -- the law of
                                 torch.rand (uniform on [0,1), independent), evaluated where it is used                    */
};

/* The dense SH + density voxel grid: VoxelGrid (thre3d_reprs/voxels.py:46-331). */
typedef struct RFGrid {
  const float* densities_dev; /* [X, Y, Z, 1]; z fastest                                              */
  const float* features_dev;  /* [X, Y, Z, F]; F = 3 * (deg+1)^2, channel-major: index = colour*K + k  */
  int32_t dims[3];            /* X, Y, Z                                                               */
  int32_t num_features;       /* F in {3, 12, 27, 48}                                                  */
  int64_t density_stride;     /* floats between consecutive voxels of densities_dev (1 = reference)   */
  int64_t feature_stride;     /* floats between consecutive voxels of features_dev  (F = reference)   */
  float aabb_min[3];          /* float32 planes of the bounding box (voxels.py:187-212)                */
  float aabb_max[3];
  float norm_scale[3];        /* q = p * scale + bias maps the AABB to [-1, 1] (voxels.py:214-223,     */
  float norm_bias[3];         /*   utils/imaging_utils.py:58-63); computed by the host in float32      */
  float density_scale;        /* expected_density_scale rho, applied BEFORE interpolation              */
  int32_t density_mode;       /* RF_DENSITY_*                                                          */
  int32_t layout;             /* RF_LAYOUT_*; strides above are then those of base / rest              */
  const uint32_t* occupancy_dev; /* optional bit mask, one bit per cell incl. the border cells:
                                    (X+1)*(Y+1)*(Z+1) bits, see rf_build_occupancy; may be NULL      */
} RFGrid;

/* A posed pinhole camera (CameraIntrinsics + CameraPose, utils/imaging_utils.py:17-30) for rays generated in-kernel:
 * cast_rays (rendering/volumetric/utils/misc.py:12-50) fused into the render.  HOST struct. */
typedef struct RFCamera {
  int32_t height, width;
  float focal;
  float pose[12]; /* [3,4] row-major = rotation | translation, camera-to-world */
} RFCamera;

/* Flat rays + sampling parameters: Rays (rendering/volumetric/render_interface.py:13-44),
 * sample_uniform_points_on_rays (rendering/volumetric/sample.py:15-68). */
typedef struct RFRayBatch {
  const float* origins_dev;    /* [N, 3]   (may be NULL when `camera` is given)                        */
  const float* directions_dev; /* [N, 3], not normalised                                               */
  int64_t num_rays;            /* N                                                                    */
  int32_t num_samples;         /* S >= 1                                                               */
  float near;                  /* CameraBounds.near / far (float32)                                    */
  float far;
  const float* t_vals_dev;     /* [S] = linspace(0, 1, S) (sample.py:46)                               */
  const float* t_rand_dev;     /* [N, S] jitter in [0,1) (sample.py:63) or NULL = perturb off / keyed  */
  uint64_t jitter_key;         /* RF_FLAG_JITTER_KEYED: key of the counter-based jitter                */
  int64_t first_ray;           /* global index of ray 0 of this batch: position in the keyed jitter stream, and the
                                  pixel (row-major) of ray 0 when `camera` generates the rays -- chunks of one frame
                                  rendered with first_ray = chunk offset give the frame's rays bit for bit      */
  const RFCamera* camera;      /* optional HOST pointer: rays r = pixel-centre rays of pixels first_ray + r of this
                                  camera (utils/misc.py:12-50); origins_dev / directions_dev are then ignored   */
} RFRayBatch;

/* Per-ray outputs: RenderOut (render_interface.py:47-83) + extra {"disparity", "accumulated_weight"}. */
typedef struct RFRenderOut {
  float* colour_dev;    /* [N, 3]                                                                      */
  float* depth_dev;     /* [N]                                                                         */
  float* acc_dev;       /* [N]                                                                         */
  float* disparity_dev; /* [N]   (NaN where acc == 0, like the reference)                              */
  /* Optional per-sample cache written by the forward pass and consumed by rf_render_backward* (all four NULL for
   * inference).  Only the samples that can carry gradient are cached -- inside the box, T != 0, and sigma != 0 under ReLU
   * (every other sample contributes exactly nothing to any adjoint) -- COMPACTED per chunk of 64 samples: the j-th such
   * sample of chunk c of ray r is entry r * S + 64 c + j, and bit l of chunk_mask_dev[r][c] says that sample 64 c + l is
   * one of them.  Everything else in the two caches is left unwritten (and unread). */
  float* sample_cache_dev; /* [N, S, 4] = (raw r, raw g, raw b, sigma)                                 */
  float* trans_cache_dev;  /* [N, S]    = transmittance T_i                                            */
  int32_t* stop_cache_dev; /* [N]       = number of samples the forward pass processed                 */
  uint64_t* chunk_mask_dev; /* [N, ceil(S / 64)] which samples of each chunk are cached               */
  /* Optional (with the cache): the forward pass also COUNTS the cached samples per (brick, flags) key of the binned
   * backward (see rf_render_backward_emit) into key_hist_dev [8 * nbricks] (added to; clear before the first use), so
   * that rf_render_backward_emit_direct can write their records straight to the final positions. */
  int32_t* key_hist_dev;
  int32_t brick_size;      /* 4, 8 or RF_BRICK_4X8X8 (only read when key_hist_dev != NULL)             */
} RFRenderOut;

/* Upstream gradients of a render (all [N, ...] device arrays; any may be NULL = zero). */
typedef struct RFRenderGrads {
  const float* grad_colour_dev; /* [N, 3] */
  const float* grad_depth_dev;  /* [N]    */
  const float* grad_acc_dev;    /* [N]    */
} RFRenderGrads;

int rf_abi_version(void);
const char* rf_error_string(int code);
/* sizeof() of the ABI structs as this library was compiled, so that a binding can verify its own mirrors before the first
 * call: which = 0 RFGrid, 1 RFRayBatch, 2 RFRenderOut, 3 RFRenderGrads, 4 RFBrickList, 5 RFAdamState, 6 RFCamera,
 * 7 RFRaySelection, 8 RFPassScratch, 9 RFTrainStep, 10 RFGeometryOut, 11 RFImage; -1 for any other value. */
int rf_abi_struct_size(int which);

/* cast_rays (rendering/volumetric/utils/misc.py:12-50) + flatten_rays (:53-57):
 * all H*W pixel-centre rays of one camera, row-major (ray = i*W + j).  rotation/translation are HOST
 * pointers to 9 / 3 floats (camera-to-world). */
int rf_cast_rays(int32_t height, int32_t width, float focal, const float* rotation_host,
                 const float* translation_host, float* origins_dev, float* directions_dev, void* stream);

/* Which kernel rf_render_forward uses for a frame of this camera (RFRayBatch.camera set, no sample cache; the frame loop of
 * modules/volumetric_model.py:143-172): 1 = ray packets (one wavefront per 8 x 8 pixel tile, the tile's 4 x 4 x 4-node neighbourhood
 * staged through LDS once per sample index), 0 = one wavefront per ray; negative = error code.  The packet kernel is chosen where a
 * tile's footprint at the volume's centre stays within 2 voxels (3 with RF_FLAG_OCCUPANCY_SKIP and a mask), on split / bricked
 * storage with a 16-byte aligned base tensor, every SH degree, keyed jitter or none (a frame with a jitter TABLE goes to the per-ray
 * kernel) and at most 1024 samples per ray (this function does not see the sample count: a frame of more goes to the per-ray kernel
 * whatever it answers -- a packet lane adds a ray's samples sequentially, and that float32 sum drifts past the parity bar at 4096+);
 * $RF_FRAME_TILES = 1 / 0 in the environment forces / forbids it within these rules.  Both kernels compute a pixel with the
 * same per-sample arithmetic and differ in the order a ray's weighted samples are added (<= 2e-6 on colours).  Host-side only: no
 * device access.  (Added to ABI version 4 compatibly: no existing struct or signature changed.) */
int rf_frame_render_kernel(const RFGrid* grid, const RFCamera* camera, uint32_t flags);

/* The training-iteration ray source (modules/trainers.py:281-303): rays of the selected pixels only.
 * pixel_index_dev[r] indexes the concatenation of B images: b*H*W + i*W + j; poses_dev is [B, 3, 4]
 * (rotation | translation) on the device. */
int rf_cast_selected_rays(int32_t height, int32_t width, float focal, const float* poses_dev,
                          int32_t num_poses, const int64_t* pixel_index_dev, int64_t num_rays,
                          float* origins_dev, float* directions_dev, void* stream);

/* sample_random_rays_and_pixels_synchronously (rendering/volumetric/utils/misc.py:117-129) fused with the ray
 * casting and pixel gathering around it (modules/trainers.py:281-303): element r of the batch is pixel
 * PRP_key(r) of the num_batch_images*H*W pixels of the image batch, PRP a keyed bijection of that range
 * (distinct pixels, uniformly distributed: the law of torch.randperm(P)[:R], without sorting P keys).
 * poses_dev [M,3,4] and pixel_table_dev [M*H*W,3] describe ALL images; image_ids_dev [num_batch_images]
 * (int64, may be NULL = images 0..B-1) picks the batch.  pixel_index_dev [R] (may be NULL) receives
 * b*H*W + i*W + j. */
int rf_select_rays_and_pixels(int32_t height, int32_t width, float focal, const float* poses_dev,
                              const int64_t* image_ids_dev, int32_t num_batch_images, const float* pixel_table_dev,
                              uint64_t key, int64_t first_index, int64_t num_rays, float* origins_dev,
                              float* directions_dev, float* pixels_dev, int64_t* pixel_index_dev, void* stream);

/* _ray_aabb_intersection (rendering/volumetric/sample.py:71-184): bounds_dev [N, 2], hit_dev [N] (0/1,
 * may be NULL). */
int rf_ray_aabb_bounds(const float* origins_dev, const float* directions_dev, int64_t num_rays, float near,
                       float far, const float* aabb_min_host, const float* aabb_max_host,
                       float* bounds_dev, float* hit_dev, void* stream);

/* render_sh_voxel_grid (thre3d_reprs/renderers.py:48-102) = sampler (sample.py) -> VoxelGrid.forward
 * (voxels.py:276-331) -> SH (utils/spherical_harmonics.py:64-116) -> AABB mask (process.py:80-84) ->
 * compositing (accumulate.py:31-113), fused in one launch. */
int rf_render_forward(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* out,
                      void* stream);

/* The adjoint of rf_render_forward into the grid (the reference gets it from autograd:
 * grid_sampler_3d_backward, cumprod_backward, ...).  `fwd` must hold the caches written by the matching
 * forward call.  grad_densities_dev [X,Y,Z,1] and grad_features_dev [X,Y,Z,F] are accumulated into. */
int rf_render_backward(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* fwd,
                       const RFRenderGrads* grads, float* grad_densities_dev, float* grad_features_dev,
                       void* stream);

/* ---- binned backward: the same adjoint as rf_render_backward without float atomics ----------------------------------
 * The atomic scatter of rf_render_backward is bound by the memory-side atomic unit.  The binned variant turns every
 * contributing sample into a RECORD, puts the records in (brick, flags) order and lets one workgroup per brick sum them
 * on chip under exclusive ownership:
 *
 *   key  = ((((bx * 2 + f_x) * NBY + by) * NBZ + bz) << 2) | f_y | f_z << 1;  (bx, by, bz) = the brick (brick_size^3 nodes,
 *          brick_size in {4, 8}; or RF_BRICK_4X8X8: 4 x 8 x 8 nodes, the bricks of the single-GPU optimizer pass -- four
 *          256-thread workgroups per CU instead of two 512-thread ones; accepted by the render / emit / offset functions, by
 *          rf_brick_accumulate, rf_brick_accumulate_adam[_mirror|_range] and rf_train_step: SH degree 0 or 2 -- or base-channel lists
 *          alone --, and with the optimizer every grid tensor below 2^30 elements)
 *          holding the LOWER node of the sample's cell;  f_a = the cell's upper node on axis a belongs
 *          to the next brick (so the record also touches that neighbour's nodes).  8 * nbricks keys.  The order is x-slab
 *          major with the x flag directly below the slab index: everything that touches the nodes of the x-slabs [s0, s1)
 *          of bricks is ONE contiguous key range, [key(s0 - 1, f_x = 1), key(s1, f_x = 0)) -- what a data-parallel rank
 *          sends the owner of those slabs is a single slice of its sorted list (see rf_brick_accumulate_adam_range).
 *   record = rf_expanded_record_floats(F) floats, COMPACT:
 *          F > 3:  (continuous index x, y, z, dL/d density) (dL/d raw r, g, b, v_x) (v_y, v_z, 0, 0) -- 48 B; v = the ray's
 *                  unit viewing direction.  The per-channel values dL/d raw[colour] * Y_k(v) of a node's 3K + 1 channels are
 *                  expanded by rf_brick_accumulate in LDS (the reference's evaluate_spherical_harmonics operation order):
 *                  they never exist in HBM.
 *          F == 3, and every list of a render_diffuse pass whatever the grid's degree:  (index x, y, z, 0) (dL/d density,
 *                  dL/d sh0 r, g, b) -- 32 B.
 *   offsets [8 * nbricks + 1] (int64): start of every key class in the record list (last = end).
 *
 * Three front ends produce (records in key order, offsets); rf_brick_accumulate consumes them:
 *   A. fused (default of the trainer): rf_render_forward with RFRenderOut.key_hist_dev COUNTS the records per key ->
 *      rf_bin_offsets -> rf_render_backward_emit_direct writes each record at the next free position of its key.
 *      No per-slot arrays; integer atomics only (counters, cursors); any number of bricks up to 2^18.
 *   B. counting sort after the fact: rf_render_backward_emit (per-slot 16-bit keys + per-slot records, hist_dev) ->
 *      rf_bin_offsets -> rf_scatter_records.
 *   C. deterministic: rf_render_backward_emit -> torch.sort of the keys (stable radix) + searchsorted ->
 *      rf_expand_records.  Fixed float32 summation order: bit-reproducible gradients.
 *   B and C use 16-bit keys: at most 4096 bricks.  The order inside a key class depends on atomic timing in A and B.
 *
 * rf_brick_accumulate: one workgroup per brick OWNS the brick's nodes: it reads exactly the key classes that touch them
 * (its own and, per flags, up to 7 lower neighbours'), sums them in MFMA accumulators (node sums = trilinear weights x the
 * records' channel values, four records per v_mfma_f32_16x16x4_f32: exact float32 fma chains, no atomics of any kind,
 * summation order fixed by the record order) and writes the brick with plain coalesced stores: accumulate = 0 OVERWRITES every
 * element of the gradient tensors (no zero-fill needed; diffuse lists: only density + degree-0 gradients), accumulate = 1
 * adds.  Up to 16 lists per call, at most 8 of a kind, the full-width lists first: (specular list, render_diffuse list) = BOTH
 * renders of a training iteration (modules/trainers.py:306-341) in one pass (the base-channel records go into the first four
 * channel columns of the same accumulators); under data parallelism one pair per source rank.  Cubic bricks take any SH degree: what
 * decides is the LDS check of the launch (batch buffers or accumulator image above 150 KB are refused), and degree 3 passes it with
 * brick_size 8 (123 KB, one workgroup per CU) as well as with brick_size 4.  A call whose lists are all render_diffuse lists runs on
 * the four base channels whatever the grid's degree and leaves every higher-degree element untouched.
 * RF_ERR_UNSUPPORTED combinations of the brick pass (checked before anything is launched; tests/test_hip_brick_matrix.py asserts them):
 *   - RF_BRICK_4X8X8 with full-width lists on a grid of SH degree 1 or 3 (rf_brick_accumulate and the optimizer variants alike);
 *   - the optimizer variants with accumulate semantics, on RF_LAYOUT_REFERENCE, on a grid of SH degree 1 or 3, or with base-channel
 *     lists alone on an SH grid (the update needs the complete gradient of whole float4s);
 *   - RF_BRICK_4X8X8 with the optimizer when a grid tensor has 2^30 elements or more, or the padded grid more than 2^24 nodes;
 *   - rf_brick_accumulate_adam_mirror unless RF_BRICK_4X8X8, RF_LAYOUT_SPLIT, the whole grid, dims multiples of (4, 8, 8);
 *   - rf_brick_accumulate_adam_split unless brick_size 8 and the one-round flush. */
typedef struct RFBrickList {
  const float* records_sorted_dev; /* [capacity, rf_expanded_record_floats(F)] (diffuse lists: F = 3) */
  const int64_t* offsets_dev;      /* [8 * nbricks + 1] start of each (brick, flags) class            */
  int32_t render_diffuse;          /* records come from a render_diffuse pass                         */
} RFBrickList;

int32_t rf_expanded_record_floats(int32_t num_features);

/* exclusive prefix sums of the per-key counters hist_dev [num_keys] -> offsets_dev [num_keys + 1] (positions start at 0)
 * and an int32 copy cursor_dev [num_keys] for the atomic cursors of A / B */
int rf_bin_offsets(const int32_t* hist_dev, int32_t num_keys, int64_t* offsets_dev, int32_t* cursor_dev, void* stream);

/* A: every sample counted (= cached) by the forward call that produced `fwd` writes its record -- zeros if its gradient
 * happens to vanish -- at the next free position of its key; hist_clear_dev
 * [8 * nbricks] (may be NULL) is cleared for the next iteration. */
int rf_render_backward_emit_direct(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* fwd,
                                   const RFRenderGrads* grads, int32_t brick_size, int32_t* cursor_dev,
                                   float* records_sorted_dev, int32_t* hist_clear_dev, void* stream);

/* B / C: per contributing sample its record (format above) at its SLOT: records_dev [N*S, rf_expanded_record_floats(F)]
 * (render_diffuse passes: F = 3), and, for EVERY slot, keys_dev [N*S] (-1 = no gradient).  hist_dev [8 * nbricks] (may be NULL;
 * zero before the first use) is incremented by the number of records per key (B). */
int rf_render_backward_emit(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* fwd,
                            const RFRenderGrads* grads, int32_t brick_size, int16_t* keys_dev, float* records_dev,
                            int32_t* hist_dev, void* stream);
/* B: every keyed slot's record goes to the next free position of its key; clears hist_dev (may be NULL) */
int rf_scatter_records(const RFGrid* grid, const int16_t* keys_dev, const float* records_dev, int64_t capacity,
                       int32_t* cursor_dev, int32_t render_diffuse, float* records_sorted_dev, int32_t* hist_dev, int32_t num_keys,
                       void* stream);
/* C: records_sorted[i] = record of slot perm_dev[i] for *begin_dev (= offsets[0]: unkeyed slots sort in front) <= i < capacity */
int rf_expand_records(const RFGrid* grid, const float* records_dev, const int64_t* perm_dev, const int64_t* begin_dev,
                      int64_t capacity, int32_t render_diffuse, float* records_sorted_dev, void* stream);

int rf_brick_accumulate(const RFGrid* grid, int32_t brick_size, const RFBrickList* lists, int32_t num_lists,
                        float* grad_densities_dev, float* grad_features_dev, int32_t accumulate, void* stream);

/* The optimizer of the training iteration (torch.optim.Adam(betas, eps), modules/trainers.py:242-250,339-341) fused into the
 * brick pass: the workgroup that owns a brick holds the COMPLETE gradient of its parameters on chip (when the lists carry
 * every render of the iteration), so it applies the Adam update right there -- the gradient tensor never exists in HBM and
 * the separate optimizer pass (7 x 4 B per parameter) becomes 6 x 4 B inside this one.  Same arithmetic as rf_adam_step
 * (hardware square root and reciprocal, 1 ulp).
 * Requirements: RF_LAYOUT_SPLIT / RF_LAYOUT_BRICKED with F in {3, 27} (whole float4s per node), all six pointers 16-byte
 * aligned, param_*_dev the very tensors `grid` describes.  Bricks without records still take their (zero-gradient) step. */
typedef struct RFAdamState {
  float* param_first_dev;      /* = grid->densities_dev (base)  */
  float* param_second_dev;     /* = grid->features_dev  (rest; NULL when F == 3) */
  float* exp_avg_first_dev;    /* first moments, same shapes    */
  float* exp_avg_second_dev;
  float* exp_avg_sq_first_dev; /* second moments                */
  float* exp_avg_sq_second_dev;
  float lr, beta1, beta2, eps;
  int32_t step;                /* 1-based step count (bias correction) */
} RFAdamState;

int rf_brick_accumulate_adam(const RFGrid* grid, int32_t brick_size, const RFBrickList* lists, int32_t num_lists,
                             const RFAdamState* adam, void* stream);

/* The same pass (whole grid, brick_size == RF_BRICK_4X8X8) for a grid held in the REFERENCE's two tensors whose forward passes run
 * from a split-layout shadow: `grid` / `adam` describe the shadow (RF_LAYOUT_SPLIT, F in {3, 27}), and the flush writes every
 * updated parameter a second time, in the reference's own layout -- mirror_densities_dev [X,Y,Z,1], mirror_features_dev [X,Y,Z,F]
 * with feature index = colour * K + k (thre3d_atom/thre3d_reprs/voxels.py:70-71, rendering/volumetric/process.py:61,66), both
 * contiguous and 16-byte aligned -- so that the nn.Parameters a reference user holds stay in sync with the shadow without a
 * re-layout launch (rf_convert_grid: 235 MB read + 235 MB written per iteration at 128^3 / SH degree 2; here +235 MB written out
 * of LDS).  Grid dims must be multiples of (4, 8, 8); RF_ERR_UNSUPPORTED otherwise (use rf_brick_accumulate_adam, then
 * rf_convert_grid).  This is what optimizer.step() of modules/trainers.py:341 becomes for the strict drop-in.  (Added to ABI
 * version 4 compatibly: no existing struct or signature changed.) */
int rf_brick_accumulate_adam_mirror(const RFGrid* grid, int32_t brick_size, const RFBrickList* lists, int32_t num_lists,
                                    const RFAdamState* adam, float* mirror_densities_dev, float* mirror_features_dev, void* stream);

/* The same pass restricted to the bricks [first_brick, first_brick + num_bricks) (brick id = (bx * NBY + by) * NBZ + bz): the
 * OWNER-COMPUTES step of data-parallel training.  The reference trains on one device (modules/trainers.py:338-341 is its
 * loss.backward(); optimizer.step()); with N ranks each rank owns a range of x-slabs of bricks, receives from every rank the
 * slice of that rank's sorted record lists that touches its slabs (one contiguous key range, see the key order above; the
 * lists here are then one (specular, render_diffuse) pair per source rank, each with that rank's offsets table and a records
 * pointer positioned such that records_sorted_dev + offsets[k] * record size is the first record of key k), sums them and
 * applies Adam to its own parameters only; an all-gather of the parameters follows.  Scale the losses by 1 / N
 * (RFTrainStep.loss_scale) so that the sum over the ranks' records is the mean gradient. */
int rf_brick_accumulate_adam_range(const RFGrid* grid, int32_t brick_size, const RFBrickList* lists, int32_t num_lists,
                                   const RFAdamState* adam, int32_t first_brick, int32_t num_bricks, void* stream);

/* The owner's pass with SEVERAL workgroups per brick.  With N ranks an owned brick receives N times the records of the single-GPU
 * case while the launch covers only 1 / N of the bricks: one workgroup per brick leaves most of the machine idle behind the
 * heaviest bricks (measured at N = 8 on the bench workload: 0.35 ms for the x-slab through the middle of the volume, half of the
 * 512 workgroup slots unused).  Here `parts` (1..8) workgroups share a brick: workgroup (brick, part) sums the lists l of each kind
 * with l % parts == part -- the source ranks are dealt out --, the partial accumulator images meet in `scratch_dev`, and the last
 * workgroup of a brick to arrive adds them and applies Adam (no workgroup waits for another).  scratch_dev: caller-owned,
 * rf_brick_split_scratch_bytes(grid, num_bricks, parts) bytes, 16-byte aligned, ZERO before the first launch; every launch leaves
 * its counters zero again (launches that share a scratch buffer must not overlap).  Needs 8^3 bricks and the one-round flush (the
 * grid tensors below 2^30 elements); RF_ERR_UNSUPPORTED otherwise (use rf_brick_accumulate_adam_range).  (Added to ABI
 * version 4 compatibly: no existing struct or signature changed.) */
int64_t rf_brick_split_scratch_bytes(const RFGrid* grid, int32_t num_bricks, int32_t parts);
int rf_brick_accumulate_adam_split(const RFGrid* grid, int32_t brick_size, const RFBrickList* lists, int32_t num_lists,
                                   const RFAdamState* adam, int32_t first_brick, int32_t num_bricks, int32_t parts, void* scratch_dev,
                                   int64_t scratch_bytes, void* stream);

/* ---- beside the render path and the training step (those, i.e. whatever no unit is named for: csrc/relu_field_kernels.hip) ----
 * csrc/grid_kernels.hip      rf_grid_query, rf_grid_query_backward, rf_build_occupancy, rf_upsample_grid, rf_convert_grid,
 *                            rf_tv_grad, rf_prune_grid, rf_node_bounds, rf_resample_grid
 * csrc/ray_grad_kernels.hip  rf_grid_query_backward_points, rf_render_backward_rays
 * csrc/ray_walk_kernels.hip  rf_node_max_weight, rf_distortion, rf_render_geometry */

/* VoxelGrid.forward (thre3d_reprs/voxels.py:276-331) as a standalone point query: points_dev [M,3] (any
 * points: zeros padding outside the grid, no AABB mask) -> out_dev [M, F+1] = (F interpolated features in the
 * reference order colour*K + k, activated density).  Bit-for-bit the ATen grid_sample recipe. */
int rf_grid_query(const RFGrid* grid, const float* points_dev, int64_t num_points, float* out_dev, void* stream);

/* Its adjoint into the grid tensors (accumulates, storage layout of `grid`); grad_out_dev is [M, F+1]. */
int rf_grid_query_backward(const RFGrid* grid, const float* points_dev, int64_t num_points,
                           const float* grad_out_dev, float* grad_densities_dev, float* grad_features_dev,
                           void* stream);

/* Its adjoint into the query points (the reference gets it from autograd: grid_sample's gradient with respect to its
 * sampling grid, through the normalisation of voxels.py:214-223): grad_points_dev [M, 3] is WRITTEN (not accumulated) from
 * grad_out_dev [M, F+1]; every layout and density mode, the density channel through its activation slope.  (Added to ABI
 * version 4 without a version change: additive.) */
int rf_grid_query_backward_points(const RFGrid* grid, const float* points_dev, int64_t num_points,
                                  const float* grad_out_dev, float* grad_points_dev, void* stream);

/* dL/d(origins), dL/d(directions) of rf_render_forward (the reference gets them from autograd through
 * _ray_aabb_intersection of sample.py:71-184, grid_sample's grid gradient, the SH basis of utils/spherical_harmonics.py and
 * the interval lengths of accumulate.py:50-55): grad_origins_dev / grad_directions_dev [N, 3] are WRITTEN (not accumulated;
 * either may be NULL).  `fwd` holds the caches of the matching forward call.  One result per ray, no atomics: bitwise
 * deterministic.  Rays generated in-kernel (RFRayBatch.camera != NULL) -> RF_ERR_UNSUPPORTED.  The jitter (t_rand) gets no
 * gradient.  (Added to ABI version 4 without a version change: additive.) */
int rf_render_backward_rays(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, const RFRenderOut* fwd,
                            const RFRenderGrads* grads, float* grad_origins_dev, float* grad_directions_dev, void* stream);

/* Exact empty-cell mask for RF_FLAG_OCCUPANCY_SKIP (BASELINE.json configs[4]):
 * bit (cx, cy, cz), cx in [0, X] etc., is set iff any of the (up to 8) grid nodes
 * (cx-1..cx, cy-1..cy, cz-1..cz) that exist has a raw density that can yield sigma != 0 under
 * `density_mode` (ReLU: D*rho > threshold; other modes: every cell is occupied).  With threshold = 0 and
 * ReLU the skip is bit-exact.  occupancy_dev holds ceil((X+1)(Y+1)(Z+1)/32) words. */
int rf_build_occupancy(const RFGrid* grid, float threshold, uint32_t* occupancy_dev, void* stream);

/* Stage transition of the trainer: scale_voxel_grid_with_required_output_size (thre3d_reprs/voxels.py:334-373), i.e.
 * F.interpolate(mode="trilinear", align_corners=False) of the whole [F+1]-channel volume, from `src` into the tensors `dst`
 * describes (any dims, any layout on either side, same num_features; dst's tensors are overwritten; dst's AABB / activation
 * fields are not used).  ATen's index and weight arithmetic and the summation order of its channels-last CPU kernel (8-wide
 * vector body, scalar tail): bit-identical to what the reference's function returns on the CPU.  (Added to ABI version 3
 * compatibly: no existing struct or signature changed.) */
int rf_upsample_grid(const RFGrid* src, const RFGrid* dst, void* stream);

/* Re-layout: every (node, channel) of `src` copied into the tensors `dst` describes (same dims and num_features, any layouts;
 * dst's tensors are overwritten, its AABB / activation fields are not used).  A binding that must keep the reference's own two
 * Parameters (thre3d_reprs/voxels.py:70-71) can keep an RF_LAYOUT_SPLIT shadow of them for the forward passes this way. */
int rf_convert_grid(const RFGrid* src, const RFGrid* dst, void* stream);

/* Total-variation regulariser of the grid parameters (Plenoxels / DVGO / TensoRF ship the same term): for node n, channel c and
 * axis a, d_a = theta[n + e_a] - theta[n] (0 where n + e_a is outside the grid), r = sqrt(epsilon + sum_a d_a^2),
 *   TV_density = mean over nodes of r(density),  TV_features = mean over nodes and the F feature channels of r.
 * The density is the RAW parameter (before density_scale and the activation: independent of density_mode).  The call ADDS
 *   weight_density * d TV_density / d theta   and   weight_features * d TV_features / d theta
 * to grad_first_dev / grad_second_dev, which follow the layout of `grid` like every gradient buffer of this ABI (split / bricked:
 * the base record holds the density and the three degree-0 coefficients; padding nodes of bricked storage are neither read nor
 * written).  One thread owns an element and gathers its six terms: no atomics on the gradient, bitwise reproducible.  A channel whose
 * weight is 0 is left bit-untouched, and the tensor it alone lives in may be NULL (grad_second_dev is NULL anyway for F == 3 on split /
 * bricked storage).  sums_dev (optional, 2 floats, the caller zeroes them): sums_dev[0] += sum of r(density), sums_dev[1] += sum of
 * r(features), UNWEIGHTED -- the caller divides by N and N * F for the two TV values (the convention of rf_l1_loss_grad).
 * Both weights 0: nothing is launched (sums included), RF_OK.  Before any device access: RF_ERR_NULL_POINTER (grid, its tensors, a
 * gradient tensor a non-zero weight needs), RF_ERR_BAD_SHAPE (dims, a non-finite or non-positive epsilon, a negative or non-finite
 * weight, a gradient pointer that IS the parameter tensor it belongs to).  Every F in {3, 12, 27, 48}, every density mode, dims >= 1.
 * (Added to ABI version 4 compatibly: no existing struct or signature changed.) */
int rf_tv_grad(const RFGrid* grid, float weight_density, float weight_features, float epsilon, float* grad_first_dev,
               float* grad_second_dev, float* sums_dev, void* stream);

/* Visibility statistics of a trained field (what Plenoxels / DVGO prune their grids by): for every ray of the batch and every
 * sample i the forward pass treats as inside the box, w_i = T_i * alpha_i exactly as rf_render_forward computes it (same sampling,
 * jitter, first_ray / camera, RF_FLAG_AABB_SAMPLING and RF_FLAG_OCCUPANCY_SKIP handling, last interval 1e10), and for each of the 8
 * corners k of the sample's cell with trilinear weight b_k:   M[n_k] = max(M[n_k], w_i * b_k)   (one float32 multiply; a product
 * equal to 0 updates nothing).  max_weight_dev is [X, Y, Z] float32, z fastest, in PLAIN node order whatever grid->layout is; the
 * caller owns and initialises it (normally zeros; finite values >= 0) and the call only RAISES entries: one call per view
 * accumulates over views.  The update is an atomic max on the bit pattern behind a plain load, so the result does not depend on
 * the order of arrival: bitwise reproducible.  RF_FLAG_WHITE_BKGD / RF_FLAG_RENDER_DIFFUSE are accepted and change nothing; only the
 * density element of a node is read (split / bricked: of its base record), never a feature.  Every density mode, layout, F and
 * num_samples >= 1.  Before any device access: RF_ERR_NULL_POINTER, RF_ERR_BAD_SHAPE (dims, num_samples < 1).  (Added to ABI
 * version 4 compatibly: no existing struct or signature changed.) */
int rf_node_max_weight(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float* max_weight_dev, void* stream);

/* Prune by that statistic: keep(n) iff some node m inside the grid with |m - n|_inf <= dilate has M[m] > threshold (strict:
 * threshold = 0 prunes exactly the nodes no sample ever weighted).  The raw density of a pruned node becomes min(D, fill_density)
 * under RF_DENSITY_RELU / SOFTPLUS / IDENTITY (pruning never raises a density) and 0 under RF_DENSITY_ABS (fill_density != 0 is
 * RF_ERR_BAD_SHAPE there).  densities_dev is the grid's own writable density / base tensor (strides and node order of `grid`);
 * kept nodes, every feature and the padding nodes of bricked storage keep their bits.  keep_dev (optional, [X, Y, Z] bytes, plain
 * node order) receives the mask; counts_dev (optional, 2 x int64) is ADDED to: (kept, pruned).  Gather form: one thread owns a
 * node, no atomics but the two counters.  RF_ERR_BAD_SHAPE: dilate outside [0, 4], a negative or non-finite threshold, a NaN fill;
 * RF_ERR_NULL_POINTER: grid, max_weight_dev, densities_dev.  (Added to ABI version 4 compatibly.) */
int rf_prune_grid(const RFGrid* grid, const float* max_weight_dev, float threshold, int32_t dilate, float fill_density,
                  float* densities_dev, uint8_t* keep_dev, int64_t* counts_dev, void* stream);

/* The content box of a field: node n PASSES iff its own activated density sigma_n = post(pre(D_n * density_scale)) > threshold
 * (strict; the helpers of the render under grid->density_mode, no interpolation: a node's value, not a sample's).  The call MERGES
 * into bounds_dev [6] (int32): bounds[a] = min(bounds[a], i_a) and bounds[3 + a] = max(bounds[3 + a], i_a) over the passing nodes
 * (i_a = the node's index on axis a), and ADDS their number to count_dev[0] (int64, optional).  The caller initialises bounds to
 * {X, Y, Z, -1, -1, -1}; a field without a passing node leaves all seven values untouched.  Several calls (several grids, or
 * thresholds) accumulate.  One thread per node; a wave without a passing node does nothing, any other reduces its six values
 * across the wave and issues six int32 atomic min / max and one 64-bit add: integer atomics, so the result does not depend on the
 * order of arrival -- exact and reproducible.  Every layout, F and density mode; only the density element of a node is read
 * (split / bricked: of its base record), never a feature, never a padding node of bricked storage.  Before any device access:
 * RF_ERR_NULL_POINTER (grid, its tensors, bounds_dev), RF_ERR_BAD_SHAPE (dims, a NaN or negative threshold).  (Added to ABI
 * version 4 compatibly: no existing struct or signature changed.) */
int rf_node_bounds(const RFGrid* grid, float threshold, int32_t* bounds_dev, int64_t* count_dev, void* stream);

/* A field moved into another box: crop, re-grid, refine.  scale / offset are HOST arrays of 3 floats.  Destination node
 * (i_x, i_y, i_z) of `dst` sits, on axis a, at the continuous source index   s_a = fmaf(scale_a, (float)i_a, offset_a).
 * If any s_a < -0.5 or s_a > n_a - 0.5 (n = src dims: nodes are voxel centres, so this is the source BOX) the node becomes
 * (density fill_density, every feature 0).  Otherwise s_a is clamped to [0, n_a - 1], i0 = min(floor(s), n - 1),
 * i1 = min(i0 + 1, n - 1), lambda = s - i0, and each of the F + 1 RAW channels (no density_scale, no activation: what a stage
 * transition resamples) is the trilinear sum of the 8 corners in a FIXED order: corner k = dx * 4 + dy * 2 + dz ascending with
 * weight w_k = (wx * wy) * wz (w = 1 - lambda for d = 0, lambda for d = 1), v = val_0 * w_0, then v = fmaf(val_k, w_k, v),
 * k = 1 .. 7.  Consequences: scale 1 with an integer offset makes every weight exactly 1 or 0 -- a bit-exact copy of the source
 * sub-volume for finite values (an exact crop); scale_a = n_src / n_dst with offset_a = 0.5 scale_a - 0.5 restates
 * F.interpolate(trilinear, align_corners=False), though not bit for bit (rf_upsample_grid keeps that job).  Any layout on either
 * side, same num_features, any dims >= 1; dst's tensors are overwritten (padding nodes of bricked storage are not touched), its
 * AABB / activation fields are not used.  One thread per (destination node, channel), values landing in the destination's layout.
 * Before any device access: RF_ERR_NULL_POINTER (grids, tensors, scale, offset), RF_ERR_BAD_SHAPE (dims, num_features mismatch, a
 * non-finite or non-positive scale, a non-finite offset, a NaN fill, a destination tensor that IS a source tensor).  (Added to ABI
 * version 4 compatibly: no existing struct or signature changed.) */
int rf_resample_grid(const RFGrid* src, const RFGrid* dst, const float* scale, const float* offset, float fill_density, void* stream);

/* Distortion loss of the rendered rays (mip-NeRF 360; DVGOv2's O(S) form): the regulariser that acts ALONG the ray and pulls its
 * compositing weights into one compact interval.  For every ray of the batch, with the samples i = 0 .. S-1 and the weights
 * w_i = T_i * alpha_i exactly as rf_render_forward computes them (same sampling, t_rand_dev / jitter key, first_ray / camera,
 * RF_FLAG_AABB_SAMPLING and RF_FLAG_OCCUPANCY_SKIP handling, last interval 1e10; w_i = 0 for samples outside the box),
 * s_i = (z_i - near) / (far - near) with the near / far of `rays` (the camera bounds, also under AABB sampling), and sample i
 * standing for the interval it composites over:
 *   i < S-1: d_i = s_{i+1} - s_i, m_i = (s_i + s_{i+1}) / 2;     i = S-1: d_i = 0, m_i = s_{S-1}   (the 1e10 interval has no width here)
 *   l = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i                                    (num_samples == 1: l = 0)
 * loss_dev (optional, [N]) is OVERWRITTEN with the unweighted l_r.  grad_first_dev (optional) follows the layout of `grid` like every
 * gradient buffer of this ABI (split / bricked: the base record, whose element 0 is the density) and is ADDED to with
 *   scale * grad_loss_dev[r] * d l_r / d D      (grad_loss_dev NULL: 1)
 * for the RAW density parameter D only (through the activation, density_scale, sign(D) under RF_DENSITY_ABS and the trilinear
 * weights, like the density lane of rf_render_backward): features do not enter, RF_FLAG_WHITE_BKGD / RF_FLAG_RENDER_DIFFUSE are
 * accepted and change nothing, and NO gradient goes to rays or poses.  Float atomics: the sum order is not fixed; l itself is
 * bitwise reproducible.  Only samples whose gradient is non-zero touch memory; padding nodes of bricked storage are never addressed.
 * Both outputs NULL, scale == 0 without loss_dev, or zero rays: nothing is launched, RF_OK.  The kernel needs no scratch memory for
 * any num_samples >= 1.  Before any device access: RF_ERR_NULL_POINTER (grid, its tensors, the rays' tensors, RF_FLAG_OCCUPANCY_SKIP
 * without a mask), RF_ERR_BAD_SHAPE (dims, num_samples < 1, far == near, non-finite near / far / scale, a gradient pointer that IS
 * the density tensor).  (Added to ABI version 4 compatibly: no existing struct or signature changed.) */
int rf_distortion(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float scale, const float* grad_loss_dev, float* loss_dev,
                  float* grad_first_dev, void* stream);

/* Surface normals and quantile depth of the rendered rays: the geometry of a field seen from a camera.  For every ray of the batch,
 * with the samples i = 0 .. S-1, their ray parameters z_i and the weights w_i = T_i * alpha_i exactly as rf_render_forward computes
 * them (same sampling, t_rand_dev / jitter key, first_ray / camera, RF_FLAG_AABB_SAMPLING and RF_FLAG_OCCUPANCY_SKIP handling, last
 * interval 1e10; w_i = 0 for samples outside the box):
 *   acc_dev [N]             sum_i w_i -- the bits of RFRenderOut.acc_dev of the per-ray forward kernel
 *   normal_dev [N,3]        sum_i w_i n_i in world space, NOT renormalised (its length is at most acc).  n_i = -g_i / |g_i|, and 0 where
 *                           g_i = 0: g_i is the gradient with respect to the point of the trilinearly interpolated PRE-activation
 *                           density (D * density_scale, |.| of it under RF_DENSITY_ABS; nodes outside the grid count as 0) at sample i,
 *                           g_a = d pre / d idx_a * dims_a * norm_scale_a / 2.  The activation's slope is a positive scalar and does
 *                           not enter; the sign convention is that of rf_mesh_emit's normals (out of the dense side).  A sample with
 *                           w_i == 0 contributes nothing.
 *   quantile_depth_dev [N]  z_i of the first sample with 1 - T_{i+1} >= quantile (the opacity accumulated through sample i; the same
 *                           un-normalised ray parameter RFRenderOut.depth_dev sums), 0 if no sample reaches it.  quantile = 0.5: the
 *                           median depth.
 * Each output may be NULL (not all three).  One wave per ray, one result per ray, no atomics: bitwise reproducible.
 * RF_FLAG_WHITE_BKGD / RF_FLAG_RENDER_DIFFUSE are accepted and change nothing; only the density element of a node is read (split /
 * bricked: of its base record), never a feature.  Every density mode, layout, F and num_samples >= 1.  Zero rays: nothing is launched,
 * RF_OK.  Before any device access: RF_ERR_NULL_POINTER (grid, its tensors, rays, their tensors, out, three NULL outputs,
 * RF_FLAG_OCCUPANCY_SKIP without a mask), RF_ERR_BAD_SHAPE (dims, num_samples < 1, quantile outside (0, 1) or not finite),
 * RF_ERR_UNSUPPORTED (num_features, density_mode).  (Added to ABI version 4 compatibly: no existing struct or signature changed;
 * rf_abi_struct_size(10) is sizeof(RFGeometryOut).) */
typedef struct RFGeometryOut {
  float* normal_dev;          /* [N,3] sum_i w_i n_i, world space, NOT renormalised; may be NULL */
  float* quantile_depth_dev;  /* [N]   see above; may be NULL                                     */
  float* acc_dev;             /* [N]   sum_i w_i; may be NULL                                     */
} RFGeometryOut;
int rf_render_geometry(const RFGrid* grid, const RFRayBatch* rays, uint32_t flags, float quantile, const RFGeometryOut* out, void* stream);

/* Iso-surface extraction (csrc/mesh_kernels.hip; the contract -- field, lattice, Kuhn tetrahedra, edge keys, orientation and
 * canonical order -- is in that file's header and in DESIGN.md).  The level set sigma = iso_level of the grid's density on the
 * lattice of `subdivisions` (1..8) points per voxel and axis plus one guard plane on each AABB face, as a closed oriented mesh.
 * Three steps: rf_mesh_tiles (host only) gives the number of tiles nt of the lattice; rf_mesh_count writes the vertex counts
 * of the tiles to counts_dev[0 : nt] and their triangle counts to counts_dev[nt : 2 nt] (int64); the caller turns both rows into
 * exclusive prefix sums (offsets_dev, same shape) and allocates V = sum of row 0 vertices, T = sum of row 1 triangles;
 * rf_mesh_emit writes, in canonical order, edge_keys_dev [V] (int64, ascending), positions_dev [V,3], colours_dev [V,3] and
 * normals_dev [V,3] (both optional: NULL skips them) and face_edges_dev [T,3] (the edge keys of each triangle's vertices: their
 * positions in edge_keys_dev are the vertex indices).  Only the density and the three degree-0 coefficients are read.
 * RF_ERR_NULL_POINTER / RF_ERR_BAD_SHAPE (dims, subdivisions outside [1, 8], a non-finite iso_level) before any device access;
 * rf_mesh_tiles returns the code instead of a count.  (Added to ABI version 4 compatibly: no existing struct or signature
 * changed.) */
int64_t rf_mesh_tiles(const RFGrid* grid, int32_t subdivisions);
int rf_mesh_count(const RFGrid* grid, int32_t subdivisions, float iso_level, int64_t* counts_dev, void* stream);
int rf_mesh_emit(const RFGrid* grid, int32_t subdivisions, float iso_level, const int64_t* offsets_dev, int64_t num_vertices,
                 int64_t num_faces, int64_t* edge_keys_dev, float* positions_dev, float* colours_dev, float* normals_dev,
                 int64_t* face_edges_dev, void* stream);

/* ---- image metrics (csrc/image_kernels.hip) ------------------------------------------------------------------------------
 * SSIM (Wang et al. 2004) of two float32 images of data range 1, per colour channel, and its adjoint -- the structural metric
 * beside PSNR in held-out evaluation, and the D-SSIM term of full-frame losses (pose refinement).  The contract:
 *   window   Gaussian, 11 x 11, sigma = 1.5, separable: g_k ~ exp(-(k - 5)^2 / (2 * 1.5^2)), normalised to sum 1;
 *   moments  mu_x = G*x, mu_y = G*y, s_xx = G*x^2 - mu_x^2, s_yy = G*y^2 - mu_y^2, s_xy = G*xy - mu_x mu_y.  Variances are NOT
 *            clamped (the form of pytorch-msssim and of 3DGS; jaxnerf's clamps are not applied);
 *   S        = (A1 * A2) / (B1 * B2) with A1 = 2 mu_x mu_y + C1, A2 = 2 s_xy + C2, B1 = mu_x^2 + mu_y^2 + C1,
 *            B2 = s_xx + s_yy + C2, C1 = 0.01^2, C2 = 0.03^2, in exactly this association: the SSIM of an image with itself is
 *            exactly 1.0 in float32;
 *   padding  RF_SSIM_VALID (what the NeRF literature's numbers use): only windows inside the image, map [H - 10, W - 10, C], H and
 *            W at least 11.  RF_SSIM_SAME (the D-SSIM convention of 3DGS): the image zero-padded by 5, map [H, W, C], any H, W >= 1;
 *   result   the mean of the map over pixels and channels.
 * An image is addressed by ELEMENT strides (RFImage): a contiguous [H, W, C] tensor, a [C, H, W] tensor seen as [H, W, C], and a
 * crop of a larger frame all go in without a copy, and all give the same bits for the same values.
 *
 * rf_ssim_tiles (host only): the number of workgroups of the forward launch = the length of partials_dev; a negative RF_ERR_* code
 *   for shapes rf_ssim_forward refuses.
 * rf_ssim_forward: two launches.  One workgroup per (16 x 32 map tile, channel) stages both images' tile and halo in LDS, filters
 *   along the rows and then down the columns, and writes its float32 partial sum to partials_dev [rf_ssim_tiles]; one workgroup
 *   then adds the partials in float64 and writes the mean to mean_dev [1].  Every sum has a fixed order and there are no atomics:
 *   the result is bitwise reproducible.  Optional outputs, PLANAR: map_dev [C, Hm, Wm] (the map), dmaps_dev [3, C, Hm, Wm] (what the
 *   adjoint reads: the total dS / d mu_x, dS / d s_xx, dS / d s_xy); NULL: not written.
 * rf_ssim_backward: the gradient of the mean with respect to `image`, dL/dx_p = (g / N) [ (G*d_mu)_p + 2 x_p (G*d_sxx)_p +
 *   y_p (G*d_sxy)_p ] (the derivative maps count as 0 outside the map's extent), gathered per pixel -- no atomics, reproducible --
 *   and WRITTEN to grad_image (any strides of its own).  g = grad_mean_dev[0] is read by the kernel: no host synchronisation.
 * Before any device access: RF_ERR_NULL_POINTER (an image struct, its data pointer, partials_dev / mean_dev, dmaps_dev /
 * grad_mean_dev of the adjoint), RF_ERR_BAD_SHAPE (height, width or channels < 1, a zero stride, RF_SSIM_VALID below 11 x 11),
 * RF_ERR_UNSUPPORTED (an unknown padding).  Every accepted shape holds at least one window: there is no zero-sized call.  (Added
 * to ABI version 4 compatibly: no existing struct or signature changed; rf_abi_struct_size(11) is sizeof(RFImage).) */
enum { RF_SSIM_VALID = 0, RF_SSIM_SAME = 1 };
typedef struct RFImage {
  float* data_dev;                      /* element (0, 0, 0)                               */
  int64_t stride_h, stride_w, stride_c; /* floats between rows, columns, channels; non-zero */
} RFImage;
int64_t rf_ssim_tiles(int32_t height, int32_t width, int32_t channels, int32_t padding);
int rf_ssim_forward(const RFImage* image, const RFImage* target, int32_t height, int32_t width, int32_t channels, int32_t padding,
                    float* map_dev, float* dmaps_dev, float* partials_dev, float* mean_dev, void* stream);
int rf_ssim_backward(const RFImage* image, const RFImage* target, int32_t height, int32_t width, int32_t channels, int32_t padding,
                     const float* dmaps_dev, const float* grad_mean_dev, const RFImage* grad_image, void* stream);

/* ---- vector quantisation (csrc/vq_kernels.hip) ---------------------------------------------------------------------------
 * The two halves of an importance-weighted Lloyd iteration over feature vectors: what compresses a trained field (VQRF, Li et al.
 * 2023; thr3ed_atom_amd/compression.py).  Sizes: 1 <= dim <= 64, 1 <= num_codes <= 65536.
 *
 * rf_vq_assign: for every row x of vectors_dev [num_vectors, dim] (float32, rows row_stride >= dim floats apart) the index of the
 *   nearest row of codebook_dev [num_codes, dim] (float32, contiguous) by squared Euclidean distance -> index_out_dev [num_vectors],
 *   and that distance -> dist_out_dev [num_vectors].  Codes are RANKED by s = ||c||^2 - 2 x.c, one k-ordered float32 fma chain per
 *   pair on the exact-f32 MFMA starting from ||c||^2 (float64 sum, rounded once): every ranked value is within
 *   (dim + 1) u (||c||^2 + 2 sum_k |x_k c_k|), u = 2^-24, of the true one.  Among computed-equal values the LOWEST index wins; the
 *   same inputs give the same bits; the distances are never stored and there are no atomics.  dist_out is not the ranked value: it
 *   is sum_k (x_k - c_jk)^2 of the winner j recomputed in ascending k in float32 without contraction -- within (dim + 2) u,
 *   relative, of the true distance to the returned code.  num_vectors == 0 is a no-op that returns RF_OK.
 * rf_vq_centroids: the weighted Lloyd update in gather form.  order_dev [num_vectors] (int32) lists the vector indices sorted by
 *   assigned code, offsets_dev [num_codes + 1] (int64) bounds the segment of every code in it.  A code with a non-empty segment and a
 *   positive weight sum gets codebook_inout_dev[c] = sum w x / sum w over its segment; any other code keeps its bits.
 *   weight_sum_out_dev [num_codes] (optional, NULL: not written) receives every code's weight sum (0 for an empty segment).  The order
 *   of every sum is fixed by the segment alone (16 interleaved sequential streams, then a fixed tree): no atomics, reproducible bits.
 *   The entries of order_dev must be valid row indices: the caller answers for that.
 * Before any launch: RF_ERR_NULL_POINTER (any array but the optional one; rf_vq_assign with num_vectors == 0 needs the codebook
 * only), RF_ERR_UNSUPPORTED (dim or num_codes out of range), RF_ERR_BAD_SHAPE (num_vectors < 0, row_stride < dim, more than 2^31 - 1
 * workgroups, an output that is another argument's array).  (Added to ABI version 4 compatibly: no struct or signature changed.) */
int rf_vq_assign(const float* vectors_dev, int64_t num_vectors, int32_t dim, int64_t row_stride, const float* codebook_dev, int32_t num_codes,
                 int32_t* index_out_dev, float* dist_out_dev, void* stream);
int rf_vq_centroids(const float* vectors_dev, int64_t row_stride, int32_t dim, const float* weights_dev, const int32_t* order_dev,
                    const int64_t* offsets_dev, int32_t num_codes, float* codebook_inout_dev, float* weight_sum_out_dev, void* stream);

/* ---- connected components (csrc/component_kernels.hip) ---------------------------------------------------------------------
 * Labels the connected components of the OCCUPIED nodes of a field: what floater removal is built on
 * (thr3ed_atom_amd/components.py).  Node n is occupied iff its own activated density
 * sigma_n = post(pre(D_n * density_scale)) > threshold -- the predicate of rf_node_bounds bit for bit (strict; |.| on the
 * pre-activation under RF_DENSITY_ABS; no interpolation; only the node's density element is read, never a padding node of bricked
 * storage).  connectivity 6 / 18 / 26: face, face + edge, face + edge + corner neighbours on the node lattice.
 *   labels_dev [X, Y, Z] (int32, plain node order whatever the layout): -1 for an unoccupied node, otherwise the SMALLEST plain
 *     linear index (x * Y + y) * Z + z of any node of the same component.  Canonical: independent of launch order, storage and run;
 *     two calls give identical bits.  Every element is written.
 *   sizes_dev [X * Y * Z] (int32, optional): sizes[r] = the number of nodes of the component labelled r, 0 everywhere else.  Every
 *     element is written (no pre-zeroing).
 * Three launches on `stream` (per-tile labelling in LDS, a lock-free union of the tiles' trees with integer atomicMin, flatten +
 * count), no host synchronisation, no scratch beyond the two outputs; no kernel waits for another workgroup.  Before any device
 * access: RF_ERR_NULL_POINTER (grid, its tensors, labels_dev), RF_ERR_BAD_SHAPE (dims, a NaN or negative threshold, a connectivity
 * other than 6 / 18 / 26, more than 2^31 - 1 nodes, sizes_dev == labels_dev).  (Added to ABI version 4 compatibly: no existing
 * struct or signature changed.) */
int rf_label_components(const RFGrid* grid, float threshold, int32_t connectivity, int32_t* labels_dev, int32_t* sizes_dev, void* stream);

/* ---- mesh simplification by vertex clustering with quadric-error representatives (csrc/mesh_simplify_kernels.hip; DESIGN.md
 * section 20; thr3ed_atom_amd/mesh_simplify.py sorts, builds the lists and rewrites the faces between the two calls) ----------
 * A uniform lattice of cubic cells of edge h = cell size starts at `origin` (HOST float[3]); `cells` (HOST int32[3]) is the number
 * n_a of cells per axis, each in [1, 2^20].  Any indexed triangle mesh: vertices_dev [V, 3] float32, faces_dev [T, 3] int64.
 * rf_mesh_cluster_keys: keys_dev[v] = (k_x n_y + k_y) n_z + k_z with k_a = floor(fl32(fl32(v_a - origin_a) * r)), r = fl32(1 / h)
 *   computed by the caller (two rounded float32 operations: the library is built without contraction).  A vertex with a k_a outside
 *   [0, n_a) -- below the origin, beyond the cells, NaN, infinite -- gets the key -1 and sets status_dev[0] (int32, zeroed by the
 *   caller) to 1 in the same pass.  One pointwise launch.
 * rf_mesh_cluster_vertices: the representative of every cluster, ONE launch, gather form, no atomics, float64 accumulators, every
 *   sum in an order fixed by the lists alone (two calls give identical bits).  cluster_keys_dev [C] are the distinct keys, ascending;
 *   members_dev [V] the vertex indices stably sorted by cluster and corners_dev [3 T] the corner ids 3 f + j stably sorted by the
 *   cluster of vertex faces[f][j], with member_begin_dev / corner_begin_dev [C + 1] bounding the segment of every cluster (all
 *   int64).  In coordinates local to the centre m of the cluster's cell, q = p - m in float64: every corner record adds its face's
 *   n = (q1 - q0) x (q2 - q0), d = n . q0 as A += n n^T, b += d n; xbar = the mean of the members.  placement
 *   RF_MESH_PLACEMENT_MEAN, or tr A == 0: x = xbar.  RF_MESH_PLACEMENT_QUADRIC: x = xbar + (A + regularisation tr(A) I)^-1
 *   (b - A xbar), clamped per axis to [-h/2, h/2].  vertices_out_dev [C, 3] = float32(m + x); colours_out_dev [C, 3] = the mean of the
 *   members' colours; normals_out_dev [C, 3] = the members' normal sum over its norm ((0,0,0) where the sum is 0).  colours / normals
 *   are optional: input and output are both given or both NULL.  Indices read from the lists are checked against their arrays.
 * Before any launch, in this order: RF_ERR_NULL_POINTER (any array but the optional pairs; an optional pair given by halves), then
 * RF_ERR_BAD_SHAPE for negative counts, num_vertices >= 2^31 (num_clusters > num_vertices, num_faces >= 2^40), h or r (or 1 / h) not
 * finite or <= 0, a non-finite origin, a cell count outside [1, 2^20], a placement other than the two, a regularisation outside
 * [1e-6, 1]; then zero vertices / zero clusters return RF_OK without a launch.  (Added to ABI version 4 compatibly: no existing
 * struct or signature changed.) */
enum { RF_MESH_PLACEMENT_QUADRIC = 0, RF_MESH_PLACEMENT_MEAN = 1 };
int rf_mesh_cluster_keys(const float* vertices_dev, int64_t num_vertices, const float* origin, float r, const int32_t* cells, int64_t* keys_dev,
                         int32_t* status_dev, void* stream);
int rf_mesh_cluster_vertices(const float* vertices_dev, const float* colours_dev, const float* normals_dev, int64_t num_vertices,
                             const int64_t* faces_dev, int64_t num_faces, const int64_t* members_dev, const int64_t* member_begin_dev,
                             const int64_t* corners_dev, const int64_t* corner_begin_dev, const int64_t* cluster_keys_dev, int64_t num_clusters,
                             const float* origin, float h, const int32_t* cells, int32_t placement, float regularisation,
                             float* vertices_out_dev, float* colours_out_dev, float* normals_out_dev, void* stream);

/* ---- texture baking of a field onto a triangle mesh (csrc/texture_kernels.hip; thr3ed_atom_amd/texture.py
 * lays the atlas out, computes the UVs and writes the OBJ / MTL / PNG) -------------------------------------------------------------
 * Any indexed triangle mesh: vertices_dev [V, 3] float32, faces_dev [T, 3] int64.  The atlas is a uniform per-triangle one: blocks
 * of B = patch + 4 texels square, `cols` x `rows` of them, block b at column (b % cols) B and row (b / cols) B of the image, holding
 * triangle 2 b (lower) and 2 b + 1 (upper).  Texel (i, j) of a block (i the column, j the row, centre at (i, j)) belongs to the lower
 * triangle when i + j <= patch + 3, else to the upper one; a triangle index >= num_faces leaves it UNOWNED.  The corners (v0, v1, v2)
 * sit at (1, 1), (P, 1), (1, P) (lower) and (P + 2, P + 2), (3, P + 2), (P + 2, 3) (upper); with (a, b) the texel centre minus corner 0
 * along the patch's legs, beta1 = a / (P - 1), beta2 = b / (P - 1), beta0 = 1 - beta1 - beta2, the texel's point is
 * p = beta0 v0 + beta1 v1 + beta2 v2 (owned texels outside the triangle: the same affine map).
 *   n = the unit normal (v1 - v0) x (v2 - v0), (0, 0, 0) for a zero-area triangle; D = 2 reach / samples; for s = 0 .. samples - 1
 *   q_s = p + (reach - (s + 1/2) D) n; sigma_s = the renderer's activated density at q_s (grid's density_mode and density_scale; 0 on
 *   or outside the AABB, strict test); alpha_s = 1 - exp(-sigma_s D); w_s = alpha_s prod_{r<s} (1 - alpha_r);
 *   c(x) = sigmoid(sum_k Y_k(-n) f_k(x)) per colour on the features interpolated as rf_grid_query does (zero padding, no AABB test);
 *   under RF_FLAG_RENDER_DIFFUSE c(x) = sigmoid(C0 f_0(x)) and split / bricked storage is read in its base record only.
 *   texture_dev [rows B, cols B, 3] = sum_s w_s c(q_s) + (1 - sum_s w_s) c(p);  opacity_dev [rows B, cols B] (optional) = sum_s w_s.
 *   Unowned texels are 0 in both images.  reach == 0 gives exactly c(p).
 * ONE launch writes every texel of both images (no memset needed), one lane per texel, no atomics: two calls give identical bits.
 * Every storage layout, density mode and SH degree 0-3.  A face index outside [0, num_vertices) sets status_dev[0] (int32, zeroed by
 * the caller) to 1 and its texels to 0; it is never dereferenced.  Before any launch, in this order: RF_ERR_NULL_POINTER (grid, its
 * tensors, texture_dev, status_dev, vertices_dev / faces_dev with a non-zero count), RF_ERR_BAD_SHAPE (grid dims, negative counts,
 * patch outside [2, 64], samples outside [1, 256], a negative or non-finite reach, cols or rows < 1, an image edge above 16384,
 * 2 cols rows < num_faces), RF_ERR_UNSUPPORTED (num_features, density_mode, layout, a flag bit other than RF_FLAG_RENDER_DIFFUSE).
 * num_faces == 0 with a valid shape still clears the images.  (Added to ABI version 4 compatibly: no existing struct or signature
 * changed.) */
int rf_texture_bake(const RFGrid* grid, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch,
                    int32_t cols, int32_t rows, float reach, int32_t samples, uint32_t flags, float* texture_dev, float* opacity_dev, int32_t* status_dev,
                    void* stream);

/* ---- a rasteriser for triangle meshes (csrc/mesh_raster_kernels.hip; thr3ed_atom_amd/mesh_raster.py allocates
 * the buffers and compares the result with the field's own render) ------------------------------------------------------------------
 * Any indexed triangle mesh: vertices_dev [V, 3] float32, faces_dev [T, 3] int64; `camera` a HOST RFCamera.  Pixel (i, j) has the ray
 * of rf_cast_rays, the same float32 operations in the same order: o = t, d = R ((j + 1/2 - W/2) / f, -(i + 1/2 - H/2) / f, -1).  With
 * p_k = v_k - o: e0 = d . (p1 x p2), e1 = d . (p2 x p0), e2 = d . (p0 x p1), every cross product evaluated from the lower to the higher
 * vertex index of its edge and negated when the face runs the other way, so that two faces sharing an edge see e and -e bit for bit
 * (the library is built with -ffp-contract=off).  s = (e0 + e1) + e2.
 *   The ray HITS the face when all e_k >= 0 or all e_k <= 0, and s != 0: edges are inclusive, zero-area and edge-on faces are never
 *   drawn.  With (v1 - v0) x (v2 - v0) pointing out of the solid (the orientation of extract_mesh) a face seen from outside has
 *   s < 0; under RF_RASTER_CULL_BACKFACES only s < 0 counts.  w_k = e_k / s.  z_k = the camera depth of corner k = -(p_k . R[:, 2]);
 *   z = z0 + (w1 (z1 - z0) + w2 (z2 - z0)), the ray parameter of the hit (what RenderOut.depth holds).  A face with any z_k < near is
 *   not drawn at all (not clipped).  A hit whose z is negative or not finite is no hit.
 * rf_mesh_raster_visibility: visibility_dev [H, W] uint64, set to all ones by the CALLER (all ones = no hit); every hit does a
 *   device-scope 64-bit atomic minimum of float_bits(z) << 32 | face.  The minimum does not depend on the order of arrival and the
 *   lower face index wins exact depth ties: two calls give identical bits.  One lane per face; a face whose conservative pixel box
 *   is at most 8 x 8 pixels is walked by its lane, larger boxes by the whole wavefront in 8 x 8 blocks.  A face index outside
 *   [0, num_vertices) sets status_dev[0] (int32, zeroed by the caller) to 1 and the face is skipped; it is never dereferenced.
 *   num_faces == 0 returns RF_OK without a launch.
 * rf_mesh_raster_shade: one lane per pixel, no atomics.  depth_dev [H, W] = z, face_ids_dev [H, W] int32 = the face (0 and -1 where
 *   nothing was hit), barycentrics_dev [H, W, 3] (optional) = w (0 where nothing was hit), re-evaluated by the same code as the
 *   visibility pass (the same bits).  colour_dev [H, W, 3] (optional): with uvs_dev [T, 3, 2] and texture_dev [H_t, W_t, 3] (both or
 *   neither; image row 0 on top, v = 1 there) the bilinear fetch at texel coordinates (u W_t - 1/2, (1 - v) H_t - 1/2) of the
 *   interpolated (u, v) = sum_k w_k uv_k, taps clamped to the image; else sum_k w_k colours_dev[v_k] (colours_dev [V, 3]).  The texture
 *   wins when both are given.  Pixels without a hit get 0, or 1 under RF_FLAG_WHITE_BKGD.  Both calls take the same camera, mesh and
 *   flag word.  (rf_mesh_raster_taps, further down, records the four taps and two fractions of this fetch per pixel instead of
 *   fetching through them: the same device code up to the fetch.)
 * Before any launch, in this order: RF_ERR_NULL_POINTER (camera, visibility_dev, status_dev / depth_dev, face_ids_dev, vertices_dev /
 * faces_dev with a non-zero count, uvs_dev and texture_dev given by halves, colour_dev without a texture or colours_dev);
 * RF_ERR_BAD_SHAPE (negative counts, num_faces >= 2^31, an image edge outside [1, 16384], a focal that is not finite or <= 0, a pose
 * that is not finite, a near that is not finite or < 0, a texture edge outside [1, 16384]); RF_ERR_UNSUPPORTED (a flag bit other than
 * RF_FLAG_WHITE_BKGD and RF_RASTER_CULL_BACKFACES).  (Added to ABI version 4 compatibly: no existing struct or signature changed.) */
enum { RF_RASTER_CULL_BACKFACES = 32 };
int rf_mesh_raster_visibility(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                              float near, uint32_t flags, uint64_t* visibility_dev, int32_t* status_dev, void* stream);
int rf_mesh_raster_shade(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                         const uint64_t* visibility_dev, const float* uvs_dev, const float* texture_dev, int32_t texture_height, int32_t texture_width,
                         const float* colours_dev, uint32_t flags, float* colour_dev, float* depth_dev, int32_t* face_ids_dev, float* barycentrics_dev,
                         void* stream);

/* ---- texture baking from posed views (csrc/texture_views_kernels.hip; thr3ed_atom_amd/texture.py chunks the
 * views, runs rf_mesh_raster_visibility per view and finalises) ---------------------------------------------------------------------
 * The mesh and the atlas (patch, cols, rows) are those of rf_texture_bake: the same texel -> face -> point p and unit normal n, bit
 * for bit (n = 0 for a zero-area face, which no view ever counts).  `cameras` is a HOST array of num_views (0 .. 16) RFCamera of one
 * height H and width W (focals and poses are free); images_dev [n, H, W, 3] float32; visibility_dev [n, H, W] uint64, exactly what
 * rf_mesh_raster_visibility writes per view; alphas_dev [n, H, W] float32 or NULL.  accum_dev [rows B, cols B, 4] float32 (three colour
 * sums and one weight sum) and the optional count_dev [rows B, cols B] int32 are IN/OUT.  Per owned texel, for each view k in order:
 *   1. c = R_k^T (p - t_k), z = -c_z; rejected unless z is finite and z > near.
 *   2. x = W/2 + f c_x / z, y = H/2 - f c_y / z (the inverse of the ray of rf_cast_rays: pixel (i, j) has its centre at (j + 1/2, i + 1/2));
 *      rejected unless 0 <= x < W and 0 <= y < H; j = floor(x), i = floor(y).
 *   3. key = visibility[k, i, j]; rejected when it is all ones; z_buf = the float in its high 32 bits; rejected unless
 *      z <= z_buf + depth_bias (a shadow-map test with a bias; the face id in the low word is not used).
 *   4. cos = n . (t_k - p) / |t_k - p|, |cos| under RF_TEXTURE_VIEWS_TWO_SIDED; rejected unless cos > min_cos; omega = cos^cos_power by
 *      repeated multiplication (power 0 gives exactly 1).
 *   5. C = the bilinear fetch of image k at (x - 1/2, y - 1/2), taps clamped to the image; m = the same fetch of the alpha plane, or 1.
 *   6. accum.rgb += omega m (C - (1 - m) background), accum.w += omega m m, count += 1: the sums of the least-squares texel
 *      sum omega m (C - (1 - m) background) / sum omega m^2 of pixels read as C = m c + (1 - m) background.
 * One launch, one lane per texel, no atomics: the lane loads its accumulator words, adds its views in order and stores them, so two
 * calls give identical bits and successive calls over chunks of views do the float additions of one long loop.  Unowned texels are
 * not touched.  A face index outside [0, num_vertices) sets status_dev[0] (int32, zeroed by the caller) to 1 and leaves the face's
 * texels as they were; it is never dereferenced.  Before any launch, in this order: RF_ERR_NULL_POINTER (accum_dev, status_dev,
 * vertices_dev / faces_dev with a non-zero count, cameras / images_dev / visibility_dev with num_views > 0), RF_ERR_BAD_SHAPE (negative
 * counts, num_views > 16, patch outside [2, 64], cols or rows < 1, an atlas or image edge outside [1, 16384], 2 cols rows < num_faces,
 * views of unequal size, a focal that is not finite or <= 0, a pose that is not finite, near / depth_bias / background not finite or
 * negative, min_cos outside [0, 1), cos_power outside [0, 8]), RF_ERR_UNSUPPORTED (a flag bit other than RF_TEXTURE_VIEWS_TWO_SIDED).
 * num_views == 0 or num_faces == 0 returns RF_OK without a launch.  (Added to ABI version 4 compatibly: no existing struct or
 * signature changed.) */
enum { RF_TEXTURE_VIEWS_TWO_SIDED = 64 };
int rf_texture_project_views(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, int32_t patch, int32_t cols,
                             int32_t rows, int32_t num_views, const RFCamera* cameras, const float* images_dev, const uint64_t* visibility_dev,
                             const float* alphas_dev, float near, float depth_bias, float min_cos, int32_t cos_power, float background, uint32_t flags,
                             float* accum_dev, int32_t* count_dev, int32_t* status_dev, void* stream);

/* ---- texture gradients of the mesh render (csrc/mesh_raster_kernels.hip and csrc/texture_fit_kernels.hip; DESIGN.md section 24;
 * thr3ed_atom_amd/texture_fit.py builds the transposed tap list and runs the optimiser) ----------------------------------------------
 * With mesh, UVs and cameras fixed the colour image of rf_mesh_raster_shade is a sparse linear map of the texture: four bilinear taps
 * per hit pixel.  RFTextureTap is one pixel's row of it: the tap columns x0, x1 and rows y0, y1 (already clamped to the texture) and
 * the fractions fx, fy; x0 == 0xFFFF marks a pixel without a hit (texture edges are at most 16384).
 * rf_mesh_raster_taps: one lane per pixel over the visibility buffer rf_mesh_raster_visibility filled, with the camera, mesh and flag
 *   word of that call.  taps_dev [H, W] holds exactly what rf_mesh_raster_shade computes before its fetch (both kernels call the same
 *   two device functions), for the pixels it would give a face id >= 0; the others get x0 = x1 = y0 = y1 = 0xFFFF, fx = fy = 0.
 *   Before any launch: RF_ERR_NULL_POINTER (camera, visibility_dev, taps_dev, vertices_dev / faces_dev / uvs_dev with a non-zero
 *   count), RF_ERR_BAD_SHAPE (as rf_mesh_raster_shade; a texture edge outside [1, 16384]), RF_ERR_UNSUPPORTED (a flag bit other than
 *   RF_FLAG_WHITE_BKGD and RF_RASTER_CULL_BACKFACES).
 * rf_texture_sample: colour_dev [P, 3] from taps_dev [P] (the records of any number of views, P < 2^31) and texture_dev [H_t, W_t, 3]:
 *   top = (1 - fx) T[y0, x0] + fx T[y0, x1], bot = (1 - fx) T[y1, x0] + fx T[y1, x1], colour = (1 - fy) top + fy bot -- the operations
 *   of rf_mesh_raster_shade in its order, so the colours are its colours bit for bit -- and `background` where x0 == 0xFFFF.  A tap
 *   outside the texture sets status_dev[0] (int32, zeroed by the caller) to 1 and gives the background; it is never dereferenced.
 *   One lane per pixel, a pure gather.
 * rf_texture_sample_backward: grad_texture_dev [H_t W_t, 3] = the transposed map applied to grad_colour_dev [P, 3], in gather form:
 *   offsets_dev [H_t W_t + 1] int64 (ascending, offsets[0] = 0, offsets[H_t W_t] = num_entries) delimits every texel's segment of
 *   entries_dev [num_entries] RFTextureTapEntry (pixel, weight), sorted by texel, ties in ascending pixel order.  Texel k gets
 *   sum_e weight_e grad_colour[pixel_e] over its segment in float32 -- 0 for an empty one: EVERY texel is written, the caller clears
 *   nothing.  A segment of at most `long_segment` entries (0: the library's default, 16) is summed by its own lane in entry order; a
 *   longer one by the whole wavefront: lane l sums entries l, l + 64, ... in entry order, then the 64 partial sums are combined by
 *   the fixed tree x_l += x_(l + 32), (l + 16), ..., (l + 1).  No atomics; the order of the additions depends on the entry list and
 *   long_segment alone, so two calls give identical bits.  An entry whose pixel lies outside [0, P) sets status_dev[0] to 1 and is
 *   skipped; it is never dereferenced.
 * Before any launch, in this order: RF_ERR_NULL_POINTER (texture_dev / colour_dev / taps_dev, offsets_dev / grad_texture_dev /
 * status_dev, grad_colour_dev / entries_dev with a non-zero count), RF_ERR_BAD_SHAPE (P < 0 or >= 2^31, a texture edge outside
 * [1, 16384], a background that is not finite or negative, num_entries < 0 or >= 2^33, long_segment < 0), RF_ERR_UNSUPPORTED (any flag
 * bit: none is defined).  P == 0 returns RF_OK from rf_texture_sample without a launch.  (Added to ABI version 4 compatibly: no
 * existing struct or signature changed.) */
typedef struct RFTextureTap {
  uint16_t x0, x1, y0, y1;
  float fx, fy;
} RFTextureTap; /* 16 bytes */
typedef struct RFTextureTapEntry {
  int32_t pixel;
  float weight;
} RFTextureTapEntry; /* 8 bytes */
/* (taps_dev and entries_dev are device arrays of the two records above, passed untyped like every device array of records) */
int rf_mesh_raster_taps(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                        const uint64_t* visibility_dev, const float* uvs_dev, int32_t texture_height, int32_t texture_width, uint32_t flags,
                        void* taps_dev, void* stream);
int rf_texture_sample(const void* taps_dev, int64_t num_pixels, const float* texture_dev, int32_t texture_height, int32_t texture_width,
                      float background, uint32_t flags, float* colour_dev, int32_t* status_dev, void* stream);
int rf_texture_sample_backward(const float* grad_colour_dev, int64_t num_pixels, const int64_t* offsets_dev, const void* entries_dev,
                               int64_t num_entries, int32_t texture_height, int32_t texture_width, int32_t long_segment, uint32_t flags,
                               float* grad_texture_dev, int32_t* status_dev, void* stream);

/* ---- geometry gradients of the mesh render (csrc/mesh_fit_kernels.hip over the rasteriser's device functions in
 * csrc/mesh_raster.h; DESIGN.md section 25;
 * thr3ed_atom_amd/mesh_fit.py sorts the hit pixels, builds the corner lists and runs the optimiser) -------------------------------
 * Two images per view that are differentiable with respect to vertices_dev, in the rasteriser's own quantities (d, p_k = v_k - o,
 * e_k, s, w_k = e_k / s, z as defined above, computed by the device functions the visibility and shade kernels call):
 *   DEPTH     D[i, j] = z of the winning face at hit pixels, 0 elsewhere: the bits of rf_mesh_raster_shade.  At a hit pixel with
 *             winning face (v0, v1, v2): dz/dv_k = w_k n / s with n = (v1 - v0) x (v2 - v0).  (Moving corner k by delta moves the
 *             face's plane; its hit moves along the ray by w_k (n . delta) / (n . d), n . d = s, and d has camera-z -1, so the ray
 *             parameter is the camera depth.)
 *   COVERAGE  A[i, j] in [0, 1]: the edge-crossing anti-aliasing of nvdiffrast restricted to pairs of a HIT pixel a (winning face F)
 *             and a 4-neighbour b inside the image that is a MISS.  F's edge values at both centres, sigma = sign(s(a)); for every k
 *             with sigma e_k(b) < 0: tau_k = e_k(a) / (e_k(a) - e_k(b)); tau = min_k tau_k (the lowest k on ties) clamped to
 *             [0, 1] -- where F's silhouette crosses the segment, measured from a's centre.  No such k (F covers b's centre but was
 *             rejected there, by `near` for example): the pair contributes nothing.  b gains max(tau - 1/2, 0), a loses
 *             max(1/2 - tau, 0).  Miss pixel: A = min(1, sum over its hit neighbours of the gains); hit pixel: A = max(0, 1 - sum
 *             over its miss neighbours of the losses); float32 sums in the order left, right, up, down; pixels outside the image
 *             are no neighbours.  Hit and miss are the visibility buffer's, so `near` and culling act through it.
 * rf_mesh_raster_coverage: one lane per pixel over the visibility buffer rf_mesh_raster_visibility filled, with that call's camera,
 *   mesh and cull flag; writes depth_dev, coverage_dev [H, W] float32 and face_ids_dev [H, W] int32 (-1: miss).  No atomics.
 * rf_mesh_geometry_backward_pixels: one lane per pixel of ONE view, given the face_ids_dev and coverage_dev the forward wrote and the
 *   upstream grad_depth_dev, grad_coverage_dev [H, W].  A hit pixel writes records_dev[pixel] = 9 floats, the gradient on the three
 *   corners of its winning face: grad_depth w_k n / s, plus for every pair (itself, a missed neighbour b) with minimising edge k
 *   (corners k1 = k + 1, k2 = k + 2 mod 3): G p_k2 x D on corner k1 and G D x p_k1 on corner k2, D = (e_k(a) d_b - e_k(b) d_a) /
 *   (e_k(a) - e_k(b))^2 (e_k = d . (p_k1 x p_k2) is linear in the ray), G = [tau > 1/2][A(b) < 1] grad_coverage(b) +
 *   [tau < 1/2][A(a) > 0] grad_coverage(a).  Saturation (A(b) = 1, A(a) = 0) is decided from the SAVED coverage image and passes no
 *   gradient; tau = 1/2 exactly passes none either.  Both terms of a pair are owned by the hit pixel.  Miss pixels write NOTHING
 *   (their records are never read).  A face id >= num_faces or a vertex index outside [0, num_vertices) sets status_dev[0] to 1 and
 *   the pixel's record is written as 0.  num_faces == 0 returns RF_OK without a launch.
 * rf_mesh_geometry_backward_gather: grad_vertices_dev [V, 3] from the records of all views (records_dev [num_pixels, 9]) by two
 *   segmented sums without atomics.  hit_pixels_dev [num_hits] int32: the hit pixels sorted by face id, ties in ascending pixel order;
 *   face_offsets_dev [num_faces + 1] int64 delimits each face's segment; face_grads_dev [num_faces, 9] (scratch, every row written)
 *   gets the per-face sums.  corner_slots_dev [3 num_faces] int32: the slots 3 face + corner sorted by the vertex they name, ascending
 *   within a vertex; vertex_offsets_dev [V + 1] int64 delimits them; vertex v gets the sum of face_grads[slot] over its segment, 0
 *   for an empty one (EVERY vertex is written).  A segment of at most `long_segment` entries (0: the default, 16) is summed by its
 *   own lane in entry order, a longer one by the whole wavefront: lane l sums entries l, l + 64, ..., then the fixed tree
 *   x_l += x_(l + 32), (l + 16), ..., (l + 1).  The additions and their order depend on the lists and long_segment alone: two calls
 *   give identical bits.  An entry outside its rows sets status_dev[0] to 1 and is skipped; offsets are clamped to the list.
 * Before any launch, in this order: RF_ERR_NULL_POINTER (any array a non-zero count needs, camera, status_dev); RF_ERR_BAD_SHAPE (as
 * rf_mesh_raster_shade; num_pixels >= 2^31, num_hits > num_pixels, 3 num_faces >= 2^31, a negative count or long_segment);
 * RF_ERR_UNSUPPORTED (a flag bit other than RF_RASTER_CULL_BACKFACES; any flag bit for the gather).  (Added to ABI version 4
 * compatibly: no existing struct or signature changed.) */
int rf_mesh_raster_coverage(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                            const uint64_t* visibility_dev, uint32_t flags, float* depth_dev, float* coverage_dev, int32_t* face_ids_dev, void* stream);
int rf_mesh_geometry_backward_pixels(const RFCamera* camera, const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                                     const int32_t* face_ids_dev, const float* coverage_dev, const float* grad_depth_dev, const float* grad_coverage_dev,
                                     uint32_t flags, float* records_dev, int32_t* status_dev, void* stream);
int rf_mesh_geometry_backward_gather(const float* records_dev, int64_t num_pixels, const int32_t* hit_pixels_dev, int64_t num_hits, const int64_t* face_offsets_dev,
                                     int64_t num_faces, const int32_t* corner_slots_dev, const int64_t* vertex_offsets_dev, int64_t num_vertices,
                                     int32_t long_segment, uint32_t flags, float* face_grads_dev, float* grad_vertices_dev, int32_t* status_dev, void* stream);

/* ---- TSDF fusion of posed depth views (csrc/fusion_kernels.hip; thr3ed_atom_amd/fusion.py chunks the views,
 * finalises and hands the volume to rf_mesh_count / rf_mesh_emit as an identity-mode grid) ----------------------------------------
 * The volume is a lattice of dims = (X, Y, Z) nodes in the box [aabb_min, aabb_max] (HOST arrays of 3), placed as an RFGrid's nodes
 * are: node (ix, iy, iz) sits at aabb_min + (aabb_max - aabb_min) * ((2i + 1) / (2 dim)) per axis in float32 (the interior lattice
 * points of rf_mesh_count at subdivisions = 1) and has plain index n = (ix Y + iy) Z + iz.  `cameras` is a HOST array of num_views
 * (0 .. 16) RFCamera of one height H and width W (focals and poses are free); depths_dev [n, H, W] float32, the ray parameter of the
 * first surface per pixel (= the camera-space depth: what rf_mesh_raster_shade and rf_render_geometry write); alphas_dev [n, H, W]
 * float32 or NULL; images_dev [n, H, W, 3] float32 or NULL.  tsdf_sum_dev [N] float32, counts_dev [N, 2] int32 = (observed, hidden)
 * and colour_sum_dev [N, 4] float32 (three colour sums and their count; required with images_dev, else NULL or carried through) are
 * IN/OUT; counts_dev is 8-byte and colour_sum_dev 16-byte aligned.  Per node p, for each view k in order:
 *   1. c = R_k^T (p - t_k), z = -c_z (the products and the sum order of rf_texture_project_views); skipped unless z is finite and
 *      z > near.
 *   2. x = W/2 + f c_x / z, y = H/2 - f c_y / z; skipped unless 0 <= x < W and 0 <= y < H; j = floor(x), i = floor(y).  The fetch is
 *      nearest-pixel: interpolating depth across a discontinuity invents surfaces.
 *   3. D = depths[k, i, j], A = alphas[k, i, j] when alphas are given.  D not finite: skipped (no information).  The pixel is a MISS
 *      when D <= 0, or when alphas are given and A < min_alpha; otherwise a hit.
 *   4. Miss: under RF_FUSE_CARVE the ray crosses the node in free space, s = 1, observed; without the flag: skipped.
 *   5. Hit: sdf = D - z.  sdf < -truncation: HIDDEN, counts.hidden += 1 and nothing else.  Otherwise s = min(1, sdf / truncation),
 *      observed.
 *   6. Observed: tsdf_sum += s, counts.observed += 1.
 *   7. With images, a hit with |sdf| <= truncation: colour_sum.rgb += images[k, i, j, :], colour_sum.w += 1.
 * Weights are 1: no angle weights, no running-average cap, no bilinear fetch.  One launch, one lane per node, no atomics: the lane
 * loads its accumulators, adds its views in order and stores them, so two calls give identical bits and successive calls over
 * chunks of views do the float additions of one long loop; a node no view of the chunk touches gets back what was loaded.  Every
 * pixel index is formed only after the tests of step 2 held (NaN fails them).  Before any launch, in this order:
 * RF_ERR_NULL_POINTER (the box, dims, tsdf_sum_dev, counts_dev; cameras / depths_dev with num_views > 0; images_dev without
 * colour_sum_dev), RF_ERR_BAD_SHAPE (a dim outside [1, 4096] or N >= 2^31, a box that is not finite or has max <= min on an axis,
 * num_views outside [0, 16], an image edge outside [1, 16384], views of unequal size, a focal that is not finite or <= 0, a pose that
 * is not finite, near not finite or < 0, truncation not finite or <= 0, min_alpha outside [0, 1], a misaligned counts_dev or
 * colour_sum_dev), RF_ERR_UNSUPPORTED (a flag bit other than RF_FUSE_CARVE).  num_views == 0 returns RF_OK without a launch.  (Added
 * to ABI version 4 compatibly: no existing struct or signature changed.) */
enum { RF_FUSE_CARVE = 128 };
int rf_fuse_depth_views(const float* aabb_min, const float* aabb_max, const int32_t* dims, int32_t num_views, const RFCamera* cameras,
                        const float* depths_dev, const float* alphas_dev, const float* images_dev, float near, float truncation, float min_alpha,
                        uint32_t flags, float* tsdf_sum_dev, int32_t* counts_dev, float* colour_sum_dev, void* stream);

/* ---- Closest points on a triangle mesh (csrc/mesh_distance_kernels.hip; docs/mesh_distance_errors.md;
 * thr3ed_atom_amd/mesh_distance.py builds the lists, samples surfaces and reduces the distances) -------------------------------------
 * The search structure is a lattice of cells = (n_x, n_y, n_z) cubic cells (each in [1, 1024], n_x n_y n_z < 2^25) of edge h from
 * `origin` (HOST arrays of 3).  The cell of a coordinate v along an axis is floor(fl32(fl32(v - origin) * r)), r = fl32(1 / h), clamped
 * into [0, n - 1]; the key of a cell is (k_x n_y + k_y) n_z + k_z.  A face is registered in every cell of the cell range of its
 * axis-aligned box.
 * rf_mesh_grid_pairs: offsets_dev [num_faces + 1] int64 is the exclusive prefix sum of the cells per face (the caller computes it with
 *   the rule above), num_pairs its last entry.  One lane per face writes keys_dev [num_pairs] int64 and pair_faces_dev [num_pairs]
 *   int32 from offsets[f] on, x-major; a box of more than 64 cells is written by the whole wavefront.  A face that indexes outside the
 *   vertices or has a non-finite corner writes nothing and sets status_dev[0] (int32, zeroed by the caller) to 1; one whose own count
 *   differs from its offsets writes nothing and sets it to 2.  No atomics.
 * rf_mesh_closest_points: cell_begin_dev [n_x n_y n_z + 1] int32 bounds every cell's segment of cell_faces_dev [num_pairs] int32 (the
 *   pairs' faces stably sorted by key).  points_dev [num_points, 3] float32; order_dev [num_points] int64 or NULL is the order in which
 *   lanes take the queries (a permutation; results land at the query's own index).  Per query: distance_dev [num_points] float32,
 *   face_dev [num_points] int64, point_dev [num_points, 3] float32 = the smallest float32 distance over ALL faces under the rule of
 *   docs/mesh_distance_errors.md (closest_on_face of csrc/mesh_distance.h), the lowest face index on an exact tie, and that face's
 *   closest point; (+inf, -1, NaN) when no face lies within max_distance (inclusive; +inf: no limit).  The result does not depend on
 *   the lattice, bit for bit.  rings_dev [num_points] int32 or NULL receives the Chebyshev radius at which the query stopped.
 *   status_dev[0] is set to 1 for a non-finite query (which gets (+inf, -1, NaN)) or a face outside the vertices, to 2 for a list
 *   entry outside its array.  One launch, no atomics, no LDS: one lane per query for the first two shells of cells, then the whole
 *   wavefront per query that is still walking (the same minimum, the same bits).
 * Before any launch, in this order: RF_ERR_NULL_POINTER (origin, cells, status_dev; every array a non-zero count needs),
 * RF_ERR_BAD_SHAPE (a negative count, 2^31 or more vertices, faces or pairs, h or 1 / h not positive and finite, a non-finite origin, a
 * cell count outside [1, 1024] or a lattice of 2^25 cells or more, a max_distance that is negative or NaN), RF_ERR_UNSUPPORTED (any
 * flag bit: none is defined); then zero faces (or zero points) return RF_OK without a launch.  (Added to ABI version 4 compatibly: no
 * existing struct or signature changed.) */
int rf_mesh_grid_pairs(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const float* origin, float h,
                       const int32_t* cells, const int64_t* offsets_dev, int64_t num_pairs, int64_t* keys_dev, int32_t* pair_faces_dev, int32_t* status_dev,
                       void* stream);
int rf_mesh_closest_points(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces, const float* origin, float h,
                           const int32_t* cells, const int32_t* cell_begin_dev, const int32_t* cell_faces_dev, int64_t num_pairs, const float* points_dev,
                           const int64_t* order_dev, int64_t num_points, float max_distance, uint32_t flags, float* distance_dev, int64_t* face_dev,
                           float* point_dev, int32_t* rings_dev, int32_t* status_dev, void* stream);

/* ---- Gradients of the distance to a triangle mesh (csrc/mesh_distance_grad_kernels.hip; DESIGN.md section 28;
 * docs/mesh_distance_grad_errors.md; thr3ed_atom_amd/mesh_distance_grad.py wires it into autograd, the Chamfer loss and the fit) ------
 * For query p = points_dev[i] whose closest face, as rf_mesh_closest_points found it, is face_dev[i] = f = (a, b, c): let q be the
 * closest point of the rule of docs/mesh_distance_errors.md (closest_on_face of csrc/mesh_distance.h), beta its barycentrics in f,
 * r = p - q per component in float32, len = sqrt(dot(r, r)) with the rule's dot, u = r / len when len > 0 and u = 0 otherwise (the
 * subgradient at the surface).  With upstream G = grad_distance_dev[i] = dL/d(distance):
 *   dL/dp = G u,   dL/d(corner k) = -beta_k G u.
 * Exact wherever the distance is differentiable, in the interior, edge and vertex regions alike: the squared distance is a minimum
 * over beta, so only the explicit dependence on the corners survives (docs/mesh_distance_grad_errors.md has the argument).
 * beta comes from the candidate that won, found by running the four candidates in the forward rule's order with its strict <:
 *   a segment (x, y) with parameter t won:  beta_x = 1 - t, beta_y = t, the third 0;
 *   the plane candidate won:  with the three edge values of the accept test, E_ab, E_bc, E_ca = dot((y - x) x (q - x), n) at the
 *     UNCLAMPED q:  S = (E_ab + E_bc) + E_ca, beta_c = E_ab / S, beta_a = E_bc / S, beta_b = E_ca / S;
 *   S not > 0: the best segment candidate is used instead.
 * A zero-length edge, a zero-area face or a repeated vertex gives a segment's or a point's beta and never a NaN.  The selected q and
 * d2 are the forward's bits.
 * One lane per query, one launch, no atomics, no LDS.  A query with face_dev[i] >= 0 writes grad_points_dev[i] (3 floats),
 * records_dev[i] (9 floats, corner-major: -beta_k G u), barycentrics_dev[i] (3 floats) and region_dev[i] (0, 1, 2 for the segments
 * ab, bc, ca; 3 for the plane).  A query with face -1 (nothing within max_distance) writes zeros to grad_points_dev[i] and
 * barycentrics_dev[i], -1 to region_dev[i] and does NOT write its record.  A face id >= num_faces or a vertex index outside
 * [0, num_vertices) sets status_dev[0] (int32, zeroed by the caller) to 1 and writes zeros (region -1).  Each of the four outputs may
 * be NULL.  The per-vertex sum of the records is rf_mesh_geometry_backward_gather's, with num_pixels = num_points and hit_pixels =
 * the queries that have a face, stably sorted by face.
 * Before any launch, in this order: RF_ERR_NULL_POINTER (status_dev; vertices_dev / faces_dev with num_faces > 0; points_dev,
 * face_dev, grad_distance_dev with num_points > 0; all four outputs NULL with num_points > 0), RF_ERR_BAD_SHAPE (a negative count;
 * num_vertices, num_faces or num_points >= 2^31), RF_ERR_UNSUPPORTED (any flag bit: none is defined); then num_points == 0 or
 * num_faces == 0 return RF_OK without a launch.  (Added to ABI version 4 compatibly: no existing struct or signature changed.) */
int rf_mesh_closest_gradients(const float* vertices_dev, int64_t num_vertices, const int64_t* faces_dev, int64_t num_faces,
                              const float* points_dev, const int64_t* face_dev, const float* grad_distance_dev, int64_t num_points,
                              uint32_t flags, float* grad_points_dev, float* records_dev, float* barycentrics_dev,
                              int32_t* region_dev, int32_t* status_dev, void* stream);

/* The loss of the training iteration (modules/trainers.py:311-317, 329-336) in one launch:
 * grad_colour_dev [N,3] = scale * d(mean |colour - target|)/d colour = scale * sign(colour - target) / (3N);
 * sums_dev[0] += sum |colour - target|, sums_dev[1] += sum (colour - target)^2  (L1 loss and MSE/PSNR for
 * logging; the caller zeroes sums_dev). */
int rf_l1_loss_grad(const float* colour_dev, const float* target_dev, int64_t num_rays, float scale,
                    float* grad_colour_dev, float* sums_dev, void* stream);

/* Fused Adam step on a flat float32 parameter buffer (torch.optim.Adam semantics, betas/eps/lr given;
 * modules/trainers.py:242-250,339-341).  step is the 1-based step count used for bias correction.
 * zero_grad != 0 also clears grad_dev after reading it (optimizer.zero_grad() of the next iteration). */
int rf_adam_step(float* param_dev, float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t numel,
                 float lr, float beta1, float beta2, float eps, int32_t step, int32_t zero_grad, void* stream);

/* ---- the training iteration as ONE call -------------------------------------------------------------------------------
 * modules/trainers.py:278-341 (ray/pixel subset -> specular render -> L1 -> diffuse render -> L1 -> backward of both ->
 * Adam) enqueued by a single host call: select -> forward (counts records), twice -> loss gradients + offsets -> emit, twice
 * -> ONE brick pass over both record lists [-> Adam inside its flush].  Seven launches, no host round trip between them; the
 * caller (a Python trainer, or any host language) pays one FFI crossing per iteration instead of ~20.  Every buffer is
 * caller-owned scratch that can be reused from step to step. */
typedef struct RFRaySelection { /* arguments of rf_select_rays_and_pixels */
  int32_t height, width;
  float focal;
  const float* poses_dev;
  const int64_t* image_ids_dev;
  int32_t num_batch_images;
  const float* pixel_table_dev;
  uint64_t key;
  int64_t first_index;
} RFRaySelection;

typedef struct RFPassScratch { /* one per render of the iteration: [0] specular, [1] render_diffuse */
  RFRenderOut out;           /* all eight per-ray / per-sample buffers, key_hist_dev [8 * nbricks] (zero on entry; left
                                zero) and brick_size                                                              */
  float* grad_colour_dev;    /* [N, 3]                                                                           */
  int32_t* cursor_dev;       /* [8 * nbricks]                                                                    */
  int64_t* offsets_dev;      /* [8 * nbricks + 1]                                                                */
  float* records_sorted_dev; /* [N * S, rf_expanded_record_floats(F)] ([1]: rf_expanded_record_floats(3))        */
  const float* t_rand_dev;   /* [N, S] jitter of this render, or NULL (off, or keyed with RF_FLAG_JITTER_KEYED)  */
  uint64_t jitter_key;
} RFPassScratch;

typedef struct RFTrainStep {
  const RFRaySelection* select; /* non-NULL: the batch is drawn by the fused selection INTO origins / directions / pixels;
                                   NULL: they are inputs                                                          */
  float* origins_dev;           /* [N, 3] */
  float* directions_dev;        /* [N, 3] */
  float* pixels_dev;            /* [N, 3] target colours */
  int64_t num_rays;
  int32_t num_samples;
  float near, far;
  const float* t_vals_dev;      /* [S] */
  uint32_t flags;               /* RF_FLAG_* of both renders (RF_FLAG_RENDER_DIFFUSE is added to the second one here) */
  RFPassScratch pass[2];
  float* loss_sums_dev;         /* [4], overwritten: (sum |d|, sum d^2) of the specular render, then of the diffuse render */
  const RFAdamState* adam;      /* optimizer fused into the brick flush, or NULL: the gradient of L1 + L1 is WRITTEN (not
                                   added) to grad_first_dev / grad_second_dev (layout of `grid`)                  */
  float* grad_first_dev;
  float* grad_second_dev;
  int64_t first_ray;            /* position of ray 0 in the keyed jitter streams (global-batch data parallelism: the rank's
                                   offset in the batch); 0 otherwise                                                          */
  uint32_t phases;              /* 0 = the whole iteration, else a set of RF_STEP_FORWARD (select, both forward passes, losses +
                                   offsets), RF_STEP_EMIT (both adjoints as records), RF_STEP_BRICKS (the brick pass over
                                   pass[0..1]'s lists): a data-parallel caller starts its exchange of the offset tables after
                                   FORWARD, lets it overlap EMIT, and runs rf_brick_accumulate_adam_range itself after the
                                   record exchange                                                                              */
  float loss_scale;             /* the L1 gradients are scaled by this (0 = 1): 1 / world size under data parallelism          */
  void* const* timing_events;   /* optional HOST array of RF_TRAIN_STEP_EVENTS hipEvent_t (created by the caller with timing
                                   enabled): event 0 is recorded on `stream` before the first launch, event k after launch k
                                   in the order select, forward[0], (nothing), forward[1], losses of both renders + offsets of
                                   both lists (one launch), (nothing), emit[0], (nothing), emit[1], bricks -- per-kernel durations
                                   of the very call that is timed (only with phases == 0).  A full iteration runs both forward
                                   renders in ONE launch and both adjoints in ONE launch (the render_diffuse pass walks the same
                                   rays as the specular one: it finds the base records of its corners on chip); slot [0] of a
                                   pair then holds the launch and slot [1] is empty.  $RF_FWD_PAIR=0 / $RF_EMIT_PAIR=0 in the
                                   environment restore one launch per render (A/B measurements)                                */
} RFTrainStep;

enum {
  RF_STEP_FORWARD = 1, RF_STEP_EMIT = 2, RF_STEP_BRICKS = 4,
  RF_STEP_EMIT_SPECULAR = 8, RF_STEP_EMIT_DIFFUSE = 16,  /* one adjoint at a time */
  /* RF_STEP_FORWARD in two pieces, the render_diffuse pass first: it reads the base tensor only, so a data-parallel caller runs it
     while the `rest` parameters of the previous iteration are still being all-gathered */
  RF_STEP_SELECT_AND_DIFFUSE_FORWARD = 32, RF_STEP_SPECULAR_FORWARD_AND_LOSSES = 64,
  /* the two renders' chains apart (pipelined owner-computes step): RF_STEP_DIFFUSE_CHAIN = selection, render_diffuse forward, loss +
     offsets of list [1], its adjoint as records -- everything that reads the base tensor only and needs no other rank, so it runs
     beside the arriving `rest` parameters of the previous iteration; RF_STEP_SPECULAR_FORWARD = specular forward, loss + offsets of
     list [0] (then RF_STEP_EMIT_SPECULAR).  (Added compatibly: no struct or signature changed.) */
  RF_STEP_DIFFUSE_CHAIN = 128, RF_STEP_SPECULAR_FORWARD = 256
};

#define RF_TRAIN_STEP_EVENTS 11

int rf_train_step(const RFGrid* grid, const RFTrainStep* step, void* stream);

/* ---- the two renders of an iteration, PAIRED, as separate calls ---------------------------------------------------------
 * The reference's iteration renders the same rays twice -- vol_mod.render_rays(rays) and vol_mod.render_rays(rays,
 * render_diffuse=True), each with its own jitter draw (modules/trainers.py:306, 323-325) -- and back-propagates the sum of the two
 * L1 losses (:311, 329-330, 338).  A host that keeps autograd in charge (torch.autograd.Function: one node for the PAIR of
 * renders, one for the pair of losses) enqueues the iteration's launches one by one instead of through rf_train_step:
 *
 *   rf_render_forward_pair              both saving forward renders in ONE launch ([0] specular, [1] render_diffuse; the second
 *                                       finds the base records of its corners on chip).  Both outs must carry the four cache
 *                                       buffers; key_hist_dev counts the records per key as in rf_render_forward.
 *   rf_l1_loss_grad_pair                the two losses in ONE launch and ready to use: out_dev[5] = (loss[0] + loss[1], loss[0],
 *                                       mse[0], loss[1], mse[1]) -- means, written by the last workgroup to finish;
 *                                       grad_colour_dev[i] as rf_l1_loss_grad.  workspace_dev: 8 floats, zero before the first
 *                                       use, left zero (the kernel cleans up after itself; one workspace per stream).
 *   rf_bin_offsets_pair                 rf_bin_offsets for both lists in one launch
 *   rf_render_backward_emit_direct_pair both adjoints as records in ONE launch (rf_render_backward_emit_direct twice); upstream
 *                                       gradients of the colours only (passes[i].grad_colour_dev), like every reference use.
 *
 * Every array argument holds TWO entries.  RF_ERR_UNSUPPORTED when the two renders do not pair up (different ray counts, flags
 * that do not say specular / render_diffuse): the caller then launches them one by one.  (Added to ABI version 4 compatibly: no
 * existing struct or signature changed.) */
int rf_render_forward_pair(const RFGrid* grid, const RFRayBatch* rays, const uint32_t* flags, const RFRenderOut* outs, void* stream);
int rf_l1_loss_grad_pair(const float* const* colour_dev, const float* target_dev, int64_t num_rays, float scale,
                         float* const* grad_colour_dev, float* workspace_dev, float* out_dev, void* stream);
int rf_bin_offsets_pair(const int32_t* const* hist_dev, int32_t num_keys, int64_t* const* offsets_dev, int32_t* const* cursor_dev,
                        void* stream);
int rf_render_backward_emit_direct_pair(const RFGrid* grid, const RFRayBatch* rays, const uint32_t* flags,
                                        const RFPassScratch* passes, void* stream);

/* Which instantiation of the two pair kernels (rf_render_forward_pair, rf_render_backward_emit_direct_pair, and the same launches
 * inside rf_train_step) serves this grid, these two ray batches and these two flag words: 1 = the TRAINER-SHAPED one, 0 = the
 * generic one; negative = error code (RF_ERR_UNSUPPORTED when the two renders do not pair up).  Trainer-shaped means, all of:
 * layout RF_LAYOUT_SPLIT (not bricked), a grid small enough for 32-bit corner offsets (<= 2^24 nodes, both tensors inside one 4 GB
 * window; $RF_FAR_ADDRESSING = 1 switches that off), density_mode RF_DENSITY_RELU, both batches ray lists (camera == NULL) with
 * t_rand_dev == NULL and RF_FLAG_JITTER_KEYED, neither RF_FLAG_OCCUPANCY_SKIP nor RF_FLAG_AABB_SAMPLING.  RF_FLAG_WHITE_BKGD may
 * be either.  The trainer-shaped kernels run the same per-sample code with those switches compiled in instead of read from
 * their arguments: every output is bit for bit the generic kernels'.  $RF_STEP_SPECIALISED = 0 in the environment (read at every
 * call) sends everything to the generic kernels.  Host-side only: no device access.  (Added to ABI version 4 compatibly: no
 * existing struct or signature changed.) */
int rf_step_kernel_specialised(const RFGrid* grid, const RFRayBatch* rays, const uint32_t* flags);

#ifdef __cplusplus
}
#endif
#endif /* RELU_FIELD_H_ */
