/*
 * cvr.h — C-ABI of the MI355X-native structured volume ray-caster.
 *
 * This is the drop-in boundary for cppvolrend's renderer-plugin path
 * (k2683/cpp_volume_rendering).  A reference-side adapter class
 * (`HipRayCasting1Pass : BaseVolumeRenderer`) forwards the
 * plugin calls to these functions; no GL object and no torch type crosses the
 * boundary, only plain pointers, sizes and POD structs.
 *
 * Mapping to the reference interface (paths relative to the reference root):
 *
 *   cvr_create / cvr_destroy     <- BaseVolumeRenderer ctor / Clean()
 *                                   cppvolrend/volrenderbase.cpp:5-29
 *   cvr_set_volume               <- DataManager::GenerateStructuredVolumeTexture +
 *                                   vis::GenerateRTexture (u8/255 -> float -> GL_R16F)
 *                                   libs/volvis_utils/datamanager.cpp:311-330,
 *                                   libs/volvis_utils/utils.cpp:20-56
 *   cvr_set_transfer_function    <- TransferFunction1D::GenerateTexture_1D_RGBt
 *                                   (256 x RGBA16F, alpha already converted to extinction)
 *                                   libs/volvis_utils/transferfunction1d.cpp:89-118
 *   cvr_set_gradient             <- DataManager::GenerateStructuredGradientTexture
 *                                   libs/volvis_utils/datamanager.cpp:332-352,
 *                                   libs/volvis_utils/utils.cpp:146-284 (finite differences)
 *   cvr_render_rc1pass           <- RayCasting1Pass::Update + Redraw
 *                                   cppvolrend/structured/rc1pass/rc1prenderer.cpp:72-151
 *                                   (the dispatch of ray_marching_1p.comp:85-179)
 *   cvr_set_extinction_volume    <- ExtinctionCoefficientVolume::BuildMipMappedTexture (extcoefvolumegenerator.cpp:20-40)
 *                                   (Gaussian mip pyramid of TF opacity -> extinction)
 *                                   cppvolrend/structured/rc1pdosct/extcoefvolumegenerator.cpp:230-408
 *   cvr_render_dosct             <- RC1PConeTracingDirOcclusionShading::Update + Redraw
 *                                   cppvolrend/structured/rc1pdosct/dosrcrenderer.cpp:134-260
 *                                   (the dispatch of ray_bbox_marching.comp:658-734)
 *   cvr_render_dosct_preillum    <- the same Update with "Use Pre-Illumination" on:
 *                                   PreComputeLightCache (dosrcrenderer.cpp:555-655,
 *                                   lightcachecomputation.comp) + obj_ray_marching.comp
 *   cvr_set_extinction_sat       <- RC1PExtinctionBasedShading::GenerateExtinctionSAT3DTex +
 *                                   SummedAreaTable3D<double>::BuildSAT
 *                                   cppvolrend/structured/rc1pextbsd/ebsrenderer.cpp:624-716,
 *                                   libs/vis_utils/summedareatable.h:218-278
 *   cvr_render_extbsd            <- RC1PExtinctionBasedShading::Update + Redraw
 *                                   cppvolrend/structured/rc1pextbsd/ebsrenderer.cpp:125-260
 *                                   (the dispatch of ebs_ray_bbox_marching.comp)
 *   cvr_render_extbsd_preillum   <- the same Update with "Use Pre-Illumination" on
 *                                   (ebsrenderer.cpp:46-47): PreComputeLightCache
 *                                   (rc1pextbsd/lightcachecomputation.comp) +
 *                                   _common_shaders/obj_ray_marching.comp
 *   cvr_crtgt_begin / _advance   <- RC1PConeLightGroundTruthSteps::Update + RedrawFrameTexture
 *   cvr_render_crtgt                cppvolrend/structured/rc1pcrtgt/crtgtrenderer.cpp:121-325
 *   cvr_vct_precompute           <- VCTPreProcessing::PreProcessSuperVoxels + PreProcessPreIntegrationTable
 *                                   cppvolrend/structured/rc1pvctsg/preprocessingstages.cpp:35-202
 *   cvr_render_vct               <- RC1PVoxelConeTracingSGPU::Update + Redraw
 *                                   cppvolrend/structured/rc1pvctsg/vctrenderer.cpp:124-250
 *                                   (the dispatch of vct_ray_bbox_marching.comp)
 *                                   (the dispatches of gt_ray_marching.comp, one sample per
 *                                   pixel each, until every pixel's state says "done")
 *   cvr_crtgt_build_rays         <- the ray tables of Update, crtgtrenderer.cpp:131-184
 *   cvr_status (never exit())    <- gl::ExitOnGLError  libs/gl_utils/utils.cpp:11-30
 *
 * Threading: one context per device, externally synchronised (the reference
 * renderer runs on the single GLUT thread, app_freeglut.cpp:172-175).
 * Ownership: the context owns every device allocation; no caller pointer is
 * retained after a call returns.
 */
#ifndef CVR_H
#define CVR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a public struct's layout or an entry point's meaning changes
 * (2: cvr_frame gained use_view/view).  Callers compare cvr_abi_version() with
 * the CVR_ABI_VERSION they were compiled against before the first call that
 * passes a struct.  Entry points that are only added (the pre-illumination
 * and ground-truth calls below) leave every existing caller valid and do not bump it; a caller
 * that needs them looks them up by name. */
#define CVR_ABI_VERSION 2

typedef enum cvr_status {
  CVR_OK = 0,
  CVR_ERR_ARG = 1,    /* invalid argument (null pointer, bad size, bad enum)   */
  CVR_ERR_HIP = 2,    /* a HIP runtime call failed                              */
  CVR_ERR_OOM = 3,    /* device allocation failed                               */
  CVR_ERR_STATE = 4,  /* call out of order (e.g. render before set_volume);
                         mirrors RayCasting1Pass::Init returning false when the
                         volume texture is missing, rc1prenderer.cpp:54          */
  CVR_ERR_IO = 5      /* a reader could not open / parse its file              */
} cvr_status;

typedef struct cvr_ctx cvr_ctx;

/* ----------------------------------------------------------------------------
 * Frame description: vis::Camera state + viewport + optional screen-tile split.
 * -------------------------------------------------------------------------- */
typedef struct cvr_camera {
  float eye[3];     /* Camera::GetEye                       camera.cpp:340   */
  float center[3];  /* look-at target                       camera.cpp:281   */
  float up[3];      /* up vector                            camera.cpp:281   */
  float fovy_deg;   /* 45 by default                        camera.cpp:25,44 */
  float aspect;     /* <= 0: width / height                 camera.cpp:307   */
} cvr_camera;

typedef struct cvr_frame {
  cvr_camera camera;
  int width;        /* viewport (RenderingParameters::GetScreenWidth)         */
  int height;
  /* Screen-tile split (multi-GPU): nranks <= 1 renders the whole W x H image
   * row-major.  nranks > 1: the image is cut into tile_size^2 tiles (a multiple
   * of 16; 16 recommended) on a diagonal lattice: with ntx tiles per row, this
   * rank's k-th tile is virtual tile v = rank + k*nranks, at row ty = v / ntx
   * and column tx = (v % ntx - s*ty) mod ntx, s = 3 for nranks >= 4 else 1
   * (when nranks divides ntx: rank (tx + s*ty) % nranks).  It is written packed
   * at offset k*tile_size*tile_size pixels, row-major inside the tile.  Every
   * rank gets cvr_tiles_for_rank tiles, as with plain t % nranks.  (ABI 2.)  */
  int tile_size;
  int rank;
  int nranks;
  /* use_view = 1: `view` is the column-major view matrix the reference uploads
   * as u_CameraLookAt (vis::Camera::LookAt, camera.cpp:281-284, which keeps the
   * look-at centre private) and camera.center is ignored; camera.eye is still
   * CameraEye.  use_view = 0: view = glm::lookAt(eye, center, up).          */
  int use_view;
  float view[16];
} cvr_frame;

/* Output buffers.  rgba: premultiplied RGBA, W*H pixels (or the packed tile
 * buffer), in `format`: CVR_FORMAT_RGBA32F (0, 16 B/pixel, the exact
 * composite) or CVR_FORMAT_RGBA16F (1, 8 B/pixel: binary16 rounded to nearest
 * even, the reference's own framebuffer, imageStore into the RGBA16F
 * OutputFrag image, ray_marching_1p.comp:174-176 / renderoutputframe.cpp:64-87).
 * samples (optional): per-pixel loop-iteration count of
 * ray_marching_1p.comp:124-172 (transparent samples included, stopping at the
 * ERT break).  total (optional): the sum of all iteration counts (uint64).
 * on_device = 1: all three are device pointers and the call is asynchronous
 * on the context stream; the frame's count is atomically ADDED to *total, so
 * the caller zeroes it (one counter can accumulate many frames).
 * on_device = 0: host pointers, *total is overwritten, the call blocks.      */
#define CVR_FORMAT_RGBA32F 0
#define CVR_FORMAT_RGBA16F 1
typedef struct cvr_output {
  void* rgba;
  void* samples;
  void* total;
  int on_device;
  int format;       /* CVR_FORMAT_RGBA32F | CVR_FORMAT_RGBA16F */
} cvr_output;

/* ----------------------------------------------------------------------------
 * Renderer parameters
 * -------------------------------------------------------------------------- */

/* RayCasting1Pass ("1-Pass - Ray Casting", s_1rc): rc1prenderer.cpp:18-138. */
typedef struct cvr_rc1pass_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale|, rc1prenderer.cpp:62-63 */
  int   apply_gradient_shading;/* Blinn-Phong with the gradient volume, :112        */
  float ka, kd, ks, shininess; /* renderingparameters.cpp:23-26 (0.5,0.5,0.8,30)     */
  float ispecular[3];          /* light specular colour, lightsourcelist.cpp:24      */
  float light_pos[3];          /* RenderingParameters::GetBlinnPhongLightingPosition */
} cvr_rc1pass_params;

/* Isosurface ray-casters with block empty-space skipping:
 *   variant 0: CustomRayCasting1PassIsoAdapt ("1-Pass - Custom Isosurface
 *              Raycaster Adaptive", rc1pisocustom/rc1custompisoadaptrenderer.cpp),
 *              4^3 blocks, the block chord as the skip distance;
 *   variant 1: CustomRayCasting1PassIsodfsAdapt ("Empty Sapce Skipping V2",
 *              rc1pisodfscustom/rc1custompisoadaptdfsrenderer.cpp), 32^3 blocks,
 *              the block exit distance and a tolerance of 0.001;
 *   variant 2: RayCasting1PassIsoAdapt ("1-Pass - Isosurface Raycaster
 *              Adaptive", rc1pisoadapt/rc1pisoadaptrenderer.cpp), no blocks.
 * Defaults (cvr_iso_params_default): rc1custompisoadaptrenderer.cpp:119-127. */
typedef struct cvr_iso_params {
  int   variant;               /* 0, 1 or 2                                            */
  int   num_blocks[3];         /* <= 0: 4^3 (variant 0) / 32^3 (variant 1), :190       */
  float isovalue;              /* m_u_isovalue 0.5                                     */
  float step_small;            /* m_u_step_size_small 0.05                             */
  float step_large;            /* m_u_step_size_large 1.0                              */
  float step_range;            /* m_u_step_size_range 0.1                              */
  float color[4];              /* m_u_color (0.66, 0.6, 0.05, 1.0)                     */
  int   apply_gradient_shading;/* m_apply_gradient_shading (default 0; needs gradient) */
  float ka, kd, ks, shininess; /* Blinn-Phong constants (renderingparameters.cpp:23-26) */
  float ispecular[3];          /* BlinnPhongIspecular                                  */
  float light_pos[3];          /* LightSourcePosition                                  */
} cvr_iso_params;

/* Directional-occlusion cones (RC1PConeTracingDirOcclusionShading,
 * cppvolrend/structured/rc1pdosct): the parameters of one ConeGaussianSampler
 * (conegaussiansampler.h) and the tables the renderer uploads from it. */
#define CVR_MAX_CONE_SECTIONS 1024
typedef struct cvr_cone_params {
  float half_angle_deg;    /* SetConeHalfAngle (clamped to [0.5, 89.5]); occlusion 20, shadow 0.5 */
  int   max_packing;       /* SetMaxGaussianPacking: 0 = 1 ray, 1 = 3 rays, 2 = 7 rays
                              (occlusion 1, shadow 0; dosrcrenderer.cpp:47-58)            */
  float covered_distance;  /* SetCoveredDistance (>= 10); <= 0 at render: diagonal * 0.50
                              (occlusion) / 0.75 (shadow), dosrcrenderer.cpp:112-113      */
  float ui_weight;         /* SetUIWeightPercentage; occlusion 0.35, shadow 1.0           */
  float initial_step;      /* <= 0: 3.0 (the sampler's default)                           */
} cvr_cone_params;

typedef struct cvr_cone_tables {
  int   n_sections;        /* sections below                                            */
  int   counts[3];         /* gaussian_samples_1 / _3 / _7                               */
  float initial_step;      /* Occ/SdwInitialStep                                         */
  float ray7_adj_weight;   /* (float)GetRay7AdjacentWeight                               */
  float ui_weight;         /* Occ/SdwUIWeight                                            */
  float axes[10][3];       /* Get3ConeRayID(0..2), Get7ConeRayID(0..6)                   */
  float sections[CVR_MAX_CONE_SECTIONS][4];
                           /* per section (interval distance, mip level, d_integral,
                              amplitude) as floats, before the RGBA16F upload
                              (GetConeSectionsInfoTex, conegaussiansampler.cpp:179-205) */
} cvr_cone_tables;

/* One light source of a #list_light_sources file (vis::LightSourceData,
 * lightsourcelist.cpp:97-140) as RenderingParameters hands it to the shaders:
 * WorldLightingPos, LightCamForward/Up/Right, SpotLightMaxAngle (degrees). */
typedef struct cvr_light {
  float position[3];
  float forward[3];
  float up[3];
  float right[3];
  float spot_angle_deg;
} cvr_light;

/* RC1PConeTracingDirOcclusionShading ("1-Pass - Dir. Occlusion Shading",
 * s_1rcdosct): dosrcrenderer.cpp:24-60, 134-260. */
typedef struct cvr_dos_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale| (dosrcrenderer.cpp:124-125) */
  int   apply_gradient_shading;/* ApplyPhongShading (needs cvr_set_gradient)           */
  float ka, kd, ks, shininess; /* Blinn-Phong constants (renderingparameters.cpp:23-26) */
  float ispecular[3];          /* Ispecular                                             */
  cvr_light light;             /* the current light source                              */
  int   apply_occlusion;       /* ApplyOcclusion (default 1)                            */
  int   apply_shadow;          /* ApplyShadow (default 0)                               */
  int   shadow_type;           /* TypeOfShadow: 0 point, 1 spot, 2 directional          */
  cvr_cone_params occlusion;   /* sampler_occlusion: 20 deg, packing 1, weight 0.35     */
  cvr_cone_params shadow;      /* sampler_shadow:    0.5 deg, packing 0, weight 1.0     */
} cvr_dos_params;

/* RC1PExtinctionBasedShading ("1-Pass - Extinction Based Shading", s_1rcebs):
 * ebsrenderer.cpp:19-55, 125-260. */
typedef struct cvr_ebs_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale| (ebsrenderer.cpp:116-117)   */
  int   apply_gradient_shading;/* ApplyPhongShading (needs cvr_set_gradient)           */
  float ka, kd, ks, shininess; /* Blinn-Phong constants (renderingparameters.cpp:23-26) */
  float ispecular[3];          /* Ispecular                                             */
  float light_pos[3];          /* WorldLightingPos (point light)                        */
  float light_forward[3];      /* LightCamForward (directional light)                   */
  int   apply_occlusion;       /* apply_ambient_occlusion (default 1)                   */
  int   occlusion_shells;      /* ambient_occlusion_shells (15)                         */
  float occlusion_radius;      /* ambient_occlusion_radius (1.0, in voxels)             */
  int   apply_shadow;          /* apply_directional_shadows (default 1)                 */
  int   shadow_type;           /* type_of_shadow: 0 point light, 1 directional          */
  float shadow_cone_angle_deg; /* dir_shadow_cone_angle (1.0)                           */
  float shadow_sample_interval;/* dir_shadow_sample_interval (2.0 voxels)               */
  float shadow_initial_step;   /* dir_shadow_initial_step (2.0 voxels)                  */
  float shadow_ui_weight;      /* dir_shadow_user_interface_weight (1.0)                */
  float shadow_max_distance;   /* <= 0: 0.75 * volume diagonal (ebsrenderer.cpp:98-105) */
} cvr_ebs_params;

/* ----------------------------------------------------------------------------
 * Context
 * -------------------------------------------------------------------------- */
int         cvr_abi_version(void);
const char* cvr_status_string(cvr_status s);
cvr_status  cvr_create(int device, cvr_ctx** out_ctx);
void        cvr_destroy(cvr_ctx* ctx);
const char* cvr_last_error(const cvr_ctx* ctx);
/* Launch stream (a hipStream_t); NULL = the legacy default (null) stream.
 * A new context starts on a private non-blocking stream of its own. */
cvr_status  cvr_set_stream(cvr_ctx* ctx, void* hip_stream);
/* Tuning options (results are identical for every setting):
 *   "batch"      samples addressed + fetched per batch of the march (2 or 4; default 0 =
 *                auto: 4, or 2 with gradient shading — measured 8 % faster there)
 *   "tile_order" 1: each XCD takes the tiles of its screen band longest-first (LPT),
 *                using the previous frame's per-tile critical paths (default);
 *                0: screen order, one contiguous band per XCD; 2: screen order
 *                interleaved over the XCDs (tile t on XCD t mod 8)
 *   "stale_deg"  with tile_order 1: an order learned on a view more than this many
 *                degrees away (view direction; eye moved by that chord of its
 *                distance to the volume centre; fovy changed by that fraction) is
 *                not used, the frame runs in interleaved screen order and the
 *                order is relearned (default 5; 0 = always use it)
 *   "boost"      percent of each band's longest entries launched at raised wave
 *                priority (with tile_order 1; default 5)
 *   "band_cap"   most tiles a work-balanced XCD band may take, in percent of an
 *                even eighth (100..200, default 130); the launch has 8 x that many
 *                slots, the ones past a band's tiles exit at once
 *   "quad"       percent of each band's longest tiles marched sample-parallel, four
 *                lanes per ray (with tile_order 1; default 0)
 *   "order_interval" rebuild the LPT order every n-th frame (default 8; costs
 *                drift slowly, a rebuild costs ~15 us on the frame's stream)
 *   "async_order" 1: rebuild it on a side stream instead, used 3 frames later
 *                (default 0: cross-stream events cost more than they save)
 *   "macro"      empty-space skipping: log2 of the macro cell (2..6, default 3;
 *                0 off); compiled in only when >= "skip_min_pct" % (default 15)
 *                of the macro cells are empty for the current volume and TF
 *   "tile_stats" 1: record per-tile timing of every frame (diagnostics)
 *   "kernel_timing" N > 0: time the ray-march kernel of the last N frames
 *                (cvr_read_kernel_times); 0 off (default)
 *   "cell_skip"  per-cell skip flags kept in the density cells' fp16 sign bits
 *                (rebuilt after a volume or TF change): 0 off; 1 a sample in an
 *                EMPTY cell (no density its corners interpolate to has tau > 0) skips
 *                its classification; 2 also steps over the next samples that stay
 *                within the cell's chessboard distance to non-empty cells, per lane;
 *                3 (default) the same when every marching lane of the wave can;
 *                4 the fewest steps any lane may, for the lanes that can
 *   "sat_chunk"  z planes per work item of the EBS SAT build (1..64, default 32)
 *   "sat_layout" EBS: 0 (default) = frames read a cell4 copy of the SAT (4 float
 *                corners of a plane per texel, 16 B per texel more); 1 = frames read
 *                the plain float SAT (no copy; slower)
 *   "sat_keep_scratch" EBS: 1 keeps the SAT build's double grid (8 B per texel)
 *                allocated for rebuilds; 0 (default) frees it after each build
 *   "shade_counters" 1: count shaded / shadow-lit samples of cvr_render_dosct
 *                and cvr_render_extbsd (cvr_read_shade_counters; one atomic per wave)
 *   "shade_flat" cvr_render_dosct / cvr_render_extbsd: 1 (default) = the frame's
 *                shading jobs in one list, shaded by a grid of their own and folded
 *                per pixel; one list per render stream, sized from earlier frames'
 *                totals (read back without blocking); a frame whose list would not
 *                fit renders through the per-wave kernel, decided on the device;
 *                0 = per-wave deferred shading inside the march
 *   "flat_group" flat shading: consecutive 64-job chunks per XCD turn (default 8)
 *   "debug_flat_limit" tests: a smaller job-list capacity, to exercise the fallback
 *   "split_streams" screen-tile split: render streams the caller rotates over its
 *                cvr_gather_tiles_n calls (1..32, default 1)
 *   "gather_sets" buffer sets the caller rotates over those calls (a multiple of
 *                split_streams; 0 = one per stream): exchange g uses set g % B on
 *                stream g % D, and the stream's next render waits for exchange
 *                g + D - B, the last user of the set it writes next
 *                (0..CVR_MAX_GATHER_SETS)
 *   "gather_root_idle" 1 (communicators of N >= 3 ranks): rank 0 renders nothing and
 *                only gathers and unpacks; ranks 1..N-1 render the split over N-1
 *                render ranks (their cvr_frame: rank = communicator rank - 1,
 *                nranks = N - 1; rank 0 passes a frame of that geometry).  Rank 0's
 *                block of the gather buffer stays unused.  
 *   "launch_interleave" cvr_render_rc1pass_frames under a launch order (tile_order
 *                1/2): 1 (default) = the launch deals entry e of every frame's XCD
 *                bands before entry e + 1 of any (the longest tiles of all frames
 *                first); 0 = frame after frame.  Images identical either way.
 *   "native_exp" 1: TOLERANCE MODE, not bit-exact: the emission-absorption march
 *                (cvr_render_rc1pass[_frames] with cell_skip 3, buffer addressing)
 *                takes alpha = 1 - exp through the hardware v_exp_f32 instead of the
 *                CVR-SPEC polynomial; parity is SURVEY §8(c)'s gate (|dRGBA| <= 2e-3 for
 *                99.9 % of pixels, max 2e-2, SSIM >= 0.99), measured in DESIGN §5‴.
 *                cvr_render_dosct likewise takes the CONSIDER_BORDERS attenuation of
 *                an outside cone tap through v_exp_f32 (its march, counts and ERT
 *                stay bit-exact).  Default 0.
 *   "rc1pass_variant" (read-only) which of the ray-march kernel's compiled variants the
 *                context's most recent cvr_render_rc1pass[_frames] launched, -1 before the
 *                first: bits 0-3 K (samples per batch, 2 or 4), bit 4 gradient shading,
 *                bit 5 macro-cell skip, bit 6 quad march, bits 8-9 exp (0 CVR-SPEC, 1 the
 *                same without range selects, 2 native), bits 10-11 cell addressing (0
 *                64-bit, 1 buffer offsets, 2 the 24-bit multiply-add form), bits 12-15
 *                filter_bits, bits 16-18 cell_skip.  What the options above resolve to
 *                for the frame (raymarch.hip rc1_resolve_variant holds the rules).
 * One option changes the arithmetic (and so the image) rather than the speed:
 *   "filter_bits" 0: exact float GL_LINEAR weights (CVR-SPEC, the default);
 *                8: every GL_LINEAR weight (volume, gradient, TF; ray_marching_1p.comp:133,
 *                :138; the DOS extinction pyramid, ray_bbox_marching.comp:92-112; the
 *                EBS SAT, ebs_ray_bbox_marching.comp:77-83) rounded to 8 fraction
 *                bits, the fixed-point weights of GPU texture units (CVR-SPEC-8).
 *                cvr_render_extbsd needs sat_layout 0 for it. */
cvr_status  cvr_set_option(cvr_ctx* ctx, const char* key, int value);
int         cvr_get_option(const cvr_ctx* ctx, const char* key);
cvr_status  cvr_synchronize(cvr_ctx* ctx);

/* State setters (cvr_set_volume*, cvr_set_transfer_function, cvr_set_gradient,
 * cvr_set_extinction_volume, cvr_set_extinction_sat, and the cone-table upload
 * inside cvr_render_dosct when its cone parameters change) first drain the
 * WHOLE device (hipDeviceSynchronize): frames already issued on any stream --
 * the caller may rotate several non-blocking streams -- finish with the old
 * state, and frames issued after the call see the new one (the ordering GL
 * gives the reference's Init after a TF change, renderingmanager.cpp:1050-1127).
 * The per-cell skip flags a new volume or TF needs are rebuilt lazily by the
 * next frame; if their scratch (2 B per cell) cannot be allocated, that frame
 * and the following ones render without the skip (the same pixels) until the
 * next state change. */

/* Volume: x-fastest voxels (i + j*w + k*w*h), 1 byte (u8) or 2 bytes (u16)
 * per voxel, normalised as v/255 or v/65535 (structuredgridvolume.cpp:121-151)
 * and stored with GL_R16F semantics.  The data is copied (host pointer). */
cvr_status  cvr_set_volume(cvr_ctx* ctx, const void* voxels, int bytes_per_voxel,
                           int w, int h, int d, const float scale[3]);
/* Same, from a device pointer that stays owned by the caller. */
cvr_status  cvr_set_volume_device(cvr_ctx* ctx, const void* d_voxels, int bytes_per_voxel,
                                  int w, int h, int d, const float scale[3]);

/* Transfer function as n entries of (r, g, b, extinction) floats, i.e. the
 * data GenerateTexture_1D_RGBt uploads; stored with GL_RGBA16F semantics and
 * sampled linearly at x = v*n - 0.5, clamp-to-edge. */
cvr_status  cvr_set_transfer_function(cvr_ctx* ctx, const float* rgbt, int n);

/* Gradient volume for Blinn-Phong.  0 = none, 1 = finite differences
 * (GenerateGradientTexture defaults: sample size 1, no filter, normalised),
 * 2 = Sobel-Feldman (GenerateSobelFeldmanGradientTexture, unnormalised). */
#define CVR_GRADIENT_NONE 0
#define CVR_GRADIENT_FINITE_DIFFERENCES 1
#define CVR_GRADIENT_SOBEL_FELDMAN 2
cvr_status  cvr_set_gradient(cvr_ctx* ctx, int mode);

/* Device bytes held by the context (volume layouts, TF, gradient, ...). */
size_t      cvr_device_bytes(const cvr_ctx* ctx);

/* Copy the volume's cell grid back (diagnostics and tests): (W+1)(H+1)(D+1)
 * cells, x-fastest, 16 B each = the 8 R16F corners GL_LINEAR reads for a
 * sample in the cell.  The corners' sign bits carry the per-cell skip flags of
 * the current TF (option "cell_skip").  No reference counterpart:
 * the reference keeps the volume in a GL_R16F texture (utils.cpp:20-56). */
cvr_status  cvr_copy_cells(cvr_ctx* ctx, void* out, size_t capacity);

/* ----------------------------------------------------------------------------
 * Rendering
 * -------------------------------------------------------------------------- */
/* Number of tiles rank `rank` owns under the split described by `frame`. */
int         cvr_tiles_for_rank(const cvr_frame* frame, int rank);

cvr_status  cvr_render_rc1pass(cvr_ctx* ctx, const cvr_frame* frame,
                               const cvr_rc1pass_params* params, const cvr_output* out);

/* nframes frames (1..16) in ONE ray-march launch: frames[i] is rendered into
 * outs[i] exactly as nframes calls of cvr_render_rc1pass would render it (same
 * pixels, same per-pixel counts).  The frames share the viewport and the screen
 * split (width, height, tile_size, rank, nranks) and may differ in camera; the
 * outputs are device buffers of one format.  outs[0].total (if set) receives the
 * samples of all the frames; the other totals must be NULL.  One launch holds
 * nframes x the waves of a frame, so the tail of one frame's longest rays
 * overlaps the next frame's, and the host pays one call.  The
 * launch order learned on frame 0's view is used when every frame is within
 * "stale_deg" of it.  No reference counterpart: the reference draws one frame
 * per Redraw (rc1prenderer.cpp:100-151); this is the batch form of that call. */
cvr_status  cvr_render_rc1pass_frames(cvr_ctx* ctx, const cvr_frame* frames, int nframes,
                                      const cvr_rc1pass_params* params, const cvr_output* outs);

/* Extinction-coefficient mip pyramid of the current volume for the DOS
 * renderer (ExtinctionCoefficientVolume, extcoefvolumegenerator.cpp:230-408): level 0 at
 * res (NULL: 128^3) is a 7^3 Gaussian (sigma0, default 1) of the opacity TF
 * over the volume, level L the sigma 2^L Gaussian of level L-1 at res >> L,
 * each stored R16F and converted to tau = -log(1 - opacity).  tf_rgba is the
 * RGBA TF (GenerateTexture_1D_RGBA, alpha = opacity), n entries. */
cvr_status  cvr_set_extinction_volume(cvr_ctx* ctx, const float* tf_rgba, int n,
                                      const int res[3], float sigma0);
/* Copy level `level` back as float (NULL out: dims / level count only). */
cvr_status  cvr_copy_extinction_level(cvr_ctx* ctx, int level, float* out, int dims[3],
                                      int* n_levels);

/* One directional-occlusion frame: the ray-march of cvr_render_rc1pass with
 * each sample shaded by cone-traced ambient occlusion and/or a cone shadow
 * toward the light.  Needs cvr_set_extinction_volume. */
cvr_status  cvr_render_dosct(cvr_ctx* ctx, const cvr_frame* frame,
                             const cvr_dos_params* params, const cvr_output* out);

/* ----------------------------------------------------------------------------
 * Pre-illumination of the DOS renderer: the reference's "Use Pre-Illumination"
 * switch (PreIlluminationStructuredVolume, cppvolrend/utils/preillumination.cpp;
 * dosrcrenderer.cpp:63-64, 134-143, 555-655).  The occlusion and shadow cones are
 * traced once per voxel of a small object-space grid, the LIGHT CACHE
 * (rc1pdosct/lightcachecomputation.comp:523-547; 32^3 in the reference), stored
 * as an RG16F image: per voxel two binary16 values (Idao, Idcs), x-fastest, 4
 * bytes per voxel.  The march (_common_shaders/obj_ray_marching.comp:211-333)
 * then shades each sample with ONE GL_LINEAR fetch of that image in place of two
 * cone traces, and composites a sample only when occlusion or shadow is on.  An
 * approximation, in the reference too: the image differs from cvr_render_dosct's
 * (DESIGN.md §5b′ gives SSIM per cache resolution).  A new volume, transfer
 * function, extinction pyramid or SAT drops the cache.  Group contexts
 * (cvr_create_group) refuse these calls with CVR_ERR_STATE.
 * -------------------------------------------------------------------------- */

/* PreComputeLightCache: fills a cache of dims[3] voxels (each in [2, 512]) with
 * the cones of `params` seen from frame->camera (the eye and its up vector reach
 * the occlusion cones only), queued on the context stream.  Needs the volume, the
 * TF and cvr_set_extinction_volume (else CVR_ERR_STATE).  Honours filter_bits;
 * with option native_exp set it returns CVR_ERR_ARG (the cache has no tolerance
 * form). */
cvr_status  cvr_compute_light_cache_dosct(cvr_ctx* ctx, const cvr_frame* frame,
                                          const cvr_dos_params* params, const int dims[3]);
/* Upload a cache computed elsewhere (tests, or a producer of the caller's own):
 * 2 * dims[0] * dims[1] * dims[2] binary16 values.  The library's two producers
 * are cvr_compute_light_cache_dosct and cvr_compute_light_cache_extbsd; all
 * three fill the one cache object of the context, which cvr_render_preillum
 * marches over.  An uploaded cache is never taken for a computed one: the next
 * cvr_render_dosct_preillum / cvr_render_extbsd_preillum computes its own. */
cvr_status  cvr_set_light_cache(cvr_ctx* ctx, const uint16_t* rg_half, const int dims[3]);
/* Copy the cache back after draining the context stream; capacity counts
 * binary16 values.  out = NULL: dims only. */
cvr_status  cvr_copy_light_cache(cvr_ctx* ctx, uint16_t* out, size_t capacity, int dims[3]);
/* The cached march over whatever cache is set (CVR_ERR_STATE without one); of
 * `params` it reads the step, the Blinn-Phong constants, the light position and
 * the occlusion / shadow switches.  Outputs and counts as cvr_render_dosct. */
cvr_status  cvr_render_preillum(cvr_ctx* ctx, const cvr_frame* frame,
                                const cvr_dos_params* params, const cvr_output* out);
/* RC1PConeTracingDirOcclusionShading::Update with the switch on: compute, then
 * march.  The compute is skipped while nothing the cache depends on has changed
 * since this context last computed it: the volume, the pyramid, dims, the
 * switches, filter_bits, the parameters of a cone that is on, the light (shadow
 * on), the eye and camera up (occlusion on).  A shadow-only cache therefore
 * survives camera motion.  cvr_get_option(ctx, "light_cache_builds") counts the
 * computes of a context. */
cvr_status  cvr_render_dosct_preillum(cvr_ctx* ctx, const cvr_frame* frame,
                                      const cvr_dos_params* params, const int dims[3],
                                      const cvr_output* out);

/* Extinction summed-area table of the current volume for the EBS renderer
 * (GenerateExtinctionSAT3DTex, ebsrenderer.cpp:624-716): a (W+2)(H+2)(D+2)
 * grid, zero on its border, holding ext_lut[voxel] inside, summed in double
 * exactly as SummedAreaTable3D<double>::BuildSAT and stored as float.
 * ext_lut: GetExtN(v / (2^bits - 1)) for every voxel value v (256 entries for
 * 8-bit volumes, 65536 for 16-bit; cvr_tf1d_ext_lut builds it). */
cvr_status  cvr_set_extinction_sat(cvr_ctx* ctx, const float* ext_lut, int lut_n);
/* Copy the float SAT back (x-fastest); out = NULL: dims only. */
cvr_status  cvr_copy_extinction_sat(cvr_ctx* ctx, float* out, size_t capacity, int dims[3]);

/* Host check of the SAT fetch addressing (no device work): for a SAT of
 * sat_dims = (W+2, H+2, D+2) texels in `layout` (0 = cell4 copy, 1 = the plain
 * float SAT; option "sat_layout"), evaluates every load of a fetch at every
 * clamped corner texel with the kernels' own index arithmetic and reports
 * out[0] = one past the last byte read, out[1] = bytes the library allocates
 * for that layout, out[2] = 1 if any 24-bit operand or 32-bit index would
 * wrap, out[3] = 1 if the addressing is safe (out[0] <= out[1] and no wrap).
 * pad_planes < 0 = the library's padding; >= 0 evaluates another padding (the
 * round-3 variant's one plane: tests/test_ebs.py).  No reference counterpart:
 * the reference samples the SAT through a GL texture (ebsrenderer.cpp:700-716). */
cvr_status  cvr_sat_layout_check(const int sat_dims[3], int layout, int pad_planes,
                                 unsigned long long out[4]);

/* One extinction-based shading frame: the ray-march with each sample shaded by
 * a SAT ambient occlusion and a SAT box-chain shadow.  Needs
 * cvr_set_extinction_sat. */
cvr_status  cvr_render_extbsd(cvr_ctx* ctx, const cvr_frame* frame,
                              const cvr_ebs_params* params, const cvr_output* out);

/* ----------------------------------------------------------------------------
 * Pre-illumination of the EBS renderer: the same switch (ebsrenderer.cpp:46-47)
 * and the same cache object and march as the DOS renderer's above.  The SAT
 * ambient occlusion and the SAT box-chain shadow are evaluated once per voxel
 * of the light cache (rc1pextbsd/lightcachecomputation.comp), at the voxel
 * centre, with the arithmetic of cvr_render_extbsd's shader; the march then
 * fetches the cache once per sample.  Neither term reads the camera (the boxes
 * are centred on the voxel, the chain points at the light), so an EBS cache
 * survives every camera motion.  A new volume, transfer function or SAT drops
 * the cache.  Group contexts refuse these calls with CVR_ERR_STATE.
 * -------------------------------------------------------------------------- */

/* PreComputeLightCache: fills a cache of dims[3] voxels (each in [2, 512]) with
 * the occlusion and shadow of `params`, queued on the context stream.  It takes
 * no frame: nothing camera-dependent reaches the cache.  Needs the volume and
 * cvr_set_extinction_sat (else CVR_ERR_STATE).  Honours sat_layout and
 * filter_bits as cvr_render_extbsd does (filter_bits 8 with sat_layout 1 is
 * CVR_ERR_ARG); with option native_exp set it returns CVR_ERR_ARG, as the DOS
 * compute.  Counted by "light_cache_builds". */
cvr_status  cvr_compute_light_cache_extbsd(cvr_ctx* ctx, const cvr_ebs_params* params,
                                           const int dims[3]);
/* RC1PExtinctionBasedShading::Update with the switch on: compute, then march
 * (cvr_render_preillum's march, fed the step, the Blinn-Phong constants,
 * light_pos and the two switches of `params`).  The compute is skipped while
 * none of these changed since this context last computed: the producer (a DOS
 * compute in between counts), the volume, the SAT, dims, the two switches,
 * filter_bits, the occlusion parameters (occlusion on), the shadow parameters
 * and light_pos (type 0) or light_forward (type 1) (shadow on).  The camera is
 * not among them: an orbit around a fixed light computes once. */
cvr_status  cvr_render_extbsd_preillum(cvr_ctx* ctx, const cvr_frame* frame,
                                       const cvr_ebs_params* params, const int dims[3],
                                       const cvr_output* out);

/* ----------------------------------------------------------------------------
 * Ground-truth cone ray-caster: RC1PConeLightGroundTruthSteps ("1-Pass - Ray
 * Casting - Cone Ground Truth (Steps)", s_1rc_gt_c; cppvolrend/structured/
 * rc1pcrtgt/crtgtrenderer.cpp, gt_ray_marching.comp).  The yardstick of the DOS
 * and EBS approximations: the march of cvr_render_rc1pass with every sample of
 * alpha > 0 shaded by brute force, a bundle of secondary rays marched through
 * the volume and the transfer function toward the eye (cone occlusion, :109-169)
 * and a second bundle toward the light (cone shadow, :171-252); a ray's
 * transmittance is the trapezoid rule over the TF's extinction at light_step
 * intervals, starting light_gap away from the sample and stopping at the box,
 * at the term's distance or at 99 % opacity, and a term is the mean of its rays'
 * transmittances weighted by the cosine to the cone axis.  ShadeSample (:254-302)
 * combines them as the DOS renderer does, with a white specular term.
 *
 * As written in the shader, the spot shadow (shadow_type 1) tests
 * dot(v_dir, LightCamForward) < 30.0, which always holds: its shadow term is 0.0
 * for every sample.  That is reproduced, as the (u, v) swap of the DOS shadow is.
 *
 * The frame is progressive, as in the reference, whose Redraw takes one sample per
 * pixel: cvr_crtgt_begin resets a per-pixel state held by the context (ray
 * parameter s, RGBA, iteration count, done flag: 32 bytes per pixel), and each
 * cvr_crtgt_advance extends every unfinished ray.  Unlike the reference, which
 * parks s and the colour in RG16F / RGBA16F images between dispatches, the state
 * is float: the converged frame is the shader's arithmetic carried through in
 * float and does not depend on how the march was cut into calls, and a pixel
 * whose box lies behind the eye (D <= 0) is finished at once (DESIGN.md 5d').
 * A new volume, transfer function or gradient invalidates the state.  Honours
 * filter_bits; with option native_exp set these calls return CVR_ERR_ARG.  Group
 * contexts (cvr_create_group) refuse them with CVR_ERR_STATE.
 * -------------------------------------------------------------------------- */
#define CVR_CRTGT_MAX_RAYS 10000      /* the reference UI's bound on either table      */
#define CVR_CRTGT_MAX_RAY_STEPS 65536 /* most light_step intervals one secondary ray
                                         may take, (distance - light_gap) / light_step */
typedef struct cvr_crtgt_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale| (crtgtrenderer.cpp:107-108) */
  int   apply_gradient_shading;/* m_apply_gradient (needs cvr_set_gradient)             */
  float ka, kd, ks, shininess; /* Blinn-Phong constants (renderingparameters.cpp:23-26) */
  cvr_light light;             /* the current light source (forward = -LightCamForward) */
  float light_gap, light_step; /* LightRayInitialGap 1.0, LightRayStepSize 0.5 (> 0)    */
  int   apply_occlusion;       /* m_apply_occlusion (default 0)                         */
  float occ_distance;          /* OccConeDistanceEvaluation; <= 0: diagonal * 0.50      */
  int   apply_shadow;          /* m_apply_shadows (default 0)                           */
  float sdw_distance;          /* SdwConeDistanceEvaluation; <= 0: diagonal * 0.75      */
  int   shadow_type;           /* 0 point, 1 spot, 2 directional                        */
} cvr_crtgt_params;
/* The reference's defaults (crtgtrenderer.cpp:23-51, 107-113): step 0 (the default
 * step), no Phong, (0.5, 0.5, 0.8, 30), light 0 of the reference's light list, gap
 * 1.0, step 0.5, both terms off with distance 0 (the diagonal fractions), type 0. */
void        cvr_crtgt_params_default(cvr_crtgt_params* out);
/* The two ray tables of Update (:131-184), n x (r, g, b) floats each (out_occ /
 * out_sdw may be NULL when its n is 0).  Touches no device.  One generator is drawn
 * for the occlusion table first and then for the shadow table: per ray u1, u2 with
 * theta = u1 * (pi * (aperture / 180)), phi = u2 * (pi * (360 / 180)) in float, and
 * the vector Rodrigues(Rodrigues((0,0,1), theta, (0,1,0)), phi, (0,0,1)).  The
 * reference's std::default_random_engine is platform-defined; this one is
 * minstd_rand0: x <- 16807 x mod (2^31 - 1), x0 = seed (0 -> 1), and
 * u = (float)((double)(x - 1) / 2147483646.0).  n in [0, CVR_CRTGT_MAX_RAYS]. */
cvr_status  cvr_crtgt_build_rays(float occ_aperture_deg, int n_occ, float sdw_aperture_deg,
                                 int n_sdw, unsigned seed, float* out_occ, float* out_sdw);
/* Resets the per-pixel state for `frame` (a whole frame: nranks <= 1, else
 * CVR_ERR_ARG) and keeps the parameters and the two ray tables (stored with RGB16F
 * semantics: every coefficient rounded to binary16, as SetData(GL_RGB16F) +
 * texelFetch).  n must be in [1, CVR_CRTGT_MAX_RAYS] for a term that is on (the
 * reference's UI allows 0, which divides 0 by 0); the table of a term that is off
 * is not read.  Needs the volume and the TF, and the gradient with Phong on (else
 * CVR_ERR_STATE).  light_step must be > 0 and large enough to advance a float at
 * the term's distance, and a ray may take at most CVR_CRTGT_MAX_RAY_STEPS steps.
 * Device memory, all counted by cvr_device_bytes: 32 B per pixel of state, 24 B of
 * counters, the two tables (12 B per ray, at least one ray), and the job storage of one launch round, which shades at
 * most 4 samples per pixel: 4 x (36 B, or 52 B with Phong) per pixel. */
cvr_status  cvr_crtgt_begin(cvr_ctx* ctx, const cvr_frame* frame, const cvr_crtgt_params* params,
                            const float* occ_rays, int n_occ, const float* sdw_rays, int n_sdw);
/* Extends every unfinished ray by at most max_samples (>= 1) loop iterations, in
 * launch rounds of at most 4 iterations per pixel (the bound of the job storage),
 * and stops early once every pixel is done.  Writes the current image and counts to
 * `out` (NULL: no copy; host or device pointers, either format; total: the sum of the
 * counts so far -- added to a device total, as every renderer does).  Reports the
 * pixels still unfinished; 0 = converged, after which the call only copies.  Blocks
 * until the rounds are done.  CVR_ERR_STATE without a cvr_crtgt_begin, and after a
 * new volume, transfer function or gradient. */
cvr_status  cvr_crtgt_advance(cvr_ctx* ctx, int max_samples, const cvr_output* out,
                              unsigned long long* unfinished_pixels);
/* cvr_crtgt_begin, then cvr_crtgt_advance until converged. */
cvr_status  cvr_render_crtgt(cvr_ctx* ctx, const cvr_frame* frame, const cvr_crtgt_params* params,
                             const float* occ_rays, int n_occ, const float* sdw_rays, int n_sdw,
                             const cvr_output* out);

/* ----------------------------------------------------------------------------
 * Voxel cone tracing (RC1PVoxelConeTracingSGPU, "1-Pass - Ray Casting - Voxel Cone
 * Tracing", s_1rc_vct: rc1pvctsg/vctrenderer.cpp, preprocessingstages.cpp,
 * vct_ray_bbox_marching.comp).  The march of cvr_render_rc1pass with every sample
 * of alpha > 0 shaded by one cone toward the light (:97-144): up to `samples`
 * quadrilinear fetches of a (mean, standard deviation) supervoxel pyramid of the
 * volume, each mapped to an opacity by a 2-D pre-integration table of the transfer
 * function, the transmittances multiplied.  ShadeSample (:146-189) has no occlusion
 * term: ka is Kambient with apply_occlusion on, kd / ks are nonzero with
 * apply_shadow on, and with both off the colour is 0 * (1 / 0) = NaN, as written.
 * corr_fact is apply_correction * correction_factor, so with the correction off the
 * exponent is 0 and every shadow vanishes (pow(x, 0) = 1, also for x = 0), as written.
 *
 * Scope: 1-byte volumes only (the reference scales the mean by a hard-coded 255 but
 * normalises 16-bit data by 65535: a 2-byte volume returns CVR_ERR_ARG).  A volume
 * whose maximum standard deviation is 0 (constant over every 2x2x2 block of every
 * level) gives a table of height 0 and returns CVR_ERR_ARG.  A mipmap level at or
 * above the last computed one reads the last level only (the reference uploads no
 * level beyond it).  The object-space light-cache mode (lightcachecomputation.comp)
 * is not built.  Honours filter_bits; with native_exp set the calls return
 * CVR_ERR_ARG.
 *
 * The pyramid depends on the volume only; the table on the volume (its height) and
 * on the opacities of cvr_vct_set_opacity.  cvr_set_volume drops both;
 * cvr_set_transfer_function drops the table and the opacities (they belong to the
 * old TF), so the next frame needs a new cvr_vct_set_opacity and rebuilds only the
 * table.  Device memory, counted by cvr_device_bytes once built: 4 B per texel of
 * every pyramid level (level i has floor(dim / 2^i) texels per axis), 640 B of level
 * addressing, 2 B x 255 x ceil(max_stddev) of table, and 96 B per cone sample of the
 * last frame's cone schedule (at least one sample).
 * -------------------------------------------------------------------------- */
#define CVR_VCT_MAX_LEVELS 16
#define CVR_VCT_MAX_SAMPLES 10000     /* the reference UI's bound                      */
#define CVR_VCT_TABLE_WIDTH 255       /* ceil(GetMaxDensity()) of a 1-byte volume      */
typedef struct cvr_vct_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale| (vctrenderer.cpp:114-115)   */
  int   apply_gradient_shading;/* m_apply_gradient_shading (needs cvr_set_gradient)     */
  float ka, kd, ks, shininess; /* Blinn-Phong constants (renderingparameters.cpp:23-26) */
  float ispecular[3];          /* Ispecular                                             */
  cvr_light light;             /* the current light source (its position is read)       */
  int   apply_occlusion;       /* apply_ambient_occlusion (default 1)                   */
  int   apply_shadow;          /* apply_voxel_cone_tracing (default 1)                  */
  float cone_step;             /* cone_step_size (2.0, world units, > 0)                */
  float cone_step_increase_rate; /* cone_step_size_increase_rate (1.0, >= 1)            */
  float cone_initial_step;     /* cone_initial_step (2.0)                               */
  float cone_apex_angle_deg;   /* cone_apex_angle (2.0, in (0, 90))                     */
  int   apply_correction;      /* apply_correction_factor (default 1)                   */
  float correction_factor;     /* opacity_correction_factor (2.0)                       */
  int   samples;               /* cone_number_of_samples (50, in [0, CVR_VCT_MAX_SAMPLES]) */
} cvr_vct_params;
/* The reference's defaults (vctrenderer.cpp:33-43): step 0 (the default step), no
 * Phong, (0.5, 0.5, 0.8, 30), white specular, light 0 of the reference's light list. */
void        cvr_vct_params_default(cvr_vct_params* out);
typedef struct cvr_vct_pyramid_info {
  int    levels;                          /* 0: not built                              */
  int    dims[CVR_VCT_MAX_LEVELS][3];
  double max_stddev;                      /* maximum_standard_deviation                */
  int    table_width, table_height;       /* 255 x ceil(max_stddev); height 0: no table */
} cvr_vct_pyramid_info;
/* TransferFunction1D::GetOpc(i, 255) for i = 0 .. 254 (transferfunction1d.cpp:132-167),
 * the opacities the pre-integration table integrates, from the control points of
 * cvr_tf1d_build_rgbt.  n must be CVR_VCT_TABLE_WIDTH.  Touches no device. */
cvr_status  cvr_tf1d_opacity_lut(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                                 int max_density, int n, float* out_opacity);
/* The opacities of the current transfer function (n = CVR_VCT_TABLE_WIDTH); drops
 * the table. */
cvr_status  cvr_vct_set_opacity(cvr_ctx* ctx, const float* opacity, int n);
/* Builds what is stale: the pyramid (PreProcessSuperVoxels, preprocessingstages.cpp
 * :35-145, on the GPU in double) and, when the opacities are set, the table
 * (PreProcessPreIntegrationTable, :147-202, on the host in double).  Idempotent.
 * Option "vct_pyramid_builds" (read-only) counts the pyramid builds. */
cvr_status  cvr_vct_precompute(cvr_ctx* ctx);
cvr_status  cvr_vct_info(cvr_ctx* ctx, cvr_vct_pyramid_info* out);
/* Level `level` as w*h*d (mean, stddev) pairs, x fastest, and the table as
 * table_height rows of 255: the stored binary16 values widened to float. */
cvr_status  cvr_vct_read_pyramid(cvr_ctx* ctx, int level, float* out_rg);
cvr_status  cvr_vct_read_table(cvr_ctx* ctx, float* out);
/* One frame; builds whatever is stale first.  Screen tiles (cvr_frame rank / nranks)
 * and group contexts as cvr_render_dosct.  CVR_ERR_STATE without a volume, a TF, the
 * opacities, or (with Phong) a gradient; CVR_ERR_ARG for samples outside
 * [0, CVR_VCT_MAX_SAMPLES], cone_step <= 0, an increase rate < 1 or an angle outside
 * (0, 90). */
cvr_status  cvr_render_vct(cvr_ctx* ctx, const cvr_frame* frame, const cvr_vct_params* params,
                           const cvr_output* out);

/* ----------------------------------------------------------------------------
 * Slice-based directional occlusion (SBTMDirectionalOcclusionShading, "Slice-based -
 * Directional Occlusion", s_sbtm_dos: structured/sbtmdos/sbtmdosrenderer.cpp,
 * evaluationslice.vert / .frag).  Schott et al.'s original algorithm, of which
 * cvr_render_dosct, cvr_render_extbsd and cvr_render_vct are the ray-casting
 * approximations: view-aligned slices front to back, each a 2-D pass over the
 * screen that composites its sample into an RGBA16F eye buffer, weighted by an
 * occlusion buffer, and writes the next occlusion buffer as the mean of grid_x x
 * grid_y bilinear taps of the previous one inside the cone's footprint, attenuated
 * by the sample's extinction (DESIGN.md 5d''' holds the arithmetic).  The reference
 * rasterises the slices; here every fragment is the point of its pixel's view ray
 * at the slice's depth, so a slice is a kernel over the screen.
 *
 * Reproduced as written: every slice is drawn with slice 0's quad moved by
 * cam_dir * pos_from_near, so it lies half a first step deeper than its own centre;
 * the quad's half side is the volume diagonal in voxels, unscaled, so a scaled
 * volume can stick out of it; a pixel whose fragment is discarded keeps, in the
 * occlusion buffer being written, the value of two slices earlier, which its
 * neighbours then read; a slice outside [z_near, z_far] is a pass that discards
 * every fragment; a camera looking along (0, 1, 0) has a NaN quad and a transparent
 * black frame.  No early ray termination, no light, no gradient.
 *
 * The pixels of a frame depend on their neighbours, so a frame is whole: screen
 * tiles (cvr_frame nranks > 1) and group contexts (cvr_create_group), which would
 * cut the screen into independent shares, return CVR_ERR_ARG.  Honours filter_bits (the
 * volume, TF and occlusion-buffer fetches); with native_exp set the call returns
 * CVR_ERR_ARG.  Device memory, counted by cvr_device_bytes from the first frame to
 * the next volume or transfer function: 16 B per pixel (the RGBA16F eye buffer and
 * two sets of the two R16F occlusion buffers: a launch of several slices reads one
 * set and writes the other).
 *
 * Options: "sbtm_slices_per_launch" (1..16): slices one kernel launch advances with
 * the occlusion buffers of its screen tile and a halo in LDS; a batch whose halo
 * does not fit runs one launch per slice.  Every value gives the same bits.
 * Read-only after a frame: "sbtm_slices" (slices drawn) and "sbtm_launches" (slice
 * kernel launches).
 * -------------------------------------------------------------------------- */
#define CVR_SBTM_MAX_GRID 16          /* taps per axis                                 */
#define CVR_SBTM_MAX_SLICES 1000000   /* slices the step may cut [minimum_z, maximum_z] into */
typedef struct cvr_sbtm_params {
  float step;                  /* <= 0: 0.5/sqrt(3)*|scale| (sbtmdosrenderer.cpp:112)   */
  float cone_half_angle_deg;   /* cone_half_angle (50, in (0, 90))                      */
  int   grid_x, grid_y;        /* grid_size (2 x 2, in [1, CVR_SBTM_MAX_GRID])          */
  float attenuation;           /* occ_ui_weight_percentage (1.0, in [0, 1])             */
  int   max_passes;            /* max_number_of_passes (90000, >= 0)                    */
  float z_near, z_far;         /* the camera's clip planes (1, 5000; 0 < near <= far)   */
} cvr_sbtm_params;
void        cvr_sbtm_params_default(cvr_sbtm_params* out);
/* One frame.  samples: per pixel, the fragments kept (neither clipped nor
 * discarded); total: their sum.  CVR_ERR_STATE without a volume or a TF;
 * CVR_ERR_ARG for a parameter out of its range, a step that cannot advance a float
 * at maximum_z or cuts more than CVR_SBTM_MAX_SLICES slices, and screen tiles. */
cvr_status  cvr_render_sbtm(cvr_ctx* ctx, const cvr_frame* frame, const cvr_sbtm_params* params,
                            const cvr_output* out);
/* The two occlusion buffers as the last frame left them: 2 planes of width x height
 * floats (the stored binary16 values widened), plane 0 first; blocks.  CVR_ERR_STATE
 * without a frame since the last volume or transfer function, CVR_ERR_ARG when width x
 * height is not that frame's viewport. */
cvr_status  cvr_sbtm_read_occlusion(cvr_ctx* ctx, int width, int height, float* out);

/* ----------------------------------------------------------------------------
 * DeferredShading ("Deferred Rendering", abbreviation "iso"; cppvolrend/structured/
 * DeferredShading): a first-hit isosurface march that stores the hit's texture-space
 * position and central-difference normal into a G-buffer (geometry_pass.comp), a
 * Blinn-Phong pass over the G-buffer (lighting_pass.comp) and a tone map
 * (post_process.frag).  The G-buffer belongs to the context, so a change of light,
 * material, colour, exposure or gamma re-shades the kept frame without marching a ray
 * (cvr_deferred_shade).
 *
 * Reproduced as written: a ray that misses the box keeps the G-buffer's
 * clear value (gbuffer_clear, the application's (1, 1, 1, 0)) and is then LIT with the
 * unnormalised normal (1, 1, 1); normalize of a zero gradient is NaN and is stored;
 * the lighting pass mixes the texture-space position with the world-space light and
 * eye; it samples the G-buffer with GL_NEAREST at pixel / size, a texel edge, which for
 * some sizes is the texel to the left or below (CVR-SPEC:
 * clamp(int(floor(fl(fl(p / s) * s))), 0, s - 1) in float).  A lane stops after 2^22
 * iterations (iso.hip's deviation).
 *
 * A pixel may read its neighbour's G-buffer texel, so a frame is whole: screen tiles
 * (cvr_frame nranks > 1) and group contexts return CVR_ERR_ARG.  Device memory, counted
 * by cvr_device_bytes from the first geometry pass to the next volume: 32 B per pixel.
 * Read-only options: "deferred_hits" (pixels with a hit in the last geometry pass;
 * reading it waits for that pass) and "deferred_launches" (geometry launches so far).
 * -------------------------------------------------------------------------- */
typedef struct cvr_deferred_params {
  float isovalue;              /* m_u_isovalue 0.5                                       */
  float step_small;            /* m_u_step_size_small 0.05 (> 0)                          */
  float step_large;            /* m_u_step_size_large 1.0 (> 0)                           */
  float step_range;            /* m_u_step_size_range 0.1 (> 0)                           */
  int   num_blocks[3];         /* numBlocks (4, 4, 4), DeferredShading.cpp:348; 1..1024   */
  float color[4];              /* m_u_color (0.66, 0.6, 0.05, 1.0): objectColor           */
  float ka, kd, ks, shininess; /* the values Update binds (renderingparameters.cpp:23-26:
                                  0.5, 0.5, 0.8, 30); LightingPass's 0.1 / 0.7 / 0.2 / 32
                                  are stored after the last BindUniforms and never bound  */
  float light_color[3];        /* lightColor (1, 1, 1), bound from the second Update on   */
  float light_pos[3];          /* LightSourcePosition (light 0 of the reference's list)   */
  float exposure;              /* 1.0 (Redraw); <= 0: no exposure map                     */
  float gamma;                 /* 2.2 (Redraw); <= 0: no gamma map                        */
  float gbuffer_clear[4];      /* glClear's colour (1, 1, 1, 0), renderingmanager.cpp:108 */
} cvr_deferred_params;
void        cvr_deferred_params_default(cvr_deferred_params* out);
/* One frame: the geometry pass, then the shade pass, on the context stream with no
 * host synchronisation between them.  samples: per pixel, the texture(TexVolume)
 * evaluations of the geometry pass; total: their sum.  CVR_ERR_STATE without a volume;
 * CVR_ERR_ARG for screen tiles, a group context, a step that is not positive, a
 * negative material, colour or light-colour term, a NaN parameter, or a block count
 * outside 1..1024. */
cvr_status  cvr_render_deferred(cvr_ctx* ctx, const cvr_frame* frame, const cvr_deferred_params* params,
                                const cvr_output* out);
/* The geometry pass alone: marches `frame` and keeps the G-buffer (asynchronous). */
cvr_status  cvr_deferred_geometry(cvr_ctx* ctx, const cvr_frame* frame, const cvr_deferred_params* params);
/* The shade pass alone over the kept G-buffer (the relight path): only the lighting,
 * material, colour and tone-map fields of `params` are read; the camera eye is the kept
 * frame's; samples and total are the kept geometry pass's.  The output's size is the
 * G-buffer's: width x height pixels.  CVR_ERR_STATE without a G-buffer, CVR_ERR_ARG
 * when width x height is not its viewport. */
cvr_status  cvr_deferred_shade(cvr_ctx* ctx, int width, int height, const cvr_deferred_params* params,
                               const cvr_output* out);
/* gPosition and gNormal of the kept G-buffer, width x height x 4 floats each; blocks.
 * CVR_ERR_STATE without a G-buffer, CVR_ERR_ARG for another viewport. */
cvr_status  cvr_deferred_read_gbuffer(cvr_ctx* ctx, int width, int height, float* out_position,
                                      float* out_normal);

/* ----------------------------------------------------------------------------
 * AdvancedDeferredShading ("Advanced Deferred Rendering", abbreviation "iso";
 * cppvolrend/structured/AdvancedDeferredShading): DeferredShading's geometry pass and
 * tone map, with a screen-space curvature pass over the G-buffer's normals
 * (curvature_pass.comp: principal curvatures k1, k2 and the projected direction of k1)
 * and a feature-lighting pass (lighting_pass.comp: Blinn-Phong, accessibility shading,
 * a curvature colour map, ridge and valley lines, a curvature "flow" term) between
 * them.  The G-buffer is the context's own (cvr_deferred_geometry fills the same one);
 * the curvature planes are kept next to it, valid for one G-buffer and one pair of
 * projection scales: any geometry pass invalidates them.
 *
 * Where the reference leaves the result undefined: texel lookups are
 * floor(fl(u * size)) wrapped modulo size (GL_NEAREST, GL_REPEAT), texel 0 for a
 * coordinate that is not finite; the curvature direction's angle is never formed (cos
 * and sin are the normalised (k1 - A00, A01), (1, 0) for a zero vector); screenSize and
 * time, which the application never sets, are parameters.  A negative discriminant
 * gives NaN curvatures, which are stored and compare false everywhere.
 *
 * Whole frames only, like cvr_render_deferred.  Device memory, counted by
 * cvr_device_bytes: 16 B per pixel for the curvature planes (from the first curvature
 * pass to the next volume or viewport) and 260 KiB for the two tables (from the first
 * lighting pass to the context's end).  Read-only options:
 * "advdeferred_curvature_launches" (curvature launches so far) and
 * "advdeferred_ridge_pixels" (pixels of the last lighting pass whose feature colour has
 * red or green set, after show_ridges / show_valleys; reading it waits for that pass;
 * -1 before the first).
 * -------------------------------------------------------------------------- */
typedef struct cvr_advdeferred_params {
  float isovalue;              /* the march and tone-map fields of cvr_deferred_params     */
  float step_small;
  float step_large;
  float step_range;
  int   num_blocks[3];         /* (4, 4, 4), AdvancedDeferredShading.cpp:561               */
  float color[4];              /* m_u_color: only its alpha reaches the frame (>= 0)       */
  float ka, kd, ks, shininess; /* lighting_pass.comp:200-207's constants 0.1 0.7 0.2 32    */
  float light_color[3];        /* lightColor (1, 1, 1), AdvancedDeferredShading.cpp:380    */
  float light_pos[3];          /* lightPos (light 0 of the reference's list)               */
  float exposure;              /* 1.0 (Redraw :752); <= 0: no exposure map                 */
  float gamma;                 /* 2.2 (Redraw :753); <= 0: no gamma map                    */
  float gbuffer_clear[4];      /* Redraw's glClearColor (1, 1, 1, 1), :724                 */
  float flow_speed;            /* m_flow_speed 1 (AdvancedDeferredShading.h:129)           */
  float flow_scale;            /* m_flow_scale 10 (:130)                                   */
  float time;                  /* m_current_time 0 (constructor :130; never advanced)      */
  int   show_ridges;           /* m_show_ridges true (:131)                                */
  int   show_valleys;          /* m_show_valleys true (:132)                               */
  float accessibility_strength;/* m_accessibility_strength 0.5 (:133)                      */
  float screen_size[2];        /* screenSize, never set by the application (:379 is a
                                  comment): (0, 0); a component <= 0 is the frame's width
                                  or height                                                */
  float colormap_s;            /* s 0.6 (Init :536): the colour map's saturation           */
  float colormap_v;            /* v 0.2 (Init :537): its value                             */
} cvr_advdeferred_params;
void        cvr_advdeferred_params_default(cvr_advdeferred_params* out);
/* One frame: geometry, curvature and lighting pass on the context stream, no host
 * synchronisation between them.  samples and total are the geometry pass's counts.
 * Errors as cvr_render_deferred; also CVR_ERR_ARG for a NaN feature parameter. */
cvr_status  cvr_render_advdeferred(cvr_ctx* ctx, const cvr_frame* frame, const cvr_advdeferred_params* params,
                                   const cvr_output* out);
/* The curvature pass alone over the kept G-buffer, for `frame`'s projection (only its
 * size, fovy_deg and aspect are read; `params` is checked, nothing of it is read).
 * CVR_ERR_STATE without a G-buffer of that size. */
cvr_status  cvr_advdeferred_curvature(cvr_ctx* ctx, const cvr_frame* frame, const cvr_advdeferred_params* params);
/* The lighting pass alone over the kept G-buffer and curvature planes (the relight
 * path): the lighting, feature, colour-map and tone-map fields of `params` are read.
 * CVR_ERR_STATE without valid curvature planes, CVR_ERR_ARG for another viewport. */
cvr_status  cvr_advdeferred_shade(cvr_ctx* ctx, int width, int height, const cvr_advdeferred_params* params,
                                  const cvr_output* out);
/* The kept curvature planes: k1 and k2 (width x height floats each) and the direction
 * (width x height x 2); blocks.  CVR_ERR_STATE without valid planes. */
cvr_status  cvr_advdeferred_read_curvature(cvr_ctx* ctx, int width, int height, float* out_k1, float* out_k2,
                                           float* out_dir);

/* The reference renderers' default parameters for `variant`. */
void        cvr_iso_params_default(int variant, cvr_iso_params* out);
/* One isosurface frame (first hits composited front to back with Color).  The
 * block min/max table (ComputeBlocksFromVolume, rc1custompisoadaptrenderer.cpp
 * :20-117) is built on the GPU when the volume or num_blocks changes. */
cvr_status  cvr_render_iso(cvr_ctx* ctx, const cvr_frame* frame, const cvr_iso_params* params,
                           const cvr_output* out);
/* Copy the current block table back (x-fastest, num_blocks of the last build);
 * builds it first for `num_blocks` when needed.  Empty blocks hold (FLT_MAX,
 * -FLT_MAX) as in the reference. */
cvr_status  cvr_iso_block_ranges(cvr_ctx* ctx, const int num_blocks[3], float* out_min,
                                 float* out_max);

/* Rank-0 side of the screen-tile split: `d_packed` holds nranks consecutive
 * blocks of `tiles_per_rank_max` packed tiles (rank r's block at offset
 * r*tiles_per_rank_max*tile_size^2 pixels); scatter them into the W x H
 * device image `d_rgba`.  Both buffers hold pixels of `format`
 * (CVR_FORMAT_RGBA32F or CVR_FORMAT_RGBA16F).  Asynchronous on the context
 * stream. */
cvr_status  cvr_unpack_tiles_device(cvr_ctx* ctx, const cvr_frame* frame,
                                    const void* d_packed, int tiles_per_rank_max,
                                    int format, void* d_rgba);

/* The same for frame `frame_index` of a grouped exchange: `d_gathered` holds
 * nranks blocks of nframes * tiles_per_rank_max tiles (rank r's frame j at
 * tile slot (r * nframes + j) * tiles_per_rank_max), as cvr_gather_tiles_n
 * leaves it. */
cvr_status  cvr_unpack_tiles_device_n(cvr_ctx* ctx, const cvr_frame* frame,
                                      const void* d_gathered, int tiles_per_rank_max,
                                      int nframes, int frame_index, int format, void* d_rgba);

/* Lossless per-tile code of RGBA16F screen tiles (every world
 * size was bound by rank 0's inbound bytes, and a rendered tile's channels span few
 * bits; the exchange moves this code since round 6).  d_tiles: ntiles tiles of
 * tile x tile RGBA16F pixels, each row-major (the packed layout of a screen-tile
 * share).  The stream, 32-bit words: ntiles + 1 tile starts (the last = the
 * stream's end), then per tile 3 header words (four 16-bit channel bases, four
 * 5-bit widths) and each channel's differences from its base at its width.
 * Every bit pattern round-trips.  cvr_tile_code_bound: the largest stream
 * (bytes) for these sizes (tile 16..64, a multiple of 16; 0 = invalid);
 * cvr_encode_tiles writes the stream and its length (bytes, a device u64) on
 * the context stream; cvr_decode_tiles restores the tiles.  Option "encode_onepass"
 * 1: cvr_encode_tiles runs the exchange's ONE-launch encode instead of three (each
 * tile claims its words with an atomic, so the codes follow in claim order, not
 * tile order; the start table says where each is, the length and the decode are
 * the same).  The multi-rank exchange uses the code (option exchange_code). */
size_t      cvr_tile_code_bound(int tile, int ntiles);
cvr_status  cvr_encode_tiles(cvr_ctx* ctx, const void* d_tiles, int tile, int ntiles,
                             void* d_stream, unsigned long long* d_bytes);
cvr_status  cvr_decode_tiles(cvr_ctx* ctx, const void* d_stream, int tile, int ntiles, void* d_tiles);

/* ----------------------------------------------------------------------------
 * After the march: pixel multiscaling and the screenshot
 * (libs/vis_utils/renderoutputframe.cpp:89-146, 265-539 and its
 * shader/renderoutputframe/ compute shaders; renderingmanager.cpp:103-112,
 * 476-492)
 * -------------------------------------------------------------------------- */

/* BaseVolumeRenderer multiscaling modes (volrenderbase.h:28-33) */
#define CVR_SINGLE_RAY_PER_PIXEL    0
#define CVR_MULTIPLE_RAYS_PER_PIXEL 1
#define CVR_DOWN_SCALING_RENDER     2
#define CVR_UP_SCALING_RENDER       3
/* vis::IMAGE_FILTER_KERNEL (libs/vis_utils/filters/utils.hpp:8-15); K2_HAT is
 * RenderFrameToScreen's default (renderoutputframe.cpp:34) */
#define CVR_FILTER_BOX                0
#define CVR_FILTER_HAT                1
#define CVR_FILTER_CATMULL_ROM        2
#define CVR_FILTER_MITCHELL_NETRAVALI 3
#define CVR_FILTER_CARDINAL_BSPLINE_3 4
#define CVR_FILTER_CARDINAL_OMOMS3    5

/* Render resolution of a mode at screen size (w, h): 2w x 2h for modes 1-2,
 * w/2 x h/2 for mode 3 (UpdateScreenResolutionMultiScaling with the 2 x 2
 * multiplier of cppvolrend/defines.h:16-17). */
cvr_status  cvr_multiscale_resolution(int mode, int screen_w, int screen_h, int* render_w,
                                      int* render_h);

/* Filter a rendered RGBA16F frame (fw x fh, device) to the RGBA16F screen
 * image (sw x sh, device): mode 1 = multisample_filter (bilinear), 2 = kernel
 * downscale (+ the digital filter over the result for the cardinal kernels),
 * 3 = kernel upscale (the cardinal kernels' digital prefilter runs IN PLACE on
 * d_frame first, as the reference does).  Asynchronous on the context stream. */
cvr_status  cvr_multiscale_filter(cvr_ctx* ctx, int mode, int kernel, void* d_frame, int fw,
                                  int fh, void* d_screen, int sw, int sh);

/* Screenshot: the frame (device, CVR_FORMAT_*) blended over the white clear
 * colour with SRC_ALPHA / ONE_MINUS_SRC_ALPHA and stored as RGB8, row 0 =
 * bottom as glReadPixels returns it (w*h*3 bytes, device).  Asynchronous. */
cvr_status  cvr_screenshot_rgb8(cvr_ctx* ctx, const void* d_frame, int format, int w, int h,
                                void* d_rgb);

/* ----------------------------------------------------------------------------
 * Multi-GPU: the screen-tile split's gather, native RCCL over xGMI
 * (the reference renders on one GPU, so this has no reference
 * counterpart beyond the Redraw it feeds, rc1prenderer.cpp:140-151).
 * One context per GPU, one process (or thread) per context.
 * -------------------------------------------------------------------------- */

#define CVR_COMM_ID_BYTES 128
/* The most exchange buffer sets (option "gather_sets"): the library keeps the
 * end events of the last 64 exchanges. */
#define CVR_MAX_GATHER_SETS 64

/* Rank 0 creates the communicator id (ncclGetUniqueId) and hands it to every
 * rank out of band (e.g. torch.distributed broadcast). */
cvr_status  cvr_comm_unique_id(unsigned char out_id[CVR_COMM_ID_BYTES]);

/* Collective over the nranks contexts: joins this context to the communicator. */
cvr_status  cvr_comm_init(cvr_ctx* ctx, int nranks, int rank,
                          const unsigned char id[CVR_COMM_ID_BYTES]);
cvr_status  cvr_comm_destroy(cvr_ctx* ctx);

/* The same protocol without RCCL, for n contexts of THIS process (rank i =
 * ctxs[i]; the devices may repeat, e.g. n contexts on one GPU): the bytes move
 * as device copies (over xGMI between GPUs).  Every exchange call
 * (cvr_gather_tiles_n) must be made by ranks 1..n-1 before rank 0 makes it, and
 * the buffer sets must exceed the render streams (gather_sets > split_streams):
 * a rank's next render waits for rank 0's completed exchange of its buffers.
 * cvr_create_group uses it; tests use it to run the multi-rank exchange on one
 * GPU (RCCL refuses several ranks per device). */
cvr_status  cvr_comm_init_local(cvr_ctx* const* ctxs, int n);

/* Gather one frame's packed tiles on rank 0 (one ncclGather) and unpack them
 * into the image.
 * Every rank calls it right after rendering its tiles (frame->rank/nranks
 * must match the communicator) into `d_packed` (tiles_per_rank_max tiles,
 * padding allowed).  Rank 0 also passes `d_gathered` (nranks blocks of
 * tiles_per_rank_max tiles; when d_packed == d_gathered, rank 0 rendered
 * straight into its block 0 and no copy is made) and the W x H image `d_rgba`.
 * Asynchronous: the gather and unpack run on the context's communication
 * stream after the render.  Callers alternate two packed (and, on rank 0, two
 * gather) buffers, frame n using buffer n % 2 (see split_streams for more).  With option split_streams = 1
 * (default) the context stream then waits only for the PREVIOUS gather, so the
 * next render overlaps this gather.  With split_streams = D >= 2 the caller
 * rotates D streams and D buffer sets (frame n on stream n % D, cvr_set_stream
 * before each render) and the stream waits for THIS gather, so D consecutive
 * frames overlap on the device as well.
 * Frames on different streams each use their own LPT order state; frames that
 * count samples (cvr_output.total) must not overlap.  Before reading the image
 * on the context stream, call cvr_gather_sync.  With a one-rank communicator
 * the frame is rendered whole (nranks 1) and the gather copies it to d_rgba. */
cvr_status  cvr_gather_tiles(cvr_ctx* ctx, const cvr_frame* frame, const void* d_packed,
                             int tiles_per_rank_max, int format, void* d_gathered,
                             void* d_rgba);

/* The same for `nframes` frames rendered by this rank one after another on the
 * context stream into consecutive blocks of `d_packed` (frame j at j *
 * tiles_per_rank_max tiles), exchanged in ONE ncclGather (fewer, larger
 * collectives: a gather's host and launch cost is shared by nframes frames).
 * `frame` gives the tile layout (the camera is not used).  Rank 0's
 * `d_gathered` holds nranks blocks of nframes * tiles_per_rank_max tiles, and
 * frame j is unpacked into d_images[j] (in frame order; NULL skips it).
 * A call that returns CVR_ERR_ARG or CVR_ERR_STATE has issued no exchange: this
 * rank's exchange count, its buffers and images, and what the other ranks see of
 * it are as before the call, so the same exchange can be issued again. */
cvr_status  cvr_gather_tiles_n(cvr_ctx* ctx, const cvr_frame* frame, int nframes,
                               const void* d_packed, int tiles_per_rank_max, int format,
                               void* d_gathered, void* const* d_images);

/* The context stream waits for every gather issued so far (posting any whose
 * data phase still trails, see exchange_lag). */
cvr_status  cvr_gather_sync(cvr_ctx* ctx);

/* Exchange form (options, set on every rank alike):
 *   "exchange_code" 1 (default): RGBA16F exchanges of N > 1 ranks move the lossless
 *                per-tile code (cvr_encode_tiles' stream, encoded in one launch per
 *                exchange on the render stream) instead of raw tiles, and rank 0
 *                decodes every rank's stream straight into the images in one
 *                launch; 0: raw tiles (one ncclGather, then the unpack).  RGBA32F
 *                always moves raw tiles.  The images are identical either way.
 *   "exchange_lag" the coded exchange's sizes vary, so they travel first (an 8-byte
 *                gather on a second communicator, right after the encode) and
 *                exchange g's data is posted when a later call reads g's sizes on
 *                the host: at most this many exchanges later (-1, the default:
 *                split_streams - 1; bounded by gather_sets - split_streams so a
 *                render stream never waits for an unposted exchange; 0: at once,
 *                which blocks the host until this rank's encode is done). */

/* ----------------------------------------------------------------------------
 * One context over several GPUs of this process (SURVEY.md §8b threading row:
 * multi-GPU inside cvr_render when ndev > 1).  The reference app is one GLUT
 * process with one GL thread (app_freeglut.cpp:125,174), so its plugin cannot be
 * one process per GPU.  cvr_create_group returns a context whose state setters
 * (volume, TF, gradient, extinction pyramid, SAT, options) apply to one member
 * context per device, and whose render calls (rc1pass, rc1pass_frames, dosct,
 * extbsd, iso; whole frames, nranks <= 1) split the frame into 16 x 16 screen
 * tiles on the diagonal lattice over the members, render every share on its own
 * device concurrently, and gather the tiles on devices[0] (the in-process
 * transport of cvr_comm_init_local; RGBA16F as the per-tile code) into the
 * caller's outputs, which live on devices[0] (or the host).  Same pixels, counts
 * and totals as one context.  Devices may repeat.  The group's stream
 * (cvr_set_stream) is devices[0]'s; member 0 renders on it.  Host outputs block;
 * device outputs are queued on the group's stream.  Options split_streams,
 * gather_sets, gather_root_idle and exchange_lag belong to the group's own
 * exchange and are refused. */
cvr_status  cvr_create_group(const int* devices, int n, cvr_ctx** out_ctx);
/* Members of a group (1 for a plain context) and member i's context (NULL if none;
 * owned by the group: for inspection, not for cvr_destroy). */
int         cvr_group_size(const cvr_ctx* ctx);
cvr_ctx*    cvr_group_member(cvr_ctx* ctx, int i);

/* Diagnostics (tile_stats option): for each 8x8 tile of the last frame, four
 * uint64: start and end stamp (s_memrealtime, 100 MHz), its longest ray's
 * iteration count, (workgroup << 32 | HW_ID).  out = NULL queries *out_tiles. */
cvr_status  cvr_copy_tile_stats(cvr_ctx* ctx, uint64_t* out, int max_tiles, int* out_tiles);

/* Measurement (kernel_timing option = ring of N frames): milliseconds of the
 * ray-march kernel alone (HIP events recorded on the context stream around its
 * launch) for the most recent min(N, frames since the last read, max_frames)
 * frames, oldest first.  Waits for those frames; resets the frame count. */
cvr_status  cvr_read_kernel_times(cvr_ctx* ctx, float* ms, int max_frames, int* out_frames);

/* Self-check of the device arithmetic the kernels take shortcuts with
 * (cvr_device.h), exhaustive over every significand: out[0] = floats b with
 * |b| in [2^-100, 2^100) whose rcp_cr(b) differs from the IEEE 1.0f / b,
 * out[1] = floats x in [2^-96, 2^126) whose sqrt_cr_normal(x) differs from the
 * correctly rounded sqrtf(x), out[2] = (x, y) pairs (every positive normal
 * x < 4 at five exponents y, and the special arguments) whose branch-free
 * cvr_powf_nb differs from cvr_powf.  All must be 0; synchronous (~1 s). */
cvr_status  cvr_selftest_arith(cvr_ctx* ctx, uint64_t out[3]);

/* Measurement (shade_counters option), for the last shaded frame
 * (cvr_render_dosct / cvr_render_extbsd; cvr_render_rc1pass: out[0] the
 * Blinn-Phong shaded samples, out[1] the samples the per-cell skip stepped over
 * without a load, out[2] (emission-absorption, cell_skip > 0) the waves' march
 * rounds, each K = 4 cell loads per wave): out[0] samples that ran the shading
 * (alpha > 0), out[1] those whose shadow was traced (spot cut-off excluded),
 * out[2] the secondary trilinear fetches actually issued (extinction pyramid /
 * SAT): the secondary traffic of the roofline.  For DOS the reference's own tap
 * count is out[0] * (n1 + 3 n3 + 7 n7)_occlusion + out[1] * (...)_shadow; out[2]
 * leaves out the taps whose CONSIDER_BORDERS factor is exactly 0 (not fetched). */
cvr_status  cvr_read_shade_counters(cvr_ctx* ctx, uint64_t out[3]);

/* ----------------------------------------------------------------------------
 * Host-side helpers (native replacements for the reference's MSVC-only
 * readers and its CPU table builders).  They touch no device.
 * -------------------------------------------------------------------------- */
/* ConeGaussianSampler::ComputeConeIntegrationSteps + ComputeAdditionalInfo
 * (conegaussiansampler.cpp:212-414) for one cone; sigma0 = the extinction
 * volume's base Gaussian sigma (ExtinctionCoefficientVolume default 1). */
cvr_status  cvr_build_cone_tables(const cvr_cone_params* params, float sigma0,
                                  cvr_cone_tables* out);

/* Derived render constants, exposed for testing: the view matrix the ray
 * generator uses (glm::lookAt, column-major 4x4) and tan(fovy/2). */
cvr_status  cvr_camera_lookat(const cvr_camera* cam, float out_view[16], float* out_tan_half_fovy);
/* Default integration step for a voxel scale: 0.5/sqrt(3)*|scale|. */
float       cvr_default_step(const float scale[3]);

/* TransferFunction1D built from control points (BuildLinear,
 * transferfunction1d.cpp:319-358) and converted like GenerateTexture_1D_RGBt
 * (:89-118).  rgb_cp: n_rgb x (r, g, b, isovalue); a_cp: n_a x (a, isovalue).
 * out_rgbt receives (max_density+1) x 4 floats. */
cvr_status  cvr_tf1d_build_rgbt(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                                int max_density, int extinction_input, float* out_rgbt);

/* TransferFunction1D::GetExtN (transferfunction1d.cpp:132-157, 189-197) of
 * every voxel value v / (2^bits - 1), bits = 8 * bytes_per_voxel: the cell
 * values of the EBS SAT.  out_lut receives 256 or 65536 floats. */
cvr_status  cvr_tf1d_ext_lut(const double* rgb_cp, int n_rgb, const double* a_cp, int n_a,
                             int max_density, int extinction_input, int bytes_per_voxel,
                             float* out_lut);

/* .tf1d reader (TransferFunctionReader::readtf1d, reader.cpp:744-814) and the
 * built table.  out_rgbt must hold 4*(max_density+1) floats; pass NULL to
 * query *out_n first. */
cvr_status  cvr_read_tf1d(const char* path, float* out_rgbt, int* out_n);

/* .raw reader: dims and bytes per voxel parsed from "name.<bytes>.<W>x<H>x<D>.raw"
 * (VolumeReader::readraw, reader.cpp:162-225).  Pass voxels = NULL to query. */
cvr_status  cvr_read_raw(const char* path, void* voxels, size_t capacity,
                         int* out_w, int* out_h, int* out_d, int* out_bytes_per_voxel);

/* .pvm reader (VolumeReader::readpvm, reader.cpp:100-159; DDSV3 decoder,
 * libs/file_utils/pvm.cpp:191-620): plain or DDS-compressed PVM/PVM2/PVM3,
 * 1 component -> u8, 2 -> u16 (data[2i] + 256*data[2i+1], as Pvm::PostProcessData).
 * out_scale (may be NULL) receives the PVM2/3 voxel spacing.  voxels = NULL queries. */
cvr_status  cvr_read_pvm(const char* path, void* voxels, size_t capacity, int* out_w,
                         int* out_h, int* out_d, int* out_bytes_per_voxel, float out_scale[3]);

/* .syn reader (VolumeReader::readsyn, reader.cpp:283-371); u8 voxels. */
cvr_status  cvr_read_syn(const char* path, uint8_t* voxels, size_t capacity,
                         int* out_w, int* out_h, int* out_d);

/* #list_camera_states (CameraStateList::ReadCameraStates, camerastatelist.cpp:26-87):
 * returns the index-th ARCBALL state. */
cvr_status  cvr_read_camera_state(const char* path, int index, cvr_camera* out_cam,
                                  char* out_name, int name_capacity, int* out_count);

/* #list_light_sources (LightSourceList::ReadLightSourceLists, lightsourcelist.cpp:81-148):
 * position of light `light` of list `list`. */
cvr_status  cvr_read_light_position(const char* path, int list, int light, float out_pos[3],
                                    int* out_count);
/* The same light with its camera frame and spot angle (forward = -z_axis). */
cvr_status  cvr_read_light(const char* path, int list, int light, cvr_light* out,
                           int* out_count);

#ifdef __cplusplus
}
#endif

#endif /* CVR_H */
