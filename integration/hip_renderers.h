/**
 * MI355X drop-ins for the reference's structured single-pass renderers, each a
 * BaseVolumeRenderer (cppvolrend/volrenderbase.h:25-96) that forwards to libcvr.so:
 *
 *   HipRayCasting1Pass               <- RayCasting1Pass        (rc1pass/rc1prenderer.h:31-76)
 *   HipDirOcclusionShading           <- RC1PConeTracingDirOcclusionShading
 *                                                              (rc1pdosct/dosrcrenderer.h:40-120)
 *   HipExtinctionBasedShading        <- RC1PExtinctionBasedShading
 *                                                              (rc1pextbsd/ebsrenderer.h:47-123)
 *   HipRC1PConeLightGroundTruthSteps <- RC1PConeLightGroundTruthSteps
 *   HipVoxelConeTracingSGPU          <- RC1PVoxelConeTracingSGPU
 *                                                              (rc1pcrtgt/crtgtrenderer.h:50-118)
 *   HipSBTMDirectionalOcclusionShading <- SBTMDirectionalOcclusionShading
 *                                                              (sbtmdos/sbtmdosrenderer.h)
 *   HipDeferredShading                 <- DeferredShading      (DeferredShading/DeferredShading.h)
 *   HipAdvancedDeferredShading         <- AdvancedDeferredShading (AdvancedDeferredShading/AdvancedDeferredShading.h)
 *   HipRayCasting1PassIsoAdapt       <- RayCasting1PassIsoAdapt (rc1pisoadapt/rc1pisoadaptrenderer.h)
 *   HipCustomRayCasting1PassIsoAdapt <- CustomRayCasting1PassIsoAdapt (rc1pisocustom/...)
 *   HipCustomRayCasting1PassIsodfsAdapt <- CustomRayCasting1PassIsodfsAdapt (rc1pisodfscustom/...)
 *
 * Parameters keep the reference's member names and defaults; the GLSL uniforms
 * they fed become the plain structs of include/cvr.h.
 */
#ifndef CVR_HIP_RENDERERS_H
#define CVR_HIP_RENDERERS_H

#include "hip_renderer_base.h"

class HipRayCasting1Pass : public HipRendererBase
{
public:
  HipRayCasting1Pass ();
  const char* GetName () override { return "1-Pass - Ray Casting (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_1rc_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;
  void FillParameterSpace (ParameterSpace& pspace) override;

  float m_u_step_size;                 // rc1prenderer.h:63
  bool m_apply_gradient_shading;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_rc1pass_params m_params;
};

class HipDirOcclusionShading : public HipRendererBase
{
public:
  HipDirOcclusionShading ();
  const char* GetName () override { return "1-Pass - Ray Casting - Dir. Occlusion Shading (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_1rc_dos_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;

  // dosrcrenderer.cpp:29-60
  bool glsl_apply_occlusion;
  bool glsl_apply_shadow;
  int type_of_shadow;                  // 0 point, 1 spot, 2 directional
  cvr_cone_params sampler_occlusion;   // ConeGaussianSampler settings
  cvr_cone_params sampler_shadow;
  float m_u_step_size;
  bool m_apply_gradient_shading;

  // m_pre_illum_str_vol (dosrcrenderer.h:69, PreIlluminationStructuredVolume): the
  // "Use Pre-Illumination" switch and the light cache's resolution (32^3,
  // dosrcrenderer.cpp:63-64).  The two setters are what the reference's
  // SetImGuiComponents does on its checkbox and its "Update" button
  // (preillumination.cpp:88-122, dosrcrenderer.cpp:330-336): they take the place of
  // SetActive / SetLightCacheResolution + GenerateLightCacheTexture.
  bool pre_illumination;
  int light_cache_resolution[3];
  void SetPreIllumination (bool active);
  void SetLightCacheResolution (int w, int h, int d);

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_dos_params m_params;
};

class HipExtinctionBasedShading : public HipRendererBase
{
public:
  HipExtinctionBasedShading ();
  const char* GetName () override { return "1-Pass - Ray Casting - Extinction-based (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_1rc_eb_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;

  // ebsrenderer.cpp:18-51
  float m_u_step_size;
  bool m_apply_gradient_shading;
  bool apply_ambient_occlusion;
  int ambient_occlusion_shells;
  float ambient_occlusion_radius;
  bool apply_directional_shadows;
  float dir_shadow_cone_angle;
  float dir_shadow_sample_interval;
  float dir_shadow_initial_step;
  float dir_shadow_user_interface_weight;
  float dir_cone_max_distance;
  int type_of_shadow;                  // 0 point, 1 directional

  // m_pre_illum_str_vol (PreIlluminationStructuredVolume, ebsrenderer.cpp:46-47): the
  // "Use Pre-Illumination" switch and the light cache's resolution, as
  // HipDirOcclusionShading's.
  bool pre_illumination;
  int light_cache_resolution[3];
  void SetPreIllumination (bool active);
  void SetLightCacheResolution (int w, int h, int d);

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  bool UploadExtinctionSAT ();         // GenerateExtinctionSAT3DTex (:624-723), on the GPU
  cvr_ebs_params m_params;
};

// The ground truth of the two renderers above: every sample shaded by secondary rays
// cast through the volume.  Progressive, as the reference: Update resets the frame
// (cvr_crtgt_begin) and every Redraw extends each unfinished ray by
// samples_per_redraw iterations (the reference: one) until the frame is ready; the
// state lives in the library, in float (DESIGN.md 5d').  One GPU: the library's group
// contexts refuse these calls.
class HipRC1PConeLightGroundTruthSteps : public HipRendererBase
{
public:
  HipRC1PConeLightGroundTruthSteps ();
  const char* GetName () override { return "1-Pass - Ray Casting - Cone Ground Truth (Steps) (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_1rc_gt_c_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;

  // crtgtrenderer.cpp:23-51
  bool m_frame_outdated;
  float m_u_step_size;
  bool m_apply_gradient;
  float m_u_light_ray_initial_step;
  float m_u_light_ray_step_size;
  bool m_light_parameters_outdated;
  bool m_apply_occlusion;
  int m_occ_num_rays_sampled;
  float m_occ_cone_aperture_angle;
  float m_occ_cone_distance_eval;
  bool m_apply_shadows;
  int m_sdw_num_rays_sampled;
  float m_sdw_cone_aperture_angle;
  float m_sdw_cone_distance_eval;
  int m_shadow_type;                   // 0 point, 1 spot, 2 directional
  int samples_per_redraw;              // iterations per pixel and Redraw (>= 1)
  unsigned ray_seed;                   // the tables' generator (cvr_crtgt_build_rays)

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_crtgt_params m_params;
  std::vector<float> m_occ_rays, m_sdw_rays;
};

// The third approximate shadow technique: one voxel cone toward the light per sample,
// through a (mean, stddev) supervoxel pyramid and a pre-integration table (image-space
// mode; the reference's light-cache mode of this renderer is not built).  1-byte
// volumes only.
class HipVoxelConeTracingSGPU : public HipRendererBase
{
public:
  HipVoxelConeTracingSGPU ();
  const char* GetName () override { return "1-Pass - Ray Casting - Voxel Cone Tracing (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_1rc_vct_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;

  // vctrenderer.cpp:27-43
  float m_u_step_size;
  bool m_apply_gradient_shading;
  bool apply_ambient_occlusion;
  bool apply_voxel_cone_tracing;
  float cone_step_size;
  float cone_step_size_increase_rate;
  float cone_initial_step;
  float cone_apex_angle;
  bool apply_correction_factor;
  float opacity_correction_factor;
  int cone_number_of_samples;
  float covered_distance;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  bool UploadOpacities ();             // GetOpc(i, 255) for the pre-integration table
  cvr_vct_params m_params;
};

// Schott et al.'s slice-based directional occlusion: view-aligned slices composited
// through an eye buffer and two occlusion buffers (cvr_render_sbtm).  No light, no
// gradient; whole frames only.
class HipSBTMDirectionalOcclusionShading : public HipRendererBase
{
public:
  HipSBTMDirectionalOcclusionShading ();
  const char* GetName () override { return "Slice-based - Directional Occlusion (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "s_sbtm_dos_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;

  // sbtmdosrenderer.cpp:20-48
  float m_u_step_size;
  float cone_half_angle;
  bool evaluate_dir_occlusion;
  glm::vec2 grid_size;
  int max_number_of_passes;
  float occ_ui_weight_percentage;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_sbtm_params m_params;
};

// The three single-pass isosurface ray-casters share one library entry point
// (cvr_render_iso) and differ in `variant`: 2 = no blocks, 0 = 4^3 block chords,
// 1 = 32^3 block exit distances.
class HipIsoRayCasterBase : public HipRendererBase
{
public:
  explicit HipIsoRayCasterBase (int variant);
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;
  void FillParameterSpace (ParameterSpace& pspace) override;

  float m_u_isovalue;
  float m_u_step_size_small;
  float m_u_step_size_large;
  float m_u_step_size_range;
  glm::vec4 m_u_color;
  bool m_apply_gradient_shading;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_iso_params m_params;
};

class HipRayCasting1PassIsoAdapt : public HipIsoRayCasterBase
{
public:
  HipRayCasting1PassIsoAdapt () : HipIsoRayCasterBase(2) {}
  const char* GetName () override { return "1-Pass - Isosurface Raycaster Adaptive (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "iso_hip"; }
};

class HipCustomRayCasting1PassIsoAdapt : public HipIsoRayCasterBase
{
public:
  HipCustomRayCasting1PassIsoAdapt () : HipIsoRayCasterBase(0) {}
  const char* GetName () override { return "1-Pass - Custom Isosurface Raycaster Adaptive (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "iso_hip"; }
};

class HipCustomRayCasting1PassIsodfsAdapt : public HipIsoRayCasterBase
{
public:
  HipCustomRayCasting1PassIsodfsAdapt () : HipIsoRayCasterBase(1) {}
  const char* GetName () override { return "Empty Space Skipping V2 (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "iso_hip"; }
};

// DeferredShading (DeferredShading/DeferredShading.cpp): the isosurface march into a
// G-buffer the library keeps, the lighting pass and the tone map (cvr_render_deferred).
// Update marches again only when the frame or a march parameter changed; otherwise
// Redraw re-shades the kept G-buffer (cvr_deferred_shade).  Whole frames only.
class HipDeferredShading : public HipRendererBase
{
public:
  HipDeferredShading ();
  const char* GetName () override { return "Deferred Rendering (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "iso_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;
  void FillParameterSpace (ParameterSpace& pspace) override;

  // DeferredShading.cpp:123-128
  float m_u_isovalue;
  float m_u_step_size_small;
  float m_u_step_size_large;
  float m_u_step_size_range;
  glm::vec4 m_u_color;
  bool m_apply_gradient_shading;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_deferred_params m_params;
  cvr_frame m_kept_frame;              // what the kept G-buffer was marched from
  cvr_deferred_params m_kept_params;
  bool m_geometry_kept;
};

// AdvancedDeferredShading (AdvancedDeferredShading/AdvancedDeferredShading.cpp): the same
// march, a curvature pass over the kept G-buffer and the feature-lighting pass with the tone
// map (cvr_render_advdeferred).  Update marches again only when the frame or a march
// parameter changed; otherwise Redraw runs the lighting pass over the kept planes
// (cvr_advdeferred_shade).  Whole frames only.
class HipAdvancedDeferredShading : public HipRendererBase
{
public:
  HipAdvancedDeferredShading ();
  const char* GetName () override { return "Advanced Deferred Rendering (HIP, MI355X)"; }
  const char* GetAbbreviationName () override { return "iso_hip"; }
  bool Init (int shader_width, int shader_height) override;
  bool Update (vis::Camera* camera) override;
  void FillParameterSpace (ParameterSpace& pspace) override;

  // AdvancedDeferredShading.cpp:124-130, AdvancedDeferredShading.h:129-133, Init :536-537
  float m_u_isovalue;
  float m_u_step_size_small;
  float m_u_step_size_large;
  float m_u_step_size_range;
  glm::vec4 m_u_color;
  float m_current_time;
  float m_flow_speed;
  float m_flow_scale;
  bool m_show_ridges;
  bool m_show_valleys;
  float m_accessibility_strength;
  float s, v;

protected:
  cvr_status RenderFrame (const cvr_output* out) override;
  cvr_advdeferred_params m_params;
  cvr_frame m_kept_frame;              // what the kept planes were computed from
  cvr_advdeferred_params m_kept_params;
  bool m_geometry_kept;
};

// Adds every HIP renderer to the RenderingManager (register_hip_renderers.cpp;
// call it next to main.cpp:65).
void RegisterHipRenderers ();

#endif
