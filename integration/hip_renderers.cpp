#include "hip_renderers.h"

#include "../../utils/parameterspace.h"

#include <volvis_utils/structuredgridvolume.h>
#include <volvis_utils/transferfunction.h>

#include <cstring>
#include <vector>

// Blinn-Phong constants and the light of RenderingParameters
// (renderingparameters.h:45-74), as every Update uploads them.
template <typename P>
static void fill_phong (P* p, vis::RenderingParameters* rp)
{
  p->ka = rp->GetBlinnPhongKambient();
  p->kd = rp->GetBlinnPhongKdiffuse();
  p->ks = rp->GetBlinnPhongKspecular();
  p->shininess = rp->GetBlinnPhongNshininess();
  const glm::vec3 is = rp->GetLightSourceSpecular();
  for (int i = 0; i < 3; i++) p->ispecular[i] = is[i];
}

static void copy3 (float* dst, const glm::vec3& v)
{
  dst[0] = v.x; dst[1] = v.y; dst[2] = v.z;
}

////////////////////////////////////////////////////////////////////////////////
// RayCasting1Pass (rc1prenderer.cpp:18-151)
////////////////////////////////////////////////////////////////////////////////
HipRayCasting1Pass::HipRayCasting1Pass ()
  : m_u_step_size(0.5f)
  , m_apply_gradient_shading(false)
  , m_params()
{
}

bool HipRayCasting1Pass::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;   // :54
  if (!UploadVolume() || !UploadTransferFunction() || !UploadGradient(m_apply_gradient_shading))
    return false;
  m_u_step_size = DefaultStep();                                                // :62-63
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipRayCasting1Pass::Update (vis::Camera* camera)
{
  FillFrame(camera);
  m_params.step = m_u_step_size;
  m_params.apply_gradient_shading =
      (m_apply_gradient_shading && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  fill_phong(&m_params, m_ext_rendering_parameters);
  copy3(m_params.light_pos, m_ext_rendering_parameters->GetBlinnPhongLightingPosition());
  return true;
}

cvr_status HipRayCasting1Pass::RenderFrame (const cvr_output* out)
{
  return cvr_render_rc1pass(m_cvr, &frame_, &m_params, out);
}

// rc1prenderer.cpp:225-229: the evaluation sweep over StepSize
void HipRayCasting1Pass::FillParameterSpace (ParameterSpace& pspace)
{
  pspace.ClearParameterDimensions();
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSize", &m_u_step_size, 0.2, 2.0, 0.1));
}

////////////////////////////////////////////////////////////////////////////////
// RC1PConeTracingDirOcclusionShading (dosrcrenderer.cpp:29-260)
////////////////////////////////////////////////////////////////////////////////
HipDirOcclusionShading::HipDirOcclusionShading ()
  : glsl_apply_occlusion(true)
  , glsl_apply_shadow(false)
  , type_of_shadow(0)
  , m_u_step_size(0.5f)
  , m_apply_gradient_shading(false)
  , pre_illumination(false)                    // m_pre_illum_str_vol.SetActive(false) (:63)
  , light_cache_resolution{32, 32, 32}         // SetLightCacheResolution(32, 32, 32) (:64)
  , m_params()
{
  // ConeGaussianSampler settings of the constructor (:47-58); the covered
  // distances are set from the volume diagonal in Init (:110-113)
  sampler_occlusion.half_angle_deg = 20.0f;
  sampler_occlusion.max_packing = 1;           // CONEPACKING::_3
  sampler_occlusion.covered_distance = 0.0f;
  sampler_occlusion.ui_weight = 0.35f;
  sampler_occlusion.initial_step = 0.0f;       // the sampler's default
  sampler_shadow.half_angle_deg = 0.5f;
  sampler_shadow.max_packing = 0;              // CONEPACKING::_1
  sampler_shadow.covered_distance = 0.0f;
  sampler_shadow.ui_weight = 1.0f;
  sampler_shadow.initial_step = 0.0f;
}

bool HipDirOcclusionShading::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume() || !UploadTransferFunction() || !UploadGradient(m_apply_gradient_shading))
    return false;
  vis::StructuredGridVolume* vol = m_ext_data_manager->GetCurrentStructuredVolume();
  sampler_occlusion.covered_distance = (float)(vol->GetDiagonal() * 0.50f);
  sampler_shadow.covered_distance = (float)(vol->GetDiagonal() * 0.75f);
  // GenerateExtCoefVolume (:745-764): the Gaussian pyramid of the RGBA (opacity) TF
  // at ExtinctionCoefficientVolume's defaults (128^3, sigma0 1)
  std::vector<float> rgba;
  int n = 0;
  if (!ReadTransferFunctionRGBA(&rgba, &n)) return false;
  if (cvr_set_extinction_volume(m_cvr, rgba.data(), n, nullptr, 1.0f) != CVR_OK)
    return Fail("cvr_set_extinction_volume");
  m_u_step_size = DefaultStep();
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipDirOcclusionShading::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  m_params.step = m_u_step_size;
  m_params.apply_gradient_shading =
      (m_apply_gradient_shading && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  fill_phong(&m_params, rp);
  copy3(m_params.light.position, rp->GetBlinnPhongLightingPosition());
  copy3(m_params.light.forward, rp->GetBlinnPhongLightSourceCameraForward());
  copy3(m_params.light.up, rp->GetBlinnPhongLightSourceCameraUp());
  copy3(m_params.light.right, rp->GetBlinnPhongLightSourceCameraRight());
  m_params.light.spot_angle_deg = rp->GetSpotLightMaxAngle();
  m_params.apply_occlusion = glsl_apply_occlusion ? 1 : 0;
  m_params.apply_shadow = glsl_apply_shadow ? 1 : 0;
  m_params.shadow_type = type_of_shadow;
  m_params.occlusion = sampler_occlusion;
  m_params.shadow = sampler_shadow;
  return true;
}

void HipDirOcclusionShading::SetPreIllumination (bool active)
{
  pre_illumination = active;
  SetOutdated();
}

void HipDirOcclusionShading::SetLightCacheResolution (int w, int h, int d)
{
  light_cache_resolution[0] = w;
  light_cache_resolution[1] = h;
  light_cache_resolution[2] = d;
  SetOutdated();
}

// Update (:134-143): with the switch on, PreComputeLightCache and the march of
// obj_ray_marching.comp; the library owns the cache (4 bytes per voxel) and
// recomputes it only when something it depends on changed.
cvr_status HipDirOcclusionShading::RenderFrame (const cvr_output* out)
{
  if (pre_illumination)
    return cvr_render_dosct_preillum(m_cvr, &frame_, &m_params, light_cache_resolution, out);
  return cvr_render_dosct(m_cvr, &frame_, &m_params, out);
}

////////////////////////////////////////////////////////////////////////////////
// RC1PConeLightGroundTruthSteps (crtgtrenderer.cpp:23-325)
////////////////////////////////////////////////////////////////////////////////
HipRC1PConeLightGroundTruthSteps::HipRC1PConeLightGroundTruthSteps ()
  : HipRendererBase(0)
  , m_frame_outdated(true)
  , m_u_step_size(0.5f)
  , m_apply_gradient(false)
  , m_u_light_ray_initial_step(1.0f)
  , m_u_light_ray_step_size(0.5f)
  , m_light_parameters_outdated(true)
  , m_apply_occlusion(false)
  , m_occ_num_rays_sampled(1)
  , m_occ_cone_aperture_angle(90.f)
  , m_occ_cone_distance_eval(100.0f)
  , m_apply_shadows(false)
  , m_sdw_num_rays_sampled(1)
  , m_sdw_cone_aperture_angle(1.0f)
  , m_sdw_cone_distance_eval(100.0f)
  , m_shadow_type(0)
  , samples_per_redraw(1)
  , ray_seed(1)
  , m_params()
{
}

bool HipRC1PConeLightGroundTruthSteps::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;   // :98
  if (!UploadVolume() || !UploadTransferFunction() || !UploadGradient(m_apply_gradient))
    return false;
  m_u_step_size = DefaultStep();                                                // :107-108
  vis::StructuredGridVolume* vol = m_ext_data_manager->GetCurrentStructuredVolume();
  m_occ_cone_distance_eval = (float)(vol->GetDiagonal() * 0.50f);               // :112-113
  m_sdw_cone_distance_eval = (float)(vol->GetDiagonal() * 0.75f);
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

// Update (:121-260): new ray tables when a count or an aperture changed, the
// uniforms, and a frame that starts over.
bool HipRC1PConeLightGroundTruthSteps::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  if (m_light_parameters_outdated)
  {
    m_occ_rays.assign((size_t)(m_occ_num_rays_sampled > 0 ? m_occ_num_rays_sampled : 0) * 3, 0.0f);
    m_sdw_rays.assign((size_t)(m_sdw_num_rays_sampled > 0 ? m_sdw_num_rays_sampled : 0) * 3, 0.0f);
    if (cvr_crtgt_build_rays(m_occ_cone_aperture_angle, (int)(m_occ_rays.size() / 3),
                             m_sdw_cone_aperture_angle, (int)(m_sdw_rays.size() / 3), ray_seed,
                             m_occ_rays.empty() ? nullptr : m_occ_rays.data(),
                             m_sdw_rays.empty() ? nullptr : m_sdw_rays.data()) != CVR_OK)
      return Fail("cvr_crtgt_build_rays");
    m_light_parameters_outdated = false;
  }
  cvr_crtgt_params_default(&m_params);
  m_params.step = m_u_step_size;
  m_params.apply_gradient_shading =
      (m_apply_gradient && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  m_params.ka = rp->GetBlinnPhongKambient();
  m_params.kd = rp->GetBlinnPhongKdiffuse();
  m_params.ks = rp->GetBlinnPhongKspecular();
  m_params.shininess = rp->GetBlinnPhongNshininess();
  copy3(m_params.light.position, rp->GetBlinnPhongLightingPosition());
  copy3(m_params.light.forward, rp->GetBlinnPhongLightSourceCameraForward());
  copy3(m_params.light.up, rp->GetBlinnPhongLightSourceCameraUp());
  copy3(m_params.light.right, rp->GetBlinnPhongLightSourceCameraRight());
  m_params.light.spot_angle_deg = rp->GetSpotLightMaxAngle();
  m_params.light_gap = m_u_light_ray_initial_step;
  m_params.light_step = m_u_light_ray_step_size;
  m_params.apply_occlusion = m_apply_occlusion ? 1 : 0;
  m_params.occ_distance = m_occ_cone_distance_eval;
  m_params.apply_shadow = m_apply_shadows ? 1 : 0;
  m_params.sdw_distance = m_sdw_cone_distance_eval;
  m_params.shadow_type = m_shadow_type;
  m_frame_outdated = true;
  if (cvr_crtgt_begin(m_cvr, &frame_, &m_params, m_occ_rays.data(), (int)(m_occ_rays.size() / 3),
                      m_sdw_rays.data(), (int)(m_sdw_rays.size() / 3)) != CVR_OK)
    return Fail("cvr_crtgt_begin");
  return true;
}

// RedrawFrameTexture (:272-325): one more dispatch while a pixel is unfinished; a
// ready frame is only copied.
cvr_status HipRC1PConeLightGroundTruthSteps::RenderFrame (const cvr_output* out)
{
  unsigned long long left = 0;
  const cvr_status st = cvr_crtgt_advance(m_cvr, samples_per_redraw > 0 ? samples_per_redraw : 1, out, &left);
  if (st == CVR_OK) m_frame_outdated = left > 0;
  return st;
}

////////////////////////////////////////////////////////////////////////////////
// RC1PExtinctionBasedShading (ebsrenderer.cpp:18-260, 624-723)
////////////////////////////////////////////////////////////////////////////////
HipExtinctionBasedShading::HipExtinctionBasedShading ()
  : m_u_step_size(0.5f)
  , m_apply_gradient_shading(false)
  , apply_ambient_occlusion(true)
  , ambient_occlusion_shells(15)
  , ambient_occlusion_radius(1.0f)
  , apply_directional_shadows(true)
  , dir_shadow_cone_angle(1.0f)
  , dir_shadow_sample_interval(2.0f)
  , dir_shadow_initial_step(2.0f)
  , dir_shadow_user_interface_weight(1.0f)
  , dir_cone_max_distance(0.0f)
  , type_of_shadow(0)
  , pre_illumination(false)                    // m_pre_illum_str_vol.SetActive(false) (ebsrenderer.cpp:46)
  , light_cache_resolution{32, 32, 32}         // SetLightCacheResolution(32, 32, 32) (:47)
  , m_params()
{
}

void HipExtinctionBasedShading::SetPreIllumination (bool active)
{
  pre_illumination = active;
  SetOutdated();
}

void HipExtinctionBasedShading::SetLightCacheResolution (int w, int h, int d)
{
  light_cache_resolution[0] = w;
  light_cache_resolution[1] = h;
  light_cache_resolution[2] = d;
  SetOutdated();
}

// The SAT cells are GetExtN(value / max) of the CPU transfer function
// (ebsrenderer.cpp:636-662); the library sums them on the GPU with the
// reference's double recurrence (SummedAreaTable3D<double>::BuildSAT).
bool HipExtinctionBasedShading::UploadExtinctionSAT ()
{
  vis::StructuredGridVolume* v = m_ext_data_manager->GetCurrentStructuredVolume();
  vis::TransferFunction* tf = m_ext_data_manager->GetCurrentTransferFunction();
  const bool u16 = v->m_data_storage_size == vis::DataStorageSize::_16_BITS;
  const double vmax = u16 ? 65535.0 : 255.0;
  std::vector<float> lut(u16 ? 65536 : 256);
  for (size_t i = 0; i < lut.size(); i++) lut[i] = tf->GetExtN((double)i / vmax);
  if (cvr_set_extinction_sat(m_cvr, lut.data(), (int)lut.size()) != CVR_OK)
    return Fail("cvr_set_extinction_sat");
  return true;
}

bool HipExtinctionBasedShading::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume() || !UploadTransferFunction() || !UploadGradient(m_apply_gradient_shading) ||
      !UploadExtinctionSAT())
    return false;
  vis::StructuredGridVolume* vold = m_ext_data_manager->GetCurrentStructuredVolume();
  float v_w = vold->GetWidth() * vold->GetScaleX();                            // :98-105
  float v_h = vold->GetHeight() * vold->GetScaleY();
  float v_d = vold->GetDepth() * vold->GetScaleZ();
  dir_cone_max_distance = 0.75f * glm::sqrt(v_w * v_w + v_h * v_h + v_d * v_d);
  m_u_step_size = DefaultStep();
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipExtinctionBasedShading::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  m_params.step = m_u_step_size;
  m_params.apply_gradient_shading =
      (m_apply_gradient_shading && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  fill_phong(&m_params, rp);
  copy3(m_params.light_pos, rp->GetBlinnPhongLightingPosition());
  copy3(m_params.light_forward, rp->GetBlinnPhongLightSourceCameraForward());
  m_params.apply_occlusion = apply_ambient_occlusion ? 1 : 0;
  m_params.occlusion_shells = ambient_occlusion_shells;
  m_params.occlusion_radius = ambient_occlusion_radius;
  m_params.apply_shadow = apply_directional_shadows ? 1 : 0;
  m_params.shadow_type = type_of_shadow;
  m_params.shadow_cone_angle_deg = dir_shadow_cone_angle;
  m_params.shadow_sample_interval = dir_shadow_sample_interval;
  m_params.shadow_initial_step = dir_shadow_initial_step;
  m_params.shadow_ui_weight = dir_shadow_user_interface_weight;
  m_params.shadow_max_distance = dir_cone_max_distance;
  return true;
}

// With pre-illumination on, Update's PreComputeLightCache and the cached march are
// one library call; the EBS cache does not depend on the camera, so the library
// recomputes it only when the light, the shading parameters, the volume or the SAT change.
cvr_status HipExtinctionBasedShading::RenderFrame (const cvr_output* out)
{
  if (pre_illumination)
    return cvr_render_extbsd_preillum(m_cvr, &frame_, &m_params, light_cache_resolution, out);
  return cvr_render_extbsd(m_cvr, &frame_, &m_params, out);
}

////////////////////////////////////////////////////////////////////////////////
// RC1PVoxelConeTracingSGPU (vctrenderer.cpp:27-250, preprocessingstages.cpp)
////////////////////////////////////////////////////////////////////////////////
HipVoxelConeTracingSGPU::HipVoxelConeTracingSGPU ()
  : m_u_step_size(0.5f)
  , m_apply_gradient_shading(false)
  , apply_ambient_occlusion(true)              // vctrenderer.cpp:33-43
  , apply_voxel_cone_tracing(true)
  , cone_step_size(2.0f)
  , cone_step_size_increase_rate(1.0f)
  , cone_initial_step(2.0f)
  , cone_apex_angle(2.0f)
  , apply_correction_factor(true)
  , opacity_correction_factor(2.0f)
  , cone_number_of_samples(50)
  , covered_distance(0.0f)
  , m_params()
{
  cvr_vct_params_default(&m_params);
}

// The table integrates GetOpc(i, GetMaxDensity()) of the CPU transfer function
// (preprocessingstages.cpp:153-173); the library builds the supervoxel pyramid on the
// GPU and the table on the host (cvr_vct_precompute).
bool HipVoxelConeTracingSGPU::UploadOpacities ()
{
  vis::TransferFunction* tf = m_ext_data_manager->GetCurrentTransferFunction();
  std::vector<float> opc(CVR_VCT_TABLE_WIDTH);
  for (size_t i = 0; i < opc.size(); i++) opc[i] = tf->GetOpc((double)i, 255.0);
  if (cvr_vct_set_opacity(m_cvr, opc.data(), (int)opc.size()) != CVR_OK) return Fail("cvr_vct_set_opacity");
  if (cvr_vct_precompute(m_cvr) != CVR_OK) return Fail("cvr_vct_precompute");
  return true;
}

bool HipVoxelConeTracingSGPU::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume() || !UploadTransferFunction() || !UploadGradient(m_apply_gradient_shading) ||
      !UploadOpacities())
    return false;
  m_u_step_size = DefaultStep();                                               // :114-115
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipVoxelConeTracingSGPU::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  m_params.step = m_u_step_size;
  m_params.apply_gradient_shading =
      (m_apply_gradient_shading && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  fill_phong(&m_params, rp);
  copy3(m_params.light.position, rp->GetBlinnPhongLightingPosition());
  copy3(m_params.light.forward, rp->GetBlinnPhongLightSourceCameraForward());
  copy3(m_params.light.up, rp->GetBlinnPhongLightSourceCameraUp());
  copy3(m_params.light.right, rp->GetBlinnPhongLightSourceCameraRight());
  m_params.light.spot_angle_deg = rp->GetSpotLightMaxAngle();
  m_params.apply_occlusion = apply_ambient_occlusion ? 1 : 0;
  m_params.apply_shadow = apply_voxel_cone_tracing ? 1 : 0;
  m_params.cone_step = cone_step_size;
  m_params.cone_step_increase_rate = cone_step_size_increase_rate;
  m_params.cone_initial_step = cone_initial_step;
  m_params.cone_apex_angle_deg = cone_apex_angle;
  m_params.apply_correction = apply_correction_factor ? 1 : 0;
  m_params.correction_factor = opacity_correction_factor;
  m_params.samples = cone_number_of_samples;
  return true;
}

cvr_status HipVoxelConeTracingSGPU::RenderFrame (const cvr_output* out)
{
  return cvr_render_vct(m_cvr, &frame_, &m_params, out);
}

////////////////////////////////////////////////////////////////////////////////
// SBTMDirectionalOcclusionShading (sbtmdosrenderer.cpp:20-174)
////////////////////////////////////////////////////////////////////////////////
HipSBTMDirectionalOcclusionShading::HipSBTMDirectionalOcclusionShading ()
  : m_u_step_size(0.5f)
  , cone_half_angle(50.0f)                     // sbtmdosrenderer.cpp:37-43
  , evaluate_dir_occlusion(true)
  , grid_size(2.0f)
  , max_number_of_passes(90000)
  , occ_ui_weight_percentage(1.0f)
  , m_params()
{
  cvr_sbtm_params_default(&m_params);
}

bool HipSBTMDirectionalOcclusionShading::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume() || !UploadTransferFunction()) return false;
  m_u_step_size = DefaultStep();                                               // :111-112
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipSBTMDirectionalOcclusionShading::Update (vis::Camera* camera)
{
  FillFrame(camera);
  m_params.step = m_u_step_size;
  m_params.cone_half_angle_deg = cone_half_angle;
  m_params.grid_x = (int)grid_size.x;
  m_params.grid_y = (int)grid_size.y;
  m_params.attenuation = occ_ui_weight_percentage;
  m_params.max_passes = max_number_of_passes;
  return true;
}

cvr_status HipSBTMDirectionalOcclusionShading::RenderFrame (const cvr_output* out)
{
  return cvr_render_sbtm(m_cvr, &frame_, &m_params, out);
}

////////////////////////////////////////////////////////////////////////////////
// The isosurface ray-casters (rc1pisoadapt, rc1pisocustom, rc1pisodfscustom)
////////////////////////////////////////////////////////////////////////////////
HipIsoRayCasterBase::HipIsoRayCasterBase (int variant)
  : m_u_isovalue(0.5f)                 // rc1custompisoadaptrenderer.cpp:121-126
  , m_u_step_size_small(0.05f)
  , m_u_step_size_large(1.0f)
  , m_u_step_size_range(0.1f)
  , m_u_color(0.66f, 0.6f, 0.05f, 1.0f)
  , m_apply_gradient_shading(false)
  , m_params()
{
  cvr_iso_params_default(variant, &m_params);
}

// No transfer function: the block min/max table ComputeBlocksFromVolume builds on
// the CPU (rc1custompisoadaptrenderer.cpp:20-117) is built by the library on the GPU.
bool HipIsoRayCasterBase::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume() || !UploadGradient(m_apply_gradient_shading)) return false;
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

bool HipIsoRayCasterBase::Update (vis::Camera* camera)
{
  FillFrame(camera);
  m_params.isovalue = m_u_isovalue;
  m_params.step_small = m_u_step_size_small;
  m_params.step_large = m_u_step_size_large;
  m_params.step_range = m_u_step_size_range;
  for (int i = 0; i < 4; i++) m_params.color[i] = m_u_color[i];
  m_params.apply_gradient_shading =
      (m_apply_gradient_shading && m_ext_data_manager->GetCurrentGradientTexture()) ? 1 : 0;
  fill_phong(&m_params, m_ext_rendering_parameters);
  copy3(m_params.light_pos, m_ext_rendering_parameters->GetBlinnPhongLightingPosition());
  return true;
}

cvr_status HipIsoRayCasterBase::RenderFrame (const cvr_output* out)
{
  return cvr_render_iso(m_cvr, &frame_, &m_params, out);
}

// rc1custompisoadaptrenderer.cpp:349-355
void HipIsoRayCasterBase::FillParameterSpace (ParameterSpace& pspace)
{
  pspace.ClearParameterDimensions();
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeSmall", &m_u_step_size_small, 0.01f, 0.25f, 0.05f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeLarge", &m_u_step_size_large, 0.25f, 2.0f, 0.25f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeRange", &m_u_step_size_range, 0.05f, 0.26f, 0.05f));
}

////////////////////////////////////////////////////////////////////////////////
// DeferredShading (DeferredShading.cpp:118-131, 322-551)
////////////////////////////////////////////////////////////////////////////////
HipDeferredShading::HipDeferredShading ()
  : m_u_isovalue(0.5f)                 // DeferredShading.cpp:123-128
  , m_u_step_size_small(0.05f)
  , m_u_step_size_large(1.0f)
  , m_u_step_size_range(0.1f)
  , m_u_color(0.66f, 0.6f, 0.05f, 1.0f)
  , m_apply_gradient_shading(false)
  , m_params()
  , m_kept_frame()
  , m_kept_params()
  , m_geometry_kept(false)
{
  cvr_deferred_params_default(&m_params);
}

// No transfer function and no gradient texture: the normal is the shader's own central
// difference.  The block table (ComputeBlocksFromVolume, :20-113) is the library's.
bool HipDeferredShading::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume()) return false;
  m_geometry_kept = false;
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

// UpdateGeometryPassUniforms / UpdateLightingPassUniforms (:447-484).  fill_phong's
// BlinnPhongIspecular is no uniform of lighting_pass.comp.
bool HipDeferredShading::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  m_params.isovalue = m_u_isovalue;
  m_params.step_small = m_u_step_size_small;
  m_params.step_large = m_u_step_size_large;
  m_params.step_range = m_u_step_size_range;
  for (int i = 0; i < 4; i++) m_params.color[i] = m_u_color[i];
  m_params.ka = rp->GetBlinnPhongKambient();
  m_params.kd = rp->GetBlinnPhongKdiffuse();
  m_params.ks = rp->GetBlinnPhongKspecular();
  m_params.shininess = rp->GetBlinnPhongNshininess();
  copy3(m_params.light_pos, rp->GetBlinnPhongLightingPosition());
  return true;
}

// The march parameters of two parameter blocks are the same
static bool same_geometry (const cvr_deferred_params& a, const cvr_deferred_params& b)
{
  return a.isovalue == b.isovalue && a.step_small == b.step_small && a.step_large == b.step_large &&
         a.step_range == b.step_range && !std::memcmp(a.num_blocks, b.num_blocks, sizeof(a.num_blocks)) &&
         !std::memcmp(a.gbuffer_clear, b.gbuffer_clear, sizeof(a.gbuffer_clear));
}

cvr_status HipDeferredShading::RenderFrame (const cvr_output* out)
{
  if (m_geometry_kept && !std::memcmp(&frame_, &m_kept_frame, sizeof(cvr_frame)) &&
      same_geometry(m_params, m_kept_params))
    return cvr_deferred_shade(m_cvr, frame_.width, frame_.height, &m_params, out);
  m_geometry_kept = false;
  const cvr_status st = cvr_render_deferred(m_cvr, &frame_, &m_params, out);
  if (st == CVR_OK) {
    m_kept_frame = frame_;
    m_kept_params = m_params;
    m_geometry_kept = true;
  }
  return st;
}

// DeferredShading.cpp:545-551
void HipDeferredShading::FillParameterSpace (ParameterSpace& pspace)
{
  pspace.ClearParameterDimensions();
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeSmall", &m_u_step_size_small, 0.01f, 0.25f, 0.05f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeLarge", &m_u_step_size_large, 0.25f, 2.0f, 0.25f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeRange", &m_u_step_size_range, 0.05f, 0.26f, 0.05f));
}

////////////////////////////////////////////////////////////////////////////////
// AdvancedDeferredShading (AdvancedDeferredShading.cpp:119-135, 532-765)
////////////////////////////////////////////////////////////////////////////////
HipAdvancedDeferredShading::HipAdvancedDeferredShading ()
  : m_u_isovalue(0.5f)                 // AdvancedDeferredShading.cpp:124-130
  , m_u_step_size_small(0.05f)
  , m_u_step_size_large(1.0f)
  , m_u_step_size_range(0.1f)
  , m_u_color(0.66f, 0.6f, 0.05f, 1.0f)
  , m_current_time(0.0f)
  , m_flow_speed(1.0f)                 // AdvancedDeferredShading.h:129-133
  , m_flow_scale(10.0f)
  , m_show_ridges(true)
  , m_show_valleys(true)
  , m_accessibility_strength(0.5f)
  , s(0.6f)                            // Init (:536-537)
  , v(0.2f)
  , m_params()
  , m_kept_frame()
  , m_kept_params()
  , m_geometry_kept(false)
{
  cvr_advdeferred_params_default(&m_params);
}

bool HipAdvancedDeferredShading::Init (int swidth, int sheight)
{
  if (IsBuilt()) Clean();
  if (m_ext_data_manager->GetCurrentVolumeTexture() == nullptr) return false;
  if (!UploadVolume()) return false;
  m_geometry_kept = false;
  Reshape(swidth, sheight);
  SetBuilt(true);
  SetOutdated();
  return true;
}

// UpdateGeometryPassUniforms (:661-689) and LightingPass's uniforms (:371-380).  Ka, Kd, Ks
// and the shininess are constants of lighting_pass.comp: the library's defaults stay.
bool HipAdvancedDeferredShading::Update (vis::Camera* camera)
{
  vis::RenderingParameters* rp = m_ext_rendering_parameters;
  FillFrame(camera);
  m_params.isovalue = m_u_isovalue;
  m_params.step_small = m_u_step_size_small;
  m_params.step_large = m_u_step_size_large;
  m_params.step_range = m_u_step_size_range;
  for (int i = 0; i < 4; i++) m_params.color[i] = m_u_color[i];
  copy3(m_params.light_pos, rp->GetBlinnPhongLightingPosition());
  m_params.time = m_current_time;
  m_params.flow_speed = m_flow_speed;
  m_params.flow_scale = m_flow_scale;
  m_params.show_ridges = m_show_ridges ? 1 : 0;
  m_params.show_valleys = m_show_valleys ? 1 : 0;
  m_params.accessibility_strength = m_accessibility_strength;
  m_params.colormap_s = s;
  m_params.colormap_v = v;
  return true;
}

static bool same_geometry (const cvr_advdeferred_params& a, const cvr_advdeferred_params& b)
{
  return a.isovalue == b.isovalue && a.step_small == b.step_small && a.step_large == b.step_large &&
         a.step_range == b.step_range && !std::memcmp(a.num_blocks, b.num_blocks, sizeof(a.num_blocks)) &&
         !std::memcmp(a.gbuffer_clear, b.gbuffer_clear, sizeof(a.gbuffer_clear));
}

cvr_status HipAdvancedDeferredShading::RenderFrame (const cvr_output* out)
{
  if (m_geometry_kept && !std::memcmp(&frame_, &m_kept_frame, sizeof(cvr_frame)) &&
      same_geometry(m_params, m_kept_params))
    return cvr_advdeferred_shade(m_cvr, frame_.width, frame_.height, &m_params, out);
  m_geometry_kept = false;
  const cvr_status st = cvr_render_advdeferred(m_cvr, &frame_, &m_params, out);
  if (st == CVR_OK) {
    m_kept_frame = frame_;
    m_kept_params = m_params;
    m_geometry_kept = true;
  }
  return st;
}

// AdvancedDeferredShading.cpp:759-765
void HipAdvancedDeferredShading::FillParameterSpace (ParameterSpace& pspace)
{
  pspace.ClearParameterDimensions();
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeSmall", &m_u_step_size_small, 0.01f, 0.25f, 0.05f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeLarge", &m_u_step_size_large, 0.25f, 2.0f, 0.25f));
  pspace.AddParameterDimension(new ParameterRangeFloat("StepSizeRange", &m_u_step_size_range, 0.05f, 0.26f, 0.05f));
}
