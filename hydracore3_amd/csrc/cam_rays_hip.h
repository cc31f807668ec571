// Host-side C++ adapters over the camera part of the C ABI (include/hydra_hip.h: hpt_cam_*), shaped like the reference's camera plug-ins so
// that they drop in where a driver creates its ICamRaysAPI2 camera (cam_plugin/main_with_cam.cpp:96-166, main_with_cam_gpu.cpp:149-266):
//
//   hydra_hip::CamPinHoleHIP    <->  CamPinHole    (cam_plugin/CamPinHole.h, CamPinHole.cpp)
//   hydra_hip::CamTableLensHIP  <->  CamTableLens  (cam_plugin/CamTableLens.h, CamTableLens.cpp)
//
// The method set is ICamRaysAPI2's (cam_plugin/CamPluginAPI.h:39-77). The reference's headers cannot be included here (they need the absent
// LiteMath), so CamParameters carries the inverse projection the reference derives with perspectiveMatrix / inverse4x4: the caller's matrix
// code makes it, as it does for the scene's camera. Header-only; link against hydracore3_amd/libhydra_hip.so. Failures print the library's
// message and return, the reference's convention.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hydra_hip.h"

namespace hydra_hip {

struct RayPosAndW { float origin[3]; float wave; };        // CamPluginAPI.h:27-31
struct RayDirAndT { float direction[3]; float time; };     // :33-37

struct CamParameters                                       // CamPluginAPI.h:7-15, with m_projInv in place of the four numbers it is made from
{
  float projInv[16];                                       // inverse4x4(perspectiveMatrix(fov, aspect, nearPlane, farPlane)), column-major
  int   spectralMode = 0;
};

class CamRaysHIP                                           // ICamRaysAPI2 over one hpt_cam
{
public:
  CamRaysHIP(hpt_ctx* a_ctx, int a_kind, const char* a_name) : m_ctx(a_ctx), m_name(a_name)
  { if (hpt_cam_create(a_ctx, a_kind, &m_cam) != HPT_OK) { report("constructor"); m_cam = nullptr; } }
  virtual ~CamRaysHIP() { if (m_cam) hpt_cam_destroy(m_cam); }          // (before the context it was made from)
  CamRaysHIP(const CamRaysHIP&) = delete;
  CamRaysHIP& operator=(const CamRaysHIP&) = delete;
  bool valid() const { return m_cam != nullptr; }
  hpt_cam* handle() const { return m_cam; }

  virtual void SetParameters(int a_width, int a_height, const CamParameters& a_params)
  { if (hpt_cam_set_parameters(m_cam, uint32_t(a_width), uint32_t(a_height), a_params.projInv, a_params.spectralMode) != HPT_OK) report("SetParameters"); }
  virtual void SetBatchSize(int a_tileSize) { if (hpt_cam_set_batch_size(m_cam, uint32_t(a_tileSize)) != HPT_OK) report("SetBatchSize"); }
  virtual void MakeRaysBlock(RayPosAndW* out_rayPosAndNear4f, RayDirAndT* out_rayDirAndFar4f, uint32_t in_blockSize, int subPassId)
  { if (hpt_cam_make_rays_block(m_cam, &out_rayPosAndNear4f->origin[0], &out_rayDirAndFar4f->direction[0], in_blockSize, subPassId) != HPT_OK) report("MakeRaysBlock"); }
  virtual void AddSamplesContributionBlock(float* out_color4f, const float* colors4f, uint32_t in_blockSize, uint32_t a_width, uint32_t a_height, int subPassId)
  { if (hpt_cam_add_samples_contribution_block(m_cam, out_color4f, colors4f, in_blockSize, a_width, a_height, subPassId) != HPT_OK) report("AddSamplesContributionBlock"); }
  virtual void CommitDeviceData() {}                                     // the state lives on the device from SetBatchSize on
  virtual void GetExecutionTime(const char* a_funcName, float a_out[4]) { (void)hpt_cam_get_execution_time(m_cam, a_funcName, a_out); }

  // the *Cmd forms of the generated classes (main_with_cam_gpu.cpp:252-254): device pointers, enqueued on a stream
  bool MakeRaysBlockDev(float* rayPosDev, float* rayDirDev, uint32_t in_blockSize, int subPassId, void* stream = nullptr)
  { return check(hpt_cam_make_rays_block_dev(m_cam, rayPosDev, rayDirDev, in_blockSize, subPassId, stream), "MakeRaysBlock"); }
  bool AddSamplesContributionBlockDev(float* out_color4fDev, const float* colorsDev, uint32_t in_blockSize, uint32_t a_width, uint32_t a_height, int subPassId, void* stream = nullptr)
  { return check(hpt_cam_add_samples_contribution_block_dev(m_cam, out_color4fDev, colorsDev, in_blockSize, a_width, a_height, subPassId, stream), "AddSamplesContributionBlock"); }
  // the loop of main_with_cam_gpu.cpp:230-266 for `passes` samples per pixel, frame resident on the device
  bool RenderDev(float* frame4fDev, uint32_t passes, void* stream = nullptr) { return check(hpt_cam_render_dev(m_ctx, m_cam, frame4fDev, passes, stream), "RenderDev"); }

protected:
  bool check(int rc, const char* what) { if (rc != HPT_OK) report(what); return rc == HPT_OK; }
  void report(const char* what) { std::printf("[%s::%s]: %s\n", m_name, what, hpt_last_error(m_ctx)); }
  hpt_ctx* m_ctx; hpt_cam* m_cam = nullptr; const char* m_name;
};

class CamPinHoleHIP : public CamRaysHIP
{
public:
  explicit CamPinHoleHIP(hpt_ctx* a_ctx) : CamRaysHIP(a_ctx, 0, "CamPinHoleHIP") {}
};

class CamTableLensHIP : public CamRaysHIP
{
public:
  explicit CamTableLensHIP(hpt_ctx* a_ctx) : CamRaysHIP(a_ctx, 1, "CamTableLensHIP") {}
  // `lines` and m_physSize of CamTableLens::Init (CamTableLens.cpp:87-112): a_lines4 = n x {curvatureRadius, thickness, eta, apertureRadius}, film side first
  void SetLens(const float* a_lines4, uint32_t a_n, float a_physSizeX, float a_physSizeY)
  { if (hpt_cam_set_lens(m_cam, a_lines4, a_n, a_physSizeX, a_physSizeY) != HPT_OK) report("SetLens"); }
};

} // namespace hydra_hip
