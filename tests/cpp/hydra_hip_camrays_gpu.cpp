// The driver loop of cam_plugin/main_with_cam_gpu.cpp:149-284 on the C ABI: a device camera (CamPinHoleHIP / CamTableLensHIP, cam_rays_hip.h)
// makes the rays of every tile, Integrator::PathTraceFromInputRaysBlock traces them, the camera adds the colours to the frame - rays, colours
// and frame stay in device memory (hpt_cam_render_dev); the frame comes back once, at the end.
//
//   hydra_hip_camrays_gpu <scene.xml> <width> <height> <spp> <out.bin> [tile] [pinhole|tablelens] [--spectral]
//
// The pinhole has the scene camera's field of view. The table lens takes the scene's <optical_system> when it has one, else the double-Gauss
// 50 mm f/2 prescription of tests/golden/make_env_scene.py on a 35 mm sensor diagonal.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../hydracore3_amd/csrc/scene_loader.h"
#include "../../hydracore3_amd/csrc/cam_rays_hip.h"

int main(int argc, char** argv)
{
  const char* tag = "[hydra_hip_camrays_gpu]";
  bool spectral = false, tableLens = false; std::vector<const char*> pos;
  for (int i = 1; i < argc; i++) {
    if (!std::strcmp(argv[i], "--spectral")) spectral = true;
    else if (!std::strcmp(argv[i], "tablelens")) tableLens = true;
    else if (!std::strcmp(argv[i], "pinhole")) tableLens = false;
    else pos.push_back(argv[i]);
  }
  if (pos.size() < 5) { std::fprintf(stderr, "usage: %s <scene.xml> <width> <height> <spp> <out.bin> [tile] [pinhole|tablelens] [--spectral]\n", argv[0]); return 2; }
  const int W = std::atoi(pos[1]), H = std::atoi(pos[2]), spp = std::atoi(pos[3]);
  const int MEGA_TILE_SIZE = pos.size() > 5 ? std::atoi(pos[5]) : 512 * 512;                   // main_with_cam_gpu.cpp:99
  if (W <= 0 || H <= 0 || spp <= 0 || MEGA_TILE_SIZE <= 0) { std::fprintf(stderr, "%s: bad sizes\n", tag); return 2; }
  hydra_hip::LoadedScene sc; std::string err;
  if (!hydra_hip::LoadHydraXml(pos[0], W, H, sc, err, spectral)) { std::fprintf(stderr, "%s: %s\n", tag, err.c_str()); return 1; }
  std::vector<float> lines = sc.lensLines; float physSize[2] = { sc.physSize[0], sc.physSize[1] };
  sc.lensLines.clear();                                                                      // the integrator is a plain consumer of the camera's rays
  hpt_ctx* ctx = nullptr;
  if (hpt_create(0, &ctx) != HPT_OK) { std::fprintf(stderr, "%s: no HIP device\n", tag); return 1; }
  if (sc.upload(ctx) != HPT_OK) { std::fprintf(stderr, "%s: %s\n", tag, hpt_last_error(ctx)); return 1; }
  if (hpt_init_random_gens(ctx, (uint32_t)MEGA_TILE_SIZE) != HPT_OK) { std::fprintf(stderr, "%s: %s\n", tag, hpt_last_error(ctx)); return 1; }

  hydra_hip::CamParameters cp; cp.spectralMode = spectral ? 1 : 0;
  { const hpt_params p = sc.params(); std::memcpy(cp.projInv, p.projInv, sizeof(cp.projInv)); }
  hydra_hip::CamPinHoleHIP pinhole(ctx); hydra_hip::CamTableLensHIP lens(ctx);
  hydra_hip::CamRaysHIP* pCamImpl = tableLens ? static_cast<hydra_hip::CamRaysHIP*>(&lens) : &pinhole;
  if (tableLens) {
    if (lines.empty()) {
      static const float dgauss[11][4] = { {29.475f, 3.76f, 1.67f, 12.6f}, {84.83f, 0.12f, 1.0f, 12.6f}, {19.275f, 4.025f, 1.67f, 11.5f}, {40.77f, 3.275f, 1.699f, 11.5f},
        {12.75f, 5.705f, 1.0f, 9.0f}, {0.0f, 4.5f, 0.0f, 8.55f}, {-14.495f, 1.18f, 1.603f, 8.5f}, {40.77f, 6.065f, 1.658f, 10.0f}, {-20.385f, 0.19f, 1.0f, 10.0f},
        {437.065f, 3.22f, 1.717f, 10.0f}, {-39.73f, 36.9f, 1.0f, 10.0f} };                    // millimetres, front element first
      for (int i = 10; i >= 0; i--) { lines.push_back(0.001f * dgauss[i][0]); lines.push_back(0.001f * dgauss[i][1]); lines.push_back(dgauss[i][2]); lines.push_back(0.001f * dgauss[i][3]); }
      const float diagonal = 0.035f, aspect = float(H) / float(W);
      physSize[0] = 2.0f * std::sqrt(diagonal * diagonal / (1.0f + aspect * aspect)); physSize[1] = aspect * physSize[0];
    }
    lens.SetLens(lines.data(), (uint32_t)(lines.size() / 4), physSize[0], physSize[1]);
  }
  pCamImpl->SetParameters(W, H, cp);
  pCamImpl->SetBatchSize(MEGA_TILE_SIZE);

  void* frameDev = nullptr;
  const size_t frameBytes = (size_t)W * H * 4 * sizeof(float);
  if (hpt_device_malloc(ctx, frameBytes, &frameDev) != HPT_OK || hpt_device_memset(ctx, frameDev, 0, frameBytes) != HPT_OK) { std::fprintf(stderr, "%s: %s\n", tag, hpt_last_error(ctx)); return 1; }
  std::vector<float> realColor((size_t)W * H * 4, 0.0f);
  const auto start = std::chrono::high_resolution_clock::now();
  if (!pCamImpl->RenderDev((float*)frameDev, (uint32_t)spp)) return 1;
  if (hpt_device_copy(ctx, realColor.data(), frameDev, frameBytes, 2) != HPT_OK) { std::fprintf(stderr, "%s: %s\n", tag, hpt_last_error(ctx)); return 1; }   // waits for the loop
  const double wallMs = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - start).count();
  float tMake[4] = {0, 0, 0, 0}, tTrace[4] = {0, 0, 0, 0}, tContrib[4] = {0, 0, 0, 0}, tRender[4] = {0, 0, 0, 0};
  pCamImpl->GetExecutionTime("MakeRaysBlock", tMake); pCamImpl->GetExecutionTime("PathTraceFromInputRays", tTrace);
  pCamImpl->GetExecutionTime("AddSamplesContributionBlock", tContrib); pCamImpl->GetExecutionTime("Render", tRender);
  (void)hpt_device_free(ctx, frameDev);

  FILE* f = std::fopen(pos[4], "wb");
  if (!f) { std::fprintf(stderr, "cannot write %s\n", pos[4]); return 1; }
  std::fwrite(realColor.data(), sizeof(float), realColor.size(), f); std::fclose(f);
  double s = 0.0; for (size_t i = 0; i < realColor.size(); i += 4) s += realColor[i] + realColor[i + 1] + realColor[i + 2];
  std::printf("%s: %dx%d @ %d spp in tiles of %d, %s%s, mean radiance %.5f, wall (loop + read-back) = %.3f ms, device loop = %.3f ms over %.0f tiles; "
              "of the first %.0f tiles: MakeRaysBlock = %.3f ms, PathTraceFromInputRays = %.3f ms, AddSamplesContributionBlock = %.3f ms\n", tag, W, H, spp, MEGA_TILE_SIZE,
              tableLens ? "table lens" : "pinhole", spectral ? ", spectral" : "", s / (3.0 * W * H * spp), wallMs, tRender[0], tRender[1], tRender[2], tMake[0], tTrace[0], tContrib[0]);
  return 0;
}
