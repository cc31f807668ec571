// The HR2 driver in the render mode the reference's driver is in today (hydra_api/hydra_cpu.cpp:105): Render() = SetFrameBufferSize, SetViewport,
// UpdateMembersPlainData, PackXYBlock, CastSingleRayBlock - the preview frame, 4 floats per pixel, assigned.
//   hydra_hip_hr2_preview <scene.xml> <width> <height> <out.bin>
// The driver reads the meshes from the scene's files here (hydra_hip_hr2 covers the by-pointer leg). The frame starts as a bit pattern, so the
// test sees that every pixel was assigned; it compares the file with HipIntegrator.CastSingleRayBlock of the same scene: bit-identical.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../hydracore3_amd/csrc/hydra_driver_hip.h"

using namespace hydra_hip;

int main(int argc, char** argv)
{
  if (argc < 5) { std::fprintf(stderr, "usage: %s <scene.xml> <width> <height> <out.bin>\n", argv[0]); return 2; }
  const std::string xmlPath = argv[1];
  const int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  std::vector<uint8_t> raw; if (!detail::readFile(xmlPath, raw)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  const std::string text(raw.begin(), raw.end());
  const size_t slash = xmlPath.find_last_of("/\\");
  const std::string folder = slash == std::string::npos ? std::string(".") : xmlPath.substr(0, slash);

  auto driver = std::make_shared<HR2::HydraHipRenderDriver>(0);
  if (!driver->valid()) { std::fprintf(stderr, "[hydra_hip_hr2_preview]: no HIP device\n"); return 1; }
  HR2::RDScene_Input none;
  if (!driver->LoadScene(text, folder, none, HR2::SCN_UPDATE_ALL)) { std::fprintf(stderr, "[hydra_hip_hr2_preview]: %s\n", driver->lastError().c_str()); return 1; }
  driver->CommitDeviceData();
  driver->SetRenderMode(HR2::HydraHipRenderDriver::RENDER_CAST_SINGLE_RAY);
  std::vector<float> frame((size_t)W * H * 4);
  const uint32_t pattern = 0xDEADBEEFu;
  for (float& v : frame) std::memcpy(&v, &pattern, 4);
  driver->Render(0, 0, W, (uint32_t)H, 4, frame.data(), 1);
  if (!driver->lastError().empty()) { std::fprintf(stderr, "[hydra_hip_hr2_preview]: %s\n", driver->lastError().c_str()); return 1; }
  FILE* f = std::fopen(argv[4], "wb"); if (!f) return 1;
  std::fwrite(frame.data(), sizeof(float), frame.size(), f); std::fclose(f);
  std::printf("[hydra_hip_hr2_preview]: %dx%d, CastSingleRayBlock\n", W, H);
  return 0;
}
