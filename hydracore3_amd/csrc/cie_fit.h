// The CIE 1931 observer table the loaders hand over as m_cie_xyz (scene_loader.h) and the camera plug-in falls back to when no spectral scene
// was uploaded (hpt_host.hip: hpt_cam_*). Header-only host C++.
#pragma once
#include <cmath>
#include <vector>

namespace hydra_hip {

// m_cie_xyz for the fixture tools: the reference carries the tabulated CIE 1931 observer in its source; this image has no other copy, so the
// loaders use the multi-lobe analytic fit of Wyman, Sloan and Shirley (JCGT 2013). A HydraCore3 host passes its own table instead.
inline std::vector<float> cieXyzFit()
{
  std::vector<float> t(471 * 4, 0.0f);
  auto g = [](double lam, double mu, double s1, double s2) { const double q = (lam - mu) / (lam < mu ? s1 : s2); return std::exp(-0.5 * q * q); };
  for (int c = 0; c < 471; c++) {
    const double lam = 360.0 + c;
    t[4 * c + 0] = (float)(1.056 * g(lam, 599.8, 37.9, 31.0) + 0.362 * g(lam, 442.0, 16.0, 26.7) - 0.065 * g(lam, 501.1, 20.4, 26.2));
    t[4 * c + 1] = (float)(0.821 * g(lam, 568.8, 46.9, 40.5) + 0.286 * g(lam, 530.9, 16.3, 31.1));
    t[4 * c + 2] = (float)(1.217 * g(lam, 437.0, 11.8, 36.0) + 0.681 * g(lam, 459.0, 26.0, 13.8));
  }
  return t;
}

} // namespace hydra_hip
