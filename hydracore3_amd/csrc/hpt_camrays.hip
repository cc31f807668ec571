// The camera plug-in's two cameras on the device: kernel1D_MakeEyeRay and kernel1D_ContribSample of CamPinHole (cam_plugin/CamPinHole.cpp:52-131)
// and CamTableLens (cam_plugin/CamTableLens.cpp:219-319), so that the loop of cam_plugin/main_with_cam_gpu.cpp:230-266 - make rays, trace them,
// add the colours to the frame - keeps rays, colours and frame in HBM (hpt_host.hip: hpt_cam_*).
//
// One lane per ray in blocks of 256, the grid sized to the tile (the cost per ray is uniform: no work queue). A ray record and a frame pixel are
// one 16-byte access each; the camera's scalars and the lens lines are kernel arguments / one small buffer read at wave-uniform addresses.
// The arithmetic is the reference's in the reference's order (-ffp-contract=off like every unit); the lens trace is hpt_shade.h's with the
// cameras' own root finder, which works in double where the integrator's is float throughout.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"

namespace hpt {

// Quadratic of CamTableLens.cpp:15-38: the discriminant and its root in double, the root rounded to float, q = -.5 * (B -+ root) a double
// product of float operands rounded to float (the double literal only scales the float difference by a power of two)
struct CamQuadratic
{
  HPT_DEV bool operator()(float A, float B, float C, float& t0, float& t1) const
  {
    const double discrim = (double)B * (double)B - 4. * (double)A * (double)C;
    if (discrim < 0.) return false;
    const float floatRootDiscrim = float(__builtin_sqrt(discrim));
    const float q = (B < 0) ? float(-.5 * double(B - floatRootDiscrim)) : float(-.5 * double(B + floatRootDiscrim));
    t0 = q / A; t1 = C / q;
    if (t0 > t1) { const float temp = t0; t0 = t1; t1 = temp; }
    return true;
  }
};

// SampleWavelengths (spectrum.h:58-75), the first of the four (the cameras keep wavelengths.x only)
HPT_DEV float camFirstWavelength(float u) { return lerpf(LAMBDA_MIN, LAMBDA_MAX, u); }

// SpectrumToXYZ(color, wavelengths, 360, 830, cie, false) + XYZToRGB (spectrum.h:151-219) for four equal samples at four equal wavelengths
HPT_DEV V3 camSpectrumToRGB(const float4* cie, uint numCie, float data, float wave)
{
  const float pdf = 1.0f / (LAMBDA_MAX - LAMBDA_MIN);
  const float CIE_Y_integral = 106.856895f;
  const float s = (pdf != 0.0f) ? data / pdf : 0.0f;
  const uint offset = (uint)(floorf(wave + 0.5f) - LAMBDA_MIN);
  float cx = 0.0f, cy = 0.0f, cz = 0.0f;
  if (offset < 471u && offset < numCie) { const float4 c = cie[offset]; cx = c.x; cy = c.y; cz = c.z; }
  const float X = cx * s, Y = cy * s, Z = cz * s;
  const float x = ((((X + X) + X) + X) / 4.0f) / CIE_Y_integral;          // SpectrumAverage: left-to-right sum / SPECTRUM_SAMPLE_SZ
  const float y = ((((Y + Y) + Y) + Y) / 4.0f) / CIE_Y_integral;
  const float z = ((((Z + Z) + Z) + Z) / 4.0f) / CIE_Y_integral;
  return v3(+3.240479f * x - 1.537150f * y - 0.498535f * z, -0.969256f * x + 1.875991f * y + 0.041556f * z, +0.055648f * x - 0.204043f * y + 1.057311f * z);
}

template <int KIND, bool SPECTRAL>
__global__ void __launch_bounds__(256) camMakeRaysKernel(const CamJob job)
{
  const uint tid = blockIdx.x * 256u + threadIdx.x;
  if (tid >= job.n) return;
  const uint p = job.firstPixel + tid;
  const uint x = p % job.width, y = p / job.width;                        // pitch-linear layout
  const float xn = (float(x) + 0.5f) / float(job.width), yn = (float(y) + 0.5f) / float(job.height);
  V3 rayPos = v3(0, 0, 0), rayDir;
  float wave = 0.0f;
  if (KIND == CAM_PINHOLE) {
    V4 pos = v4(2.0f * xn - 1.0f, 2.0f * yn - 1.0f, 0.0f, 1.0f);          // EyeRayDirNormalized (cglobals.h:49-55)
    pos = mul4x4(job.projInv, pos);
    rayDir = normalize(v3(pos.x / pos.w, pos.y / pos.w, pos.z / pos.w));
    if (SPECTRAL) {                                                       // the generator is touched in spectral mode only
      Rng gen = job.gens[tid];
      wave = camFirstWavelength(rng_float1(gen));
      job.gens[tid] = gen;
      job.waves[tid] = wave;                                              // (RGB: the stored wave stays the 0 hpt_cam_set_parameters left)
    }
  } else {
    Rng gen = job.gens[tid];
    const V4 rands = rng_float4(gen);
    job.gens[tid] = gen;
    if (SPECTRAL) wave = camFirstWavelength(rands.z);
    rayPos = v3(0.25f * job.physSize[0] * (2.0f * xn - 1.0f), 0.25f * job.physSize[1] * (2.0f * yn - 1.0f), 0.0f);
    const float4 rear = job.lensLines[0];                                 // LensRearZ() = thickness, LensRearRadius() = apertureRadius of the first line
    const V2 rs = mapSamplesToDisc(v2(rands.x - 0.5f, rands.y - 0.5f));
    const float k = rear.w * 2.0f;
    rayDir = normalize(v3(k * rs.x, k * rs.y, rear.y) - rayPos);
    const float cosTheta = absf(rayDir.z);
    if (!traceLensesFromFilm<CamQuadratic>(job.lensLines, job.lensCount, rayPos, rayDir)) { rayPos = v3(0, -10000000.0f, 0.0f); rayDir = v3(0, -1, 0); }   // "shoot ray under the floor"
    else { rayDir = v3(-1, -1, -1) * normalize(rayDir); rayPos = v3(-1, -1, -1) * rayPos; }
    job.waves[tid] = wave;
    job.cos4[tid] = cosTheta * cosTheta * cosTheta * cosTheta;
  }
  job.rayPos[tid] = make_float4(rayPos.x, rayPos.y, rayPos.z, wave);
  job.rayDir[tid] = make_float4(rayDir.x, rayDir.y, rayDir.z, 0.0f);
}

// every pixel of a tile belongs to one lane: a plain read-modify-write of the pixel, alpha carried through unchanged
template <int KIND, bool SPECTRAL>
__global__ void __launch_bounds__(256) camContribKernel(const CamJob job)
{
  const uint tid = blockIdx.x * 256u + threadIdx.x;
  if (tid >= job.n) return;
  const uint p = job.firstPixel + tid;                                    // = y * width + x
  V3 color;
  if (SPECTRAL) {
    float data = job.colors[tid];
    if (KIND == CAM_TABLE_LENS) data = data * job.cos4[tid];
    color = camSpectrumToRGB(job.cie, job.numCie, data, job.waves[tid]);
  } else {
    const float4 c = ((const float4*)job.colors)[tid];
    color = v3(c.x, c.y, c.z);
    if (KIND == CAM_TABLE_LENS) color = color * job.cos4[tid];
  }
  float4 px = job.frame[p];
  px.x += color.x; px.y += color.y; px.z += color.z;
  job.frame[p] = px;
}

// CamPinHole::Init / CamTableLens::Init: m_randomGens[i] = RandomGenInit(i + 12345 * i). The reference forms the seed in int, which overflows
// from i = 173 942; defined here as 32-bit wrap-around, the wrapped value then taken as the int RandomGenInit is given (crandom.h:25-36: a
// negative seed makes no warm-up step, its a_seed % 7 being <= 0).
__global__ void __launch_bounds__(256) camInitGensKernel(Rng* gens, uint n)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint seed = i + 12345u * i;
  Rng g;
  g.sx = (seed * (seed * seed * 15731u + 74323u) + 871483u);
  g.sy = (seed * (seed * seed * 13734u + 37828u) + 234234u);
  const int warm = (int)seed % 7;
  for (int k = 0; k < warm; k++) rng_next(g);
  gens[i] = g;
}

template __global__ void camMakeRaysKernel<CAM_PINHOLE, false>(const CamJob);
template __global__ void camMakeRaysKernel<CAM_PINHOLE, true>(const CamJob);
template __global__ void camMakeRaysKernel<CAM_TABLE_LENS, false>(const CamJob);
template __global__ void camMakeRaysKernel<CAM_TABLE_LENS, true>(const CamJob);
template __global__ void camContribKernel<CAM_PINHOLE, false>(const CamJob);
template __global__ void camContribKernel<CAM_PINHOLE, true>(const CamJob);
template __global__ void camContribKernel<CAM_TABLE_LENS, false>(const CamJob);
template __global__ void camContribKernel<CAM_TABLE_LENS, true>(const CamJob);

} // namespace hpt
