// Adaptive sampling: the pass planner and the resolve of a frame with per-pixel pass counts.
//
// The ADAPT instantiations of pathTraceKernel (hpt_kernels.hip) keep one PixelMoments record per tid: the sums of the samples' luminance and of
// its square, and the number of samples. From these the planner estimates, pixel by pixel, how many passes bring the standard error of the
// pixel's mean under tol * (|mean| + lumFloor), and hands the difference to the next call as Job::passCounts.
//
// Two kernels and an image between them: m_packedXY is tile-swizzled, so the 3 x 3 neighbours of a pixel are not its neighbours in tid order.
// adaptiveNeedKernel writes every pixel's own need at y * winWidth + x; adaptivePlanKernel reads the neighbourhood there.
//
// Every float operation below is f32 and IEEE, in the order written (the unit is built with -ffp-contract=off; the divisions are the correctly
// rounded ones): tests/adaptive_reference.py restates them in numpy and is held to them bit for bit.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"

namespace hpt {

// passes the record asks for in all (not beyond those it has); nonfinite: the sums cannot be planned from
HPT_DEV uint adaptiveTotal(const PixelMoments m, const AdaptiveParams p, bool& nonfinite)
{
  nonfinite = false;
  const uint n = m.passes;
  if (n == 0u) return p.minPasses;
  if (!__builtin_isfinite(m.sumY) || !__builtin_isfinite(m.sumY2)) { nonfinite = true; return n; }
  const float fn = (float)n;
  const float mean = m.sumY / fn;
  const float var = fmaxf(m.sumY2 / fn - mean * mean, 0.0f);
  const float den = p.tol * (fabsf(mean) + p.lumFloor);
  float tf = var / (den * den);
  if (tf != tf) tf = 0.0f;                                                // 0 / 0: den * den underflowed under a variance of 0
  const uint total = tf >= 2147483648.0f ? 0x7FFFFFFFu : (uint)ceilf(tf);
  return total > p.minPasses ? total : p.minPasses;
}

__global__ void __launch_bounds__(256) adaptiveNeedKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, AdaptiveParams p, uint* need)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i >= tidCount) return;
  const uint tid = tidBegin + i;
  const PixelMoments m = moments[tid];
  bool nonfinite;
  const uint total = adaptiveTotal(m, p, nonfinite);
  const uint XY = packedXY[tid];
  need[((XY & 0xFFFF0000u) >> 16) * winWidth + (XY & 0x0000FFFFu)] = total > m.passes ? total - m.passes : 0u;
}

__global__ void __launch_bounds__(256) adaptivePlanKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, uint winHeight,
                                                          AdaptiveParams p, const uint* need, uint* counts, AdaptiveInfo* info)
{
  __shared__ unsigned long long waveSum[4];
  __shared__ uint wavePix[4], waveMax[4], waveBad[4];
  const uint i = blockIdx.x * 256u + threadIdx.x;
  uint e = 0u, n = 0u, bad = 0u;
  if (i < tidCount) {
    const uint tid = tidBegin + i;
    const PixelMoments m = moments[tid];
    n = m.passes;
    bad = (n != 0u && (!__builtin_isfinite(m.sumY) || !__builtin_isfinite(m.sumY2))) ? 1u : 0u;
    const uint XY = packedXY[tid];
    const uint x = XY & 0x0000FFFFu, y = (XY & 0xFFFF0000u) >> 16;
    if (p.dilate != 0u) {
      const uint x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < winWidth ? x + 1u : winWidth - 1u;
      const uint y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < winHeight ? y + 1u : winHeight - 1u;
      for (uint yy = y0; yy <= y1; yy++)
        for (uint xx = x0; xx <= x1; xx++) { const uint v = need[yy * winWidth + xx]; e = v > e ? v : e; }
    } else e = need[y * winWidth + x];
    const uint room = p.maxPasses - (n < p.maxPasses ? n : p.maxPasses);
    e = e < room ? e : room;
    e = e < p.step ? e : p.step;
    counts[tid] = e;
  }
  // the block's totals: the waves reduce with shuffles, lane 0 of the block adds the four partial results with one atomic per field
  unsigned long long s = e; uint px = e > 0u ? 1u : 0u, mx = n, bd = bad;
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_down(s, o); px += __shfl_down(px, o); bd += __shfl_down(bd, o);
    const uint other = __shfl_down(mx, o); mx = other > mx ? other : mx;
  }
  const uint wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) { waveSum[wave] = s; wavePix[wave] = px; waveMax[wave] = mx; waveBad[wave] = bd; }
  __syncthreads();
  if (threadIdx.x == 0u) {
    for (uint w = 1; w < 4u; w++) { s += waveSum[w]; px += wavePix[w]; bd += waveBad[w]; mx = waveMax[w] > mx ? waveMax[w] : mx; }
    if (s != 0ull) atomicAdd(&info->passes, s);
    if (px != 0u) atomicAdd(&info->pixels, px);
    if (mx != 0u) atomicMax(&info->maxPasses, mx);
    if (bd != 0u) atomicAdd(&info->nonfinite, bd);
  }
}

__global__ void __launch_bounds__(256) adaptiveResolveKernel(const float* frame, const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth,
                                                             uint channels, float* out)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i >= tidCount) return;
  const uint tid = tidBegin + i;
  const uint passes = moments[tid].passes;
  const uint XY = packedXY[tid];
  const size_t at = ((size_t)((XY & 0xFFFF0000u) >> 16) * winWidth + (XY & 0x0000FFFFu)) * channels;
  const float fp = (float)passes;
  const uint nc = channels < 3u ? channels : 3u;
  for (uint c = 0; c < nc; c++) out[at + c] = passes != 0u ? frame[at + c] / fp : 0.0f;     // (a lane reads its pixel before it writes it: out may be frame)
  if (channels > 3u) out[at + 3] = frame[at + 3];
}

// The variance plane DenoiseFrameVar reads: the estimated variance of the pixel's mean luminance, var / (n - 1) with the planner's
// var. One sample gives no spread and counts as 100 % relative error; a record without passes or with non-finite sums gives 0 (the colour of
// such a pixel is non-finite too and the filter rebuilds it from its neighbours).
__global__ void __launch_bounds__(256) adaptiveVarianceKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, float* outVar)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i >= tidCount) return;
  const uint tid = tidBegin + i;
  const PixelMoments m = moments[tid];
  const uint n = m.passes;
  float v = 0.0f;
  if (n != 0u && __builtin_isfinite(m.sumY) && __builtin_isfinite(m.sumY2)) {
    if (n == 1u) v = m.sumY * m.sumY;
    else {
      const float fn = (float)n;
      const float mean = m.sumY / fn;
      const float d = m.sumY2 / fn - mean * mean;
      const float var = d > 0.0f ? d : 0.0f;
      v = var / (fn - 1.0f);
    }
  }
  const uint XY = packedXY[tid];
  outVar[(size_t)((XY & 0xFFFF0000u) >> 16) * winWidth + (XY & 0x0000FFFFu)] = v;
}

} // namespace hpt
