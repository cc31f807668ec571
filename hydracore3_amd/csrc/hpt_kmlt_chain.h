// The Markov chain of IntegratorKMLT::PathTraceBlock (mlt/integrator_kmlt.cpp:286-444), one copy for the kernels that differ only in how a
// path is evaluated: kmltChainKernel (hpt_kmlt.hip: pssEval, RGB) and kmltChainSpectralKernel (hpt_spectral.hip: pssEvalSpec, four wavelengths
// turned into RGB before the chain sees them). contribFunc, the acceptance, the two contributions and the per-chain sums work on that RGB colour.
#pragma once
#include "hpt_decl.h"

namespace hpt {

// :230-233
HPT_DEV float kmltContribFunc(V3 c) { return smax(0.333334f * (c.x + c.y + c.z), 0.0f); }

// MutateKelemen (:64-85), float32 as written
HPT_DEV float mutateKelemen(float valueX, float rx, float ry, float p2, float p1)
{
  const float s1 = 1.0f / p1, s2 = 1.0f / p2;
  const float power = -logf(s2 / s1);
  const float dv = smax(s2 * (expf(power * sqrtf_(rx)) - expf(power)), 0.0f);
  if (ry < 0.5f) { valueX += dv; if (valueX > 1.0f) valueX -= 1.0f; }
  else           { valueX -= dv; if (valueX < 0.0f) valueX += 1.0f; }
  return valueX;
}

// One lane runs chain c = its global lane (`active`: c < job.chains; the other lanes only keep the wave's path loop company): the two generators
// live in registers, the current vector and the proposal in HBM as [slot][chain]. eval(rs, color, pixel) is PathTraceF on the proposal - every
// lane of the wave calls it at the same place, active or not, since the traversal votes across the wave.
template <class EVAL>
HPT_DEV void kmltChainBody(const KmltJob& job, const bool active, const uint glane, EVAL eval)
{
  const uint c = active ? glane : 0u;                                      // (idle lanes form addresses of chain 0 and never use them)
  const uint n = job.stateSize;
  const size_t C = job.chains;
  float* xVec = job.cur + c;                                        // slot i: xVec[i * C]
  float* xNew = job.prop + c;
  PssRands rs; rs.x = xNew; rs.stride = C; rs.n = n;

  Rng gen1 = rng_init(c * 7u + 1u), gen2 = rng_init(c);                    // :291-297
  for (uint i = 0; i < 10u + c % 17u; i++) { rng_next(gen1); rng_next(gen2); }

  V3 yColor = v3(0, 0, 0); float y = 0.0f; uint pixOld = 0u;
  uint accept = 0u, largeSteps = 0u;
  double accumBrightness = 0.0;
  const float MUTATE_COEFF_SCREEN = 128.0f, MUTATE_COEFF_BSDF = 64.0f, plarge = 0.25f;

  // trip 0 evaluates the initial state (:299-312), trip 1 + i is step i of the chain: one place where F is evaluated, one copy of the path code
  for (uint trip = 0; trip <= job.steps; trip++) {
    bool isLargeStep = false;
    if (active) {
      if (trip == 0u) { for (uint i = 0; i < n; i++) xNew[i * C] = rng_float1(gen2); }
      else {
        isLargeStep = rng_float1(gen1) < plarge;
        if (isLargeStep) {
          for (uint i = 0; i < n; i += 4u) {
            const V4 r1 = rng_float4(gen2);
            xNew[(i + 0u) * C] = r1.x; xNew[(i + 1u) * C] = r1.y; xNew[(i + 2u) * C] = r1.z; xNew[(i + 3u) * C] = r1.w;
          }
        } else {
          const V4 r1 = rng_float4(gen2);
          const V4 r2 = rng_float4(gen2);
          xNew[0 * C] = mutateKelemen(xVec[0 * C], r1.x, r1.y, MUTATE_COEFF_SCREEN * 1.0f, 1024.0f);
          xNew[1 * C] = mutateKelemen(xVec[1 * C], r1.z, r1.w, MUTATE_COEFF_SCREEN * 1.0f, 1024.0f);
          xNew[2 * C] = mutateKelemen(xVec[2 * C], r2.x, r2.y, MUTATE_COEFF_BSDF, 1024.0f);
          xNew[3 * C] = mutateKelemen(xVec[3 * C], r2.z, r2.w, MUTATE_COEFF_BSDF, 1024.0f);
          for (uint i = 4u; i < n; i += 2u) {                              // (slot 4, the wavelength sample of spectral MLT, is one of these)
            const V4 r = rng_float4(gen2);
            xNew[(i + 0u) * C] = mutateKelemen(xVec[(i + 0u) * C], r.x, r.y, MUTATE_COEFF_BSDF, 1024.0f);
            xNew[(i + 1u) * C] = mutateKelemen(xVec[(i + 1u) * C], r.z, r.w, MUTATE_COEFF_BSDF, 1024.0f);
          }
        }
      }
    }
    V3 yNewColor; uint pixNew;
    eval(rs, yNewColor, pixNew);
    if (active) {
      const float yNew = kmltContribFunc(yNewColor);
      if (trip == 0u) {
        for (uint i = 0; i < n; i++) xVec[i * C] = xNew[i * C];
        y = yNew; yColor = yNewColor; pixOld = pixNew;
        if (job.recInitColor) job.recInitColor[c] = make_float4(yNewColor.x, yNewColor.y, yNewColor.z, 0.0f);
        if (job.recInitPixel) job.recInitPixel[c] = pixNew;
      } else {
        const size_t rec = (size_t)c * job.steps + (trip - 1u);
        if (job.recProposals) { float* p = job.recProposals + rec * n; for (uint i = 0; i < n; i++) p[i] = xNew[i * C]; }
        const float yOld = y;
        const V3 yOldColor = yColor;
        const uint pixCompared = pixOld;
        const float a = (yOld == 0.0f) ? 1.0f : smin(1.0f, yNew / yOld);
        const float p = rng_float1(gen1);
        const bool accepted = p <= a;
        if (accepted) {
          for (uint i = 0; i < n; i++) xVec[i * C] = xNew[i * C];
          y = yNew; yColor = yNewColor; pixOld = pixNew;
          accept++;
        }
        if (isLargeStep) { accumBrightness += (double)yNew; largeSteps++; }
        // (5) contrib to image (:386-433), w1 = 1
        const float kY = (1.0f / smax(yNew, 1e-6f)), kX = (1.0f / smax(yOld, 1e-6f)), na = 1.0f - a;
        const V3 contribAtY = v3(1.0f * yNewColor.x * kY * a, 1.0f * yNewColor.y * kY * a, 1.0f * yNewColor.z * kY * a);
        const V3 contribAtX = v3(1.0f * yOldColor.x * kX * na, 1.0f * yOldColor.y * kX * na, 1.0f * yOldColor.z * kX * na);
        const bool addX = dot(contribAtX, contribAtX) > 1e-12f, addY = dot(contribAtY, contribAtY) > 1e-12f;
        if (addX) {
          float* o = job.outColor + (size_t)pixCompared * 4u;
          atomicAdd(o + 0, contribAtX.x); atomicAdd(o + 1, contribAtX.y); atomicAdd(o + 2, contribAtX.z);
        }
        if (addY) {
          float* o = job.outColor + (size_t)pixNew * 4u;
          atomicAdd(o + 0, contribAtY.x); atomicAdd(o + 1, contribAtY.y); atomicAdd(o + 2, contribAtY.z);
        }
        if (job.recLarge) job.recLarge[rec] = isLargeStep ? 1 : 0;
        if (job.recAccepted) job.recAccepted[rec] = accepted ? 1 : 0;
        if (job.recA) job.recA[rec] = a;
        if (job.recColor) job.recColor[rec] = make_float4(yNewColor.x, yNewColor.y, yNewColor.z, 0.0f);
        if (job.recPixel) job.recPixel[rec] = pixNew;
        if (job.recOldPixel) job.recOldPixel[rec] = pixCompared;
        if (job.recContribX) job.recContribX[rec] = make_float4(contribAtX.x, contribAtX.y, contribAtX.z, addX ? 1.0f : 0.0f);
        if (job.recContribY) job.recContribY[rec] = make_float4(contribAtY.x, contribAtY.y, contribAtY.z, addY ? 1.0f : 0.0f);
      }
    }
  }
  if (active) { job.accumBrightness[c] = accumBrightness; job.largeSteps[c] = largeSteps; job.accept[c] = accept; }
}

} // namespace hpt
