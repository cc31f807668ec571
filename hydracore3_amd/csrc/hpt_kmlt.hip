// IntegratorKMLT (mlt/integrator_kmlt.cpp; `hydra`'s MLT mode): Kelemen-style Metropolis light transport in primary sample space.
//
// Two layers:
//   * pssEval = IntegratorKMLT::PathTraceF: one path whose every number (film position, lens point, time, per bounce the light float4 with its
//     selection in .w, the material float4 and the blend numbers) is READ from a vector of hpt_kmlt_state_size(traceDepth) floats. No generator
//     is read or written. pathTracePssKernel evaluates it for a batch of caller-supplied vectors;
//   * kmltChainKernel: one lane runs one Markov chain (integrator_kmlt.cpp:286-444): its two generators live in registers, its current vector
//     and its proposal in HBM as [slot][chain] (lane-adjacent chains read adjacent addresses), the two contributions of a step go to the film
//     with no-return float atomics (the idiom of hpt_qmc.hip), every step can be recorded. kmltStatsKernel / kmltScaleKernel are the
//     brightness normalisation (:448-472).
// Every BSDF branch and the thin films (shadeVertex<.., FILM>); RGB only - m_spectral_mode runs pathTracePssSpectralKernel / kmltChainSpectralKernel
// (hpt_spectral.hip) when hpt_set_option("kmlt_spectral", 1) asked for it and is refused otherwise; megakernel schedule only.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"
#include "hpt_kmlt_chain.h"

namespace hpt {

// the slots of a vector and the PssRands policy (GetRandomNumbers*) live in hpt_decl.h: pssEvalSpec (hpt_spectral.hip) reads the same vectors

// PathTraceF (:156-228) for the lanes with `active` set; the others only keep the wave's loop company. tid: the reference's thread id (the
// camera back plate reads m_packedXY[tid]). color = accumColor * m_exposureMult (no m_camRespoceRGB in RGB mode), pixel = y * winWidth + x of
// IntegratorQMC::SampleCameraRay's clamp. The loop has the megakernel's shape - one closest-hit and one shadow query per trip, the whole wave
// leaves together - so the traversal code, which votes across the wave, is entered by every lane that has a ray at the same place.
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
HPT_DEV void pssEval(const DevScene& S, const PssRands rs, const bool active, const uint tid, const uint* __restrict__ packedXY, const uint packedCount,
                     const TravStack& stk, TravStats& st, V3& color, uint& pixel)
{
  bool alive = active;
  uint bounce = 0, flags = 0;
  Rng gen; gen.sx = gen.sy = 0;                                            // never drawn from: PssRands ignores it
  V3 rpos = v3(0, 0, 0), rdir = v3(0, 0, 1);
  V3 accum = v3(0, 0, 0), thr = v3(1, 1, 1);
  float misPdf = 1.0f, misIor = 1.0f, pathTime = 0.0f;
  const uint maxBounce = S.traceDepth;
  color = v3(0, 0, 0); pixel = 0u;
  if (alive) {                                                             // kernel_InitEyeRay with IntegratorQMC::SampleCameraRay (integrator_qmc.cpp:148-187)
    const V4 lens = v4(rs.at(0u), rs.at(1u), rs.at(2u), rs.at(3u));
    cameraRayAt<true>(S, lens.x, lens.y, lens, rpos, rdir);                // no viewport term
    uint x = (uint)(lens.x * float(S.winWidth)), y = (uint)(lens.y * float(S.winHeight));
    if (x >= (uint)(S.winWidth - 1)) x = (uint)(S.winWidth - 1);
    if (y >= (uint)(S.winHeight - 1)) y = (uint)(S.winHeight - 1);
    pixel = y * (uint)S.winWidth + x;
    if (MOTION) pathTime = rs.at(5u);
    if (maxBounce == 0u) alive = false;                                    // (the depth loop does not run: the colour stays 0 - no environment term either, RAY_FLAG_OUT_OF_SCENE is never set)
  }
  while (__any(alive)) {
    HitRec hit; hit.inst = 0xFFFFFFFFu; hit.prim = 0; hit.t = 0; hit.u = hit.v = 0;
    if (alive) traceAny<false, false, DEEP, FLAT, MOTION, SWEEP>(S, rpos, rdir, 0.0f, HPT_FLT_MAX, hit, stk, st, pathTime);
    bool wantShadow = false;
    V3 shPos = v3(0, 0, 0), shDir = v3(0, 0, 1); float shFar = 0.0f;
    V3 contrib = v3(0, 0, 0);
    V3 recA, recS, recdA, recdS, tailR; Taps recTaps; uint recTex = 0xFFFFFFFFu;       // (the DR record: unused here)
    bool didBounce = false;
    if (alive)
      didBounce = shadeVertex<false, false, false, MOTION, true, PssRands>(S, nullptr, hit, rpos, rdir, accum, thr, misPdf, misIor, flags, bounce, gen,
                                                                           wantShadow, shPos, shDir, shFar, contrib, recA, recS, recdA, recdS, recTaps, recTex, tailR, pathTime, rs);
    if (wantShadow) {
      HitRec sh;
      const bool occluded = traceAny<true, false, DEEP, FLAT, MOTION, SWEEP>(S, shPos, shDir, 0.0f, shFar, sh, stk, st, pathTime);
      if (!occluded) accum = accum + contrib;
    }
    if (alive) {
      if (didBounce) bounce++;
      if ((flags & RAY_FLAG_IS_DEAD) != 0 || bounce >= maxBounce) {        // kernel_HitEnvironment
        const uint backXY = (S.envCamBackId != 0xFFFFFFFFu && tid < packedCount) ? packedXY[tid] : 0u;
        const V3 env = environmentRadiance(S, rdir, misPdf, flags, backXY);
        if ((flags & RAY_FLAG_OUT_OF_SCENE) != 0) {
          if (S.integratorType == INTEGRATOR_STUPID_PT) accum = thr * env; else accum = accum + thr * env;
        }
        color = v3(S.exposureMult * accum.x, S.exposureMult * accum.y, S.exposureMult * accum.z);
        alive = false;
      }
    }
  }
}

template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) pathTracePssKernel(const DevScene S, const PssJob job)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint glane = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = job.stackOverflow + glane; stk.ovfStride = job.gridLanes;
  TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const bool active = glane < job.n;
  PssRands rs; rs.x = job.x + (size_t)(active ? glane : 0u) * job.vecStride; rs.stride = 1u; rs.n = job.stateSize;
  V3 color; uint pixel;
  pssEval<DEEP, FLAT, MOTION, SWEEP>(S, rs, active, glane, job.packedXY, job.packedCount, stk, st, color, pixel);
  if (active) { job.color[glane] = make_float4(color.x, color.y, color.z, 0.0f); job.pixel[glane] = pixel; }
}

// kmltContribFunc, mutateKelemen and the chain itself (kmltChainBody) live in hpt_kmlt_chain.h, shared with kmltChainSpectralKernel
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) kmltChainKernel(const DevScene S, const KmltJob job)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint glane = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = job.stackOverflow + glane; stk.ovfStride = job.gridLanes;
  TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const bool active = glane < job.chains;
  kmltChainBody(job, active, glane, [&](const PssRands& rs, V3& color, uint& pixel) {
    pssEval<DEEP, FLAT, MOTION, SWEEP>(S, rs, active, active ? glane : 0u, job.packedXY, job.packedCount, stk, st, color, pixel);
  });
}

// Sums of one block in a fixed order: every thread adds its strided share, the 256 partial sums are folded in LDS.
HPT_DEV double blockSum(double v, double* sh)
{
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint o = 128u; o > 0u; o >>= 1) { if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// :441-470. avgBrightness: the mean of accumBrightness / largeSteps over the chains that made a large step; actualBrightness: the mean of
// contribFunc over the first pixelsNum pixels of the frame; acceptance: accepted steps / (pixelsNum * passNum); normConst = float(passNum) *
// float(avg / actual), or 1 when either brightness has no value (no large step at all, a black frame).
__global__ void __launch_bounds__(256) kmltStatsKernel(const float4* frame, uint pixelsNum, uint passNum, uint chains, const double* accumBrightness,
                                                       const uint* largeSteps, const uint* accept, double* stats4)
{
  __shared__ double sh[256];
  double b = 0.0, withLarge = 0.0, acc = 0.0, actual = 0.0;
  for (uint c = threadIdx.x; c < chains; c += 256u) {
    const uint l = largeSteps[c];
    if (l != 0u) { b += accumBrightness[c] / (double)l; withLarge += 1.0; }
    acc += (double)accept[c];
  }
  for (uint i = threadIdx.x; i < pixelsNum; i += 256u) { const float4 p = frame[i]; actual += (double)kmltContribFunc(v3(p.x, p.y, p.z)); }
  b = blockSum(b, sh); withLarge = blockSum(withLarge, sh); acc = blockSum(acc, sh); actual = blockSum(actual, sh);
  if (threadIdx.x == 0u) {
    const double avgBrightness = withLarge > 0.0 ? b / withLarge : 0.0;
    const double actualBrightness = pixelsNum ? actual / (double)pixelsNum : 0.0;
    const bool ok = withLarge > 0.0 && actualBrightness != 0.0;
    stats4[0] = avgBrightness; stats4[1] = actualBrightness;
    stats4[2] = acc / ((double)pixelsNum * (double)passNum);
    stats4[3] = ok ? (double)((float)passNum * (float)(avgBrightness / actualBrightness)) : 1.0;
  }
}

__global__ void __launch_bounds__(256) kmltScaleKernel(float* frame, size_t n, const double* stats4)
{
  const float normConst = (float)stats4[3];
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n) frame[i] = frame[i] * normConst;
}

#define HPT_KMLT_INST(DEEP, FLAT, MOTION, SWEEP) \
  template __global__ void pathTracePssKernel<DEEP, FLAT, MOTION, SWEEP>(const DevScene, const PssJob); \
  template __global__ void kmltChainKernel<DEEP, FLAT, MOTION, SWEEP>(const DevScene, const KmltJob);
HPT_KMLT_INST(false, false, false, true)       // the traversal variants pathTraceQmcKernel is dispatched over
HPT_KMLT_INST(false, false, false, false)
HPT_KMLT_INST(true,  false, false, false)
HPT_KMLT_INST(false, true,  false, false)
HPT_KMLT_INST(true,  true,  false, false)
HPT_KMLT_INST(false, false, true,  false)
HPT_KMLT_INST(true,  false, true,  false)
HPT_KMLT_INST(false, true,  true,  false)
HPT_KMLT_INST(true,  true,  true,  false)

} // namespace hpt
