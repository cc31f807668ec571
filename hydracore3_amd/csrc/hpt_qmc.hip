// IntegratorQMC::PathTraceBlock (mlt/integrator_qmc.{h,cpp}, mlt/rnd_qmc.{h,cpp}; `hydra --qmc`): path tracing whose film position, lens
// point, time and first-bounce material / light numbers come from a Niederreiter base-2 sequence, everything else from the pseudo generators.
//
// The persistent megakernel of hpt_kernels.hip with three differences:
//   * a lane owns a GENERATOR SLOT g, not a pixel: it runs samples s = g, g + N, g + 2N, ... < S in that order (N = size of m_randomGens,
//     S = min(2^32 - 1, pixels x passes)) and carries the generator from one to the next in registers. The reference hands s and s + N to
//     whichever OpenMP threads come by, both reading and writing slot s % N: this order is what it computes on one thread;
//   * the pixel is derived from dimensions 0 and 1 of s, so many samples of many lanes land on one pixel: the film is summed with hardware
//     float atomics (no-return global_atomic_add_f32, as the DR adjoint's gradient scatter), one per channel and sample;
//   * optionally every sample's colour and pixel index are stored at index s: those records do not depend on the order of the atomics.
// Every BSDF branch and the thin films (shadeVertex<.., FILM>); RGB only - m_spectral_mode runs pathTraceQmcSpectralKernel (hpt_spectral.hip)
// when hpt_set_option("qmc_spectral", 1) asked for it and is refused otherwise; this schedule only.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"

namespace hpt {

// qmcFloat and the QmcRands policy (GetRandomNumbersLgts / Mats / MatB) live in hpt_decl.h: the spectral form of this kernel shares them
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) pathTraceQmcKernel(const DevScene S, const Job job, const QmcJob q)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint glane = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = job.stackOverflow + glane; stk.ovfStride = job.gridLanes;
  // cold per-sample state in LDS, as the megakernel keeps its per-pixel state: generator slot, sample index, pixel index
  __shared__ uint coldU[3 * 256];
#define SLOT    coldU[0 * 256 + threadIdx.x]
#define SAMPLE  coldU[1 * 256 + threadIdx.x]
#define PIXEL   coldU[2 * 256 + threadIdx.x]
  bool haveSlot = false, more = false, alive = false, drained = false;     // more: the slot has a sample left to start
  uint bounce = 0, flags = 0;
  Rng  gen; gen.sx = gen.sy = 0;
  V3   rpos = v3(0, 0, 0), rdir = v3(0, 0, 1);
  V3   accum = v3(0, 0, 0), thr = v3(1, 1, 1);
  float misPdf = 1.0f, misIor = 1.0f;
  float pathTime = 0.0f;
  TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const uint maxBounce = S.traceDepth;
  const bool dof = S.camLensRadius > 0.0f || S.lensCount != 0u;

  while (true) {
    // ---- (1) a slot that has run its last sample stores its generator (the chain's end: m_randomGens[s % N] after the last s) ----------
    if (!alive && haveSlot && !more) { job.gens[SLOT] = gen; haveSlot = false; }
    // ---- (2) work queue over the generator slots 0 .. min(N, S): one atomic per wave, as in pathTraceKernel -----------------------------
    {
      const bool need = !alive && !haveSlot && !drained;
      const unsigned long long mask = __ballot(need);
      if (mask != 0ull) {
        uint base = 0;
        if (need && mbcnt64(mask) == 0u) base = atomicAdd(job.queue, (uint)__popcll(mask));
        base = __shfl(base, (int)(__ffsll((long long)mask) - 1));
        if (need) {
          const uint g = base + mbcnt64(mask);
          if (g < job.tidCount) { gen = job.gens[g]; SLOT = g; SAMPLE = g; haveSlot = true; more = true; }
          else drained = true;
        }
      }
    }
    // ---- (3) regenerate: the slot's next sample (kernel_InitEyeRay2 with IntegratorQMC::SampleCameraRay) -----------------------------------
    if (!alive && haveSlot) {                                              // (more is true here: a finished slot was stored in (1))
      const uint s = SAMPLE;
      accum = v3(0, 0, 0); thr = v3(1, 1, 1); flags = 0; bounce = 0;
      misPdf = 1.0f; misIor = 1.0f;
      V4 lens = rng_float4(gen);                                           // GetRandomNumbersLens: the pseudo float4 first, then the overwrites
      lens.x = qmcFloat(q.table, s, 0u);
      lens.y = qmcFloat(q.table, s, 1u);
      if (dof && q.dofDim != 0u) { lens.z = qmcFloat(q.table, s, 2u); lens.w = qmcFloat(q.table, s, 3u); }
      cameraRayAt<true>(S, lens.x, lens.y, lens, rpos, rdir);              // EyeRayDirNormalized(x, y, m_projInv) on the numbers themselves: no viewport term
      uint x = (uint)(lens.x * float(S.winWidth)), y = (uint)(lens.y * float(S.winHeight));
      if (x >= (uint)(S.winWidth - 1)) x = (uint)(S.winWidth - 1);
      if (y >= (uint)(S.winHeight - 1)) y = (uint)(S.winHeight - 1);
      PIXEL = y * (uint)S.winWidth + x;
      if (MOTION) pathTime = (q.motionDim != 0u) ? qmcFloat(q.table, s, q.motionDim) : rng_float1(gen);   // GetRandomNumbersTime: no pseudo draw when the dimension is set
      alive = true;
    }
    if (!__any(alive)) break;

    // ---- (4) closest hit ---------------------------------------------------------------------------------------------------------------
    HitRec hit; hit.inst = 0xFFFFFFFFu; hit.prim = 0; hit.t = 0; hit.u = hit.v = 0;
    if (alive) traceAny<false, false, DEEP, FLAT, MOTION, SWEEP>(S, rpos, rdir, 0.0f, HPT_FLT_MAX, hit, stk, st, pathTime);

    // ---- (5) surface, light sample, BSDF sample ------------------------------------------------------------------------------------------
    bool wantShadow = false;
    V3 shPos = v3(0, 0, 0), shDir = v3(0, 0, 1); float shFar = 0.0f;
    V3 contrib = v3(0, 0, 0);
    V3 recA, recS, recdA, recdS, tailR; Taps recTaps; uint recTex = 0xFFFFFFFFu;       // (the DR record: unused here)
    bool didBounce = false;
    if (alive) {
      QmcRands rs; rs.table = q.table; rs.s = SAMPLE; rs.matDim = q.matDim; rs.lgtDim = q.lgtDim;
      didBounce = shadeVertex<false, false, false, MOTION, true, QmcRands>(S, nullptr, hit, rpos, rdir, accum, thr, misPdf, misIor, flags, bounce, gen,
                                                                           wantShadow, shPos, shDir, shFar, contrib, recA, recS, recdA, recdS, recTaps, recTex, tailR, pathTime, rs);
    }
    // ---- (6) shadow ray --------------------------------------------------------------------------------------------------------------------
    if (wantShadow) {
      HitRec sh;
      const bool occluded = traceAny<true, false, DEEP, FLAT, MOTION, SWEEP>(S, shPos, shDir, 0.0f, shFar, sh, stk, st, pathTime);
      if (!occluded) accum = accum + contrib;
    }
    // ---- (7) end of path: kernel_HitEnvironment, IntegratorQMC::kernel_ContributeToImage -------------------------------------------------
    if (alive) {
      if (didBounce) bounce++;
      if ((flags & RAY_FLAG_IS_DEAD) != 0 || bounce >= maxBounce) {
        const uint s = SAMPLE;
        // the camera back plate reads m_packedXY[tid] with tid = the sample index (integrator_pt.cpp:581); past the vector's end: 0, as the input-ray mode has it
        const uint backXY = (S.envCamBackId != 0xFFFFFFFFu && s < job.packedCount) ? job.packedXY[s] : 0u;
        const V3 env = environmentRadiance(S, rdir, misPdf, flags, backXY);
        if ((flags & RAY_FLAG_OUT_OF_SCENE) != 0) {
          if (S.integratorType == INTEGRATOR_STUPID_PT) accum = thr * env; else accum = accum + thr * env;
        }
        (void)rng_float4(gen);                                             // GetRandomNumbersLens once more before *gen is stored (integrator_qmc.cpp:225-226)
        const V3 c = accum * ld3(S.camRespoceRGB);
        const V3 rgb = v3(S.exposureMult * c.x, S.exposureMult * c.y, S.exposureMult * c.z);
        const float mono = 0.2126f * rgb.x + 0.7152f * rgb.y + 0.0722f * rgb.z;
        const uint pixel = PIXEL;
        if (job.outColor != nullptr) {
          if (job.channels == 1u) atomicAdd(job.outColor + pixel, mono);
          else {
            float* o = job.outColor + (size_t)pixel * job.channels;
            atomicAdd(o + 0, rgb.x); atomicAdd(o + 1, rgb.y); atomicAdd(o + 2, rgb.z);
          }
        }
        if (q.sampleColor != nullptr) {
          q.sampleColor[s] = (job.channels == 1u) ? make_float4(mono, 0.0f, 0.0f, 0.0f) : make_float4(rgb.x, rgb.y, rgb.z, 0.0f);
          q.samplePixel[s] = pixel;
        }
        more = (q.samples - 1u - s) >= q.gensCount;                        // s + N < S without wrapping at 2^32
        if (more) SAMPLE = s + q.gensCount;
        alive = false;
      }
    }
  }
#undef SLOT
#undef SAMPLE
#undef PIXEL
}

#define HPT_QMC_INST(DEEP, FLAT, MOTION, SWEEP) template __global__ void pathTraceQmcKernel<DEEP, FLAT, MOTION, SWEEP>(const DevScene, const Job, const QmcJob);
HPT_QMC_INST(false, false, false, true)      // the traversal variants pathTraceKernel is dispatched over (hpt_host.hip: launchPT, launchPTMotion)
HPT_QMC_INST(false, false, false, false)
HPT_QMC_INST(true,  false, false, false)
HPT_QMC_INST(false, true,  false, false)
HPT_QMC_INST(true,  true,  false, false)
HPT_QMC_INST(false, false, true,  false)
HPT_QMC_INST(true,  false, true,  false)
HPT_QMC_INST(false, true,  true,  false)
HPT_QMC_INST(true,  true,  true,  false)

} // namespace hpt
