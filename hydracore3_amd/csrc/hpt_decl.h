// Launch interface between the host side (hpt_host.hip) and the path-tracing kernels, which are compiled as separate translation
// units (hpt_kernels.hip once per instantiation group, hpt_wavefront.hip) and linked into one libhydra_hip.so: argument structs,
// occupancy constants and the kernel templates' declarations. The host never sees a kernel body, so a change to one kernel family
// rebuilds only that family's objects and the objects build in parallel.
#pragma once
#include <hip/hip_runtime.h>
#include "hpt_shade.h"

namespace hpt {

// ---- persistent megakernel (hpt_kernels.hip) -----------------------------------------------------------------------------------------
struct Job
{
  uint   tidBegin, tidCount;      // work items of this launch: item k renders tid = tidBegin + (k / chunk) * chunk * stride + k % chunk
  uint   tidChunk, tidStride;     // (stride 1 = one contiguous window; stride W = every W-th chunk: the interleaved multi-GPU split)
  uint   tidEnd;                  // number of threads of the whole frame (items mapping past it are dropped)
  uint   passNum, channels;
  float* outColor;                // full W*H*channels framebuffer (device)
  Rng*   gens;                    // m_randomGens (device, persistent)
  const uint* packedXY;           // m_packedXY
  uint  packedCount;              // entries in packedXY (the input-ray mode reads it only for the camera back plate)
  uint*  queue;                   // work-queue head (zeroed before launch)
  Counters* counters;             // instrumentation (STATS builds)
  // differentiable rendering; the adaptive forward call (the ADAPT instantiations, which no DR call runs) keeps its two arrays in the storage of two of
  // these pointers, both indexed by absolute tid like gens: passCounts (null: passNum for every pixel) and moments (null: no statistics)
  union { const float* refImg; const uint* passCounts; };          // refImg: a_refImg
  const float* data;              // a_data
  union { float* grad; PixelMoments* moments; };                   // grad: a_dataGrad (atomically accumulated)
  // Pass slices (SLICED instantiations of pathTraceKernel, forward calls; hpt_set_option("pass_slice")) share the storage of four fields that
  // only PathTraceDR reads, so that Job - a by-value kernel argument of every kernel family - keeps its size and layout:
  //   passSlice       s > 0: the queue holds tidCount * passSliceCount(passNum, s) items (hpt_types.h: passSliceItem) and a pixel is handed
  //                   from slice to slice through sliceMail
  //   sliceMail       [tid][SLICE_MAIL_WORDS]: the pixel and its generator as tagged 64-bit words (hpt_types.h: sliceWordPack), written by the
  //                   lane that finished a slice which has a successor and read by the lane that holds that successor; relaxed agent-scope
  //                   atomics only, no fence on either side (zeroed before the launch)
  //   slicePollLimit  polls after which a lane waiting for its predecessor gives up (a protocol bug ends as an error, not as a hang)
  //   sliceError      set to 1 by a lane that gave up (host-visible; the host reports HPT_ERR_STATE)
  union { float* lossAccum; uint* sliceError; };      // lossAccum: sum over samples of loss / passNum
  union { float* record; unsigned long long* sliceMail; };         // record: per-lane, per-bounce adjoint records: [bounce][field][lane]
  union { uint recordLanes; uint passSlice; };        // recordLanes: total lanes of the grid (stride of the record buffer)
  uint   naive;                   // the spectral kernel only: NaivePathTrace (the RGB kernels have their own instantiations)
  uint   drSkipNonFinite;         // hpt_set_option("dr_skip_nonfinite"): samples whose radiance is not finite give neither loss, colour nor gradient
                                  // (0 = the reference's PixelLossPT, which adds them like any other)
  uint*  stackOverflow;           // HBM part of the traversal stacks: [depth - LDS_STACK][global lane]
  uint   gridLanes;
  // PathTraceVJP (vjp != 0): the sweep of a path is seeded with the caller's dL/d(out_color) of its pixel instead of 2 (colour - ref): pixels of
  // `channels` floats in out_color's row order (not flipped as a_refImg is). Null: the DR path is rendered and recorded, nothing is swept.
  // No loss is computed; refImg and lossAccum are not read.
  const float* adjImg;
  union { uint vjp; uint slicePollLimit; };
  // Light-colour gradients (the LGRAD instantiations, hpt_put_diff_lights) share the storage of the input-ray pointers, which no DR kernel reads
  // (launch_path_trace fills them in after it has looked at inRayPos): DrLights' first, count and off.
  union { const float4* inRayPos; struct { uint drLightFirst, drLightCount; }; };   // inRayPos / inRayDir: PathTraceFromInputRays, RayPosAndW[tid] / RayDirAndT[tid] in camera space (MODE 2)
  // Environment maps in DR (the ENV instantiations; mutually exclusive with LGRAD) use the padding word: the env plane of the record exists.
  union { const float4* inRayDir; struct { uint drLightOff, drLightPad; }; struct { uint drEnvPad, drEnvPlaneOn; }; };
};
static_assert(sizeof(Job) == 184, "Job is a by-value argument of every kernel family: its size and layout stay");

#ifndef HPT_MIN_WAVES
#define HPT_MIN_WAVES 4   // waves per SIMD the register allocator must fit (measured: 2 -> 725, 3 -> 913..1262, 4 -> 1005..1365 Mpaths/s on the Cornell box)
#endif
// MODE: 0 = PathTrace (MIS / shadow / stupid by m_intergatorType), 1 = NaivePathTrace, 2 = PathTraceFromInputRays (the caller's rays
// instead of camera rays, linear tid -> output index, raw accumColor: integrator_pt.cpp:159-199, 659-676, 761-798),
// 3 = PathTrace for scenes with gltf + emissive materials only (shadeVertex<LEAN>), 4 / 5 / 6 = 0 / 1 / 2 for scenes with thin films (shadeVertex<FILM>), 7 = 0 built for one more wave per SIMD (scenes with few material types:
// env_map 1584 -> 1670 Mpaths/s, while typed_materials loses 3 % there and stays on MODE 0)
// waves per SIMD the kernels with every BSDF branch (MODE 0 / 1 / 2) are compiled for; the lean and DR kernels keep HPT_MIN_WAVES.
// Measured (profiles/ab_full.sh, 1024^2 x 64 spp, Mpaths/s at 4 / 3 / 2 waves): Cornell forced onto this kernel 1410 / 1531 / 1264,
// legacy_materials 1585 / 1714 / 1528, env_map 1425 / 1507 / 1369, typed_materials 1123 / 1125 / 1105.
#ifndef HPT_FULL_WAVES
#define HPT_FULL_WAVES 3
#endif
#ifndef HPT_FILM_WAVES
#define HPT_FILM_WAVES 3   // the film kernels (MODE 4 / 5 / 6)
#endif
#ifndef HPT_DR_WAVES
#define HPT_DR_WAVES HPT_MIN_WAVES   // the PathTraceDR megakernel
#endif
#define HPT_PT_BOUNDS(DR, MODE) __launch_bounds__(256, (DR) ? HPT_DR_WAVES : ((MODE) == 3 ? HPT_MIN_WAVES : ((MODE) == 7 ? HPT_FULL_WAVES + 1 : ((MODE) >= 4 ? HPT_FILM_WAVES : HPT_FULL_WAVES))))
// SLICED: work items are runs of Job::passSlice passes of a pixel (instantiated for PathTrace from the camera: MODE 3, 0, 7 and moving instances)
// LGRAD (with DR): light-colour gradients (hpt_shade.h: DrLights); the residency is the DR kernel's
// ENV (with DR, without LGRAD): environment maps and their texel gradients (hpt_shade.h: drEnvSweep); the residency is the DR kernel's
// ADAPT: per-pixel pass counts (Job::passCounts) and luminance moments (Job::moments); whole pixels, forward calls from the camera (MODE 3, 0, 7 and moving instances)
template <bool STATS, bool DR, int MODE, bool DEEP, bool FLAT, bool MOTION = false, bool SWEEP = false, bool SLICED = false, bool LGRAD = false, bool ENV = false, bool ADAPT = false>
__global__ void HPT_PT_BOUNDS(DR, MODE) pathTraceKernel(const DevScene S, const Job job);

// spectral rendering (hpt_spectral.hip): one thread per pixel, four wavelengths per path
#ifndef HPT_SPEC_WAVES
#define HPT_SPEC_WAVES 4        // waves per SIMD the spectral kernel is compiled for: scopes 0 and 1
#endif
#ifndef HPT_SPEC_WIDE_WAVES
#define HPT_SPEC_WIDE_WAVES 3   // ... scope 2
#endif
// ADAPT: per-pixel pass counts (Job::passCounts) and luminance moments (Job::moments), as in pathTraceKernel: PathTraceBlock from the camera only
template <bool DEEP, bool FLAT, bool SWEEP, bool MOTION, int SCOPE, bool ADAPT = false>   // SCOPE 0: the reference's spectral fixtures' needs; 1: + gltf; 2: + glass / blends / normal maps / environment maps / lens; 3: the same at 4 waves per SIMD
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) pathTraceSpectralKernel(const DevScene S, const Job job);

template <bool DEEP, bool FLAT, bool WIDE, int SCOPE>   // the same integrator under the block-local schedule (work queue, LDS ray pool, ray replacement; hpt_spectral.hip)
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) pathTraceBlockSpectralKernel(const DevScene S, const Job job, uint refillBelow, uint nodeMin);

// ---- megakernel with block-local ray repacking (hpt_block.hip) --------------------------------------------------------------------------
#ifndef HPT_BW_FWD_WAVES
#define HPT_BW_FWD_WAVES 4
#endif
#ifndef HPT_BW_DR_WAVES
#define HPT_BW_DR_WAVES 4
#endif
#ifndef HPT_BW_FULL_WAVES
#define HPT_BW_FULL_WAVES 3      // every BSDF branch: 74 .. 98 VGPRs spilled at 4 waves per SIMD
#endif
#define HPT_BW_WAVES(DR, LEAN) ((DR) ? HPT_BW_DR_WAVES : ((LEAN) ? HPT_BW_FWD_WAVES : HPT_BW_FULL_WAVES))
// VJP (with DR): PathTraceVJP's form of the path end. A template parameter here, a run-time branch on Job::vjp in the other two DR kernels: this
// kernel already spills at its four waves per SIMD and the branch raised that (18 -> 25 VGPRs on the single-level variant; profiles/dr_vjp.md)
template <bool DR, bool LEAN, bool DEEP, bool FLAT, bool WIDE = false, bool VJP = false>   // WIDE: walk DevScene::nodes4 (heavy single-level scenes)
__global__ void __launch_bounds__(256, HPT_BW_WAVES(DR, LEAN)) pathTraceBlockKernel(const DevScene S, const Job job, uint refillBelow, uint nodeMin);

// ---- wavefront schedule (hpt_wavefront.hip) --------------------------------------------------------------------------------------------
static const uint WF_RANGES = 64u;                   // the trace kernel pulls rays from this many ranges of the queue (work stealing)
static const uint WF_CTR_WORDS = 32u * (1u + WF_RANGES);
static const uint WF_SUSP_WORDS = 10u;               // cur, sp, curInst, hitT, hitU, hitV, hitPrim, hitInst, found, (spare)
static const uint WF_ALIVE = 1u, WF_PEND = 2u, WF_ENDING = 4u;   // status bits; passes left in bits 8..31

struct WfPool
{
  float4* rayO;      // rpos.xyz, misPdf
  float4* rayD;      // rdir.xyz, misIor
  float4* thr;       // throughput.xyz, flags
  float4* acc;       // accumulated radiance.xyz, bounce
  float4* shO;       // shadow ray origin.xyz, far
  float4* shD;       // shadow ray direction.xyz
  float4* contrib;   // thr * shade of the pending light sample
  float4* hit;       // t, u, v, primId
  uint*   hitInst;   // instId or 0xFFFFFFFF
  uint*   occl;      // shadow ray result
  uint*   status;
  float*  lossSlot;  // DR: per-slot sum of the pixel's sample losses (reduced in double at the end: one float accumulator for 10^7..10^8
                     // samples loses the small increments - measured 1.5 % low on the 1M-triangle scene)
  float*  time;      // motion blur: the path's time in [0, 1] (drawn at regeneration, read by the trace pass and by the shading of every vertex)
  float4* waves;     // spectral rendering (wfShadeSpecKernel): the path's four wavelengths; thr / acc / contrib then hold four samples each and
  uint2*  fb;        // ... the flags and the bounce counter live here
  uint*   inflight;  // bit 0 / 1: the slot's closest-hit / shadow ray was suspended by a trace pass and has not finished yet
  uint*   rayQ[2];   // compacted ray queue of round (iteration & 1): slot id | (shadow ray ? 1 << 31 : 0) | (resumed ray ? 1 << 30 : 0)
  uint*   susp[2];   // traversal state of the rays a trace pass suspended, written for the NEXT round: [WF_SUSP_WORDS + stack][maxSusp],
                     // record k belongs to queue entry k of that round (suspended rays are queued first)
  uint    maxSusp;   // records per buffer (= lanes of the trace grid: a lane suspends at most one ray per pass)
  uint    suspStack; // stack entries per record
  uint*   ctr;       // two sets of WF_CTR_WORDS (set iteration & 1 is live): [0] rays queued by the shade pass;
                     // [32 * (1 + r)] head of queue range r for the trace pass (one 128-byte line each: the atomics of different
                     // ranges go to different L2 channels instead of serialising on one address)
};

struct WfJob
{
  uint   itemBase, itemCount;     // pool slot s renders work item itemBase + s (item -> tid as in Job)
  uint   tidBegin, tidChunk, tidStride, tidEnd;
  uint   passNum, channels, iter;
  uint   drSkipNonFinite;         // as in Job
  float* outColor;
  Rng*   gens;
  const uint* packedXY;
  // differentiable rendering (wfShadeKernel<DR = true>): a_refImg, a_data, a_dataGrad, loss accumulator, adjoint records [bounce][field][slot];
  // the adaptive forward call (wfShadeKernel<.., ADAPT>, wfInitCountsKernel; no DR call runs them) keeps its two arrays in the storage of two of
  // these pointers, as Job does: passCounts (null: passNum for every pixel) and moments (null: no statistics), both indexed by absolute tid
  union { const float* refImg; const uint* passCounts; }; const float* data; union { float* grad; PixelMoments* moments; }; float* lossAccum; float* record;
  const float* adjImg; uint vjp;  // PathTraceVJP: as in Job
  union { uint drLightFirst; uint drEnvPlaneOn; };   // (wfShadeKernel<.., ENV>, where no light is registered: the env plane of the record exists)
  uint drLightCount, drLightOff;                 // light-colour gradients (wfShadeKernel<.., LGRAD>): DrLights; count 0 otherwise
};
static_assert(sizeof(WfJob) == 128, "WfJob is a by-value argument of every shade kernel: its size and layout stay");
static const uint WF_MAX_PASSES = 0xFFFFFFu;         // passes of a pixel per call: what bits 8..31 of the status word hold

#ifndef HPT_WF_SHADE_FULL_WAVES
#define HPT_WF_SHADE_FULL_WAVES 3      // the shade kernel with every BSDF branch: 1 M-triangle interior forced onto it 209 (4 waves) -> 214 Mpaths/s (profiles/ab_wfs.sh)
#endif
#ifndef HPT_WF_SHADE_WAVES
#define HPT_WF_SHADE_WAVES 5           // the lean forward shade kernel (98 VGPRs, no spills): 1 M triangles 4 / 5 / 6 waves -> 286.8 / 291.8 / 270.4 Mpaths/s (profiles/ab.sh)
#endif
#ifndef HPT_WF_SHADE_DR_WAVES
#define HPT_WF_SHADE_DR_WAVES 4        // the DR shade kernel holds the adjoint record's terms as well (112 VGPRs)
#endif
#ifndef HPT_WF_WAVES
#define HPT_WF_WAVES 5   // measured on the 1M-triangle scene: 4 -> 213, 5 -> 224, 6 -> 217 Mpaths/s (96 VGPRs: no spills; 24 KB of LDS per block)
#endif
#define HPT_WFS_BOUNDS(DR, LEAN) __launch_bounds__(256, (DR) ? HPT_WF_SHADE_DR_WAVES : ((LEAN) ? HPT_WF_SHADE_WAVES : HPT_WF_SHADE_FULL_WAVES))

// Ray compaction of the shade kernels. Every wave ballots its two kinds of rays and prefix-sums the lanes (mbcnt); the four waves of the block add
// their counts in LDS and ONE atomicAdd per block reserves the block's run of the queue. (One atomic per wave was measured at
// 0.97 ms per shade pass over 2M slots: ~100 K atomics on one address serialise in a single L2 channel.)
HPT_DEV void blockAppend(uint* counter, bool qNear, bool qShad, uint& posNear, uint& posShad)
{
  __shared__ uint waveCnt[4];
  __shared__ uint blockBase;
  const unsigned long long mn = __ballot(qNear), ms = __ballot(qShad);
  const uint cn = (uint)__popcll(mn), cs = (uint)__popcll(ms);
  const uint wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) waveCnt[wave] = cn + cs;
  __syncthreads();
  if (threadIdx.x == 0u) {
    const uint tot = waveCnt[0] + waveCnt[1] + waveCnt[2] + waveCnt[3];
    blockBase = tot ? atomicAdd(counter, tot) : 0u;
  }
  __syncthreads();
  uint base = blockBase;
  for (uint w = 0; w < wave; w++) base += waveCnt[w];
  posNear = base + mbcnt64(mn);
  posShad = base + cn + mbcnt64(ms);
}

__global__ void wfInitKernel(WfPool P, uint n, uint passNum);
// Adaptive sampling under the wavefront schedule ("Wavefront form").
// wfInitCountsKernel: wfInitKernel with the slot's own pass count - slot s of job.itemCount serves the tid the shade kernel maps it to and starts
// with job.passCounts[tid] passes (null: job.passNum); a slot whose tid lies past job.tidEnd gets none.
__global__ void __launch_bounds__(256) wfInitCountsKernel(WfPool P, const WfJob job);
// WfCountsSummary: what the host has to know of the counts before it writes anything - the largest, how many are above 0 (the call's active
// pixels) and how many exceed WF_MAX_PASSES. wfCountsSummaryKernel: one lane per work item of the call (job.itemBase .. + job.itemCount, item -> tid
// as in the shade kernel); wave shuffles, then one integer atomic per block and field into *out (zeroed before).
struct WfCountsSummary { uint maxCount, active, over; };
__global__ void __launch_bounds__(256) wfCountsSummaryKernel(const WfJob job, WfCountsSummary* out);
#ifndef HPT_STREAM_WAVES
#define HPT_STREAM_WAVES 5
#endif
template <bool DEEP>                                                    // block-owned streaming form of the wavefront schedule (hpt_stream.hip; schedule 4)
__global__ void __launch_bounds__(256, HPT_STREAM_WAVES) streamKernel(const DevScene S, const WfPool P, const WfJob job, uint slotsPerBlock, uint refillBelow, uint* blockQueues,
                                                                      uint* stackOverflow, uint gridLanes);
template <int SCOPE, bool ADAPT = false>                                // spectral rendering under the wavefront schedule (hpt_spectral.hip); ADAPT: the moments of WfJob::moments, as in wfShadeKernel
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) wfShadeSpecKernel(const DevScene S, const WfPool P, const WfJob job);
// FILM: shadeVertex<FILM> (thin films, hpt_film.h); LGRAD (with DR): light-colour gradients; ENV (with DR): environment maps;
// ADAPT (forward, without FILM): the luminance moments of WfJob::moments at kernel_ContributeToImage (the per-pixel pass counts are the slots' initial status)
template <bool DR, bool LEAN, bool MOTION = false, bool FILM = false, bool LGRAD = false, bool ENV = false, bool ADAPT = false>
__global__ void HPT_WFS_BOUNDS(DR, LEAN) wfShadeKernel(const DevScene S, const WfPool P, const WfJob job);
template <bool DEEP, bool FLAT, bool STATS, bool MOTION = false, bool WIDE = false>   // WIDE: walk DevScene::nodes4 (4-wide compressed nodes) instead of the BVH2
__global__ void __launch_bounds__(256, HPT_WF_WAVES) wfTraceKernel(const DevScene S, const WfPool P, uint iter, uint refillBelow, uint grace,
                                                                   uint* stackOverflow, uint gridLanes, Counters* counters);
// ---- EvalGBuffer (hpt_gbuffer.hip) -----------------------------------------------------------------------------------------------------
struct GBufferPixel { float depth, norm[3], texc[2], rgba[4], shadow, coverage; int matId, objId, instId; };   // integrator_pt.h:187-198 = hpt_gbuffer_pixel
static_assert(sizeof(GBufferPixel) == 60, "GBufferPixel is 15 dwords");
// one lane per (pixel, sample): 16 * blockNum lanes in blocks of 256; `samples` (null or 16 * blockNum records) receives the records before the reduction
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) gbufferKernel(const DevScene S, const uint* packedXY, uint blockNum, GBufferPixel* out, GBufferPixel* samples, uint* stackOverflow);
// ---- DenoiseFrame (hpt_denoise.hip) -----------------------------------------------------------------------------------------
// The pack kernel reads color / gbuffer and writes cin, planeN, planeA; a pass reads cin, planeN, planeA and writes cout (the last pass: the
// caller's frame, with the alpha from color). Planes: C = {r, g, b, instId}, N = {n.xyz, depth}, A = {albedo.rgb, matId}.
struct DenoiseJob
{
  const float4* color; const GBufferPixel* gbuffer;   // the caller's frame and records (pack kernel; color also by the last pass)
  float4* cin; float4* cout; float4* planeN; float4* planeA;
  size_t pixels; uint width, height;
  uint  step;                     // s = 1 << i
  uint  normalSquarings, flags;
  uint  terms;                    // bit 0 / 1 / 2: sigmaDepth / sigmaColor / sigmaAlbedo is not 0
  float normConst;
  float sigmaDepthStep;           // sigmaDepth * float(s)
  float sigmaColor2;              // sc * sc, sc = sigmaColor * 2^-i
  float sigmaAlbedo2;             // sigmaAlbedo * sigmaAlbedo
};
__global__ void __launch_bounds__(256) denoisePackKernel(const DenoiseJob job);                   // one lane per pixel, blocks of 256
// one lane per pixel, a block = 32 x 8 pixels; TILE 0: taps loaded from memory; 1 / 2: from an LDS tile with a halo of 2 * TILE pixels, for step TILE.
// Measured at 1920 x 1080 (profiles/denoise.md): the passes at steps 1 and 2 take 0.185 / 0.122 ms from the tile against 0.227 / 0.151 ms with direct
// loads, the call 0.783 against 0.859 ms, the results equal bit for bit. -DHPT_DENOISE_LDS=0 builds the direct-load form for A/B.
#ifndef HPT_DENOISE_LDS
#define HPT_DENOISE_LDS 1
#endif
template <bool LAST, int TILE = 0> __global__ void __launch_bounds__(256) denoisePassKernel(const DenoiseJob job);
// ---- DenoiseFrameVar (hpt_denoise.hip): the same filter with a variance-scaled luminance stop and a fourth plane V ---------------
// A job of its own and kernels of their own: DenoiseJob and the instantiations of DenoiseFrame stay as they are. d.sigmaColor2 and bit 1 of d.terms
// are not used. V: one float per pixel, the variance of the (prepared) pixel, two buffers that ping-pong with the colours.
struct DenoiseVarJob
{
  DenoiseJob d;
  const float* variance;          // the caller's plane (pack kernel)
  float* vin; float* vout;
  float* outVar;                  // the caller's filtered variance (last pass) or null
  float sigmaLum2;                // sigmaLum * sigmaLum
  float varFloor;
  uint  prefilter;                // not 0: the stop reads the 3 x 3 binomial mean of V at unit spacing
  uint  useLum;                   // sigmaLum is not 0
};
__global__ void __launch_bounds__(256) denoiseVarPackKernel(const DenoiseVarJob job);            // one lane per pixel, blocks of 256
// mapping and tiles as denoisePassKernel; the tile gains TW * TH floats of V (22 464 / 33 280 B at TILE 1 / 2)
template <bool LAST, int TILE = 0> __global__ void __launch_bounds__(256) denoiseVarPassKernel(const DenoiseVarJob job);
// ---- CastSingleRayBlock / RayTraceBlock (hpt_raytrace.hip) -----------------------------------------------------------------------------
// one lane per pixel of packedXY[0 .. tidCount); outColor: winWidth * winHeight pixels of 4 floats (assigned) / of `channels` = 3 or 4 floats (added to)
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) castSingleRayKernel(const DevScene S, const uint* packedXY, uint tidCount, float* outColor, uint* stackOverflow);
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) rayTraceKernel(const DevScene S, const uint* packedXY, uint tidCount, uint channels, float* outColor, uint* stackOverflow);
// ---- IntegratorDR::RayTraceDR (hpt_raytrace_dr.hip) ------------------------------------------------------------------------------------
// one lane per pixel of packedXY[0 .. tidCount); outColor: pixels of 4 floats (hits assigned, misses untouched); refImg: pixels of `channels` = 3 or 4
// floats, bottom-up; GRAD: registered textures are fetched from `data` and `grad` is accumulated into; lossPerPixel [tidCount] and lossAccum may be null
template <bool FLAT, bool MOTION, bool SWEEP, bool GRAD>
__global__ void __launch_bounds__(256) rayTraceDrKernel(const DevScene S, const uint* packedXY, uint tidCount, uint channels, float passNum, float* outColor,
                                                        const float* refImg, const float* data, float* grad, float* lossPerPixel, float* lossAccum, uint* stackOverflow);

// ---- IntegratorQMC::PathTraceBlock (hpt_qmc.hip) ---------------------------------------------------------------------------------------
static const uint QMC_DIMENSIONS = 11u, QMC_RESOLUTION = 31u;
struct QmcJob
{
  const uint* table;              // QMC_DIMENSIONS x QMC_RESOLUTION generator-matrix columns (qmc_table.h; uploaded once per context)
  uint   samples;                 // S = min(2^32 - 1, pixels x passes)
  uint   gensCount;               // N = size of m_randomGens: sample s runs on generator s % N
  uint   dofDim, motionDim, matDim, lgtDim;   // EnableQMC's dimension offsets (0: that draw stays pseudo)
  float4* sampleColor;            // per-sample records, indexed by s (both null or both set): the colour as added ...
  uint*   samplePixel;            // ... and the pixel index y * winWidth + x
  uint    spdDim;                 // spectral QMC: the hero-wavelength dimension (0: pseudo) ...
  float4* sampleWaves;            // ... and a third record, the sample's four wavelengths (null, or set with the other two)
};
// qmc::rndFloat (rnd_qmc.cpp:189-196). `dim` is wave-uniform, so the 31 columns are scalar loads from the 1364-byte table.
HPT_DEV float qmcFloat(const uint* __restrict__ table, uint pos, uint dim)
{
  const uint* __restrict__ col = table + dim * QMC_RESOLUTION;
  uint r = 0u;
#pragma unroll
  for (uint bit = 0; bit < QMC_RESOLUTION; bit++) r ^= ((pos >> bit) & 1u) ? col[bit] : 0u;
  return (float)(r + 1u) * (1.0f / 2147483648.0f);             // uint -> float rounds to nearest; INT_SCALE = 1 / float(0x80000001) = 2^-31
}
// IntegratorQMC::GetRandomNumbersLgts / GetRandomNumbersMats (integrator_qmc.cpp:117-139): the pseudo draws are made at every bounce - the
// lights' float4 BEFORE the selection float, the reverse of the base class - and the first bounce's .x / .y (and the light selection)
// are then replaced by the sample's QMC dimensions, unless EnableQMC left them to the generator (dimension 0).
// The policy of shadeVertex (hpt_qmc.hip) and of shadeVertexSpec (hpt_spectral.hip: pathTraceQmcSpectralKernel).
struct QmcRands
{
  const uint* table; uint s, matDim, lgtDim;
  HPT_DEV V4 lights(Rng& gen, uint bounce, float& rndId) const
  {
    V4 r = rng_float4(gen);
    rndId = rng_float1(gen);
    if (bounce == 0u && lgtDim != 0u) { r.x = qmcFloat(table, s, lgtDim); r.y = qmcFloat(table, s, lgtDim + 1u); rndId = qmcFloat(table, s, lgtDim + 2u); }
    return r;
  }
  HPT_DEV V4 mats(Rng& gen, uint bounce) const
  {
    V4 r = rng_float4(gen);
    if (bounce == 0u && matDim != 0u) { r.x = qmcFloat(table, s, matDim); r.y = qmcFloat(table, s, matDim + 1u); }
    return r;
  }
  HPT_DEV float blend(Rng& gen, uint /*bounce*/, uint /*layer*/) const { return rng_float1(gen); }   // IntegratorQMC::GetRandomNumbersMatB: pseudo
};
// Job carries outColor (may be null when the records are asked for), channels, gens, queue, packedXY / packedCount (camera back plate),
// the stack overflow area and tidCount = min(N, S) generator slots with work
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) pathTraceQmcKernel(const DevScene S, const Job job, const QmcJob q);
// The same sample loop under the wavefront schedule (hpt_wavefront.hip; hpt_set_option "qmc_wavefront"): pool slot s of the launch serves generator
// slot itemBase + s. wfInitQmcKernel gives it its number of samples, (samples - 1 - slot) / gensCount + 1 <= WF_MAX_PASSES, as its pass count;
// wfShadeQmcKernel is wfShadeKernel's pass with pathTraceQmcKernel's sample start, QmcRands and path end (RGB without thin films, traceDepth > 0;
// packedCount: entries of WfJob::packedXY, read for the camera back plate only). MOTION: moving instances.
__global__ void __launch_bounds__(256) wfInitQmcKernel(WfPool P, uint itemBase, uint itemCount, uint samples, uint gensCount);
template <bool MOTION>
__global__ void __launch_bounds__(256, HPT_WF_SHADE_FULL_WAVES) wfShadeQmcKernel(const DevScene S, const WfPool P, const WfJob job, const QmcJob q, const uint packedCount);
// the same sample loop on four wavelengths per path (hpt_spectral.hip); SCOPE and its launch bounds as pathTraceSpectralKernel
template <bool DEEP, bool FLAT, bool SWEEP, bool MOTION, int SCOPE>
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) pathTraceQmcSpectralKernel(const DevScene S, const Job job, const QmcJob q);

// ---- IntegratorKMLT (mlt/integrator_kmlt.cpp; hpt_kmlt.hip) ------------------------------------------------------------------------------
static const uint KMLT_BOUNCE_START = 6u, KMLT_LGHT_ID = 0u, KMLT_MATS_ID = 4u, KMLT_BLND_ID = 8u, KMLT_PER_BOUNCE = 10u;   // integrator_kmlt.cpp:33-37
// IntegratorKMLT::GetRandomNumbers* (:87-151): slot i of the lane's vector is x[i * stride]. A blend layer of 2 or more reads into the next
// bounce's light numbers, as the reference indexes it; a slot past the vector's end reads 0. Slots 0 - 3 are the film and lens
// point, 4 the wavelength sample (GetRandomNumbersSpec; read under m_spectral_mode only), 5 the time.
// The policy of shadeVertex (hpt_kmlt.hip: pssEval) and of shadeVertexSpec (hpt_spectral.hip: pssEvalSpec).
struct PssRands
{
  const float* x; size_t stride; uint n;
  HPT_DEV float at(uint i) const { return i < n ? x[(size_t)i * stride] : 0.0f; }
  HPT_DEV V4 lights(Rng&, uint bounce, float& rndId) const
  {
    const uint b = KMLT_BOUNCE_START + bounce * KMLT_PER_BOUNCE + KMLT_LGHT_ID;
    const V4 r = v4(at(b), at(b + 1u), at(b + 2u), at(b + 3u));
    rndId = r.w;
    return r;
  }
  HPT_DEV V4 mats(Rng&, uint bounce) const
  {
    const uint b = KMLT_BOUNCE_START + bounce * KMLT_PER_BOUNCE + KMLT_MATS_ID;
    return v4(at(b), at(b + 1u), at(b + 2u), at(b + 3u));
  }
  HPT_DEV float blend(Rng&, uint bounce, uint layer) const { return at(KMLT_BOUNCE_START + bounce * KMLT_PER_BOUNCE + KMLT_BLND_ID + layer); }
};
// PathTraceF over caller-supplied number vectors: lane i < n reads vector i at x[i * vecStride + slot] and writes color[i], pixel[i]
struct PssJob
{
  const float* x; uint n, vecStride, stateSize;
  float4* color; uint* pixel;
  const uint* packedXY; uint packedCount;    // the camera back plate reads m_packedXY[tid], tid = the lane (past the vector's end: 0)
  uint* stackOverflow; uint gridLanes;
  float4* waves; float4* accum;              // spectral pass only, each may be null: the path's four wavelengths, its raw exposure * accumColor[i]
};
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) pathTracePssKernel(const DevScene S, const PssJob job);
// the same pass under m_spectral_mode (hpt_spectral.hip: pssEvalSpec); SCOPE and its launch bounds as pathTraceSpectralKernel
template <bool DEEP, bool FLAT, bool SWEEP, bool MOTION, int SCOPE>
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) pathTracePssSpectralKernel(const DevScene S, const PssJob job);
// the Markov chains: lane c < chains runs chain c for `steps` steps; cur / prop: the chain's current vector and its proposal, [slot][chain]
struct KmltJob
{
  uint chains, steps, stateSize;
  float* cur; float* prop;
  float* outColor;                           // winWidth * winHeight * 4 floats, added to with float atomics
  const uint* packedXY; uint packedCount;
  uint* stackOverflow; uint gridLanes;
  double* accumBrightness; uint* largeSteps; uint* accept;   // per chain
  // records (hpt_kmlt_records; each may be null): per chain and step [c * steps + i], per chain [c], per chain, step and slot
  unsigned char* recLarge; unsigned char* recAccepted; float* recA; float4* recColor; uint* recPixel; uint* recOldPixel;
  float4* recInitColor; uint* recInitPixel; float* recProposals;
  float4* recContribX; float4* recContribY;   // the two contributions of a step as formed, .w = 1 when the step added it to the film (the > 1e-12 test)
};
template <bool DEEP, bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256, HPT_FILM_WAVES) kmltChainKernel(const DevScene S, const KmltJob job);
// the same chains (hpt_kmlt_chain.h: kmltChainBody) around pssEvalSpec
template <bool DEEP, bool FLAT, bool SWEEP, bool MOTION, int SCOPE>
__global__ void __launch_bounds__(256, SCOPE == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES) kmltChainSpectralKernel(const DevScene S, const KmltJob job);
// stats4 = { avgBrightness, actualBrightness, acceptance rate, normConst } from the per-chain sums and the frame (one block); then frame *= normConst
__global__ void __launch_bounds__(256) kmltStatsKernel(const float4* frame, uint pixelsNum, uint passNum, uint chains, const double* accumBrightness,
                                                       const uint* largeSteps, const uint* accept, double* stats4);
__global__ void __launch_bounds__(256) kmltScaleKernel(float* frame, size_t n, const double* stats4);

// ---- camera plug-in: CamPinHole / CamTableLens (cam_plugin/CamPinHole.cpp, CamTableLens.cpp; hpt_camrays.hip) -----------------------------
// One lane per ray of a tile: lane tid serves pixel p = firstPixel + tid (x = p % width, y = p / width: the reference's pitch-linear split) and
// owns slot tid of the three per-lane arrays. The scalars and the lens lines are the same for every lane (scalar loads).
struct CamJob
{
  uint   n, firstPixel, width, height;   // rays of this tile; subPassId * batchSize
  float  projInv[16];                    // m_projInv, column-major
  float  physSize[2];                    // m_physSize
  uint   lensCount, numCie;
  const float4* lensLines;               // {curvatureRadius, thickness, eta, apertureRadius}, film side first
  const float4* cie;                     // m_cie_xyz
  Rng*   gens;                           // m_randomGens
  float* waves;                          // m_storedWaves
  float* cos4;                           // m_storedCos4
  float4* rayPos; float4* rayDir;        // MakeRaysBlock: RayPosAndW / RayDirAndT [n]
  const float* colors;                   // AddSamplesContributionBlock: 4 floats per ray, 1 in spectral mode
  float4* frame;                         // ... and the width * height frame
};
enum : int { CAM_PINHOLE = 0, CAM_TABLE_LENS = 1 };
template <int KIND, bool SPECTRAL> __global__ void __launch_bounds__(256) camMakeRaysKernel(const CamJob job);
template <int KIND, bool SPECTRAL> __global__ void __launch_bounds__(256) camContribKernel(const CamJob job);
__global__ void __launch_bounds__(256) camInitGensKernel(Rng* gens, uint n);   // RandomGenInit(i + 12345 * i), 32-bit wrap-around

__global__ void __launch_bounds__(256) wfLossReduceKernel(const float* lossSlot, uint n, double* acc);
__global__ void wfLossFinishKernel(const double* acc, float* loss);

// ---- adaptive sampling: planner and resolve (hpt_adaptive.hip) ---------------------------------------------------------------
struct AdaptiveParams { float tol, lumFloor; uint minPasses, maxPasses, step, dilate; };                       // = hpt_adaptive_params
struct AdaptiveInfo { unsigned long long passes; uint pixels, maxPasses, nonfinite, rounds; float deviceMs; uint reserved; };   // = hpt_adaptive_info
static_assert(sizeof(AdaptiveParams) == 24 && sizeof(AdaptiveInfo) == 32, "the planner's records are 6 and 8 dwords");
// one lane per tid of [tidBegin, tidBegin + tidCount): need[y * winWidth + x] = passes the pixel's moments ask for beyond those it has
__global__ void __launch_bounds__(256) adaptiveNeedKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, AdaptiveParams p, uint* need);
// ... counts[tid] = the (dilated) need, clipped to maxPasses and to step; the totals are added to *info: one integer atomic per block and field
__global__ void __launch_bounds__(256) adaptivePlanKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, uint winHeight,
                                                          AdaptiveParams p, const uint* need, uint* counts, AdaptiveInfo* info);
// ... out[pixel] = frame[pixel] / passes for the first three channels (0 for a pixel without passes), the fourth copied; out may be frame
__global__ void __launch_bounds__(256) adaptiveResolveKernel(const float* frame, const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth,
                                                             uint channels, float* out);
// one lane per tid of the window: outVar[y * winWidth + x] = the estimated variance of the pixel's mean luminance; other pixels are not written
__global__ void __launch_bounds__(256) adaptiveVarianceKernel(const PixelMoments* moments, const uint* packedXY, uint tidBegin, uint tidCount, uint winWidth, float* outVar);

// ---- helper kernels (hpt_helpers.hip) ---------------------------------------------------------------------------------------------------
__global__ void packXYKernel(uint* out, int W, int H, uint ts);
__global__ void initRandomGensKernel(Rng* gens, uint n, uint firstSeed);
template <bool FLAT, bool MOTION, bool SWEEP>                           // batched RayQuery_NearestHit / RayQuery_AnyHit; `time` is read by the MOTION variants
__global__ void __launch_bounds__(256) rayQueryKernel(const DevScene S, const float4* posNear, const float4* dirFar, uint n, void* out, int anyHit, uint* stackOverflow, float time);
__global__ void image2D4fRegularizerKernel(int w, int h, const float4* data, float4* grad);
__global__ void adamStepKernel(float* state, const float* grad, float* momentum, float* gsq, size_t n, float gamma);
__global__ void refitTriBoxesKernel(const BvhTri* tris, const float* instMat, uint n, float* triBox);
__global__ void refitLevelKernel(BvhNode* nodes, const uint* ids, uint count, const float* triBox, float* bounds);
__global__ void refitNodes4Kernel(BvhNode4* nodes4, const uint* src, const BvhNode* nodes2, uint count);
__global__ void __launch_bounds__(256) refitSahKernel(const BvhNode* nodes, const uint* ids, uint count, uint rootId, double* out);   // out[0] += the inner children's half-areas, out[1] = the root's
__global__ void buildShadeTrisKernel(const DevScene S, uint n, float4* out);

} // namespace hpt
