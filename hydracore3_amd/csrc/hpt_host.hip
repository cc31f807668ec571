// Host side of the C ABI (include/hydra_hip.h): context, BVH2 build + upload, scene tables, launches, timing.
// Compiled by hipcc and linked with the kernel units; exports only the extern "C" hpt_* symbols.
#include "plastic_precompute.h"
#include "film_precompute.h"
#include "jpeg_decode.h"
#include "qmc_table.h"
#include "cie_fit.h"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <new>
#include <stdexcept>
#include <vector>
#include <set>
#include <chrono>
#include <dlfcn.h>
#include <sched.h>
#include <thread>
#include <atomic>
#include <type_traits>

#include "../../include/hydra_hip.h"
#include "hpt_decl.h"
#include "bvh_build.h"
#include "hpt_lbvh.h"

// Pass slices of the forward megakernel when hpt_set_option("pass_slice") was never called (passSliceAuto below). The hand-over is a mailbox of
// tagged words with no release and no acquire (hpt_kernels.hip), so slices shorter than the 256 passes of the fenced form pay; what stands
// behind each constant is measured in profiles/slice_mailbox.md (m = pixels per lane of the grid, Mpaths/s, whole pixels -> best slice):
//   PASS_SLICE_MIN_M 2    m = 2 gains with every slice tried (5703 -> 6992 at 64); m = 1 and m = 0.5 lose with every slice (9336 -> 9182 at best,
//                         14615 -> 13184); nothing between one and two was measured, so two is the smallest value known to gain
//   PASS_SLICE_MAX_M 8    m = 4 gains, m = 16 loses with 64 and with 128 (3782 -> 3574, 3693): sixteen whole pixels per lane already even out the
//                         end of the call. Nothing between was measured; eight is the middle of the two in ratio
//   PASS_SLICE_MIN_PASSES 256   the shortest call measured, and it gains (m = 4: 3372 -> 3532 at 64); shorter calls keep whole pixels
//   64 or 128             m = 4 at 1024 passes: 128 is best (3650 ... 3654; 64: 3603 ... 3609, 256: 3630 ... 3636, 32: 3364 ... 3366, 512: 3550 ... 3556);
//                         at 512 passes 128 and 64 are close (3590, 3575); at 256 passes 64 (3532; 128: 3490); m = 2 at 1024 passes 64 (6992; 128: 6911).
//                         In lane-passes, m x passes: 4096 -> 128, 2048 -> either, 1024 -> 64, 2048 -> 64: 128 where it still leaves a lane
//                         PASS_SLICE_LONG_ITEMS = 32 items, 64 elsewhere. 32 passes per item lose everywhere.
static const uint PASS_SLICE_MIN_M = 2u, PASS_SLICE_MAX_M = 8u, PASS_SLICE_MIN_PASSES = 256u, PASS_SLICE_SHORT = 64u, PASS_SLICE_LONG = 128u, PASS_SLICE_LONG_ITEMS = 32u;
static uint passSliceAuto(uint64_t tidCount, uint64_t gridLanes, uint64_t passNum)
{
  if (tidCount < PASS_SLICE_MIN_M * gridLanes || tidCount >= PASS_SLICE_MAX_M * gridLanes || passNum < PASS_SLICE_MIN_PASSES) return 0u;
  return tidCount * passNum >= (uint64_t)PASS_SLICE_LONG_ITEMS * PASS_SLICE_LONG * gridLanes ? PASS_SLICE_LONG : PASS_SLICE_SHORT;
}
static const float BLOCK_SAH_VISITS = 8.0f;                     // automatic schedule: from this many expected inner-node visits per ray the megakernel repacks rays block-locally (hpt_block.hip)
static const uint MAX_STACK = 64;                           // traversal stack entries per lane: LDS_STACK in LDS + the rest in an HBM overflow buffer
// Static scenes with at most this many INSTANCED triangles get the single-level world-space BVH (48 B + ~32 B of nodes per triangle:
// 32 M triangles = 2.6 GB of the 288 GB); beyond it (heavy instancing) the two-level TLAS/BLAS layout is kept.
static const size_t FLAT_TRI_BUDGET = size_t(32) << 20;

using namespace hpt;

// Scenes with at least this many instanced triangles count as "heavy": wavefront schedule, single-level BVH, voted exit of the node loop.
// A "heavy" scene is one whose committed BVH is expected to cost a ray at least this many inner-node visits (sah_node_visits, the
// surface-area estimate): it gets the wavefront schedule (when the call has enough pixels) and the voted node-loop exit. Measured
// (profiles/sah_info.py, crossover.sh, crossover_small.sh, full_kernel.py): Cornell box 8.5, test_228 (8 202 triangles) 10.3, the own fixtures
// 3.7 ... 4.8 - all fastest on the megakernel without the vote (test_228: 667 vs 531 Mpaths/s); the interior generator from 4 850 to 1 M
// triangles 30 ... 60 - all fastest on the wavefront schedule with the vote (4 850 triangles: 340 vs 254). The triangle count does not
// separate the two families (test_228 has more triangles than the smallest interior).
static const float  HEAVY_SAH_VISITS = 20.0f;
static const uint   WF_AUTO_PIXELS = 1u << 19;            // fewer pixels per call cannot keep the wavefront trace kernel's lanes supplied (see useWavefront)
static const size_t FLAT_AUTO_TRIS = size_t(1) << 12;      // instanced triangles from which the single-level layout is chosen whatever the instance count
// Tiny scenes (the Cornell-box class): no tree walk at all, the wave sweeps the instances' triangles with scalar loads (hpt_device.h: traceSweep).
// Cost is linear in the triangle count (one exact triangle test per lane and triangle, ~72 VALU instructions at 100 % lane utilisation) against
// ~2 450 issue slots per ray of the BVH walk on the Cornell box at 31 % utilisation: the crossover sits around 32 instanced triangles.
static const size_t SWEEP_MAX_TRIS = 32, SWEEP_MAX_INSTS = 8;
// Pair cull of the sweep (hpt_types.h: sweepPairPlane, hpt_device.h: traceSweep): on by default, hpt_set_option("sweep_cull", 0) for A/B.
#ifndef HPT_SWEEP_CULL
#define HPT_SWEEP_CULL 1
#endif
// Per-lane pair pass of the sweep (hpt_types.h: sweepPairBox, hpt_device.h: traceSweep): on by default, hpt_set_option("sweep_lanes", 0) for A/B.
#ifndef HPT_SWEEP_LANES
#define HPT_SWEEP_LANES 1
#endif
static const size_t MANY_INSTANCES = 6;                      // instances from which the single-level layout is chosen for light scenes too (see hpt_commit_scene)

// What the sections of this file share besides the context: kept in a hidden namespace, so that none of it becomes a dynamic export when the
// sections are compiled as units of their own (tests/test_cpu.py: test_library_exports_every_declared_symbol)
namespace hpt { namespace host __attribute__((visibility("hidden"))) {

struct Geom
{
  std::vector<float> pos;        // xyz per vertex (tightly packed copy)
  std::vector<uint>  idx;
  Bvh2               bvh;        // local references
  std::vector<BvhTri> tris;      // BVH order
  bool               dirty = true;
};

struct Inst { uint geomId; float m[16]; bool motion = false; float m1[16] = {0}; };   // m1: the matrix at time 1 of a moving instance (AddInstanceMotion)

template <class T>
struct DevBuf                      // owning device array; freed on scope exit (locals on error paths) or with its owner (the context, a wavefront group, a camera)
{
  T* p = nullptr; size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  hipError_t alloc(size_t count) { if (count <= n && p) return hipSuccess; release(); n = count; return count ? hipMalloc((void**)&p, count * sizeof(T)) : hipSuccess; }
  hipError_t upload(const T* src, size_t count)
  {
    hipError_t e = alloc(count); if (e != hipSuccess) return e;
    return count ? hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
};

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} } // namespace hpt::host
using namespace hpt::host;

enum TimeSlot { T_PATH_TRACE, T_NAIVE, T_DR, T_FROM_RAYS, T_CAST_SINGLE_RAY, T_RAY_TRACE, T_PATH_TRACE_QMC, T_RAY_TRACE_DR, T_VJP, T_KMLT, T_DENOISE, T_DENOISE_VAR, T_SLOT_COUNT };   // (hpt_get_execution_time maps the reference's names to them)

struct hpt_ctx
{
  int device = 0, numCUs = 256;
  std::string err, devName;

  // ISceneObject state
  std::vector<Geom> geoms;
  std::vector<Inst> insts;
  bool accelCommitted = false;
  uint stackNeeded = 0;

  // device buffers
  DevBuf<BvhNode> dNodes; DevBuf<BvhTri> dTris; DevBuf<BvhInst> dInsts, dSweepInsts; DevBuf<BvhTri> dSweepTris; DevBuf<float> dSweepBoxes; DevBuf<SweepPlane> dSweepPlanes; DevBuf<SweepPairBox> dSweepPairBoxes;
  DevBuf<uint> dTriIndices, dMatIdByPrim, dMatVertOffset, dPackedXY;
  DevBuf<float> dVData, dNormMat;
  DevBuf<int> dRemapInst, dRemapLists;
  DevBuf<MaterialRec> dMaterials; DevBuf<LightRec> dLights; DevBuf<TexRec> dTextures;
  std::vector<void*> texData; std::vector<TexRec> hTextures;
  DevBuf<float> dSpecValues; DevBuf<uint> dSpecOffsetSz; DevBuf<float4> dCieXYZ;   // spectral tables (m_spec_values, m_spec_offset_sz, m_cie_xyz)
  bool spectralOk = false; std::string spectralWhyNot;   // whether the uploaded scene is within the spectral kernel's scope
  bool fewMaterialTypes = false;                         // at most three reachable material types, no blends / plastic / normal maps: the full-material kernel built for 4 waves (MODE 7)
  bool spectralGltfMats = true, spectralHeavyMats = true;   // a reachable material needs scope 1 (gltf) / scope 2 (glass, blend, normal map) of the spectral kernel (hpt_spectral.hip)
  // thin films (integrator_pt.h:587-590): the tables a film material indexes, and what the uploaded materials say about them
  DevBuf<float> dFilmsEtaK, dPrecompFilms; DevBuf<uint> dFilmsSpecId, dSpecTexIdsWavelengths, dSpecTexOffsetSz;
  std::vector<uint> hFilmsSpecId; size_t numFilmsEtaK = 0, numPrecompFilms = 0; uint numSpectraHost = 0;
  bool hasFilm = false, filmTablesRGB = true, filmTablesSpectral = true;   // a MAT_TYPE_THIN_FILM is in the table; its precomputed tables have the size RGB / spectral rendering reads
  DevBuf<float> dArrays1f; size_t numArrays1f = 0;       // m_arrays1f (pdf table of a sampled environment map)
  DevBuf<float4> dLensLines;                             // m_lines of the lens simulation (hpt_set_optics)
  DevBuf<float> dInstMotion, dNormMat2;                  // motion blur: key matrices of the moving instances, end-of-motion normal matrices
  // device refit of the single-level layout (refit_flat): the committed tree's nodes grouped by level, scratch boxes, what the tree was built for
  DevBuf<uint> dLevelNodes; DevBuf<float> dTriBox, dNodeBounds, dInstO2W;
  DevBuf<BvhNode4> dNodes4; DevBuf<uint> dNodes4Src;     // the single-level tree collapsed to 4-wide compressed nodes; per child the BVH2 (node << 1 | side) its box comes from
  uint nodes4Count = 0, stackNeeded4 = 0;                // (0: no wide tree)
  DevBuf<float4> dShadeTris;                             // DevScene::shadeTris (64 B per triangle record of the single-level layout), built lazily before a launch
  bool shadeTrisDirty = true, shadeTrisEnabled = true;   // (hpt_set_option("shade_records", 0): the kernels gather vertex data through the index chain)
  int  buildThreads = 0;                                 // hpt_set_option("build_threads", n): host threads of CommitScene (0: automatic)
  uint sweepCull = HPT_SWEEP_CULL;                       // hpt_set_option("sweep_cull", 0 / 1): the sweep skips the record pairs no ray of the wave can reach (DevScene::sweepCull)
  uint sweepLanes = HPT_SWEEP_LANES;                     // hpt_set_option("sweep_lanes", 0 / 1): the sweep tests each lane's candidate pairs only (DevScene::sweepLanes)
  bool statsWide = false;                                // hpt_set_option("stats_wide", 1): the instrumented probe walks the 4-wide tree (what a wavefront call on this scene does)
  bool wideEnabled = true;                               // hpt_set_option("wide_nodes", 0): the trace kernel walks the BVH2
  std::vector<uint> levelOffsets;                        // nodes of level l = dLevelNodes[levelOffsets[l] .. levelOffsets[l + 1])
  std::vector<BvhTri> flatTris;                         // host copy of the single-level layout's triangle records (BVH order)
  bool flatRefittable = false;                           // a single-level tree is committed and nothing but instance matrices / vertex positions changed since
  std::vector<uint> dirtyGeoms;                          // meshes whose vertices changed since the last commit (UpdateGeom_Triangles3f)
  bool refitEnabled = true;                              // hpt_set_option("refit", 0): always rebuild
  bool deviceRefit = false;                              // hpt_set_option("device_refit", 1): a device build leaves its level lists behind and an update of its tree is a refit
  bool flatOnDevice = false;                             // the committed single-level tree was built by hpt_lbvh.hip: no host copy of its records (flatTris), dNodes indexed by Karras node
  size_t flatNodes = 0;                                  // entries of dNodes that belong to the committed single-level tree (hpt_read_accel)
  int  refitMaxSahPct = 0;                               // hpt_set_option("refit_max_sah_pct", p): a refit whose estimate exceeds p % of the build's is followed by a build (0: never)
  float sahRefit = 0.0f; bool refitRejected = false;     // hpt_get_refit_info: the estimate after the last refit; the last commit's refit was rejected by the guard
  DevBuf<double> dRefitSah;                              // refitSahKernel's two results
  float tCommit[4] = {0, 0, 0, 0};                       // last CommitScene: host build ms, upload ms, device refit ms, 1 = refit / 0 = build
  float sahVisits = 0.0f;                                // expected inner-node visits per ray of the committed structure (sah_node_visits)
  bool anyMotion = false;                                // some instance moves: the MOTION kernel variants (either BVH layout, either schedule; no sweep, no refit)
  std::vector<MaterialRec> hMaterials;                   // host mirror of m_materials: the blend graph is validated as a whole
  std::vector<uint> hLightGeom;                          // geomType of every light, to validate m_envLightId
  std::vector<uint> hLightTex;                           // ... and its texId (dr_environment: is the map the env light reads registered?)
  std::vector<uint> hTriIndices;                         // host mirror of m_triIndices: Update_m_matIdOffsets re-validates the vertex indices a mesh will read
  bool envLightOk(uint id) const { return id < hLightGeom.size() && hLightGeom[id] == LIGHT_GEOM_ENV; }
  DevBuf<Rng> dGens;
  uint gensCount = 0;                                    // m_randomGens.size() as the last InitRandomGens / hpt_set_random_gens left it (the buffer never shrinks)
  DevBuf<uint> dQueue, dStackOvf; DevBuf<Counters> dCounters;
  // pass slices of the forward megakernel (hpt_kernels.hip): hpt_set_option("pass_slice", n), 0 = a work item is a whole pixel
  int  passSlice = -1;                                   // -1: by the rule passSliceAuto
  uint lastPassSlice = 0;
  DevBuf<unsigned long long> dSliceMail;                 // [tid][SLICE_MAIL_WORDS]: the slices' hand-over mailbox (hpt_types.h), zeroed before every sliced launch
  uint* sliceError = nullptr;                            // pinned, device-visible: a lane gave up waiting for its predecessor (sliceErrorCheck)
  // adaptive sampling (hpt_adaptive.hip): the loop's pass counts [tid], the planner's need image [pixel] and totals, the records of a
  // loop whose caller keeps none, the host forms' copies of the caller's arrays; all grown on first use, none allocated per round
  DevBuf<uint> dAdCounts, dAdNeed, dAdCountsIn; DevBuf<AdaptiveInfo> dAdInfo; DevBuf<PixelMoments> dAdMoments, dAdMomentsIn;
  bool adaptiveSpectral = false;                         // hpt_set_option("adaptive_spectral", 1): adaptive calls are served under m_spectral_mode (the ADAPT instantiations of hpt_spectral.hip)
  bool adaptiveWavefront = false;                        // hpt_set_option("adaptive_wavefront", 1): an adaptive call takes the wavefront schedule where a PathTraceBlock of its active pixels would
  DevBuf<WfCountsSummary> dAdSummary;                    // ... and the 12 bytes of its counts summary (wfCountsSummaryKernel)
  DevBuf<uint> dQmcTable;                                // the Niederreiter table of PathTraceBlockQMC: uploaded at the first call, 1364 bytes
  // PathTraceBlockKMLT (hpt_kmlt.hip): the chains' current and proposed vectors [slot][chain], the per-chain sums, the four statistics
  DevBuf<float> dKmltCur, dKmltProp; DevBuf<double> dKmltAccum, dKmltStats; DevBuf<uint> dKmltLarge, dKmltAccept;
  bool qmcSpectral = false;                              // hpt_set_option("qmc_spectral", 1): PathTraceBlockQMC serves m_spectral_mode (pathTraceQmcSpectralKernel) instead of refusing it
  bool qmcWavefront = false;                             // hpt_set_option("qmc_wavefront", 1): PathTraceBlockQMC takes the wavefront schedule (wfShadeQmcKernel) where a PathTraceBlock of as many pixels as it has generator slots would
  bool kmltSpectral = false;                             // hpt_set_option("kmlt_spectral", 1): PathTraceBlockKMLT and the PSS pass serve m_spectral_mode (kmltChainSpectralKernel / pathTracePssSpectralKernel)
  uint kmltChains = 0;                                   // hpt_set_option("kmlt_chains", n): 0 = one chain per lane of the resident grid
  uint kmltLastChains = 0;                               // chains of the last PathTraceBlockKMLT call: whose sums a normalise-only call reads
  DevBuf<float> dFrame, dRecord, dRef, dData, dGrad, dLoss; DevBuf<double> dLossAcc;
  DevBuf<float4> dDenoiseN, dDenoiseA, dDenoiseC[2];     // DenoiseFrame (hpt_denoise.hip): the guide planes and the two ping-pong colour planes; grown on demand
  DevBuf<float>  dDenoiseV[2];                           // DenoiseFrameVar: the two ping-pong variance planes (it shares the four above with DenoiseFrame)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // wavefront schedule (hpt_wavefront.hip): the pixels of a call are cut into groups, each with its own path pool, ray queue and
  // stream, so that the tail of one group's trace pass overlaps the other groups' work
  struct WfGroup
  {
    DevBuf<float4> f4[8], waves; DevBuf<uint2> fb; DevBuf<uint> u[9]; DevBuf<float> rec, lossSlot, time;
    hipStream_t stream = nullptr; hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; hipEvent_t done = nullptr;
    uint* progress = nullptr;            // pinned: rays queued after every WF_CHECK-th shade pass (0 = group finished)
    uint checkpoints = 0, itemBase = 0, itemCount = 0; unsigned long long it = 0; bool finished = false;
    WfGroup() = default; WfGroup(const WfGroup&) = delete;
    ~WfGroup()
    {
      if (progress) (void)hipHostFree(progress);
      for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
      if (done) (void)hipEventDestroy(done);
      if (stream) (void)hipStreamDestroy(stream);
    }
  };
  std::vector<WfGroup*> wfGroups;
  hipEvent_t wfFork = nullptr;
  int  wfGroupCount = 0;                 // 0 = automatic
  uint wfIterCap = 0;                    // diagnostic (hpt_set_option "dbg_wf_iter_cap"): rounds after which the wavefront loop gives up
  uint wfGrace = 16;                     // trips a trace wave keeps going after the queue ran dry before it suspends its rays (0 = never)
  // multi-GPU collectives (RCCL, loaded on first use: single-GPU users never touch it)
  void* rcclLib = nullptr; void* comm = nullptr; int commRanks = 0, commRank = 0;
  bool forceFull = false;                // diagnostic (hpt_set_option "force_full_materials")
  bool drSkipNonFinite = false;          // hpt_set_option "dr_skip_nonfinite": off = PixelLossPT as the reference has it
  bool drEnvironment = false;            // hpt_set_option "dr_environment": PathTraceDR / PathTraceVJP serve environment maps and their sampling (the ENV kernels)
  bool drGradMode = true;                // hpt_set_option "dr_grad_mode": IntegratorDR's m_gradMode, read by RayTraceDR only
  bool leanMaterials = false;            // every material is gltf or emissive: the kernels without the other BSDF branches are used
  int  schedule = 0;                     // 0 automatic, 1 megakernel, 2 wavefront, 3 megakernel with block-local ray repacking (hpt_set_schedule)
  int  bwWide = -1;                        // hpt_set_option("bw_wide"): -1 the 4-wide tree on heavy scenes only, 0 never, 1 whenever the scene has one
  uint bwRefillBelow = 48, bwNodeMin = 4;   // (profiles/bw_sweep.py: test_228 class, refill 32 .. 64 x vote 0 / 4 / 8 / 16)
  uint bwUnused = 0;   // hpt_block.hip: a wave refills when fewer lanes hold a ray; its node loop's vote
  int  nodeMinOverride = -1;             // env HPT_NODE_MIN (tuning): overrides the per-scene choice of DevScene::nodeMin
  uint wfRefillBelow = 56;               // a trace wave refills from the queue when fewer lanes than this still hold a ray
  int  wfBlocksPerCU = 0;
  size_t instTris = 0;                   // instanced triangles of the committed scene
  // CommitScene on the device (hpt_lbvh.hip): -1 = by CommitScene's options (BUILD_LOW / BUILD_MEDIUM without BUILD_HIGH), 0 = never, 1 = whenever the single-level layout is built
  int deviceBuildQuality = 0; float buildInfo[4] = { 0.0f, 0.0f, 0.0f, 0.0f };   // hpt_set_option("device_build_quality", passes); hpt_get_build_info: the last device build's treelet passes
  int deviceBuild = -1; void* lbvh = nullptr; unsigned long long geomVersion = 1, lbvhGeomVersion = 0; std::vector<size_t> lbvhPosOff, lbvhIdxOff;
  // the two-level layout built on the device (hpt_set_option("device_build_two_level", 1); hpt_lbvh.hip section 9): every mesh's slot in dNodes / dTris
  // and what the last batch left for it (host mirror); tlOnDevice: such a tree is committed; tlUpdatable: and nothing but instance matrices / vertex positions changed since - it is updated in place
  int deviceBuildTwoLevel = 0; bool tlOnDevice = false, tlUpdatable = false; std::vector<LbvhMeshSlot> tlSlots; std::vector<LbvhMeshOut> tlMeshOut;
  float tlInfo[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };          // hpt_get_two_level_info
  size_t tlNodes = 0, tlTris = 0;                        // entries of dNodes / dTris that belong to the committed two-level tree (hpt_read_accel_two_level)
  uint lastSchedule = 1, lastWfIters = 0;
  uint lastWide = 0, lastShadeRecords = 0, lastDeep = 0;          // what the last launch walked: 4-wide compressed tree, 64-byte shading records, HBM part of the stacks
  bool stackWitness = false; size_t witnessWords = 0;             // "dbg_stack_witness": dStackOvf is filled with STACK_SENTINEL before a launch; words the last launch's fill covered

  DevScene S;
  bool sceneUploaded = false, paramsSet = false;
  uint packedCount = 0;
  int  blocksPerCU = 0;
  int  accelLayout = 0;                  // 0 automatic (flat when it fits the budget), 1 force two-level, 2 force flat
  uint tidChunk = 0, tidStride = 1;      // hpt_set_tid_interleave
  bool instrument = false;
  uint64_t gradSize = 0;
  uint32_t diffLightFirst = 0, diffLightCount = 0;  // hpt_put_diff_lights: lights [first, first + count) own RGB gains at a_data[diffLightOff + 4 i]; count 0: none registered
  uint64_t diffLightOff = 0;

  float tSlots[T_SLOT_COUNT][4] = {};   // GetExecutionTime slots: kernel, copy in, copy out, overhead (ms) per TimeSlot
  float lastKernelMs = 0.0f;

  hpt_ctx() = default; hpt_ctx(const hpt_ctx&) = delete;
  ~hpt_ctx()                             // what the context owns that is not a DevBuf (hpt_destroy has set the device and waited for it)
  {
    lbvhDestroy(lbvh);
    for (WfGroup* g : wfGroups) delete g;
    for (void* p : texData) if (p) (void)hipFree(p);
    for (hipEvent_t e : { ev0, ev1, wfFork }) if (e) (void)hipEventDestroy(e);
    if (sliceError) (void)hipHostFree(sliceError);
  }
  int fail(int code, const std::string& m) { err = m; std::fprintf(stderr, "[hydra_hip] %s\n", m.c_str()); return code; }
  int hipFail(hipError_t e, const char* what) { return fail(HPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
};

#define HIPCHK(ctx, call) do { hipError_t _e = (call); if (_e != hipSuccess) return (ctx)->hipFail(_e, #call); } while (0)

// Nothing throws across the C boundary (include/hydra_hip.h): every extern "C" body is a function-try-block whose handler lands here. The host
// side builds std::vector / std::string / std::thread objects (scene tables, BVH build), so std::bad_alloc and std::system_error are real
// possibilities; they become an error code and a message for hpt_last_error like every other failure.
static int hptGuard(hpt_ctx* c, const char* where)
{
  int code = HPT_ERR_STATE; std::string what = "unknown exception";
  try { throw; }
  catch (const std::bad_alloc&) { code = HPT_ERR_NOMEM; what = "out of host memory (std::bad_alloc): sizes too large for this host"; }
  catch (const std::length_error& e) { code = HPT_ERR_NOMEM; what = std::string("container size limit exceeded (std::length_error): ") + e.what(); }
  catch (const std::exception& e) { what = e.what(); }
  catch (...) {}
  if (c) { try { return c->fail(code, std::string(where) + ": " + what); } catch (...) {} }
  return code;
}


// ---- lifetime -----------------------------------------------------------------------------------------------------------------
extern "C" int hpt_comm_destroy(hpt_ctx* c);

extern "C" int hpt_create(int device, hpt_ctx** out)
try {
  if (!out) return HPT_ERR_ARG;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) { std::fprintf(stderr, "[hydra_hip] no HIP device: %s\n", hipGetErrorString(e)); return HPT_ERR_HIP; }
  if (device < 0 || device >= n) return HPT_ERR_ARG;
  e = hipSetDevice(device);
  if (e != hipSuccess) return HPT_ERR_HIP;
  hpt_ctx* c = new hpt_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) { c->numCUs = prop.multiProcessorCount; c->devName = prop.gcnArchName; }
  (void)hipEventCreate(&c->ev0); (void)hipEventCreate(&c->ev1);
  if (const char* e = std::getenv("HPT_NODE_MIN")) c->nodeMinOverride = std::atoi(e) & 63;
  if (const char* e = std::getenv("HPT_WF_GRACE")) c->wfGrace = (uint)std::atoi(e);
  if (const char* e = std::getenv("HPT_PASS_SLICE")) c->passSlice = std::max(0, std::atoi(e));   // diagnostic, like the ones above: the slice sweep of profiles/r7_pass_slices.sh goes through bench.py, which sets no options
  if (const char* e = std::getenv("HPT_SHADE_RECORDS")) c->shadeTrisEnabled = std::atoi(e) != 0;
  if (const char* e = std::getenv("HPT_WIDE_NODES")) c->wideEnabled = std::atoi(e) != 0;   // (read before any scene is committed: CommitScene derives DevScene::megaWide from it)
  std::memset(&c->S, 0, sizeof(DevScene));
  c->S.rootRef = REF_NONE;
  *out = c;
  return HPT_OK;
}
catch (...) { return hptGuard(nullptr, "hpt_create"); }

extern "C" void hpt_destroy(hpt_ctx* c)
try {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  (void)hpt_comm_destroy(c);
  delete c;                                                    // (~hpt_ctx and its members free what the context owns)
}
catch (...) { (void)hptGuard(c, "hpt_destroy"); }

extern "C" const char* hpt_last_error(hpt_ctx* c) try { return c ? c->err.c_str() : "null context"; }
catch (...) { return ""; }

extern "C" int hpt_device_info(hpt_ctx* c, int* numCUs, int* wavefront, char* name, size_t nameLen)
try {
  if (!c) return HPT_ERR_ARG;
  if (numCUs) *numCUs = c->numCUs;
  if (wavefront) *wavefront = 64;
  if (name && nameLen) { std::strncpy(name, c->devName.c_str(), nameLen - 1); name[nameLen - 1] = 0; }
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_device_info"); }

// ---- the JPEG reader of the scene loaders (host only) ----------------------------------------------------------------------------------------
extern "C" int hpt_decode_jpeg(const uint8_t* file, uint64_t fileSize, uint32_t* outWidth, uint32_t* outHeight, uint8_t* outRGBA8, uint64_t outCapacity)
try {
  if (!file || !outWidth || !outHeight) return HPT_ERR_ARG;
  std::vector<uint8_t> rgba; std::string err; uint32_t w = 0, h = 0;
  try {                                                        // (nothing throws across the C boundary)
    std::vector<uint8_t> f(file, file + fileSize);
    if (!hydra_hip::jpeg::decode(f, w, h, rgba, err)) return HPT_ERR_UNSUPPORTED;
  } catch (const std::exception&) { return HPT_ERR_UNSUPPORTED; }
  *outWidth = w; *outHeight = h;
  if (!outRGBA8) return HPT_OK;                                // (a size query)
  if (outCapacity < rgba.size()) return HPT_ERR_ARG;
  std::memcpy(outRGBA8, rgba.data(), rgba.size());
  return HPT_OK;
}
catch (...) { return hptGuard(nullptr, "hpt_decode_jpeg"); }

// ---- precomputeThinFilmSpectral / precomputeThinFilmRGB for the scene loaders (host only, no device needed) ------------------------------------
extern "C" int hpt_film_precompute(const hpt_film_params* fp, float* outTable, uint64_t outCapacity, uint64_t* outCount, int* outPrecomputed)
try {
  if (!fp || !outCount) return HPT_ERR_ARG;
  hydra_hip::film::Params p;
  p.spectralMode = fp->spectralMode; p.extIOR = fp->extIOR; p.layers = fp->layers; p.eta = fp->eta; p.k = fp->k; p.etaSpecId = fp->etaSpecId; p.kSpecId = fp->kSpecId;
  p.thickness = fp->thickness; p.thicknessMap = fp->thicknessMap; p.thicknessMin = fp->thicknessMin; p.thicknessMax = fp->thicknessMax;
  p.specValues = fp->specValues; p.specOffsetSz = fp->specOffsetSz; p.numSpectra = fp->numSpectra; p.cieXYZ = fp->cieXYZ;
  if (p.layers < 1 || p.layers > hydra_hip::film::MAX_LAYERS) return HPT_ERR_ARG;
  if (p.specValues && !p.specOffsetSz) return HPT_ERR_ARG;
  const bool pre = hydra_hip::film::precomputed(p);
  if (outPrecomputed) *outPrecomputed = pre ? 1 : 0;
  *outCount = pre ? (uint64_t)hydra_hip::film::tableSize(p) : 0u;
  if (!pre || !outTable) return HPT_OK;                        // (a size query)
  if (outCapacity < *outCount) return HPT_ERR_ARG;
  try { return hydra_hip::film::precompute(p, outTable) ? HPT_OK : HPT_ERR_ARG; } catch (const std::exception&) { return HPT_ERR_ARG; }
}
catch (...) { return hptGuard(nullptr, "hpt_film_precompute"); }

// ---- mi::fresnel_coat_precompute for the scene loaders (host only, no device needed) --------------------------------------------------------
extern "C" int hpt_plastic_precompute(float alpha, float intIor, float extIor, const float* diffuse4, const float* specular4,
                                      float* outTransmittance64, float* outInternalReflectance, float* outSpecularSamplingWeight)
try {
  if (!diffuse4 || !specular4 || !outTransmittance64 || !outInternalReflectance || !outSpecularSamplingWeight) return HPT_ERR_ARG;
  if (!(alpha > 0.0f) || !(intIor > 0.0f) || !(extIor > 0.0f)) return HPT_ERR_ARG;
  const hydra_hip::plastic::CoatPrecomputed p = hydra_hip::plastic::fresnelCoatPrecompute(alpha, intIor, extIor, diffuse4, specular4);
  std::memcpy(outTransmittance64, p.transmittance, sizeof(p.transmittance));
  *outInternalReflectance = p.internalReflectance; *outSpecularSamplingWeight = p.specularSamplingWeight;
  return HPT_OK;
}
catch (...) { return hptGuard(nullptr, "hpt_plastic_precompute"); }

// ---- device memory for callers of the *_dev entry points that do not link the HIP runtime themselves ---------------------------------
extern "C" int hpt_device_malloc(hpt_ctx* c, size_t bytes, void** outDev)
try {
  if (!c || !outDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  *outDev = nullptr;
  HIPCHK(c, hipMalloc(outDev, bytes ? bytes : 4));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_device_malloc"); }
extern "C" int hpt_device_free(hpt_ctx* c, void* dev)
try {
  if (!c) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (dev) HIPCHK(c, hipFree(dev));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_device_free"); }
extern "C" int hpt_device_copy(hpt_ctx* c, void* dst, const void* src, size_t bytes, int kind)
try {
  if (!c || (bytes && (!dst || !src)) || kind < 1 || kind > 3) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  const hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (bytes) HIPCHK(c, hipMemcpy(dst, src, bytes, k));                      // synchronous: orders after the asynchronous *_dev launches on the null stream
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_device_copy"); }
extern "C" int hpt_device_memset(hpt_ctx* c, void* dev, int value, size_t bytes)
try {
  if (!c || (bytes && !dev)) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (bytes) HIPCHK(c, hipMemsetAsync(dev, value, bytes, nullptr));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_device_memset"); }

// ---- ISceneObject ---------------------------------------------------------------------------------------------------------------
extern "C" int hpt_clear_geom(hpt_ctx* c)
try {
  if (!c) return HPT_ERR_ARG;
  c->geoms.clear(); c->insts.clear(); c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; c->geomVersion++;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_clear_geom"); }

static int fill_geom(hpt_ctx* c, Geom& g, const float* vpos, size_t nVert, const uint32_t* idx, size_t nIdx, size_t stride)
{
  if (stride == 0) stride = sizeof(float) * 3;
  if (stride % sizeof(float) != 0) return c->fail(HPT_ERR_ARG, "AddGeom_Triangles3f: vByteStride must be a multiple of sizeof(float)");
  if (!vpos || !idx) return c->fail(HPT_ERR_ARG, "AddGeom_Triangles3f: nullptr input");
  const size_t fs = stride / sizeof(float);
  g.pos.resize(nVert * 3);
  for (size_t i = 0; i < nVert; i++) { g.pos[3 * i + 0] = vpos[fs * i + 0]; g.pos[3 * i + 1] = vpos[fs * i + 1]; g.pos[3 * i + 2] = vpos[fs * i + 2]; }
  g.idx.assign(idx, idx + (nIdx / 3) * 3);
  for (uint v : g.idx) if (v >= nVert) return c->fail(HPT_ERR_ARG, "AddGeom_Triangles3f: index out of range");
  g.dirty = true; c->geomVersion++;
  return HPT_OK;
}

extern "C" uint32_t hpt_add_geom_triangles3f(hpt_ctx* c, const float* vpos, size_t nVert, const uint32_t* idx, size_t nIdx, uint32_t, size_t stride)
try {
  if (!c) return 0xFFFFFFFFu;
  Geom g;
  if (fill_geom(c, g, vpos, nVert, idx, nIdx, stride) != HPT_OK) return 0xFFFFFFFFu;
  c->geoms.push_back(std::move(g));
  c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false;
  return (uint32_t)(c->geoms.size() - 1);
}
catch (...) { (void)hptGuard(c, "hpt_add_geom_triangles3f"); return 0xFFFFFFFFu; }

extern "C" int hpt_update_geom_triangles3f(hpt_ctx* c, uint32_t geomId, const float* vpos, size_t nVert, const uint32_t* idx, size_t nIdx, uint32_t, size_t stride)
try {
  if (!c) return HPT_ERR_ARG;
  if (geomId >= c->geoms.size()) return c->fail(HPT_ERR_ARG, "UpdateGeom_Triangles3f: bad geomId");
  Geom& g = c->geoms[geomId];
  if (nIdx > g.idx.size() || nVert * 3 > g.pos.size()) return c->fail(HPT_ERR_ARG, "UpdateGeom_Triangles3f: growing a geometry is not supported");
  c->accelCommitted = false;
  // the committed single-level tree survives a change of vertex POSITIONS (same triangles): its boxes are refitted on the device
  if ((nIdx / 3) * 3 != g.idx.size() || std::memcmp(idx, g.idx.data(), g.idx.size() * sizeof(uint32_t)) != 0) c->flatRefittable = c->tlUpdatable = false;
  else c->dirtyGeoms.push_back(geomId);
  return fill_geom(c, g, vpos, nVert, idx, nIdx, stride);
}
catch (...) { return hptGuard(c, "hpt_update_geom_triangles3f"); }

extern "C" int hpt_clear_scene(hpt_ctx* c) try { if (!c) return HPT_ERR_ARG; c->insts.clear(); c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; return HPT_OK; }
catch (...) { return hptGuard(c, "hpt_clear_scene"); }

extern "C" uint32_t hpt_add_instance(hpt_ctx* c, uint32_t geomId, const float m[16])
try {
  if (!c || !m || geomId >= c->geoms.size()) return 0xFFFFFFFFu;
  Inst in; in.geomId = geomId; std::memcpy(in.m, m, 64);
  c->insts.push_back(in);
  c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false;
  return (uint32_t)(c->insts.size() - 1);
}
catch (...) { (void)hptGuard(c, "hpt_add_instance"); return 0xFFFFFFFFu; }

extern "C" uint32_t hpt_add_instance_motion(hpt_ctx* c, uint32_t geomId, const float* matrices, uint32_t matrixNumber)
try {
  if (!c || !matrices || geomId >= c->geoms.size() || matrixNumber == 0) return 0xFFFFFFFFu;
  if (matrixNumber == 1) return hpt_add_instance(c, geomId, matrices);
  if (matrixNumber != 2) { c->fail(HPT_ERR_UNSUPPORTED, "AddInstanceMotion: two key matrices are supported (what LoadSceneInstances passes)"); return 0xFFFFFFFFu; }
  Inst in; in.geomId = geomId; std::memcpy(in.m, matrices, 64); std::memcpy(in.m1, matrices + 16, 64); in.motion = true;
  c->insts.push_back(in);
  c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false;
  return (uint32_t)(c->insts.size() - 1);
}
catch (...) { (void)hptGuard(c, "hpt_add_instance_motion"); return 0xFFFFFFFFu; }

extern "C" int hpt_update_instance(hpt_ctx* c, uint32_t instId, const float m[16])
try {
  if (!c || !m) return HPT_ERR_ARG;
  if (instId >= c->insts.size()) return HPT_OK;          // the reference silently ignores it (EmbreeRT.cpp:302-303)
  std::memcpy(c->insts[instId].m, m, 64);
  c->accelCommitted = false;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_update_instance"); }

// Expected inner-node visits of a random ray through the root box (the surface-area heuristic the builder minimises): 1 for the root plus
// area(child) / area(root) for every child that is an inner node. The number that tells a light scene from a heavy one better than the
// triangle count does (see useWavefront).
static float sah_node_visits(const Bvh2& t)
{
  const float a0 = t.bounds.halfArea();
  if (t.nodes.empty() || !(a0 > 0.0f)) return 0.0f;
  double v = 1.0;
  for (const BvhNode& n : t.nodes) for (int k = 0; k < 2; k++) {
    const uint ref = k ? n.ref1 : n.ref0;
    if (ref == REF_NONE || (ref & REF_LEAF)) continue;
    const float* q = n.q + 6 * k;
    const float dx = q[1] - q[0], dy = q[3] - q[2], dz = q[5] - q[4];
    if (dx >= 0.0f) v += double(dx * dy + dy * dz + dz * dx) / a0;
  }
  return (float)v;
}

// world -> object rows of an instance matrix (column-major 4x4, affine): cofactor inverse in double, rounded once
static void inverse_rows(const float* m, float row0[4], float row1[4], float row2[4])
{
  const double a00 = m[0], a01 = m[4], a02 = m[8],  tx = m[12];
  const double a10 = m[1], a11 = m[5], a12 = m[9],  ty = m[13];
  const double a20 = m[2], a21 = m[6], a22 = m[10], tz = m[14];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double id = 1.0 / det;
  const double i00 = c00 * id, i01 = (a02 * a21 - a01 * a22) * id, i02 = (a01 * a12 - a02 * a11) * id;
  const double i10 = c01 * id, i11 = (a00 * a22 - a02 * a20) * id, i12 = (a02 * a10 - a00 * a12) * id;
  const double i20 = c02 * id, i21 = (a01 * a20 - a00 * a21) * id, i22 = (a00 * a11 - a01 * a10) * id;
  row0[0] = (float)i00; row0[1] = (float)i01; row0[2] = (float)i02; row0[3] = (float)(-(i00 * tx + i01 * ty + i02 * tz));
  row1[0] = (float)i10; row1[1] = (float)i11; row1[2] = (float)i12; row1[3] = (float)(-(i10 * tx + i11 * ty + i12 * tz));
  row2[0] = (float)i20; row2[1] = (float)i21; row2[2] = (float)i22; row2[3] = (float)(-(i20 * tx + i21 * ty + i22 * tz));
}

static int ceil_log2(size_t v) { int l = 0; while ((size_t(1) << l) < v) l++; return l; }

// object -> world rows (3 x 4) of every instance, as refitTriBoxesKernel reads them
static void inst_o2w_rows(const std::vector<Inst>& insts, std::vector<float>& out)
{
  out.assign(12 * std::max<size_t>(insts.size(), 1), 0.0f);
  for (size_t i = 0; i < insts.size(); i++) {
    const float* m = insts[i].m; float* o = &out[12 * i];
    for (int r = 0; r < 3; r++) { o[4 * r + 0] = m[r]; o[4 * r + 1] = m[4 + r]; o[4 * r + 2] = m[8 + r]; o[4 * r + 3] = m[12 + r]; }
  }
}

// UpdateInstance / UpdateGeom_Triangles3f + CommitScene on a committed single-level scene (CrossRT.h:85-86, 134, 110): the tree's topology stays,
// its boxes are recomputed on the device (refitTriBoxesKernel + one refitLevelKernel per level, deepest first). The host only inverts the
// instance matrices again and, for meshes whose vertices moved, rewrites their triangle records.
// host threads for CommitScene (hpt_set_option("build_threads", n); default: the cores this process may use, at most 16)
static int buildThreads(const hpt_ctx* c)
{
  if (c->buildThreads > 0) return c->buildThreads;
  unsigned n = std::thread::hardware_concurrency();
  cpu_set_t set; CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int k = CPU_COUNT(&set); if (k > 0) n = std::min<unsigned>(n ? n : (unsigned)k, (unsigned)k); }
  return (int)std::min<unsigned>(std::max<unsigned>(n, 1u), 16u);
}

// contiguous chunks of [0, n) on `threads` host threads (fn(begin, end)); small ranges stay on the caller's thread
template <class F> static void parallelRanges(size_t n, int threads, F fn)
{
  if (threads <= 1 || n < 32768) { fn((size_t)0, n); return; }
  const size_t per = std::max<size_t>(n / (8 * (size_t)threads), 4096);       // chunks are handed out dynamically: a thread that could not be started costs nothing
  std::atomic<size_t> next(0);
  auto work = [&]() { for (size_t b = next.fetch_add(per); b < n; b = next.fetch_add(per)) fn(b, std::min(n, b + per)); };
  std::vector<std::thread> pool;
  try { for (int t = 1; t < threads; t++) pool.emplace_back(work); } catch (...) {}   // (no thread to be had: the caller's thread does the rest)
  work();
  for (std::thread& t : pool) t.join();
}

// Which layout a scene resolves to (hpt_set_accel_layout; the measurements behind the automatic choice stand in hpt_commit_scene): the single-level
// tree, or the two-level one - which tiny static scenes walk as a triangle sweep. A forced sweep with a moving instance is an error the caller reports.
static bool resolvesFlat(const hpt_ctx* c, size_t instTris, bool anyMotion)
{
  const bool autoFlat = !anyMotion && (instTris >= FLAT_AUTO_TRIS || c->insts.size() >= MANY_INSTANCES);
  return instTris <= FLAT_TRI_BUDGET && (c->accelLayout == 2 || (c->accelLayout == 0 && autoFlat));
}
static bool resolvesSweep(const hpt_ctx* c, size_t instTris, bool anyMotion)
{
  const size_t ni = c->insts.size();
  return !anyMotion && ni >= 1 && (c->accelLayout == 3 || (c->accelLayout == 0 && instTris <= SWEEP_MAX_TRIS && ni <= SWEEP_MAX_INSTS));
}

// ---- CommitScene on the device: hpt_lbvh.hip builds the single-level BVH2, its triangle records and the 4-wide compressed tree -------------
static int commit_flat_on_device(hpt_ctx* c, size_t instTris, double tBuild0)
{
  if (!c->lbvh) c->lbvh = lbvhCreate();
  std::string err;
  if (c->lbvhGeomVersion != c->geomVersion) {                 // the meshes' positions and indices: uploaded once, kept until a mesh changes
    std::vector<const float*> pos; std::vector<size_t> posN; std::vector<const uint*> idx; std::vector<size_t> idxN;
    for (const Geom& g : c->geoms) { pos.push_back(g.pos.data()); posN.push_back(g.pos.size()); idx.push_back(g.idx.data()); idxN.push_back(g.idx.size()); }
    if (!lbvhUploadGeometry(c->lbvh, pos, posN, idx, idxN, c->lbvhPosOff, c->lbvhIdxOff, err)) return c->fail(HPT_ERR_HIP, "CommitScene (device build): " + err);
    c->lbvhGeomVersion = c->geomVersion;
  }
  const size_t ni = c->insts.size();
  std::vector<LbvhInstance> li(ni);
  std::vector<BvhInst> dinst(std::max<size_t>(ni, 1));
  for (size_t i = 0; i < ni; i++) {
    const float* m = c->insts[i].m;
    for (int r = 0; r < 3; r++) { li[i].objectToWorld[4 * r + 0] = m[r]; li[i].objectToWorld[4 * r + 1] = m[4 + r]; li[i].objectToWorld[4 * r + 2] = m[8 + r]; li[i].objectToWorld[4 * r + 3] = m[12 + r]; }
    const uint g = c->insts[i].geomId;
    li[i].triCount = (uint)(c->geoms[g].idx.size() / 3); li[i].posOffset = c->lbvhPosOff[g]; li[i].idxOffset = c->lbvhIdxOff[g];
    inverse_rows(m, dinst[i].row0, dinst[i].row1, dinst[i].row2);
    dinst[i].root = REF_NONE; dinst[i].geomId = g; dinst[i].pad0 = 0u; dinst[i].pad1 = 0;
  }
  const uint n = (uint)instTris;
  HIPCHK(c, c->dNodes.alloc(std::max<size_t>(n, 1)));
  HIPCHK(c, c->dTris.alloc(std::max<size_t>(n, 1)));
  const bool wantWide = true;
  HIPCHK(c, c->dNodes4.alloc(std::max<size_t>(n, 1)));
  HIPCHK(c, c->dInsts.upload(dinst.data(), dinst.size()));
  LbvhRefitOut refit;                                        // "device_refit": the build groups its nodes by level and remembers where the 4-wide boxes come from
  if (c->deviceRefit) {
    HIPCHK(c, c->dLevelNodes.alloc(std::max<size_t>(n, 1)));
    HIPCHK(c, c->dNodes4Src.alloc(4 * c->dNodes4.n));
    HIPCHK(c, c->dTriBox.alloc(6 * std::max<size_t>(n, 1)));
    HIPCHK(c, c->dNodeBounds.alloc(6 * std::max<size_t>(n, 1)));
    refit.levelIds = c->dLevelNodes.p; refit.src4 = c->dNodes4Src.p;
  }
  {                                                          // (both layouts' kernels read the motion rows' pointer; none of these instances moves)
    std::vector<float> mo(24 * std::max<size_t>(ni, 1), 0.0f);
    for (size_t i = 0; i < ni; i++) for (int key = 0; key < 2; key++) for (int k = 0; k < 12; k++) mo[24 * i + 12 * (size_t)key + k] = li[i].objectToWorld[k];
    HIPCHK(c, c->dInstMotion.upload(mo.data(), mo.size()));
    c->S.instMotion = c->dInstMotion.p;
  }
  const double tDev0 = now_ms();
  LbvhResult r;
  if (!lbvhBuild(c->lbvh, li.data(), (uint)ni, n, c->dNodes.p, c->dTris.p, c->dNodes4.p, (uint)c->dNodes4.n, wantWide, refit, (uint)c->deviceBuildQuality, r, err)) return c->fail(HPT_ERR_HIP, "CommitScene (device build): " + err);
  const double tDev1 = now_ms();
  if (r.depth + 1u > MAX_STACK) return HPT_ERR_STATE;         // a degenerate input (the Morton curve cannot separate it): the host's depth-capped build takes over
  c->instTris = instTris; c->anyMotion = false;
  c->nodes4Count = 0; c->stackNeeded4 = 0; c->S.nodes4 = nullptr; c->S.root4 = REF_NONE; c->S.statsWide = 0; c->S.megaWide = 0;
  c->sahVisits = r.sahVisits;
  if (r.nodes4Count != 0u && (r.rootRef & REF_LEAF) == 0u) {
    c->nodes4Count = r.nodes4Count; c->stackNeeded4 = 3u * r.depth4 + 1u;
    c->S.nodes4 = c->dNodes4.p; c->S.root4 = 0u;
    c->S.megaWide = (c->wideEnabled && c->sahVisits >= HEAVY_SAH_VISITS) ? 1u : 0u;
  }
  // an update is answered by another device build unless "device_refit" had the build leave its level lists: then by refit_flat, like a host-built tree's
  c->flatTris.clear(); c->flatOnDevice = true; c->flatNodes = r.numNodes;
  c->levelOffsets.assign(1, 0u);
  for (uint l = 0; l < r.numLevels; l++) c->levelOffsets.push_back(c->levelOffsets.back() + r.levelCount[l]);
  c->flatRefittable = r.numLevels != 0u && (r.rootRef & REF_LEAF) == 0u && c->levelOffsets.back() <= c->dLevelNodes.n;
  c->S.nodes = c->dNodes.p; c->S.tris = c->dTris.p; c->S.insts = c->dInsts.p;
  c->S.rootRef = r.rootRef; c->S.numInsts = (uint)ni; c->S.flatMode = 1; c->S.sweep = 0; c->S.sweepInsts = nullptr; c->S.sweepTris = nullptr;
  c->S.nodeMin = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 16u : 0u);
  c->S.nodeMin4 = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 32u : 0u);
  c->stackNeeded = r.depth + 1u;
  c->buildInfo[0] = (float)r.passesRun; c->buildInfo[1] = (float)r.treeletsExamined; c->buildInfo[2] = (float)r.treeletsRewritten; c->buildInfo[3] = r.passMs;
  if (std::getenv("HPT_DEBUG_ACCEL")) std::fprintf(stderr, "[hydra_hip] device-built single-level BVH: %zu triangles, depth %u, sah visits %.2f; 4-wide: %u nodes, depth %u; %.2f ms of kernels; treelet passes %u (%u of %u treelets rewritten, %.2f ms)\n",
                                                  instTris, r.depth, c->sahVisits, r.nodes4Count, r.depth4, tDev1 - tDev0, r.passesRun, r.treeletsRewritten, r.treeletsExamined, r.passMs);
  c->tCommit[0] = float(tDev0 - tBuild0); c->tCommit[1] = 0.0f; c->tCommit[2] = float(tDev1 - tDev0); c->tCommit[3] = 2.0f;   // host preparation + uploads, -, device build, "built on the device"
  c->accelCommitted = true; c->shadeTrisDirty = true;
  return HPT_OK;
}

// ---- CommitScene on the device, two-level layout (hpt_set_option("device_build_two_level", 1)): one BLAS per mesh in a fixed slot of dNodes / dTris,
// all dirty ones built in one batch (hpt_lbvh.hip section 9), the TLAS over the live instances at the front of dNodes. update: the committed tree is
// such a tree and only instance matrices / vertex positions of the meshes in `moved` changed since - those BLAS are built again in their slots
// (none: nothing but the TLAS kernels runs) and the rest of both arrays stays byte for byte. Returns HPT_ERR_STATE when the host's builder must
// take the whole commit (deeper than the traversal stack, past the reference widths).
static int commit_two_level_on_device(hpt_ctx* c, size_t instTris, bool update, const std::vector<uint>& moved, double tBuild0)
{
  if (!c->lbvh) c->lbvh = lbvhCreate();
  std::string err;
  const size_t ng = c->geoms.size(), ni = c->insts.size();
  update = update && c->tlSlots.size() == ng && c->tlMeshOut.size() == ng && c->lbvhPosOff.size() == ng;
  std::vector<uint> dirty;
  if (!update) {
    c->tlSlots.assign(ng, LbvhMeshSlot());
    size_t nodeBase = std::max<size_t>(ni, 1), triBase = 0;   // the TLAS' nodes lie in front: ni - 1 at the most
    for (size_t g = 0; g < ng; g++) {
      const size_t nt = c->geoms[g].idx.size() / 3;
      if (nodeBase >= (size_t(1) << 31) || triBase >= (size_t(1) << 28)) return HPT_ERR_STATE;
      c->tlSlots[g].nodeBase = (uint)nodeBase; c->tlSlots[g].triBase = (uint)triBase; c->tlSlots[g].nt = (uint)nt;
      nodeBase += nt > 1 ? nt - 1 : 0; triBase += nt;
      if (nt) dirty.push_back((uint)g);
    }
    if (nodeBase >= (size_t(1) << 31) || triBase >= (size_t(1) << 28)) return HPT_ERR_STATE;
    if (c->lbvhGeomVersion != c->geomVersion) {               // the meshes' positions and indices: uploaded once, kept until a mesh changes
      std::vector<const float*> pos; std::vector<size_t> posN; std::vector<const uint*> idx; std::vector<size_t> idxN;
      for (const Geom& g : c->geoms) { pos.push_back(g.pos.data()); posN.push_back(g.pos.size()); idx.push_back(g.idx.data()); idxN.push_back(g.idx.size()); }
      if (!lbvhUploadGeometry(c->lbvh, pos, posN, idx, idxN, c->lbvhPosOff, c->lbvhIdxOff, err)) return c->fail(HPT_ERR_HIP, "CommitScene (device build, two-level): " + err);
      c->lbvhGeomVersion = c->geomVersion;
    }
    for (size_t g = 0; g < ng; g++) {
      if ((c->lbvhPosOff[g] >> 32) != 0 || (c->lbvhIdxOff[g] >> 32) != 0) return HPT_ERR_STATE;
      c->tlSlots[g].posOff = (uint)c->lbvhPosOff[g]; c->tlSlots[g].idxOff = (uint)c->lbvhIdxOff[g];
    }
    c->tlMeshOut.assign(ng, LbvhMeshOut());
    for (LbvhMeshOut& o : c->tlMeshOut) lbvhMeshOutReset(o);
    c->tlNodes = nodeBase; c->tlTris = triBase;
    HIPCHK(c, c->dNodes.alloc(nodeBase));
    HIPCHK(c, c->dTris.alloc(std::max<size_t>(triBase, 1)));
    // (unused entries - the TLAS region past its nodes, the slots of folded subtrees - read back as zeros, not as whatever the allocation held)
    HIPCHK(c, hipMemsetAsync(c->dNodes.p, 0, nodeBase * sizeof(BvhNode), nullptr));
    HIPCHK(c, hipMemsetAsync(c->dTris.p, 0, std::max<size_t>(triBase, 1) * sizeof(BvhTri), nullptr));
  } else {
    std::vector<char> seen(ng, 0);
    std::vector<const float*> pos; std::vector<size_t> posN;
    for (const Geom& g : c->geoms) { pos.push_back(g.pos.data()); posN.push_back(g.pos.size()); }
    for (uint g : moved) if (g < ng && !seen[g] && c->tlSlots[g].nt != 0u) { seen[g] = 1; dirty.push_back(g); lbvhMeshOutReset(c->tlMeshOut[g]); }
    if (!dirty.empty() && !lbvhCopyPositions(c->lbvh, dirty, pos, posN, c->lbvhPosOff, err)) return c->fail(HPT_ERR_HIP, "CommitScene (device build, two-level): " + err);
    c->lbvhGeomVersion = c->geomVersion;                      // (an updatable tree: nothing but these positions changed since the geometry was uploaded)
  }
  const double tDev0 = now_ms();
  float blasMs = 0.0f, tlasMs = 0.0f;
  if (!dirty.empty() && !lbvhBuildBlasBatch(c->lbvh, c->tlSlots.data(), (uint)ng, dirty.data(), (uint)dirty.size(), c->tlMeshOut.data(), c->dNodes.p, c->dTris.p, blasMs, err))
    return c->fail(HPT_ERR_HIP, "CommitScene (device build, two-level): " + err);
  const double tDev1 = now_ms();
  uint maxBlasDepth = 0;
  for (const LbvhMeshOut& o : c->tlMeshOut) maxBlasDepth = std::max(maxBlasDepth, o.depth);
  if (maxBlasDepth + 2u > MAX_STACK) return HPT_ERR_STATE;
  // instance records: the inverse rows decide hits and stay the host's (double, rounded once); the root is the mesh's patched BLAS root
  std::vector<BvhInst> dinst(std::max<size_t>(ni, 1));
  std::vector<uint> instGeom(std::max<size_t>(ni, 1), 0u);
  std::vector<float> mo(24 * std::max<size_t>(ni, 1), 0.0f);
  uint nLive = 0, firstLive = 0; bool anyMotion = false;
  for (size_t i = 0; i < ni; i++) {
    const Inst& in = c->insts[i];
    inverse_rows(in.m, dinst[i].row0, dinst[i].row1, dinst[i].row2);
    dinst[i].root = c->tlMeshOut[in.geomId].root; dinst[i].geomId = in.geomId; dinst[i].pad0 = in.motion ? 1u : 0u; dinst[i].pad1 = 0;
    instGeom[i] = in.geomId; anyMotion = anyMotion || in.motion;
    if (dinst[i].root != REF_NONE) { if (nLive == 0u) firstLive = (uint)i; nLive++; }
    for (int key = 0; key < 2; key++) {
      const float* m = (key && in.motion) ? in.m1 : in.m;
      float* o = &mo[24 * i + 12 * (size_t)key];
      for (int r = 0; r < 3; r++) { o[4 * r + 0] = m[r]; o[4 * r + 1] = m[4 + r]; o[4 * r + 2] = m[8 + r]; o[4 * r + 3] = m[12 + r]; }
    }
  }
  HIPCHK(c, c->dInstMotion.upload(mo.data(), mo.size()));
  HIPCHK(c, c->dInsts.upload(dinst.data(), dinst.size()));
  const double tDev2 = now_ms();
  LbvhTlasResult r;
  if (!lbvhBuildTlas(c->lbvh, instGeom.data(), (uint)ni, nLive, firstLive, c->dInstMotion.p, c->tlMeshOut.data(), (uint)ng, c->dNodes.p, r, tlasMs, err))
    return c->fail(HPT_ERR_HIP, "CommitScene (device build, two-level): " + err);
  const double tDev3 = now_ms();
  if (r.depth + 1u + maxBlasDepth + 1u > MAX_STACK) return HPT_ERR_STATE;
  c->instTris = instTris; c->anyMotion = anyMotion;
  c->sahVisits = r.sahVisits;
  c->S.instMotion = c->dInstMotion.p;
  c->S.nodes = c->dNodes.p; c->S.tris = c->dTris.p; c->S.insts = c->dInsts.p;
  c->S.rootRef = r.rootRef; c->S.numInsts = (uint)ni; c->S.flatMode = 0;
  c->S.sweep = 0; c->S.sweepInsts = nullptr; c->S.sweepTris = nullptr; c->S.sweepBoxes = nullptr; c->S.sweepPlanes = nullptr; c->S.sweepCull = 0u; c->S.sweepPairBoxes = nullptr; c->S.sweepLanes = 0u;
  c->S.nodeMin = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 16u : 0u);
  c->nodes4Count = 0; c->stackNeeded4 = 0; c->S.nodes4 = nullptr; c->S.root4 = REF_NONE; c->S.statsWide = 0; c->S.megaWide = 0; c->S.nodeMin4 = 0;
  c->flatOnDevice = false; c->flatNodes = 0; c->levelOffsets.assign(1, 0u); c->flatTris.clear();
  c->tlOnDevice = true; c->tlUpdatable = true; c->flatRefittable = false;   // the next commit may update this tree in place
  c->stackNeeded = r.depth + 1u + maxBlasDepth + 1u;
  const uint kept = (uint)std::count_if(c->tlSlots.begin(), c->tlSlots.end(), [](const LbvhMeshSlot& s) { return s.nt != 0u; }) - (uint)dirty.size();
  c->tlInfo[0] = 1.0f; c->tlInfo[1] = (float)dirty.size(); c->tlInfo[2] = (float)kept; c->tlInfo[3] = (update && dirty.empty()) ? 1.0f : 0.0f;
  c->tlInfo[4] = (float)r.depth; c->tlInfo[5] = (float)maxBlasDepth; c->tlInfo[6] = blasMs; c->tlInfo[7] = tlasMs;
  if (std::getenv("HPT_DEBUG_ACCEL")) std::fprintf(stderr, "[hydra_hip] device-built two-level BVH: %zu instances (%u live), %zu BLAS built, %u kept, TLAS depth %u, deepest BLAS %u, stack %u, sah visits %.2f; BLAS %.3f ms, TLAS %.3f ms\n",
                                                  ni, nLive, dirty.size(), kept, r.depth, maxBlasDepth, c->stackNeeded, c->sahVisits, blasMs, tlasMs);
  // host preparation + uploads, -, device build (both stages with their read-backs), "built on the device"
  c->tCommit[0] = float((tDev0 - tBuild0) + (tDev2 - tDev1)); c->tCommit[1] = 0.0f; c->tCommit[2] = float((tDev1 - tDev0) + (tDev3 - tDev2)); c->tCommit[3] = 2.0f;
  c->accelCommitted = true; c->shadeTrisDirty = true;
  return HPT_OK;
}

static const int HPT_REFIT_REJECTED = -1;                    // refit_flat: the refitted tree's estimate is over "refit_max_sah_pct"; hpt_commit_scene builds instead

// One body for both trees. They differ in where the moved vertices' records are rewritten: a host-built tree has a host copy of its records
// (flatTris) that is patched and uploaded whole, a device-built tree has none - its meshes' positions are copied to the builder's device copy
// (the changed meshes only) and a kernel rewrites the records in place (lbvhUpdatePositions).
static int refit_flat(hpt_ctx* c)
{
  const double t0 = now_ms();
  const size_t ni = c->insts.size();
  std::vector<BvhInst> dinst(std::max<size_t>(ni, 1));
  for (size_t i = 0; i < ni; i++) {
    inverse_rows(c->insts[i].m, dinst[i].row0, dinst[i].row1, dinst[i].row2);
    dinst[i].root = REF_NONE; dinst[i].geomId = c->insts[i].geomId; dinst[i].pad0 = dinst[i].pad1 = 0;
  }
  std::vector<float> o2w; inst_o2w_rows(c->insts, o2w);
  std::vector<char> dirty(c->geoms.size(), 0);
  for (uint g : c->dirtyGeoms) if (g < dirty.size()) dirty[g] = 1;
  if (!c->dirtyGeoms.empty() && !c->flatOnDevice) {             // moved vertices: the object-space records (v0, e1, e2) of those meshes' triangles
    for (BvhTri& t : c->flatTris) {
      const uint gi = c->insts[t.instId].geomId;
      if (!dirty[gi]) continue;
      const Geom& g = c->geoms[gi];
      const float* A = &g.pos[3 * g.idx[3 * t.primId + 0]]; const float* B = &g.pos[3 * g.idx[3 * t.primId + 1]]; const float* C = &g.pos[3 * g.idx[3 * t.primId + 2]];
      for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = C[a] - A[a]; }
    }
  }
  for (uint g : c->dirtyGeoms) if (g < c->geoms.size()) c->geoms[g].dirty = true;   // a later two-level build must redo these BLAS
  const double t1 = now_ms();
  HIPCHK(c, c->dInsts.upload(dinst.data(), dinst.size()));
  HIPCHK(c, c->dInstO2W.upload(o2w.data(), o2w.size()));
  if (!c->dirtyGeoms.empty() && !c->flatOnDevice) HIPCHK(c, c->dTris.upload(c->flatTris.data(), c->flatTris.size()));
  if (!c->dirtyGeoms.empty() && c->flatOnDevice) {
    std::vector<uint> moved; std::vector<const float*> pos; std::vector<size_t> posN; std::vector<unsigned char> instDirty(std::max<size_t>(ni, 1), 0);
    for (size_t g = 0; g < c->geoms.size(); g++) { pos.push_back(c->geoms[g].pos.data()); posN.push_back(c->geoms[g].pos.size()); if (dirty[g]) moved.push_back((uint)g); }
    for (size_t i = 0; i < ni; i++) instDirty[i] = dirty[c->insts[i].geomId] ? 1 : 0;
    std::string err;
    if (!lbvhUpdatePositions(c->lbvh, moved, pos, posN, c->lbvhPosOff, instDirty.data(), (uint)ni, (uint)c->instTris, c->dTris.p, err)) return c->fail(HPT_ERR_HIP, "CommitScene (device refit): " + err);
    c->lbvhGeomVersion = c->geomVersion;                        // (a refittable tree: nothing but these positions changed since the geometry was uploaded)
  }
  c->dirtyGeoms.clear();
  const double t2 = now_ms();
  const uint nt = (uint)c->instTris;
  if (nt) refitTriBoxesKernel<<<dim3((nt + 255u) / 256u), dim3(256), 0, 0>>>(c->dTris.p, c->dInstO2W.p, nt, c->dTriBox.p);
  for (size_t l = c->levelOffsets.size() - 1; l-- > 0;) {
    const uint cnt = c->levelOffsets[l + 1] - c->levelOffsets[l];
    if (cnt) refitLevelKernel<<<dim3((cnt + 255u) / 256u), dim3(256), 0, 0>>>(c->dNodes.p, c->dLevelNodes.p + c->levelOffsets[l], cnt, c->dTriBox.p, c->dNodeBounds.p);
  }
  if (c->nodes4Count) refitNodes4Kernel<<<dim3((c->nodes4Count + 255u) / 256u), dim3(256), 0, 0>>>(c->dNodes4.p, c->dNodes4Src.p, c->dNodes.p, c->nodes4Count);
  // the refitted tree's cost (hpt_get_refit_info): reported and, under "refit_max_sah_pct", compared; the schedule keeps following the build's estimate
  const uint nn = c->levelOffsets.back();
  HIPCHK(c, c->dRefitSah.alloc(2));
  HIPCHK(c, hipMemsetAsync(c->dRefitSah.p, 0, 2 * sizeof(double), 0));
  if (nn) refitSahKernel<<<dim3((nn + 255u) / 256u), dim3(256), 0, 0>>>(c->dNodes.p, c->dLevelNodes.p, nn, c->S.rootRef, c->dRefitSah.p);
  HIPCHK(c, hipGetLastError());
  double sah[2] = { 0.0, 0.0 };
  HIPCHK(c, hipMemcpy(sah, c->dRefitSah.p, sizeof(sah), hipMemcpyDeviceToHost));
  HIPCHK(c, hipDeviceSynchronize());
  c->S.insts = c->dInsts.p;
  c->sahRefit = sah[1] > 0.0 ? (float)(1.0 + sah[0] / sah[1]) : 0.0f;
  if (c->refitMaxSahPct > 0 && (double)c->sahRefit * 100.0 > (double)c->refitMaxSahPct * (double)c->sahVisits) { c->refitRejected = true; return HPT_REFIT_REJECTED; }
  c->tCommit[0] = float(t1 - t0); c->tCommit[1] = float(t2 - t1); c->tCommit[2] = float(now_ms() - t2); c->tCommit[3] = 1.0f;
  c->accelCommitted = true; c->shadeTrisDirty = true;
  return HPT_OK;
}

extern "C" int hpt_commit_scene(hpt_ctx* c, uint32_t options)
try {
  if (!c) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  c->refitRejected = false;
  for (float& v : c->buildInfo) v = 0.0f;                     // (a device build that is kept fills it in)
  for (float& v : c->tlInfo) v = 0.0f;
  const bool tlUpdate = c->tlOnDevice && c->tlUpdatable && c->refitEnabled;   // a device-built two-level tree that only saw UpdateInstance / same-index UpdateGeom
  c->tlOnDevice = false; c->tlUpdatable = false;
  const std::vector<uint> movedGeoms(c->dirtyGeoms);
  int onDevice = -1;                                         // 1 / 0: a rejected refit is followed by a build of the kind the tree came from
  if (c->flatRefittable && c->refitEnabled && c->S.flatMode == 1u && (!c->flatOnDevice || c->deviceRefit)) {
    const int rc = refit_flat(c);
    if (rc != HPT_REFIT_REJECTED) return rc;
    onDevice = c->flatOnDevice ? 1 : 0;
  }
  const double tBuild0 = now_ms();
  c->dirtyGeoms.clear();
  {
    // CommitScene(BUILD_LOW | BUILD_MEDIUM) (CrossRT.h:8-14) or hpt_set_option("device_build", 1): the single-level tree is built by kernels
    // (hpt_lbvh.hip: a few ms for 1 M triangles against a quarter of a second on the host; a linear BVH, coarser than the SAH tree)
    size_t nTris = 0; bool moving = false;
    for (const Inst& in : c->insts) { nTris += c->geoms[in.geomId].idx.size() / 3; moving = moving || in.motion; }
    const bool wantFlat = nTris <= FLAT_TRI_BUDGET && nTris < (size_t(1) << 28) && !moving &&
                          (c->accelLayout == 2 || (c->accelLayout == 0 && (nTris >= FLAT_AUTO_TRIS || c->insts.size() >= MANY_INSTANCES)));
    const bool fast = (options & 3u) != 0u && (options & 4u) == 0u;
    if (wantFlat && nTris > 0 && (onDevice == 1 || (onDevice < 0 && (c->deviceBuild == 1 || (c->deviceBuild < 0 && fast))))) {
      const int rc = commit_flat_on_device(c, nTris, tBuild0);
      if (rc != HPT_ERR_STATE) return rc;                    // (HPT_ERR_STATE: the tree came out deeper than the traversal stack - the host's depth-capped build takes over)
    }
    // "device_build_two_level": the same request on a scene that resolves to the two-level layout (the rules further down) and is no triangle sweep
    // (a forced sweep never is: with a moving instance it is the host path's error)
    if (c->deviceBuildTwoLevel == 1 && c->accelLayout != 3 && !resolvesFlat(c, nTris, moving) && !resolvesSweep(c, nTris, moving) && nTris > 0 && onDevice < 0 && (c->deviceBuild == 1 || (c->deviceBuild < 0 && fast))) {
      const int rc = commit_two_level_on_device(c, nTris, tlUpdate, movedGeoms, tBuild0);
      if (rc != HPT_ERR_STATE) return rc;                    // (HPT_ERR_STATE: deeper than the traversal stack, or past the reference widths - the whole commit goes to the host's builder)
    }
  }
  // ---- bottom level: one BVH2 per mesh over object-space triangles ----
  uint maxBlasDepth = 0;
  const int nThreads = buildThreads(c);
  // meshes are independent: the dirty ones are built by a pool of host threads (a mesh's own build stays sequential; a single big mesh - and
  // the single-level tree below - is split into subtrees instead, Bvh2Builder::build)
  std::vector<size_t> todo;
  size_t biggest = 0;
  for (size_t gi = 0; gi < c->geoms.size(); gi++) if (c->geoms[gi].dirty) { todo.push_back(gi); biggest = std::max(biggest, c->geoms[gi].idx.size() / 3); }
  const bool meshParallel = nThreads > 1 && todo.size() >= 4;
  auto buildMesh = [&](Geom& g, int threadsInside) {
    const size_t nt = g.idx.size() / 3;
    std::vector<Aabb> boxes(nt);
    for (size_t t = 0; t < nt; t++) {
      boxes[t].reset();
      for (int k = 0; k < 3; k++) boxes[t].grow(&g.pos[3 * g.idx[3 * t + k]]);
    }
    const int depthCap = std::max(24, ceil_log2((nt + BVH_LEAF_MAX - 1) / BVH_LEAF_MAX) + 2);
    g.bvh = Bvh2Builder::build(boxes, BVH_LEAF_MAX, depthCap, false, threadsInside);
    g.tris.resize(nt);
    for (size_t i = 0; i < nt; i++) {
      const uint p = g.bvh.order[i];
      const float* A = &g.pos[3 * g.idx[3 * p + 0]]; const float* B = &g.pos[3 * g.idx[3 * p + 1]]; const float* C = &g.pos[3 * g.idx[3 * p + 2]];
      BvhTri& t = g.tris[i];
      for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = C[a] - A[a]; }
      t.primId = p; t.instId = 0; t.pad1 = 0;
    }
    g.dirty = false;
  };
  if (meshParallel) {
    std::atomic<size_t> next(0);
    auto work = [&]() { for (size_t k = next.fetch_add(1); k < todo.size(); k = next.fetch_add(1)) buildMesh(c->geoms[todo[k]], 1); };
    std::vector<std::thread> pool;
    try { for (int t = 1; t < nThreads; t++) pool.emplace_back(work); } catch (...) {}
    work();
    for (std::thread& t : pool) t.join();
  } else for (size_t gi : todo) buildMesh(c->geoms[gi], nThreads);
  for (const Geom& g : c->geoms) maxBlasDepth = std::max(maxBlasDepth, g.bvh.depth);
  // ---- single-level layout: one BVH2 over all instanced triangles, world-space boxes, object-space triangle records ----
  size_t instTris = 0;
  for (const Inst& in : c->insts) instTris += c->geoms[in.geomId].idx.size() / 3;
  c->instTris = instTris;
  // Automatic choice, measured: heavy static scenes (wavefront schedule) gain 8 % from the single-level layout (1M triangles: 191 -> 207
  // Mpaths/s; no instance enter / leave trips, triangle-loop lane utilisation 0.21 -> 0.38); the Cornell-box class on the megakernel loses
  // 8 % to it (looser world-space boxes around rotated instances, per-triangle ray transform) and keeps the two-level TLAS/BLAS layout.
  // Scenes of many small instances (the own fixtures: 6 ... 16 transformed spheres on a floor) also gain from it on the megakernel:
  // typed_materials 1031 -> 1127, legacy_materials 1574 -> 1752, env_map 1526 -> 1670 Mpaths/s (profiles/ab_layout.sh), the instance
  // enter / leave trips outweigh the looser boxes once a ray meets several overlapping BLAS boxes.
  // ... and so does the 8 202-triangle test_228 with its 3 instances (megakernel: two-level 617, single-level 667 Mpaths/s).
  // Scenes with moving instances keep the two-level layout unless told otherwise: there the ray is taken to the instance's space at the
  // path's time once per instance visit, under the single-level layout once per triangle record (legacy_materials, one moving sphere of
  // ten instances: two-level 1797, single-level 1065 Mpaths/s - profiles/ab_layout_full.sh).
  c->anyMotion = false;
  for (const Inst& in : c->insts) c->anyMotion = c->anyMotion || in.motion;
  const bool flat = resolvesFlat(c, instTris, c->anyMotion);
  {                                                          // object->world rows (3x4) at both keys for the moving instances (both layouts read them)
    const size_t nim = c->insts.size();
    std::vector<float> mo(24 * std::max<size_t>(nim, 1), 0.0f);
    for (size_t i = 0; i < nim; i++) for (int key = 0; key < 2; key++) {
      const float* m = (key && c->insts[i].motion) ? c->insts[i].m1 : c->insts[i].m;
      float* o = &mo[24 * i + 12 * (size_t)key];
      for (int r = 0; r < 3; r++) { o[4 * r + 0] = m[r]; o[4 * r + 1] = m[4 + r]; o[4 * r + 2] = m[8 + r]; o[4 * r + 3] = m[12 + r]; }
    }
    HIPCHK(c, c->dInstMotion.upload(mo.data(), mo.size()));
    c->S.instMotion = c->dInstMotion.p;
  }
  if (flat) {
    const size_t ni = c->insts.size();
    std::vector<Aabb> boxes(instTris);
    std::vector<uint> triInst(instTris), triPrim(instTris);
    {
      size_t k = 0;
      for (size_t i = 0; i < ni; i++) { const size_t nt = c->geoms[c->insts[i].geomId].idx.size() / 3; for (size_t t = 0; t < nt; t++, k++) { triInst[k] = (uint)i; triPrim[k] = (uint)t; } }
    }
    parallelRanges(instTris, nThreads, [&](size_t kb, size_t ke) {
      for (size_t k = kb; k < ke; k++) {
        const size_t i = triInst[k], t = triPrim[k];
        const Geom& g = c->geoms[c->insts[i].geomId];
        Aabb b; b.reset();
        // a moving instance: every point travels on the segment between its two key positions, so the box over both keys bounds the triangle at any time
        for (int key = 0; key < (c->insts[i].motion ? 2 : 1); key++) {
          const float* m = key ? c->insts[i].m1 : c->insts[i].m;
          for (int kk = 0; kk < 3; kk++) {
            const float* p = &g.pos[3 * g.idx[3 * t + kk]];
            const float q[3] = { m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12], m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13], m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14] };
            b.grow(q);
          }
        }
        b.pad();                                            // covers the rounding of the world-space vertex positions too
        boxes[k] = b;
      }
    });
    const int depthCap = std::max(24, ceil_log2((instTris + BVH_LEAF_MAX - 1) / BVH_LEAF_MAX) + 2);
    Bvh2 tree = Bvh2Builder::build(boxes, BVH_LEAF_MAX, depthCap, false, nThreads);
    std::vector<BvhTri> tris(std::max<size_t>(instTris, 1));
    parallelRanges(instTris, nThreads, [&](size_t kb, size_t ke) {
      for (size_t k = kb; k < ke; k++) {
        const uint src = tree.order[k];
        const uint i = triInst[src], p = triPrim[src];
        const Geom& g = c->geoms[c->insts[i].geomId];
        const float* A = &g.pos[3 * g.idx[3 * p + 0]]; const float* B = &g.pos[3 * g.idx[3 * p + 1]]; const float* C = &g.pos[3 * g.idx[3 * p + 2]];
        BvhTri& t = tris[k];
        for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = C[a] - A[a]; }   // same object-space record as the two-level path
        t.primId = p; t.instId = i; t.pad1 = 0;
      }
    });
    std::vector<BvhNode> nodes(tree.nodes);
    if (nodes.empty()) nodes.push_back(BvhNode());
    if (tris.size() >= (size_t(1) << 28)) return c->fail(HPT_ERR_UNSUPPORTED, "CommitScene: scene too large for 28-bit triangle references");
    std::vector<BvhInst> dinst(std::max<size_t>(ni, 1));
    for (size_t i = 0; i < ni; i++) {
      inverse_rows(c->insts[i].m, dinst[i].row0, dinst[i].row1, dinst[i].row2);
      dinst[i].root = REF_NONE; dinst[i].geomId = c->insts[i].geomId; dinst[i].pad0 = c->insts[i].motion ? 1u : 0u; dinst[i].pad1 = 0;
    }
    const double tUp0 = now_ms();
    HIPCHK(c, c->dNodes.upload(nodes.data(), nodes.size()));
    HIPCHK(c, c->dTris.upload(tris.data(), tris.size()));
    HIPCHK(c, c->dInsts.upload(dinst.data(), dinst.size()));
    // ---- the same tree as 4-wide compressed nodes (BvhNode4, hpt_types.h) for the heavy-scene trace kernel ----
    // Collapse: a node adopts its grandchildren, largest surface first, until it has four children or only leaves are left. Child boxes are
    // the (padded) BVH2 child boxes, quantised outwards in the node's frame; `src` remembers where each box lives so that a refit can requantise.
    c->nodes4Count = 0; c->stackNeeded4 = 0; c->S.nodes4 = nullptr; c->S.root4 = REF_NONE; c->S.statsWide = 0; c->S.megaWide = 0;
    double collapseMs = 0.0;
    if (tree.rootRef != REF_NONE && !(tree.rootRef & REF_LEAF) && !c->anyMotion) {
      const double tC0 = now_ms();
      std::vector<BvhNode4> n4; std::vector<uint> src4;
      uint depth4 = 1;
      collapseToWide(tree, n4, src4, depth4);
      collapseMs = now_ms() - tC0;
      if (n4.size() < (size_t(1) << 31)) {
        HIPCHK(c, c->dNodes4.upload(n4.data(), n4.size()));
        HIPCHK(c, c->dNodes4Src.upload(src4.data(), src4.size()));
        c->nodes4Count = (uint)n4.size(); c->stackNeeded4 = 3u * depth4 + 1u;       // a visit leaves at most three children waiting
        c->S.nodes4 = c->dNodes4.p; c->S.root4 = 0u;
        c->S.megaWide = (c->wideEnabled && sah_node_visits(tree) >= HEAVY_SAH_VISITS) ? 1u : 0u;   // heavy scenes rendered by the megakernel (calls below the wavefront's pixel threshold) walk it too
        if (std::getenv("HPT_DEBUG_ACCEL")) std::fprintf(stderr, "[hydra_hip] 4-wide tree: %zu nodes (BVH2: %zu), depth %u, stack bound %u\n", n4.size(), tree.nodes.size(), depth4, c->stackNeeded4);
      }
    }
    {                                                          // what refit_flat needs: the nodes grouped by level, scratch for the boxes
      std::vector<uint> level(tree.nodes.size(), 0u), order; order.reserve(tree.nodes.size());
      uint maxLevel = 0;
      if (tree.rootRef != REF_NONE && !(tree.rootRef & REF_LEAF)) {
        std::vector<uint> stack(1, tree.rootRef);
        while (!stack.empty()) {
          const uint id = stack.back(); stack.pop_back();
          for (uint ref : { tree.nodes[id].ref0, tree.nodes[id].ref1 })
            if (ref != REF_NONE && !(ref & REF_LEAF)) { level[ref] = level[id] + 1u; maxLevel = std::max(maxLevel, level[ref]); stack.push_back(ref); }
        }
      }
      c->levelOffsets.assign(tree.nodes.empty() ? 1 : maxLevel + 2, 0u);
      for (size_t i = 0; i < tree.nodes.size(); i++) c->levelOffsets[level[i] + 1]++;
      for (size_t l = 1; l < c->levelOffsets.size(); l++) c->levelOffsets[l] += c->levelOffsets[l - 1];
      std::vector<uint> fill(c->levelOffsets.begin(), c->levelOffsets.end() - 1), ids(std::max<size_t>(tree.nodes.size(), 1), 0u);
      for (size_t i = 0; i < tree.nodes.size(); i++) ids[fill[level[i]]++] = (uint)i;
      HIPCHK(c, c->dLevelNodes.upload(ids.data(), ids.size()));
      HIPCHK(c, c->dTriBox.alloc(6 * std::max<size_t>(instTris, 1)));
      HIPCHK(c, c->dNodeBounds.alloc(6 * std::max<size_t>(tree.nodes.size(), 1)));
      c->flatTris.swap(tris); c->flatOnDevice = false; c->flatNodes = tree.nodes.size();
      c->flatRefittable = tree.rootRef != REF_NONE && !(tree.rootRef & REF_LEAF) && instTris > 0 && !c->anyMotion;   // (the refit kernels know one key only)
    }
    c->tCommit[0] = float(tUp0 - tBuild0 + collapseMs); c->tCommit[1] = float(now_ms() - tUp0 - collapseMs); c->tCommit[2] = 0.0f; c->tCommit[3] = 0.0f;   // the collapse is host build time
    c->S.nodes = c->dNodes.p; c->S.tris = c->dTris.p; c->S.insts = c->dInsts.p;
    c->S.rootRef = tree.rootRef; c->S.numInsts = (uint)ni; c->S.flatMode = 1; c->S.sweep = 0; c->S.sweepInsts = nullptr; c->S.sweepTris = nullptr;
    c->sahVisits = sah_node_visits(tree);
    c->S.nodeMin = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 16u : 0u);
    // the 4-wide walk votes earlier: 1M triangles, node_min 0 / 8 / 16 / 24 / 32 / 48 -> 176 / 254 / 273 / 286 / 288 / 269 Mpaths/s (profiles/sweep_wide.sh)
    c->S.nodeMin4 = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 32u : 0u);
    c->stackNeeded = tree.depth + 1u;
    if (std::getenv("HPT_DEBUG_ACCEL")) std::fprintf(stderr, "[hydra_hip] single-level BVH: %zu triangles, %zu nodes, depth %u, stack %u (LDS part %d), sah visits %.2f, nodeMin %u\n", instTris, tree.nodes.size(), tree.depth, c->stackNeeded, LDS_STACK, c->sahVisits, c->S.nodeMin);
    if (c->stackNeeded > MAX_STACK) return c->fail(HPT_ERR_UNSUPPORTED, "CommitScene: BVH deeper than the 64-entry traversal stack");
    c->accelCommitted = true; c->shadeTrisDirty = true;
    return HPT_OK;
  }
  // ---- top level over the instances' world boxes ----
  const size_t ni = c->insts.size();
  std::vector<Aabb> ib; std::vector<uint> liveInst;
  for (size_t i = 0; i < ni; i++) {
    const Geom& g = c->geoms[c->insts[i].geomId];
    if (g.bvh.rootRef == REF_NONE) continue;               // empty mesh: never enters the TLAS
    Aabb w; w.reset();
    // a moving instance: every point travels on a segment between its two key positions, so the union of the two key boxes bounds it
    for (int key = 0; key < (c->insts[i].motion ? 2 : 1); key++) {
      const float* m = key ? c->insts[i].m1 : c->insts[i].m;
      for (int k = 0; k < 8; k++) {
        const float p[3] = { (k & 1) ? g.bvh.bounds.hi[0] : g.bvh.bounds.lo[0], (k & 2) ? g.bvh.bounds.hi[1] : g.bvh.bounds.lo[1], (k & 4) ? g.bvh.bounds.hi[2] : g.bvh.bounds.lo[2] };
        const float q[3] = { m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12], m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13], m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14] };
        w.grow(q);
      }
    }
    w.pad();
    ib.push_back(w); liveInst.push_back((uint)i);
  }
  Bvh2 tlas = Bvh2Builder::build(ib, 1, std::max(16, ceil_log2(ib.size() + 1) + 2), true);
  {                                                          // TLAS visits + the chance of entering each instance x its BLAS visits
    double v = sah_node_visits(tlas);
    const float a0 = tlas.bounds.halfArea();
    std::vector<float> blasVisits(c->geoms.size(), -1.0f);
    for (size_t k = 0; k < ib.size() && a0 > 0.0f; k++) {
      const uint g = c->insts[liveInst[k]].geomId;
      if (blasVisits[g] < 0.0f) blasVisits[g] = sah_node_visits(c->geoms[g].bvh);
      v += double(ib[k].halfArea()) / a0 * blasVisits[g];
    }
    c->sahVisits = (float)v;
    c->S.nodeMin = c->nodeMinOverride >= 0 ? (uint)c->nodeMinOverride : (c->sahVisits >= HEAVY_SAH_VISITS ? 16u : 0u);
  }
  // instance leaves refer to positions in `ib`; map them back to real instance ids
  auto fixInst = [&](uint ref) -> uint {
    if (ref != REF_NONE && (ref & REF_LEAF) && ((ref >> 28) & 7u) == 0u) return REF_LEAF | liveInst[ref & 0x0FFFFFFFu];
    return ref;
  };
  // ---- flatten: [TLAS nodes][BLAS 0 nodes][BLAS 1 nodes]...  /  [tris 0][tris 1]... ----
  std::vector<BvhNode> nodes(tlas.nodes);
  for (BvhNode& n : nodes) { n.ref0 = fixInst(n.ref0); n.ref1 = fixInst(n.ref1); }
  const uint rootRef = fixInst(tlas.rootRef);
  std::vector<BvhTri> tris;
  std::vector<uint> geomRoot(c->geoms.size(), REF_NONE);
  for (size_t gi = 0; gi < c->geoms.size(); gi++) {
    const Geom& g = c->geoms[gi];
    const uint nodeBase = (uint)nodes.size(), triBase = (uint)tris.size();
    for (BvhNode n : g.bvh.nodes) { n.ref0 = patchRef(n.ref0, nodeBase, triBase); n.ref1 = patchRef(n.ref1, nodeBase, triBase); nodes.push_back(n); }
    tris.insert(tris.end(), g.tris.begin(), g.tris.end());
    geomRoot[gi] = patchRef(g.bvh.rootRef, nodeBase, triBase);
  }
  if (tris.size() >= (size_t(1) << 28) || nodes.size() >= (size_t(1) << 31)) return c->fail(HPT_ERR_UNSUPPORTED, "CommitScene: scene too large for 28-bit triangle references");
  std::vector<BvhInst> dinst(std::max<size_t>(ni, 1));    // (never empty: an empty scene still hands valid pointers to the kernels)
  for (size_t i = 0; i < ni; i++) {
    inverse_rows(c->insts[i].m, dinst[i].row0, dinst[i].row1, dinst[i].row2);
    dinst[i].root = geomRoot[c->insts[i].geomId]; dinst[i].geomId = c->insts[i].geomId; dinst[i].pad0 = c->insts[i].motion ? 1u : 0u; dinst[i].pad1 = 0;
  }
  // the triangle sweep keeps its own copy of the instance records: {rows, first triangle record, geomId, 0, number of record pairs}
  const bool sweep = resolvesSweep(c, instTris, c->anyMotion);
  if (c->accelLayout == 3 && c->anyMotion) return c->fail(HPT_ERR_UNSUPPORTED, "CommitScene: the triangle sweep does not hold moving instances (two-level or single-level layout)");
  if (sweep) {
    std::vector<uint> geomTriBase(c->geoms.size(), 0u);
    std::vector<BvhTri> st;                                     // every mesh's records in primitive order
    for (size_t gi = 0; gi < c->geoms.size(); gi++) {
      const Geom& g = c->geoms[gi];
      geomTriBase[gi] = (uint)st.size();
      const size_t base = st.size();
      st.resize(base + g.tris.size());
      for (const BvhTri& t : g.tris) st[base + t.primId] = t;   // g.tris is a permutation of the mesh's primitives (BVH leaf order)
      if (st.size() & 1u) { BvhTri z; std::memset(&z, 0, sizeof(z)); z.primId = 0xFFFFFFFFu; st.push_back(z); }   // pairs: an all-zero triangle has det == 0 and is never hit
    }
    if (st.empty()) st.push_back(BvhTri());
    HIPCHK(c, c->dSweepTris.upload(st.data(), st.size()));
    // one plane per record pair (traceSweep's pair cull; hpt_types.h: sweepPairPlane)
    std::vector<SweepPlane> sp((st.size() + 1) / 2);
    for (size_t k = 0; k < sp.size(); k++) sweepPairPlane(st[2 * k], 2 * k + 1 < st.size() ? st[2 * k + 1] : st[2 * k], sp[k]);
    HIPCHK(c, c->dSweepPlanes.upload(sp.data(), sp.size()));
    // one box per record pair (traceSweep's per-lane pass; hpt_types.h: sweepPairBox)
    std::vector<SweepPairBox> sbx(sp.size());
    for (size_t k = 0; k < sbx.size(); k++) sweepPairBox(st[2 * k], 2 * k + 1 < st.size() ? st[2 * k + 1] : st[2 * k], sbx[k]);
    HIPCHK(c, c->dSweepPairBoxes.upload(sbx.data(), sbx.size()));
    std::vector<BvhInst> sw(dinst);
    for (size_t i = 0; i < ni; i++) { const uint g = c->insts[i].geomId; sw[i].root = geomTriBase[g]; sw[i].pad1 = (uint)(c->geoms[g].tris.size() + 1) / 2u;
                                 sw[i].pad0 = sw[i].pad1 >= 2u && sw[i].pad1 <= 32u ? 1u : 0u; }   // per-lane pass: 2 .. 32 pairs (a 32-bit mask per lane)
    HIPCHK(c, c->dSweepInsts.upload(sw.data(), sw.size()));
    // the instances' padded world boxes (over their triangles' world-space vertices): traceSweep's wave-uniform skip
    std::vector<float> sb(8 * std::max<size_t>(ni, 1), 0.0f);
    for (size_t i = 0; i < ni; i++) {
      const Geom& g = c->geoms[c->insts[i].geomId];
      const float* m = c->insts[i].m;
      Aabb b; b.reset();
      for (size_t v = 0; v + 2 < g.pos.size(); v += 3) {
        const float* p = &g.pos[v];
        const float q[3] = { m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12], m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13], m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14] };
        b.grow(q);
      }
      if (g.pos.empty()) { for (int a = 0; a < 3; a++) { b.lo[a] = 1.0f; b.hi[a] = -1.0f; } } else b.pad();
      for (int a = 0; a < 3; a++) { sb[8 * i + a] = b.lo[a]; sb[8 * i + 4 + a] = b.hi[a]; }
    }
    HIPCHK(c, c->dSweepBoxes.upload(sb.data(), sb.size()));
  }
  c->S.sweep = sweep ? 1u : 0u; c->S.sweepInsts = sweep ? c->dSweepInsts.p : nullptr; c->S.sweepTris = sweep ? c->dSweepTris.p : nullptr; c->S.sweepBoxes = sweep ? (const float4*)c->dSweepBoxes.p : nullptr;
  c->S.sweepPlanes = sweep ? (const float4*)c->dSweepPlanes.p : nullptr; c->S.sweepCull = sweep ? c->sweepCull : 0u;
  c->S.sweepPairBoxes = sweep ? (const float4*)c->dSweepPairBoxes.p : nullptr; c->S.sweepLanes = sweep ? c->sweepLanes : 0u;
  c->tlNodes = nodes.size(); c->tlTris = tris.size();
  if (nodes.empty()) nodes.push_back(BvhNode());           // keep the pointers valid
  if (tris.empty()) tris.push_back(BvhTri());
  HIPCHK(c, c->dNodes.upload(nodes.data(), nodes.size()));
  HIPCHK(c, c->dTris.upload(tris.data(), tris.size()));
  HIPCHK(c, c->dInsts.upload(dinst.data(), dinst.size()));
  c->S.nodes = c->dNodes.p; c->S.tris = c->dTris.p; c->S.insts = c->dInsts.p;
  c->S.rootRef = rootRef; c->S.numInsts = (uint)ni; c->S.flatMode = 0;
  c->nodes4Count = 0; c->stackNeeded4 = 0; c->S.nodes4 = nullptr; c->S.root4 = REF_NONE; c->S.statsWide = 0; c->S.megaWide = 0; c->S.nodeMin4 = 0;
  c->flatRefittable = c->tlUpdatable = false; c->flatOnDevice = false; c->flatNodes = 0; c->levelOffsets.assign(1, 0u);
  c->tCommit[0] = float(now_ms() - tBuild0); c->tCommit[1] = 0.0f; c->tCommit[2] = 0.0f; c->tCommit[3] = 0.0f;
  c->stackNeeded = tlas.depth + 1u + maxBlasDepth + 1u;
  if (std::getenv("HPT_DEBUG_ACCEL")) std::fprintf(stderr, "[hydra_hip] two-level BVH: %zu instances, TLAS depth %u, deepest BLAS %u, stack %u (LDS part %d)\n", ni, tlas.depth, maxBlasDepth, c->stackNeeded, LDS_STACK);
  if (c->stackNeeded > MAX_STACK) return c->fail(HPT_ERR_UNSUPPORTED, "CommitScene: BVH deeper than the 64-entry traversal stack");
  c->accelCommitted = true; c->shadeTrisDirty = true;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_commit_scene"); }

// HBM part of the traversal stacks for a grid of `lanes` lanes (only touched by lanes whose stack outgrows LDS_STACK)
// stack entries a megakernel traversal may need: with HPT_FLAT_WIDE the single-level walk uses the 4-wide tree when the scene has one
static uint megaStackNeeded(const hpt_ctx* c) { return ((HPT_FLAT_WIDE || c->S.megaWide != 0u) && c->S.flatMode != 0u && c->S.motion == 0u && c->nodes4Count != 0u) ? std::max(c->stackNeeded, c->stackNeeded4) : c->stackNeeded; }
static hipError_t ensureStackOverflow(hpt_ctx* c, size_t lanes)
{
  const uint need = std::max(c->stackNeeded, c->stackNeeded4);                  // either tree may be walked
  const size_t extra = need > (uint)LDS_STACK ? need - LDS_STACK : 1;
  return c->dStackOvf.alloc(extra * lanes);
}

// Diagnostic ("dbg_stack_witness"): the HBM part of the stacks is filled with a word no traversal pushes before a launch, so that the words a
// launch wrote can be counted afterwards (hpt_get_stack_witness). REF_NONE is that word: a push stores a child reference whose box the ray hit -
// a node index, a leaf (both builders give every inner node two real children; the empty slots of a 4-wide node carry REF_NONE but their valid
// bit is clear, and wideNodeStep pushes valid children only) - or REF_RESTORE; a popped REF_NONE would end the walk with the rest of its stack unread.
// REF_RESTORE (all ones) IS pushed, hence the 32-bit fill. Off: no call, no fill.
static const uint STACK_SENTINEL = REF_NONE;
static hipError_t stackWitnessFill(hpt_ctx* c, hipStream_t st)
{
  c->witnessWords = 0;
  if (!c->stackWitness || !c->dStackOvf.p || c->dStackOvf.n == 0) return hipSuccess;
  c->witnessWords = c->dStackOvf.n;
  return hipMemsetD32Async((hipDeviceptr_t)c->dStackOvf.p, (int)STACK_SENTINEL, c->dStackOvf.n, st);
}

// The traversal variant of the committed layout for the kernels that are built for five of them (rayQueryKernel, gbufferKernel, castSingleRayKernel,
// rayTraceKernel): sweep; single-level with motion; single-level; two-level with motion; two-level. f gets (FLAT, MOTION, SWEEP) as
// std::bool_constant objects, i.e. as compile-time constants. (The path-tracing ladders also switch on the stack depth and are their own.)
template <class F>
static void traversalDispatch(const hpt_ctx* c, F f)
{
  const std::true_type T; const std::false_type N;
  if (c->S.sweep)                         f(N, N, T);
  else if (c->S.flatMode && c->anyMotion) f(T, T, N);
  else if (c->S.flatMode)                 f(T, N, N);
  else if (c->anyMotion)                  f(N, T, N);
  else                                    f(N, N, N);
}

// The frame of a launch of `lanes` lanes on `st`: size the HBM part of the traversal stacks, record ev0, launch(), check, record ev1. Whatever
// reads c->dStackOvf.p (a kernel argument, Job::stackOverflow) belongs into launch(). EVENTS = false: the same without the event pair.
template <bool EVENTS = true, class Launch>
static int launchFrame(hpt_ctx* c, size_t lanes, hipStream_t st, Launch launch)
{
  HIPCHK(c, ensureStackOverflow(c, lanes));
  if (c->stackWitness) HIPCHK(c, stackWitnessFill(c, st));
  if (EVENTS) HIPCHK(c, hipEventRecord(c->ev0, st));
  launch();
  HIPCHK(c, hipGetLastError());
  if (EVENTS) HIPCHK(c, hipEventRecord(c->ev1, st));
  return HPT_OK;
}

static int ray_query(hpt_ctx* c, const float* posNear, const float* dirFar, uint32_t n, void* out, int any, float time = 0.0f)
{
  if (!c || !posNear || !dirFar || !out) return HPT_ERR_ARG;
  if (!c->accelCommitted) return c->fail(HPT_ERR_STATE, "RayQuery before CommitScene");
  if (n == 0) return HPT_OK;
  (void)hipSetDevice(c->device);
  DevBuf<float4> dp, dd; DevBuf<uint> dout;
  const size_t outWords = any ? n : (size_t)n * 8;
  HIPCHK(c, dp.upload((const float4*)posNear, n));
  HIPCHK(c, dd.upload((const float4*)dirFar, n));
  HIPCHK(c, dout.alloc(outWords));
  const uint blocks = (n + 255) / 256;
  if (int rc = launchFrame<false>(c, (size_t)blocks * 256, nullptr, [&]() {
    traversalDispatch(c, [&](auto flat, auto motion, auto sweep) {         // the time goes to the motion variants only
      rayQueryKernel<flat(), motion(), sweep()><<<dim3(blocks), dim3(256), 0, 0>>>(c->S, dp.p, dd.p, n, dout.p, any, c->dStackOvf.p, motion() ? time : 0.0f);
    });
  })) return rc;
  HIPCHK(c, hipMemcpy(out, dout.p, outWords * 4, hipMemcpyDeviceToHost));
  return HPT_OK;
}

extern "C" int hpt_ray_query_nearest(hpt_ctx* c, const float* p, const float* d, uint32_t n, hpt_hit* out) try { return ray_query(c, p, d, n, out, 0); }
catch (...) { return hptGuard(c, "hpt_ray_query_nearest"); }
extern "C" int hpt_ray_query_any(hpt_ctx* c, const float* p, const float* d, uint32_t n, uint32_t* out) try { return ray_query(c, p, d, n, out, 1); }
catch (...) { return hptGuard(c, "hpt_ray_query_any"); }
extern "C" int hpt_ray_query_nearest_motion(hpt_ctx* c, const float* p, const float* d, uint32_t n, float time, hpt_hit* out) try { return ray_query(c, p, d, n, out, 0, time); }
catch (...) { return hptGuard(c, "hpt_ray_query_nearest_motion"); }
extern "C" int hpt_ray_query_any_motion(hpt_ctx* c, const float* p, const float* d, uint32_t n, float time, uint32_t* out) try { return ray_query(c, p, d, n, out, 1, time); }
catch (...) { return hptGuard(c, "hpt_ray_query_any_motion"); }

// ---- scene tables -----------------------------------------------------------------------------------------------------------------
static bool lean_materials(const MaterialRec* m, size_t n)
{
  for (size_t i = 0; i < n; i++) if ((m[i].mtype != MAT_TYPE_GLTF && m[i].mtype != MAT_TYPE_LIGHT_SOURCE) || m[i].texid[1] != 0xFFFFFFFFu) return false;
  return true;
}
static int check_materials(hpt_ctx* c, const MaterialRec* m, size_t n, size_t numTex, size_t numMats, size_t numArrays1f)
{
  for (size_t i = 0; i < n; i++) {
    const uint t = m[i].mtype;
    if (t == MAT_TYPE_BLEND) {
      if (m[i].datai[0] >= numMats || m[i].datai[1] >= numMats) return c->fail(HPT_ERR_ARG, "blend material refers to a material that does not exist");
      if (m[i].texid[0] >= numTex) return c->fail(HPT_ERR_ARG, "material refers to a texture that does not exist");
      continue;
    }
    if (t == MAT_TYPE_THIN_FILM) {                            // every index filmArgs / filmReflTrans follow (hpt_film.h)
      auto bits = [](float f) { uint u; std::memcpy(&u, &f, 4); return u; };
      const uint layers = bits(m[i].data[FILM_LAYERS_COUNT]);
      if (layers < 1u || layers > 64u) return c->fail(HPT_ERR_ARG, "thin film: FILM_LAYERS_COUNT must be 1..64");
      if ((uint64_t)bits(m[i].data[FILM_ETA_OFFSET]) + layers > c->numFilmsEtaK || (uint64_t)bits(m[i].data[FILM_K_OFFSET]) + layers > c->numFilmsEtaK)
        return c->fail(HPT_ERR_ARG, "thin film: eta / k offsets reach past m_films_eta_k_vec");
      if ((uint64_t)bits(m[i].data[FILM_ETA_SPECID_OFFSET]) + layers > c->hFilmsSpecId.size() || (uint64_t)bits(m[i].data[FILM_K_SPECID_OFFSET]) + layers > c->hFilmsSpecId.size())
        return c->fail(HPT_ERR_ARG, "thin film: spectrum id offsets reach past m_films_spec_id_vec");
      for (uint l2 = 0; l2 < layers; l2++) for (int w = 0; w < 2; w++) {
        const uint id = c->hFilmsSpecId[bits(m[i].data[w ? FILM_K_SPECID_OFFSET : FILM_ETA_SPECID_OFFSET]) + l2];
        if (id != 0xFFFFFFFFu && id >= c->numSpectraHost) return c->fail(HPT_ERR_ARG, "thin film: layer refers to a spectrum that does not exist");
      }
      const bool tmap = bits(m[i].data[FILM_THICKNESS_MAP]) != 0u, pre = bits(m[i].data[FILM_PRECOMP_FLAG]) != 0u;
      if (tmap && m[i].texid[2] >= numTex) return c->fail(HPT_ERR_ARG, "thin film: the thickness map does not exist");
      if (m[i].texid[0] >= numTex) return c->fail(HPT_ERR_ARG, "material refers to a texture that does not exist");
      const uint64_t off = bits(m[i].data[FILM_PRECOMP_OFFSET]);
      if (pre && off > c->numPrecompFilms) return c->fail(HPT_ERR_ARG, "thin film: FILM_PRECOMP_OFFSET reaches past m_precomp_thin_films");
      continue;
    }
    if (t != MAT_TYPE_GLTF && t != MAT_TYPE_GLASS && t != MAT_TYPE_CONDUCTOR && t != MAT_TYPE_DIFFUSE && t != MAT_TYPE_DIELECTRIC && t != MAT_TYPE_PLASTIC && t != MAT_TYPE_LIGHT_SOURCE)
      return c->fail(HPT_ERR_UNSUPPORTED, "material type " + std::to_string(t) + " is not one of the reference's");
    if (t == MAT_TYPE_PLASTIC && (uint64_t)m[i].datai[0] + (uint64_t)MI_ROUGH_TRANSMITTANCE_RES > numArrays1f)
      return c->fail(HPT_ERR_ARG, "plastic material: transmittance table outside m_arrays1f");
    if (m[i].texid[1] != 0xFFFFFFFFu && m[i].texid[1] >= numTex) return c->fail(HPT_ERR_ARG, "material refers to a normal map that does not exist");
    if (m[i].texid[0] >= numTex) return c->fail(HPT_ERR_ARG, "material refers to a texture that does not exist");
    if ((m[i].cflags & FLAG_FOUR_TEXTURES) && (m[i].texid[2] >= numTex || m[i].texid[3] >= numTex)) return c->fail(HPT_ERR_ARG, "material refers to a texture that does not exist");
  }
  return HPT_OK;
}
// What the material table says about thin films: whether there is one, and whether each film's precomputed table has the size RGB / spectral
// rendering reads. The loader sizes a table by the mode it loads for (LoadThinFilmMaterial, integrator_pt_scene_mat.cpp:1147-1186): RGB
// 4 x FILM_ANGLE_RES x 3 (x FILM_THICKNESS_RES with a thickness map or a single layer), spectral 4 x FILM_ANGLE_RES x FILM_LENGTH_RES or no table
// (one film with a thickness map). The tables lie back to back in m_precomp_thin_films, so a table ends where the next one starts.
static void film_scan(hpt_ctx* c)
{
  auto bits = [](float f) { uint u; std::memcpy(&u, &f, 4); return u; };
  c->hasFilm = false; c->filmTablesRGB = true; c->filmTablesSpectral = true;
  std::set<uint64_t> starts;
  for (const MaterialRec& m : c->hMaterials) if (m.mtype == MAT_TYPE_THIN_FILM && bits(m.data[FILM_PRECOMP_FLAG]) != 0u) starts.insert(bits(m.data[FILM_PRECOMP_OFFSET]));
  starts.insert(c->numPrecompFilms);
  for (const MaterialRec& m : c->hMaterials) {
    if (m.mtype != MAT_TYPE_THIN_FILM) continue;
    c->hasFilm = true;
    const bool pre = bits(m.data[FILM_PRECOMP_FLAG]) != 0u, tmap = bits(m.data[FILM_THICKNESS_MAP]) != 0u;
    const uint layers = bits(m.data[FILM_LAYERS_COUNT]);
    uint64_t size = 0;
    if (pre) { const uint64_t off = bits(m.data[FILM_PRECOMP_OFFSET]); auto it = starts.upper_bound(off); size = (it == starts.end() ? c->numPrecompFilms : *it) - off; }
    if (size != 4ull * FILM_ANGLE_RES * 3ull * ((tmap || layers == 1u) ? (uint64_t)FILM_THICKNESS_RES : 1ull)) c->filmTablesRGB = false;
    if (pre ? size != 4ull * FILM_ANGLE_RES * FILM_LENGTH_RES : !(tmap && layers <= 2u)) c->filmTablesSpectral = false;
  }
}
// A blend refers to two other materials, possibly blends: the sampling loop of shadeVertex follows such references until it meets a
// leaf, so a reference cycle would never end on the device. Three-colour depth-first search over the blend nodes.
static int check_blend_graph(hpt_ctx* c, const std::vector<MaterialRec>& m)
{
  std::vector<unsigned char> state(m.size(), 0);           // 0 not seen, 1 on the current path, 2 done
  std::vector<std::pair<uint, int>> path;
  for (uint root = 0; root < (uint)m.size(); root++) {
    if (m[root].mtype != MAT_TYPE_BLEND || state[root] != 0) continue;
    path.clear(); path.push_back({ root, 0 }); state[root] = 1;
    while (!path.empty()) {
      auto& top = path.back();
      if (top.second == 2) { state[top.first] = 2; path.pop_back(); continue; }
      const uint child = m[top.first].datai[top.second++];
      if (child >= m.size()) return c->fail(HPT_ERR_ARG, "blend material refers to a material that does not exist");
      if (m[child].mtype != MAT_TYPE_BLEND) continue;
      if (state[child] == 1) return c->fail(HPT_ERR_ARG, "blend materials refer to each other in a cycle (material " + std::to_string(child) + ")");
      if (state[child] == 0) { state[child] = 1; path.push_back({ child, 0 }); }
    }
  }
  return HPT_OK;
}
static int check_lights(hpt_ctx* c, const LightRec* l, size_t n, size_t numTex, size_t numArrays1f)
{
  for (size_t i = 0; i < n; i++) {
    if (l[i].geomType == LIGHT_GEOM_ENV) {                                // a sampled environment map: its pdf table must lie inside m_arrays1f
      const uint64_t need = (uint64_t)l[i].pdfTableSizeX * l[i].pdfTableSizeY + 1u;
      if (l[i].pdfTableSizeX == 0 || l[i].pdfTableSizeY == 0 || (uint64_t)l[i].pdfTableOffset + need > numArrays1f || l[i].pdfTableSize < need)
        return c->fail(HPT_ERR_ARG, "environment light: pdf table outside m_arrays1f");
      if (l[i].texId != 0xFFFFFFFFu && l[i].texId >= numTex) return c->fail(HPT_ERR_ARG, "environment light refers to a texture that does not exist");
    }
    if (l[i].geomType < LIGHT_GEOM_RECT || l[i].geomType > LIGHT_GEOM_ENV) return c->fail(HPT_ERR_ARG, "bad light geomType");
    if (l[i].geomType != LIGHT_GEOM_ENV && l[i].texId != 0xFFFFFFFFu && l[i].texId >= numTex) return c->fail(HPT_ERR_ARG, "light refers to a projected texture that does not exist");
    if (l[i].iesId != 0xFFFFFFFFu && l[i].iesId >= numTex) return c->fail(HPT_ERR_ARG, "light refers to an IES texture that does not exist");
  }
  return HPT_OK;
}

// Every index the kernels follow without a bounds check of their own (an out-of-range one would fault on the device, which on this class of
// machine can take the whole node down): material ids per primitive and per remap target, vertex indices, remap-list and light ids.
static int check_tables(hpt_ctx* c, const hpt_scene_desc* d)
{
  if (d->numInsts && (!d->remapInst || !d->normMatrices)) return c->fail(HPT_ERR_ARG, "m_remapInst / m_normMatrices missing");
  if (d->numTris && (!d->triIndices || !d->matIdByPrimId)) return c->fail(HPT_ERR_ARG, "m_triIndices / m_matIdByPrimId missing");
  if (d->numVerts && !d->vData8f) return c->fail(HPT_ERR_ARG, "m_vData8f missing");
  if (d->numGeoms && !d->matVertOffset) return c->fail(HPT_ERR_ARG, "m_matVertOffset missing");
  for (uint g = 0; g < d->numGeoms; g++) {
    // per-mesh counts: given (geometry handed over with the tables), or the distance to the next mesh's offsets (geometry went through
    // AddGeom_Triangles3f: the Integrator keeps only m_matVertOffset)
    const uint64_t triOff = d->matVertOffset[2 * g + 0], vertOff = d->matVertOffset[2 * g + 1];
    const uint64_t triEnd = d->geomTriCount ? triOff + d->geomTriCount[g] : (g + 1 < d->numGeoms ? d->matVertOffset[2 * (g + 1) + 0] : d->numTris);
    const uint64_t vertEnd = d->geomVertCount ? vertOff + d->geomVertCount[g] : (g + 1 < d->numGeoms ? d->matVertOffset[2 * (g + 1) + 1] : d->numVerts);
    if (triEnd < triOff || vertEnd < vertOff || triEnd > d->numTris || vertEnd > d->numVerts) return c->fail(HPT_ERR_ARG, "m_matVertOffset: geometry " + std::to_string(g) + " reaches past the tables");
    for (uint64_t t = 3 * triOff; t < 3 * triEnd; t++)
      if (d->triIndices[t] >= vertEnd - vertOff) return c->fail(HPT_ERR_ARG, "m_triIndices: vertex index out of the mesh's range (geometry " + std::to_string(g) + ")");
  }
  for (uint t = 0; t < d->numTris; t++)
    if ((d->matIdByPrimId[t] & 0x00FFFFFFu) >= d->numMaterials) return c->fail(HPT_ERR_ARG, "m_matIdByPrimId: material id " + std::to_string(d->matIdByPrimId[t]) + " does not exist");
  // m_allRemapLists = the lists back to back, then one offset per list and the total (integrator_pt_scene.cpp:909-924)
  const uint size = d->allRemapListsSize, len = d->allRemapListsLen;
  int numLists = 0;
  if (len) {
    if (!d->allRemapLists || size >= len) return c->fail(HPT_ERR_ARG, "m_allRemapLists: size does not leave room for the offsets");
    numLists = (int)(len - size) - 1;
    for (int l = 0; l <= numLists; l++) {
      const int off = d->allRemapLists[size + (uint)l];
      if (off < 0 || (uint)off > size || (off & 1) || (l > 0 && off < d->allRemapLists[size + (uint)l - 1])) return c->fail(HPT_ERR_ARG, "m_allRemapLists: bad offset table");
    }
    for (uint i = 1; i < size; i += 2)
      if (d->allRemapLists[i] < 0 || (uint)d->allRemapLists[i] >= d->numMaterials) return c->fail(HPT_ERR_ARG, "m_allRemapLists: remap target " + std::to_string(d->allRemapLists[i]) + " does not exist");
  }
  for (uint i = 0; i < d->numInsts; i++) {
    const int list = d->remapInst[2 * i + 0], light = d->remapInst[2 * i + 1];
    if (list < -1 || list >= numLists) return c->fail(HPT_ERR_ARG, "m_remapInst: remap list " + std::to_string(list) + " does not exist");
    if (light < -1 || light >= (int)d->numLights) return c->fail(HPT_ERR_ARG, "m_remapInst: light " + std::to_string(light) + " does not exist");
  }
  return HPT_OK;
}

extern "C" int hpt_upload_scene(hpt_ctx* c, const hpt_scene_desc* d)
try {
  if (!c || !d) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  const double t0 = now_ms();
  if (d->numTextures == 0 || !d->textures) return c->fail(HPT_ERR_ARG, "m_textures must at least hold the white dummy texture");
  // the film tables first: check_materials follows a film material's indices into them
  c->numFilmsEtaK = d->filmsEtaK ? d->numFilmsEtaK : 0u; c->numPrecompFilms = d->precompThinFilms ? d->numPrecompThinFilms : 0u;
  c->hFilmsSpecId.assign(d->filmsSpecId ? d->filmsSpecId : nullptr, d->filmsSpecId ? d->filmsSpecId + d->numFilmsSpecId : nullptr);
  c->numSpectraHost = (d->specValues && d->specOffsetSz) ? d->numSpectra : 0u;
  int rc = check_materials(c, (const MaterialRec*)d->materials, d->numMaterials, d->numTextures, d->numMaterials, d->numArrays1f); if (rc) return rc;
  c->leanMaterials = lean_materials((const MaterialRec*)d->materials, d->numMaterials);
  { std::vector<MaterialRec> hm((const MaterialRec*)d->materials, (const MaterialRec*)d->materials + d->numMaterials);
    rc = check_blend_graph(c, hm); if (rc) return rc;
    c->hMaterials.swap(hm); }
  film_scan(c);
  if (d->numArrays1f && !d->arrays1f) return c->fail(HPT_ERR_ARG, "m_arrays1f: count without data");
  rc = check_lights(c, (const LightRec*)d->lights, d->numLights, d->numTextures, d->numArrays1f); if (rc) return rc;
  rc = check_tables(c, d); if (rc) return rc;

  if (d->vPos4f) {                                                     // LoadSceneGeometry + LoadSceneInstances order
    hpt_clear_geom(c);
    for (uint g = 0; g < d->numGeoms; g++) {
      const uint triOff = d->matVertOffset[2 * g + 0], vertOff = d->matVertOffset[2 * g + 1];
      const uint32_t id = hpt_add_geom_triangles3f(c, d->vPos4f + 4 * (size_t)vertOff, d->geomVertCount[g], d->triIndices + 3 * (size_t)triOff,
                                                   3 * (size_t)d->geomTriCount[g], 0, 16);
      if (id == 0xFFFFFFFFu) return HPT_ERR_ARG;
    }
    hpt_clear_scene(c);
    for (uint i = 0; i < d->numInsts; i++) {
      const bool moving = d->instHasMotion && d->instMatricesMotion && d->instHasMotion[i] != 0;
      float two[32];
      if (moving) { std::memcpy(two, d->instMatrices + 16 * (size_t)i, 64); std::memcpy(two + 16, d->instMatricesMotion + 16 * (size_t)i, 64); }
      const uint32_t id = moving ? hpt_add_instance_motion(c, d->instGeomId[i], two, 2) : hpt_add_instance(c, d->instGeomId[i], d->instMatrices + 16 * (size_t)i);
      if (id == 0xFFFFFFFFu) return c->fail(HPT_ERR_ARG, "AddInstance: bad geomId");
    }
    rc = hpt_commit_scene(c, 0); if (rc) return rc;
  }
  if (!c->accelCommitted) return c->fail(HPT_ERR_STATE, "CommitDeviceData before CommitScene");
  if (d->numInsts != c->insts.size()) return c->fail(HPT_ERR_ARG, "scene tables and acceleration structure disagree on the instance count");

  HIPCHK(c, c->dTriIndices.upload(d->triIndices, 3 * (size_t)d->numTris));
  c->hTriIndices.assign(d->triIndices, d->triIndices + 3 * (size_t)d->numTris);
  HIPCHK(c, c->dVData.upload(d->vData8f, 8 * (size_t)d->numVerts));
  HIPCHK(c, c->dMatIdByPrim.upload(d->matIdByPrimId, d->numTris));
  HIPCHK(c, c->dMatVertOffset.upload(d->matVertOffset, 2 * (size_t)d->numGeoms));
  std::vector<float> nm(12 * (size_t)std::max(1u, d->numInsts), 0.0f);
  for (uint i = 0; i < d->numInsts; i++) {
    const float* m = d->normMatrices + 16 * (size_t)i;                 // rows of the upper 3x3 (column-major source)
    float* o = &nm[12 * (size_t)i];
    o[0] = m[0]; o[1] = m[4]; o[2] = m[8];  o[3] = 0.0f;
    o[4] = m[1]; o[5] = m[5]; o[6] = m[9];  o[7] = 0.0f;
    o[8] = m[2]; o[9] = m[6]; o[10] = m[10]; o[11] = 0.0f;
  }
  HIPCHK(c, c->dNormMat.upload(nm.data(), nm.size()));
  // motion blur: m_normMatrices[m_normMatrices2Offs + i] = transpose(inverse(matrix at the end of the motion)) (integrator_pt_scene.cpp:864-897)
  if (d->normMatrices2Offs != 0 && d->normMatrices2Offs != d->numInsts) return c->fail(HPT_ERR_ARG, "m_normMatrices2Offs must be 0 or the instance count");
  if ((d->normMatrices2Offs != 0) != c->anyMotion) return c->fail(HPT_ERR_ARG, "m_normMatrices2Offs and the instances added with AddInstanceMotion disagree");
  {
    std::vector<float> nm2(12 * (size_t)std::max(1u, d->numInsts), 0.0f);
    if (d->normMatrices2Offs) for (uint i = 0; i < d->numInsts; i++) {
      const float* m = d->normMatrices + 16 * ((size_t)d->normMatrices2Offs + i);
      float* o = &nm2[12 * (size_t)i];
      o[0] = m[0]; o[1] = m[4]; o[2] = m[8];  o[4] = m[1]; o[5] = m[5]; o[6] = m[9];  o[8] = m[2]; o[9] = m[6]; o[10] = m[10];
    }
    HIPCHK(c, c->dNormMat2.upload(nm2.data(), nm2.size()));
  }
  c->S.normMat2 = c->dNormMat2.p; c->S.motion = d->normMatrices2Offs ? 1u : 0u; 
  HIPCHK(c, c->dRemapInst.upload(d->remapInst, 2 * (size_t)d->numInsts));
  {
    std::vector<int> rl(d->allRemapLists ? std::vector<int>(d->allRemapLists, d->allRemapLists + d->allRemapListsLen) : std::vector<int>());
    if (rl.empty()) rl.push_back(0);
    // RemapMaterialId (integrator_pt_mat.cpp:530-573) bisects over the list's INT count while indexing PAIRS, so its probes reach up to one
    // list length past the list's end (for the last list: past the array, in the reference too). Zero padding keeps those probes in bounds
    // and makes what they read the same here and in the checker.
    rl.resize(rl.size() + (size_t)d->allRemapListsSize + 2, 0);
    HIPCHK(c, c->dRemapLists.upload(rl.data(), rl.size()));
  }
  HIPCHK(c, c->dMaterials.upload((const MaterialRec*)d->materials, d->numMaterials));
  {
    std::vector<LightRec> ll((const LightRec*)d->lights, (const LightRec*)d->lights + d->numLights);
    if (ll.empty()) ll.resize(1);
    HIPCHK(c, c->dLights.upload(ll.data(), ll.size()));
  }
  for (void* p : c->texData) if (p) (void)hipFree(p);
  c->texData.clear(); c->hTextures.resize(d->numTextures);
  for (uint i = 0; i < d->numTextures; i++) {
    const hpt_texture_desc& t = d->textures[i];
    if (t.width == 0 || t.height == 0 || !t.data || t.format > 2) return c->fail(HPT_ERR_ARG, "bad texture descriptor");
    const size_t bytes = (size_t)t.width * t.height * (t.format == 1 ? 16 : 4);
    void* dp = nullptr;
    HIPCHK(c, hipMalloc(&dp, bytes));
    c->texData.push_back(dp);
    HIPCHK(c, hipMemcpy(dp, t.data, bytes, hipMemcpyHostToDevice));
    TexRec& r = c->hTextures[i];
    r.w = t.width; r.h = t.height; r.format = t.format; r.flags = t.flags; r.addrU = t.addressU; r.addrV = t.addressV; r.filter = t.filter; r.pad = 0;
    r.data = dp; r.diffOffset = ~0ull; r.diffW = r.diffH = r.diffChannels = 0; r.pad2 = 0;
  }
  HIPCHK(c, c->dTextures.upload(c->hTextures.data(), c->hTextures.size()));
  c->gradSize = 0; c->diffLightFirst = c->diffLightCount = 0; c->diffLightOff = 0;

  DevScene& S = c->S;
  S.triIndices = c->dTriIndices.p; S.vData8f = c->dVData.p; S.matIdByPrimId = c->dMatIdByPrim.p; S.matVertOffset = c->dMatVertOffset.p;
  S.normMat = c->dNormMat.p; S.remapInst = c->dRemapInst.p; S.allRemapLists = c->dRemapLists.p; S.allRemapListsSize = d->allRemapListsSize;
  S.numLights = d->numLights; S.materials = c->dMaterials.p; S.lights = c->dLights.p; S.textures = c->dTextures.p;
  c->numArrays1f = d->numArrays1f;
  { std::vector<float> a(d->numArrays1f ? d->arrays1f : nullptr, d->numArrays1f ? d->arrays1f + d->numArrays1f : nullptr); if (a.empty()) a.push_back(0.0f);
    HIPCHK(c, c->dArrays1f.upload(a.data(), a.size())); }
  S.arrays1f = c->dArrays1f.p;
  { std::vector<float> ek(d->filmsEtaK ? d->filmsEtaK : nullptr, d->filmsEtaK ? d->filmsEtaK + d->numFilmsEtaK : nullptr), pf(d->precompThinFilms ? d->precompThinFilms : nullptr, d->precompThinFilms ? d->precompThinFilms + d->numPrecompThinFilms : nullptr);
    std::vector<uint> si(c->hFilmsSpecId);
    if (ek.empty()) ek.push_back(0.0f); if (pf.empty()) pf.push_back(0.0f); if (si.empty()) si.push_back(0xFFFFFFFFu);
    HIPCHK(c, c->dFilmsEtaK.upload(ek.data(), ek.size())); HIPCHK(c, c->dPrecompFilms.upload(pf.data(), pf.size())); HIPCHK(c, c->dFilmsSpecId.upload(si.data(), si.size()));
    S.filmsEtaK = c->dFilmsEtaK.p; S.precompThinFilms = c->dPrecompFilms.p; S.filmsSpecId = c->dFilmsSpecId.p; }
  // ---- spectral tables (all optional: RGB rendering does not read them) ----
  {
    const uint WAVES = 471u;                                   // LAMBDA_MAX - LAMBDA_MIN + 1 samples per spectrum (Spectrum::ResampleUniform)
    c->spectralOk = d->specValues && d->specOffsetSz && d->numSpectra > 0 && d->cieXYZ && d->numCieXYZ >= WAVES;
    c->spectralWhyNot = c->spectralOk ? "" : "the scene came without m_spec_values / m_spec_offset_sz / m_cie_xyz";
    std::vector<uint> so(2 * std::max(1u, d->numSpectra), 0u);
    for (uint i = 0; i < d->numSpectra && d->specOffsetSz; i++) {
      so[2 * i] = d->specOffsetSz[2 * i]; so[2 * i + 1] = d->specOffsetSz[2 * i + 1];
      if (so[2 * i] == 0xFFFFFFFFu) {                            // a spectrum given by textures (lambda_ref_ids): its bands must come with it
        so[2 * i] = 0;
        const bool bands = d->specTexOffsetSz && d->specTexIdsWavelengths && d->specTexOffsetSz[2 * i + 1] >= 2u;
        if (!bands && c->spectralOk) { c->spectralOk = false; c->spectralWhyNot = "spectrum " + std::to_string(i) + " is given by textures, but m_spec_tex_ids_wavelengths / m_spec_tex_offset_sz did not come with the scene"; }
        continue;
      }
      if ((uint64_t)so[2 * i] + std::max(so[2 * i + 1], WAVES - 1u) > d->numSpecValues) return c->fail(HPT_ERR_ARG, "m_spec_offset_sz: spectrum " + std::to_string(i) + " reaches past m_spec_values");
    }
    {
      std::vector<uint> tos(2 * std::max(1u, d->numSpectra), 0u), tiw(2 * std::max(1u, d->specTexIdsWavelengths ? d->numSpecTexBands : 0u), 0u);
      if (d->specTexIdsWavelengths && d->numSpecTexBands) std::memcpy(tiw.data(), d->specTexIdsWavelengths, 8 * (size_t)d->numSpecTexBands);
      for (uint i = 0; i < d->numSpectra && d->specTexOffsetSz && d->specTexIdsWavelengths; i++) {
        const uint off = d->specTexOffsetSz[2 * i], sz = d->specTexOffsetSz[2 * i + 1];
        if (sz == 0u) continue;                                  // ({0xFFFFFFFF, 0}: a tabulated spectrum)
        if (sz < 2u || (uint64_t)off + sz > d->numSpecTexBands) return c->fail(HPT_ERR_ARG, "m_spec_tex_offset_sz: spectrum " + std::to_string(i) + " reaches past m_spec_tex_ids_wavelengths (or holds fewer than two bands)");
        for (uint k2 = 0; k2 < sz; k2++) {
          // (LoadSpectralTextures resolves the bands' texture ids only when it loads for spectral rendering: a scene loaded for RGB keeps the XML's)
          if (d->specTexIdsWavelengths[2 * (off + k2)] >= d->numTextures) { if (c->spectralOk) { c->spectralOk = false; c->spectralWhyNot = "m_spec_tex_ids_wavelengths refers to a texture that is not in m_textures (the scene was loaded for RGB rendering)"; } tiw[2 * (off + k2)] = 0u; }
          if (k2 && d->specTexIdsWavelengths[2 * (off + k2) + 1] <= d->specTexIdsWavelengths[2 * (off + k2 - 1) + 1]) return c->fail(HPT_ERR_ARG, "m_spec_tex_ids_wavelengths: the bands of a spectrum must ascend in wavelength");
        }
        tos[2 * i] = off; tos[2 * i + 1] = sz;
      }
      HIPCHK(c, c->dSpecTexOffsetSz.upload(tos.data(), tos.size())); HIPCHK(c, c->dSpecTexIdsWavelengths.upload(tiw.data(), tiw.size()));
      S.specTexOffsetSz = c->dSpecTexOffsetSz.p; S.specTexIdsWavelengths = c->dSpecTexIdsWavelengths.p;
    }
    auto specIdOk = [&](uint id) { return id == 0xFFFFFFFFu || id < d->numSpectra; };
    const MaterialRec* mm = (const MaterialRec*)d->materials;
    for (uint i = 0; i < d->numMaterials; i++)
      for (int k2 = 0; k2 < 4; k2++) if (d->specValues && !specIdOk(mm[i].spdid[k2])) return c->fail(HPT_ERR_ARG, "material " + std::to_string(i) + " refers to a spectrum that does not exist");
    // (every material type of the RGB kernels has its branch in the spectral kernel, blends and normal maps included.) Which instantiations a
    // spectral call needs (hpt_spectral.hip: SCOPE) is decided by the materials a hit can REACH: m_matIdByPrimId through the remap list of every
    // instance of the mesh (RemapMaterialId), then through blends - an entry of the library nothing resolves to (the reference's spectral fixture
    // keeps an unused legacy material 0) does not widen the kernel
    {
      std::vector<char> reached(d->numMaterials, 0);
      std::set<std::pair<uint, int>> seen;
      for (uint inst = 0; inst < d->numInsts; inst++) {
        const uint g = d->instGeomId[inst];
        const int list = d->remapInst[2 * inst + 0];
        if (g >= d->numGeoms || !seen.insert(std::make_pair(g, list)).second) continue;
        int rOff = 0, rSize = 0;
        if (list >= 0 && d->allRemapLists && (uint)list + 1 + d->allRemapListsSize < d->allRemapListsLen) {
          rOff = d->allRemapLists[d->allRemapListsSize + list]; rSize = (d->allRemapLists[d->allRemapListsSize + list + 1] - rOff) / 2;
        }
        const uint t0 = d->matVertOffset[2 * g];
        const uint t1 = std::min(d->geomTriCount ? t0 + d->geomTriCount[g] : (g + 1 < d->numGeoms ? d->matVertOffset[2 * (g + 1)] : d->numTris), d->numTris);
        for (uint t = t0; t < t1; t++) {
          uint id = d->matIdByPrimId[t];
          if (list >= 0 && rSize > 0) {
            // the device's RemapMaterialId exactly (hpt_device.h: remapMaterialId = integrator_pt_mat.cpp:530-573): a bisection over the list's INT
            // count that indexes PAIRS, so its probes can land in the next list or in the zero padding behind the table - 'reached' must follow it
            auto at = [&](long k) -> int { return (k >= 0 && (size_t)k < d->allRemapListsLen) ? d->allRemapLists[k] : 0; };
            const int rInts = 2 * rSize;
            int low = 0, high = rInts - 1;
            while (low <= high) { const int mid = low + ((high - low) / 2); if ((uint)at((long)rOff + mid * 2) >= id) high = mid - 1; else low = mid + 1; }
            if (high + 1 < rInts && (uint)at((long)rOff + (high + 1) * 2) == id) id = (uint)at((long)rOff + (high + 1) * 2 + 1);
          }
          id &= 0x00FFFFFFu;
          if (id < d->numMaterials) reached[id] = 1;
        }
      }
      c->spectralGltfMats = c->spectralHeavyMats = false;
      uint typeMask = 0u; bool rich = false;                    // the reachable material types, for the choice between MODE 0 and MODE 7 (hpt_decl.h)
      for (uint i = 0; i < d->numMaterials; i++) {
        if (!reached[i]) continue;
        if (mm[i].mtype < 32u) typeMask |= 1u << mm[i].mtype;
        if (mm[i].mtype == MAT_TYPE_BLEND || mm[i].mtype == MAT_TYPE_PLASTIC || (mm[i].mtype != MAT_TYPE_LIGHT_SOURCE && mm[i].texid[1] != 0xFFFFFFFFu)) rich = true;
        if (mm[i].mtype == MAT_TYPE_GLTF) c->spectralGltfMats = true;
        if (mm[i].mtype == MAT_TYPE_GLASS || mm[i].mtype == MAT_TYPE_BLEND || (mm[i].mtype != MAT_TYPE_LIGHT_SOURCE && mm[i].texid[1] != 0xFFFFFFFFu)) c->spectralHeavyMats = true;   // (a reached blend: whatever its leaves are)
      }
      c->fewMaterialTypes = !rich && __builtin_popcount(typeMask) <= 3;
    }
    const LightRec* ll2 = (const LightRec*)d->lights;
    for (uint i = 0; i < d->numLights; i++) {
      if (d->specValues && !specIdOk(ll2[i].specId)) return c->fail(HPT_ERR_ARG, "light " + std::to_string(i) + " refers to a spectrum that does not exist");
    }
    for (int k2 = 0; k2 < 3; k2++) if (d->camResponseSpectrumId[k2] >= (int)d->numSpectra) return c->fail(HPT_ERR_ARG, "m_camResponseSpectrumId refers to a spectrum that does not exist");
    std::vector<float> sv(d->specValues ? std::vector<float>(d->specValues, d->specValues + d->numSpecValues) : std::vector<float>());
    if (sv.size() < WAVES) sv.resize(WAVES, 0.0f);             // (a spectrum id that stands for textures reads as offset 0 wherever a tabulated one is looked up)
    std::vector<float4> cie(std::max(d->numCieXYZ, 1u), make_float4(0, 0, 0, 0));
    for (uint i = 0; i < d->numCieXYZ && d->cieXYZ; i++) cie[i] = make_float4(d->cieXYZ[4 * i], d->cieXYZ[4 * i + 1], d->cieXYZ[4 * i + 2], d->cieXYZ[4 * i + 3]);
    HIPCHK(c, c->dSpecValues.upload(sv.data(), sv.size()));
    HIPCHK(c, c->dSpecOffsetSz.upload(so.data(), so.size()));
    HIPCHK(c, c->dCieXYZ.upload(cie.data(), cie.size()));
    S.specValues = c->dSpecValues.p; S.specOffsetSz = c->dSpecOffsetSz.p; S.cieXYZ = c->dCieXYZ.p;
    S.numCieXYZ = d->cieXYZ ? d->numCieXYZ : 0u; S.numSpectra = d->numSpectra;
    for (int k2 = 0; k2 < 3; k2++) S.camResponseSpectrumId[k2] = d->specValues ? d->camResponseSpectrumId[k2] : -1;
    S.camResponseType = d->camResponseType;
  }
  c->hLightGeom.resize(d->numLights);
  for (uint i = 0; i < d->numLights; i++) c->hLightGeom[i] = ((const LightRec*)d->lights)[i].geomType;
  c->hLightTex.resize(d->numLights);
  for (uint i = 0; i < d->numLights; i++) c->hLightTex[i] = ((const LightRec*)d->lights)[i].texId;
  // a new scene invalidates the environment ids of the previous UpdateMembersPlainData until the next one
  S.envTexId = S.envLightId = S.envCamBackId = 0xFFFFFFFFu; S.envEnableSam = 0;
  c->sceneUploaded = true; c->shadeTrisDirty = true;
  c->tSlots[T_PATH_TRACE][1] = c->tSlots[T_NAIVE][1] = c->tSlots[T_DR][1] = float(now_ms() - t0);   // host -> device time of the scene commit
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_upload_scene"); }

extern "C" int hpt_update_params(hpt_ctx* c, const hpt_params* p)
try {
  if (!c || !p) return HPT_ERR_ARG;
  if (p->spectralMode > 1) return c->fail(HPT_ERR_ARG, "bad spectral mode");
  if (p->spectralMode == 1 && !c->sceneUploaded) return c->fail(HPT_ERR_STATE, "UpdateMembersPlainData with m_spectral_mode before CommitDeviceData");
  if (p->spectralMode == 1 && !c->spectralOk) return c->fail(HPT_ERR_UNSUPPORTED, "spectral rendering: " + c->spectralWhyNot);
  if (p->spectralMode == 1 && p->envSpecIdPlus1 != 0u && p->envSpecIdPlus1 - 1u >= c->S.numSpectra) return c->fail(HPT_ERR_ARG, "m_envSpecId refers to a spectrum that does not exist");
  if (p->winWidth <= 0 || p->winHeight <= 0 || p->fbWidth <= 0 || p->fbHeight <= 0 || p->winWidth > 65535 || p->winHeight > 65535) return c->fail(HPT_ERR_ARG, "bad viewport");
  if (p->tileSize != 1 && p->tileSize != 2 && p->tileSize != 4 && p->tileSize != 8) return c->fail(HPT_ERR_ARG, "bad tile size");
  // kernel_PackXY tiles the window without a remainder (integrator_rt.cpp:13-31); SetViewport only ever picks a tile size that divides both
  // sides (integrator_pt.h:379-389). Anything else would index past W*H in PackXY and in every kernel that reads m_packedXY.
  if (p->winWidth % (int)p->tileSize != 0 || p->winHeight % (int)p->tileSize != 0)
    return c->fail(HPT_ERR_ARG, "tile size must divide the viewport's width and height (SetViewport falls back to 4 / 2 / 1, integrator_pt.h:379-389)");
  DevScene& S = c->S;
  std::memcpy(S.projInv, p->projInv, 64); std::memcpy(S.worldViewInv, p->worldViewInv, 64);
  S.winStartX = p->winStartX; S.winStartY = p->winStartY; S.winWidth = p->winWidth; S.winHeight = p->winHeight; S.fbWidth = p->fbWidth; S.fbHeight = p->fbHeight;
  S.traceDepth = p->traceDepth; S.integratorType = p->integratorType; S.renderLayer = p->renderLayer; S.tileSize = p->tileSize;
  S.exposureMult = p->exposureMult; S.camLensRadius = p->camLensRadius; S.camTargetDist = p->camTargetDist;
  S.spectralMode = p->spectralMode;
  S.envSpecId = p->envSpecIdPlus1 - 1u; S.envSpecMult = p->envSpecMult;   // (0 -> 0xFFFFFFFF: none)
  std::memcpy(S.camRespoceRGB, p->camRespoceRGB, 16); std::memcpy(S.envColor, p->envColor, 16);
  // the environment map (integrator_pt_scene.cpp:441-478): ids are checked against what CommitDeviceData uploaded
  if ((p->envTexId != 0xFFFFFFFFu || p->envCamBackId != 0xFFFFFFFFu || p->envLightId != 0xFFFFFFFFu) && !c->sceneUploaded)
    return c->fail(HPT_ERR_STATE, "UpdateMembersPlainData with an environment map before CommitDeviceData");
  if (p->envTexId != 0xFFFFFFFFu && p->envTexId >= c->hTextures.size()) return c->fail(HPT_ERR_ARG, "m_envTexId refers to a texture that does not exist");
  if (p->envCamBackId != 0xFFFFFFFFu && p->envCamBackId >= c->hTextures.size()) return c->fail(HPT_ERR_ARG, "m_envCamBackId refers to a texture that does not exist");
  if (p->envLightId != 0xFFFFFFFFu && (p->envLightId >= c->S.numLights || !c->envLightOk(p->envLightId))) return c->fail(HPT_ERR_ARG, "m_envLightId is not a LIGHT_GEOM_ENV light with a pdf table");
  if (p->envEnableSam != 0 && p->envLightId == 0xFFFFFFFFu) return c->fail(HPT_ERR_ARG, "m_envEnableSam without m_envLightId");
  S.envTexId = p->envTexId; S.envLightId = p->envLightId; S.envCamBackId = p->envCamBackId; S.envEnableSam = p->envEnableSam;
  std::memcpy(S.envSamRow0, p->envSamRow0, 16); std::memcpy(S.envSamRow1, p->envSamRow1, 16);
  c->paramsSet = true;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_update_params"); }

// SetLines / SetPhysSize + m_enableOpticSim (integrator_pt.h:353-362, integrator_pt_scene.cpp:714-720, 1078-1141): n = 0 switches it off
extern "C" int hpt_set_optics(hpt_ctx* c, const float* lines4, uint32_t n, float physSizeX, float physSizeY)
try {
  if (!c || (n && !lines4)) return HPT_ERR_ARG;
  if (n > 64) return c->fail(HPT_ERR_ARG, "SetLines: more than 64 lens interfaces");
  for (uint32_t i = 0; i < n; i++) if (!(lines4[4 * i + 3] >= 0.0f)) return c->fail(HPT_ERR_ARG, "SetLines: negative aperture radius");
  (void)hipSetDevice(c->device);
  std::vector<float4> l(std::max<uint32_t>(n, 1u), make_float4(0, 0, 0, 0));
  for (uint32_t i = 0; i < n; i++) l[i] = make_float4(lines4[4 * i], lines4[4 * i + 1], lines4[4 * i + 2], lines4[4 * i + 3]);
  HIPCHK(c, c->dLensLines.upload(l.data(), l.size()));
  c->S.lensLines = c->dLensLines.p; c->S.lensCount = n; c->S.physSize[0] = physSizeX; c->S.physSize[1] = physSizeY; c->S.padLens = 0;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_optics"); }

extern "C" int hpt_update_materials(hpt_ctx* c, size_t first, size_t count, const void* mats)
try {
  if (!c || !mats) return HPT_ERR_ARG;
  if (first + count > c->dMaterials.n) return c->fail(HPT_ERR_ARG, "Update_m_materials: range out of bounds");
  int rc = check_materials(c, (const MaterialRec*)mats, count, c->hTextures.size(), c->dMaterials.n, c->numArrays1f); if (rc) return rc;
  if (c->hMaterials.size() == c->dMaterials.n) {                                        // the blend graph of the table as it will be after the update
    std::vector<MaterialRec> hm(c->hMaterials);
    std::memcpy(hm.data() + first, mats, count * sizeof(MaterialRec));
    rc = check_blend_graph(c, hm); if (rc) return rc;
    c->hMaterials.swap(hm);
    film_scan(c);
  }
  if (!lean_materials((const MaterialRec*)mats, count)) c->leanMaterials = false;      // (an update can only widen the set of BSDFs in use)
  for (size_t i = 0; i < count; i++) {
    const MaterialRec& m = ((const MaterialRec*)mats)[i];
    if (m.mtype == MAT_TYPE_GLTF) c->spectralGltfMats = true;
    if (m.mtype == MAT_TYPE_GLASS || m.mtype == MAT_TYPE_BLEND || (m.mtype != MAT_TYPE_LIGHT_SOURCE && m.texid[1] != 0xFFFFFFFFu)) c->spectralHeavyMats = true;
  }
  c->fewMaterialTypes = false;                                 // (an update may bring in any type)
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(c->dMaterials.p + first, mats, count * sizeof(MaterialRec), hipMemcpyHostToDevice));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_update_materials"); }
extern "C" int hpt_update_lights(hpt_ctx* c, size_t first, size_t count, const void* lights)
try {
  if (!c || !lights) return HPT_ERR_ARG;
  if (first + count > c->S.numLights) return c->fail(HPT_ERR_ARG, "Update_m_lights: range out of bounds");
  int rc = check_lights(c, (const LightRec*)lights, count, c->hTextures.size(), c->numArrays1f); if (rc) return rc;
  for (size_t i = 0; i < count; i++) { c->hLightGeom[first + i] = ((const LightRec*)lights)[i].geomType; c->hLightTex[first + i] = ((const LightRec*)lights)[i].texId; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(c->dLights.p + first, lights, count * sizeof(LightRec), hipMemcpyHostToDevice));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_update_lights"); }

// Update_m_matIdOffsets (integrator_pt.h:470): m_matVertOffset changed on the host
extern "C" int hpt_update_mat_id_offsets(hpt_ctx* c, const uint32_t* mvo, size_t numGeoms)
try {
  if (!c || !mvo) return HPT_ERR_ARG;
  if (!c->sceneUploaded) return c->fail(HPT_ERR_STATE, "Update_m_matIdOffsets before CommitDeviceData");
  if (2 * numGeoms != c->dMatVertOffset.n) return c->fail(HPT_ERR_ARG, "Update_m_matIdOffsets: geometry count differs from the committed scene");
  const size_t numTris = c->dMatIdByPrim.n, numVerts = c->dVData.n / 8;
  for (size_t g = 0; g < numGeoms; g++) {                     // every mesh's range must stay inside the uploaded tables (the kernels index them unchecked)
    const size_t nt = g < c->geoms.size() ? c->geoms[g].idx.size() / 3 : 0;
    if (mvo[2 * g] > numTris || mvo[2 * g + 1] > numVerts || (size_t)mvo[2 * g] + nt > numTris)
      return c->fail(HPT_ERR_ARG, "Update_m_matIdOffsets: geometry " + std::to_string(g) + " reaches past the tables");
    for (size_t t = 3 * (size_t)mvo[2 * g]; t < 3 * ((size_t)mvo[2 * g] + nt) && t < c->hTriIndices.size(); t++)
      if ((size_t)c->hTriIndices[t] + mvo[2 * g + 1] >= numVerts)
        return c->fail(HPT_ERR_ARG, "Update_m_matIdOffsets: geometry " + std::to_string(g) + " reaches past the tables (vertex index)");
  }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(c->dMatVertOffset.p, mvo, 2 * numGeoms * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->shadeTrisDirty = true;                                   // the shading records were gathered through the old offsets
  // the meshes now point at other triangle ranges, i.e. at other materials: what a hit can REACH was scanned at hpt_upload_scene through the
  // old offsets, so the kernels chosen by it widen to the ones that hold every branch (a scope-0 spectral kernel has no glass branch)
  c->spectralGltfMats = c->spectralHeavyMats = true; c->fewMaterialTypes = false;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_update_mat_id_offsets"); }

extern "C" int hpt_pack_xy(hpt_ctx* c, uint32_t tidX, uint32_t tidY)
try {
  if (!c) return HPT_ERR_ARG;
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, "PackXYBlock before UpdateMembersPlainData");
  if ((int)tidX != c->S.winWidth || (int)tidY != c->S.winHeight) return c->fail(HPT_ERR_ARG, "PackXYBlock: size differs from the viewport");
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)tidX * tidY;
  if (c->S.tileSize == 0u || tidX % c->S.tileSize != 0u || tidY % c->S.tileSize != 0u) return c->fail(HPT_ERR_ARG, "PackXYBlock: tile size does not divide the viewport");
  HIPCHK(c, c->dPackedXY.alloc(n));
  HIPCHK(c, hipMemsetAsync(c->dPackedXY.p, 0, n * sizeof(uint), nullptr));
  packXYKernel<<<dim3((tidX + 15) / 16, (tidY + 15) / 16), dim3(16, 16), 0, 0>>>(c->dPackedXY.p, (int)tidX, (int)tidY, c->S.tileSize);
  HIPCHK(c, hipGetLastError());
  c->packedCount = (uint)n;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_pack_xy"); }
extern "C" int hpt_get_packed_xy(hpt_ctx* c, uint32_t* out, uint32_t count)
try {
  if (!c || !out || count > c->packedCount) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(out, c->dPackedXY.p, (size_t)count * 4, hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_packed_xy"); }
extern "C" int hpt_init_random_gens_from(hpt_ctx* c, uint32_t n, uint32_t firstSeed)
try {
  if (!c || n == 0) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, c->dGens.alloc(n));
  c->gensCount = n;
  initRandomGensKernel<<<dim3((n + 255) / 256), dim3(256), 0, 0>>>(c->dGens.p, n, firstSeed);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_init_random_gens_from"); }
extern "C" int hpt_init_random_gens(hpt_ctx* c, uint32_t n) try { return hpt_init_random_gens_from(c, n, 0u); }
catch (...) { return hptGuard(c, "hpt_init_random_gens"); }
extern "C" int hpt_get_random_gens(hpt_ctx* c, uint32_t* out, uint32_t count)
try {
  if (!c || !out || count > c->dGens.n) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(out, c->dGens.p, (size_t)count * 8, hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_random_gens"); }
extern "C" int hpt_set_random_gens(hpt_ctx* c, const uint32_t* in, uint32_t count)
try {
  if (!c || !in) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, c->dGens.alloc(count));
  c->gensCount = count;
  HIPCHK(c, hipMemcpy(c->dGens.p, in, (size_t)count * 8, hipMemcpyHostToDevice));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_random_gens"); }

// ---- the hot path -------------------------------------------------------------------------------------------------------------------
static int gridBlocks(hpt_ctx* c, bool dr, bool fullMaterials = false)
{
  int bpc = c->blocksPerCU;
  if (bpc <= 0) bpc = fullMaterials ? HPT_FULL_WAVES : 4;   // = the kernel's __launch_bounds__; measured for DR: 2 -> 185, 3 -> 206, 4 -> 259 Mpaths/s
  return c->numCUs * bpc;
}

// DEEP: the scene's BVH can need more than LDS_STACK stack entries, so pushes / pops check for the HBM overflow part
// FLAT: single-level world-space BVH (static scenes within FLAT_TRI_BUDGET) vs two-level TLAS/BLAS
template <bool STATS, bool DR, int NAIVE, bool SLICED = false, bool LGRAD = false, bool ENV = false, bool ADAPT = false>   // ADAPT: per-pixel pass counts and moments; LGRAD: PathTraceDR / PathTraceVJP with lights registered (hpt_put_diff_lights); ENV: over an environment map ("dr_environment")
static void launchPT(const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep)
{
  if (S.sweep) pathTraceKernel<STATS, DR, NAIVE, false, false, false, true, SLICED, LGRAD, ENV, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
  else if (S.flatMode) {
    if (deep) pathTraceKernel<STATS, DR, NAIVE, true, true, false, false, SLICED, LGRAD, ENV, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
    else      pathTraceKernel<STATS, DR, NAIVE, false, true, false, false, SLICED, LGRAD, ENV, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
  } else {
    if (deep) pathTraceKernel<STATS, DR, NAIVE, true, false, false, false, SLICED, LGRAD, ENV, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
    else      pathTraceKernel<STATS, DR, NAIVE, false, false, false, false, SLICED, LGRAD, ENV, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
  }
}

template <bool DR, bool LEAN, bool VJP = false>
static void launchBlock(const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep, uint refillBelow, uint nodeMin, bool wide = false)
{
  const dim3 g(blocks), b(256);
  if (wide && LEAN) { if (deep) pathTraceBlockKernel<DR, true, true, true, true, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockKernel<DR, true, false, true, true, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
  else if (S.flatMode) { if (deep) pathTraceBlockKernel<DR, LEAN, true, true, false, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockKernel<DR, LEAN, false, true, false, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
  else            { if (deep) pathTraceBlockKernel<DR, LEAN, true, false, false, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockKernel<DR, LEAN, false, false, false, VJP><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
}

template <int WIDE, bool ADAPT = false>                       // ADAPT: per-pixel pass counts and moments ("adaptive_spectral")
static void launchSpectral(const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep)
{
  const dim3 sg(blocks), sb(256);
  if (S.motion) {                                              // moving instances (never a sweep scene)
    if (S.flatMode) { if (deep) pathTraceSpectralKernel<true, true, false, true, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); else pathTraceSpectralKernel<false, true, false, true, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); }
    else            { if (deep) pathTraceSpectralKernel<true, false, false, true, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); else pathTraceSpectralKernel<false, false, false, true, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); }
  }
  else if (S.sweep)     pathTraceSpectralKernel<false, false, true, false, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job);
  else if (S.flatMode)  { if (deep) pathTraceSpectralKernel<true, true, false, false, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); else pathTraceSpectralKernel<false, true, false, false, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); }
  else                  { if (deep) pathTraceSpectralKernel<true, false, false, false, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); else pathTraceSpectralKernel<false, false, false, false, WIDE, ADAPT><<<sg, sb, 0, st>>>(S, job); }
}
template <bool ADAPT>
static void launchSpectralScope(int scope, const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep)
{
  if (scope == 3) launchSpectral<3, ADAPT>(S, job, blocks, st, deep);
  else if (scope == 2) launchSpectral<2, ADAPT>(S, job, blocks, st, deep); else if (scope == 1) launchSpectral<1, ADAPT>(S, job, blocks, st, deep); else launchSpectral<0, ADAPT>(S, job, blocks, st, deep);
}

template <int SCOPE>
static void launchSpectralBlock(const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep, bool wide, uint refillBelow, uint nodeMin)
{
  const dim3 g(blocks), b(256);
  if (wide)            { if (deep) pathTraceBlockSpectralKernel<true, true, true, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockSpectralKernel<false, true, true, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
  else if (S.flatMode) { if (deep) pathTraceBlockSpectralKernel<true, true, false, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockSpectralKernel<false, true, false, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
  else                 { if (deep) pathTraceBlockSpectralKernel<true, false, false, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); else pathTraceBlockSpectralKernel<false, false, false, SCOPE><<<g, b, 0, st>>>(S, job, refillBelow, nodeMin); }
}

// the MOTION variants: moving instances (two-level layout only), every BSDF branch
template <int MODE, bool SLICED = false, bool ADAPT = false>
static void launchPTMotion(const DevScene& S, const Job& job, int blocks, hipStream_t st, bool deep)
{
  if (S.flatMode) {
    if (deep) pathTraceKernel<false, false, MODE, true, true, true, false, SLICED, false, false, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
    else      pathTraceKernel<false, false, MODE, false, true, true, false, SLICED, false, false, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
  } else {
    if (deep) pathTraceKernel<false, false, MODE, true, false, true, false, SLICED, false, false, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
    else      pathTraceKernel<false, false, MODE, false, false, true, false, SLICED, false, false, ADAPT><<<dim3(blocks), dim3(256), 0, st>>>(S, job);
  }
}

// DevScene::shadeTris for this launch: gltf / emissive scenes on the single-level layout get one 64-byte record of shading data per triangle
// record (rebuilt on the device after a commit or a table upload); everything else leaves the pointer null and gathers through the index chain
static int ensureShadeTris(hpt_ctx* c, hipStream_t st)
{
  const bool want = c->shadeTrisEnabled && c->S.flatMode != 0u && c->S.motion == 0u && c->leanMaterials && !c->forceFull && c->S.lensCount == 0u &&
                    c->instTris > 0 && c->instTris < (size_t(1) << 28) && c->sceneUploaded && c->accelCommitted;
  if (!want) { c->S.shadeTris = nullptr; return HPT_OK; }
  if (c->shadeTrisDirty || c->dShadeTris.n < 4 * c->instTris) {
    HIPCHK(c, c->dShadeTris.alloc(4 * c->instTris));
    DevScene Sb = c->S; Sb.shadeTris = nullptr;
    const uint n = (uint)c->instTris;
    buildShadeTrisKernel<<<dim3((n + 255u) / 256u), dim3(256), 0, st>>>(Sb, n, c->dShadeTris.p);
    HIPCHK(c, hipGetLastError());
    c->shadeTrisDirty = false;
  }
  c->S.shadeTris = c->dShadeTris.p;
  return HPT_OK;
}

// ---- wavefront schedule ---------------------------------------------------------------------------------------------------------------
// Heavy scenes (HEAVY_SAH_VISITS) are rendered by the shade / trace kernel pair; on light ones the path state's trip through HBM costs more
// than the ray replacement gains (measured crossover: see DESIGN.md, "two schedules").
static const uint   WF_POOL_MAX = 1u << 22;        // pool slots (pixels in flight) per batch: 4M x 148 B = 620 MB
static const uint   WF_CHECK = 8;                  // progress word copied back every WF_CHECK shade passes
static const uint   WF_RING = 8;                   // ... and at most WF_RING such checkpoints in flight
static const uint   WF_GROUPS_AUTO = 1;            // pixel groups (streams) per call; measured 1M triangles: 1 -> 224, 2 -> 223, 3 -> 204 Mpaths/s

static bool useWavefront(hpt_ctx* c, bool naive, bool dr, bool stats, uint tidCount)
{
  if (naive || stats) return false;                // those variants exist as megakernels only
  if (c->schedule == 1 || c->schedule == 3) return false;
  if (c->schedule == 2) return true;                 // (4, where its kernel does not apply: the automatic choice)
  // ... and only for calls with enough pixels to keep the trace kernel's lanes supplied with replacement rays: measured on the 1M-triangle
  // scene (profiles/share.sh, 2.07 M / 1.04 M / 518 K / 259 K pixels per call): wavefront 226 / 199 / 162 / 108 vs megakernel 171 / 161 / 159 / 146 Mpaths/s
  return c->sahVisits >= HEAVY_SAH_VISITS && tidCount >= WF_AUTO_PIXELS;
}

static bool wfWide(const hpt_ctx* c) { return c->wideEnabled && c->S.flatMode != 0u && c->S.motion == 0u && c->nodes4Count != 0u; }
static uint wfStackNeeded(const hpt_ctx* c) { return std::max(std::max(c->stackNeeded, wfWide(c) ? c->stackNeeded4 : 0u), 1u); }   // entries a suspended ray may have to save

template <bool STATS>
static void launchWfTrace(hpt_ctx* c, const DevScene& S, const WfPool& P, uint iter, int blocks, hipStream_t st, bool deep, uint* ovf)
{
  const uint lanes = (uint)blocks * 256u; Counters* cn = c->dCounters.p;
  const uint grace = c->wfGrace;
  if (c->S.motion != 0u && !STATS) {                           // moving instances: the rays carry their path's time
    if (c->S.flatMode) {
      if (deep) wfTraceKernel<true, true, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
      else      wfTraceKernel<false, true, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    } else {
      if (deep) wfTraceKernel<true, false, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
      else      wfTraceKernel<false, false, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    }
    return;
  }
  if (wfWide(c)) {                                              // the 4-wide compressed tree (static single-level scenes)
    if (c->stackNeeded4 > (uint)LDS_STACK) wfTraceKernel<true, true, STATS, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    else                                   wfTraceKernel<false, true, STATS, false, true><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    return;
  }
  if (c->S.flatMode) {
    if (deep) wfTraceKernel<true, true, STATS><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    else      wfTraceKernel<false, true, STATS><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
  } else {
    if (deep) wfTraceKernel<true, false, STATS><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
    else      wfTraceKernel<false, false, STATS><<<dim3(blocks), dim3(256), 0, st>>>(S, P, iter, c->wfRefillBelow, grace, ovf, lanes, cn);
  }
}

// Environment maps in DR (hpt_set_option "dr_environment"): a DR call on a scene with a map or with env sampling runs the ENV
// kernels; the env plane of the adjoint record exists when a map one of the two lookups reads is registered (hpt_put_diff_tex2d).
static bool drEnvironmentCall(const hpt_ctx* c) { return c->drEnvironment && (c->S.envTexId != 0xFFFFFFFFu || c->S.envEnableSam != 0u); }
static bool drEnvMapRegistered(const hpt_ctx* c)
{
  const auto reg = [&](uint id) { return id < c->hTextures.size() && c->hTextures[id].diffOffset != ~0ull; };
  return reg(c->S.envTexId) || (c->S.envLightId < c->hLightTex.size() && reg(c->hLightTex[c->S.envLightId]));
}
// the textures an ENV kernel reads through texFetchAD: m_envTexId (the tail) and the texId of every light (the lookup along the shadow ray)
static bool drEnvReads(const hpt_ctx* c, uint texId)
{
  if (texId == 0xFFFFFFFFu) return false;
  if (texId == c->S.envTexId) return true;
  for (const uint t : c->hLightTex) if (t == texId) return true;
  return false;
}
// adaptMax: null, or the adaptive call's largest pass count (1 .. WF_MAX_PASSES, from the counts summary or the loop's bound): Job::passCounts /
// moments are set, the slots start with their own counts (wfInitCountsKernel) and the ADAPT shade kernels run
// qmc: null, or PathTraceBlockQMC's job ("qmc_wavefront"; hpt_path_trace_qmc_block_dev2 has made the refusals): the work items are the generator slots
// 0 .. job.tidCount, each starting with its own number of samples (wfInitQmcKernel), and wfShadeQmcKernel runs
static int launch_wavefront(hpt_ctx* c, const Job& job, hipStream_t st, bool dr, int specScope = -1, const uint* adaptMax = nullptr, const QmcJob* qmc = nullptr)   // specScope >= 0: spectral rendering (wfShadeSpecKernel<scope>)
{
  const bool adapt = adaptMax != nullptr;                       // (forward calls from the camera, RGB without thin films or spectral: adaptiveRefusal)
  const bool spec = specScope >= 0;
  const bool drEnv = dr && drEnvironmentCall(c);               // (launch_path_trace has made the refusals)
  const bool envPlane = drEnv && drEnvMapRegistered(c);
  DevScene Sw = c->S;
  if (spec || qmc) Sw.shadeTris = nullptr;           // the spectral and the QMC shade kernels fetch their surface through the primitive id: the trace pass must report that
  const uint passesMax = qmc ? (qmc->samples - 1u) / qmc->gensCount + 1u : (adapt ? *adaptMax : job.passNum);   // the largest pass count of a slot
  auto launchShade = [&](const dim3 sg, hipStream_t gs, const WfPool& P, const WfJob& wj) {
    if (qmc) {
      if (c->S.motion) wfShadeQmcKernel<true><<<sg, dim3(256), 0, gs>>>(Sw, P, wj, *qmc, job.packedCount);
      else             wfShadeQmcKernel<false><<<sg, dim3(256), 0, gs>>>(Sw, P, wj, *qmc, job.packedCount);
    }
    else if (spec && adapt) {
      if (specScope == 3) wfShadeSpecKernel<3, true><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
      else if (specScope == 2) wfShadeSpecKernel<2, true><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
      else wfShadeSpecKernel<1, true><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
    }
    else if (spec) {
      if (specScope == 3) wfShadeSpecKernel<3><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
      else if (specScope == 2) wfShadeSpecKernel<2><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
      else wfShadeSpecKernel<1><<<sg, dim3(256), 0, gs>>>(Sw, P, wj);
    }
    else if (adapt) {
      if (c->S.motion)         wfShadeKernel<false, false, true, false, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
      else if (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u) wfShadeKernel<false, true, false, false, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
      else                     wfShadeKernel<false, false, false, false, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    }
    else if (drEnv)            wfShadeKernel<true, true, false, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    else if (dr && wj.drLightCount != 0u) wfShadeKernel<true, true, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    else if (dr)               wfShadeKernel<true, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    else if (c->hasFilm)       { if (c->S.motion) wfShadeKernel<false, false, true, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj); else wfShadeKernel<false, false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj); }
    else if (c->S.motion)      wfShadeKernel<false, false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    else if (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u) wfShadeKernel<false, true><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
    else                       wfShadeKernel<false, false><<<sg, dim3(256), 0, gs>>>(c->S, P, wj);
  };
  // ---- groups: contiguous runs of work items, whole 256-item blocks each ----
  uint nGroups = c->wfGroupCount > 0 ? (uint)c->wfGroupCount : WF_GROUPS_AUTO;
  nGroups = std::max(nGroups, (job.tidCount + WF_POOL_MAX - 1) / WF_POOL_MAX);
  nGroups = std::min(nGroups, std::max(1u, job.tidCount / 4096u));             // tiny calls: one group
  nGroups = std::min(nGroups, 64u);
  const uint per = (((job.tidCount + nGroups - 1) / nGroups) + 255u) & ~255u;
  while (c->wfGroups.size() < nGroups) {
    hpt_ctx::WfGroup* g = new hpt_ctx::WfGroup();
    c->wfGroups.push_back(g);
    HIPCHK(c, hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    HIPCHK(c, hipHostMalloc((void**)&g->progress, WF_RING * sizeof(uint)));
    for (auto& e : g->ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
  }
  if (!c->wfFork) HIPCHK(c, hipEventCreateWithFlags(&c->wfFork, hipEventDisableTiming));

  int bpc = c->wfBlocksPerCU > 0 ? c->wfBlocksPerCU : HPT_WF_WAVES;
  const int traceBlocks = c->numCUs * bpc;
  // HBM part of the traversal stacks: one slice per group (their trace kernels run concurrently)
  HIPCHK(c, ensureStackOverflow(c, (size_t)traceBlocks * 256 * nGroups));
  if (c->stackWitness) HIPCHK(c, stackWitnessFill(c, st));          // (before wfFork is recorded on st: every group's stream waits for it)
  const size_t ovfPerGroup = c->dStackOvf.n / nGroups;
  const bool deep = c->stackNeeded > (uint)LDS_STACK;
  const bool stats = c->instrument;
  if (stats) { HIPCHK(c, c->dCounters.alloc(1)); HIPCHK(c, hipMemsetAsync(c->dCounters.p, 0, sizeof(Counters), st)); }

  WfJob wj;
  wj.tidBegin = job.tidBegin; wj.tidChunk = job.tidChunk; wj.tidStride = job.tidStride; wj.tidEnd = job.tidEnd;
  wj.passNum = job.passNum; wj.channels = job.channels; wj.outColor = job.outColor; wj.gens = job.gens; wj.packedXY = job.packedXY;
  wj.drSkipNonFinite = job.drSkipNonFinite;
  wj.refImg = job.refImg; wj.data = job.data; wj.grad = job.grad; wj.lossAccum = job.lossAccum; wj.record = nullptr;
  if (adapt) { wj.passCounts = job.passCounts; wj.moments = job.moments; }   // (the same storage in both structs: hpt_decl.h)
  wj.adjImg = job.adjImg; wj.vjp = job.vjp;
  const bool drLights = dr && c->diffLightCount != 0u;        // (launch_path_trace has checked the registration against the scene)
  wj.drLightFirst = drLights ? job.drLightFirst : 0u; wj.drLightCount = drLights ? job.drLightCount : 0u; wj.drLightOff = drLights ? job.drLightOff : 0u;
  if (drEnv) wj.drEnvPlaneOn = envPlane ? 1u : 0u;           // (shares drLightFirst's word: no light is registered then)
  // every path takes at most traceDepth shade passes after the one that generated it; the pass that ends it (or the next one, when a
  // shadow ray was outstanding) also generates the pixel's next path
  // safety net only (the loop ends when a round queues no ray): pixels whose rays were suspended sit rounds out, so there is no tight bound
  const unsigned long long iterCap = c->wfIterCap ? c->wfIterCap : 64ull * ((unsigned long long)passesMax * (c->S.traceDepth + 2ull) + 4ull);
  c->lastWfIters = 0;
  unsigned long long capLeft = 0;                  // rays still queued when a group ran into iterCap
  const bool drLoss = dr && job.vjp == 0u;                  // (PathTraceVJP computes no loss: the slots stay zero and are not reduced)
  if (drLoss) { HIPCHK(c, c->dLossAcc.alloc(1)); HIPCHK(c, hipMemsetAsync(c->dLossAcc.p, 0, sizeof(double), st)); }
  HIPCHK(c, hipEventRecord(c->ev0, st));
  HIPCHK(c, hipEventRecord(c->wfFork, st));

  std::vector<WfPool> pools(nGroups);
  uint live = 0;
  for (uint gi = 0; gi < nGroups; gi++) {
    hpt_ctx::WfGroup& g = *c->wfGroups[gi];
    g.itemBase = std::min(gi * per, job.tidCount); g.itemCount = std::min(per, job.tidCount - g.itemBase);
    g.it = 0; g.checkpoints = 0; g.finished = g.itemCount == 0;
    if (g.finished) continue;
    live++;
    for (int i = 0; i < 8; i++) HIPCHK(c, g.f4[i].alloc(g.itemCount));
    for (int i = 0; i < 3; i++) HIPCHK(c, g.u[i].alloc(g.itemCount));
    const size_t maxSusp = (size_t)traceBlocks * 256, suspWords = (WF_SUSP_WORDS + (size_t)wfStackNeeded(c)) * maxSusp;
    HIPCHK(c, g.u[3].alloc(2 * (size_t)g.itemCount + maxSusp)); HIPCHK(c, g.u[5].alloc(2 * (size_t)g.itemCount + maxSusp));
    HIPCHK(c, g.u[4].alloc(2 * WF_CTR_WORDS));
    HIPCHK(c, g.u[6].alloc(g.itemCount));
    HIPCHK(c, g.u[7].alloc(suspWords)); HIPCHK(c, g.u[8].alloc(suspWords));
    if (dr) { HIPCHK(c, g.rec.alloc((size_t)g.itemCount * REC_FIELDS * (c->S.traceDepth + 1) + (drLights ? drLightPlaneFloats(g.itemCount, c->S.traceDepth) : 0) +
                                        (envPlane ? drEnvPlaneFloats(g.itemCount, c->S.traceDepth) : 0))); HIPCHK(c, g.lossSlot.alloc(g.itemCount)); }
    if (c->S.motion) HIPCHK(c, g.time.alloc(g.itemCount));
    if (spec) { HIPCHK(c, g.waves.alloc(g.itemCount)); HIPCHK(c, g.fb.alloc(g.itemCount)); }
    WfPool& P = pools[gi];
    P.waves = spec ? g.waves.p : nullptr; P.fb = spec ? g.fb.p : nullptr;
    P.rayO = g.f4[0].p; P.rayD = g.f4[1].p; P.thr = g.f4[2].p; P.acc = g.f4[3].p;
    P.shO = g.f4[4].p; P.shD = g.f4[5].p; P.contrib = g.f4[6].p; P.hit = g.f4[7].p;
    P.hitInst = g.u[0].p; P.occl = g.u[1].p; P.lossSlot = dr ? g.lossSlot.p : nullptr; P.time = c->S.motion ? g.time.p : nullptr; P.status = g.u[2].p; P.rayQ[0] = g.u[3].p; P.rayQ[1] = g.u[5].p; P.ctr = g.u[4].p; P.inflight = g.u[6].p;
    P.susp[0] = g.u[7].p; P.susp[1] = g.u[8].p; P.maxSusp = (uint)maxSusp; P.suspStack = wfStackNeeded(c);
    HIPCHK(c, hipStreamWaitEvent(g.stream, c->wfFork, 0));
    HIPCHK(c, hipMemsetAsync(P.ctr, 0, 2 * WF_CTR_WORDS * sizeof(uint), g.stream));
    if (qmc) wfInitQmcKernel<<<dim3((g.itemCount + 255u) / 256u), dim3(256), 0, g.stream>>>(P, g.itemBase, g.itemCount, qmc->samples, qmc->gensCount);
    else if (adapt) { wj.itemBase = g.itemBase; wj.itemCount = g.itemCount; wfInitCountsKernel<<<dim3((g.itemCount + 255u) / 256u), dim3(256), 0, g.stream>>>(P, wj); }
    else wfInitKernel<<<dim3((g.itemCount + 255u) / 256u), dim3(256), 0, g.stream>>>(P, g.itemCount, job.passNum);
  }
  // ---- rounds: one shade + trace pass per live group, groups interleaved so that their kernels overlap on the device ----
  while (live > 0) {
    for (uint gi = 0; gi < nGroups; gi++) {
      hpt_ctx::WfGroup& g = *c->wfGroups[gi];
      if (g.finished) continue;
      const WfPool& P = pools[gi];
      wj.itemBase = g.itemBase; wj.itemCount = g.itemCount; wj.iter = (uint)g.it; wj.record = g.rec.p;
      const dim3 sg((g.itemCount + 255u) / 256u);
      launchShade(sg, g.stream, P, wj);
      if ((g.it % WF_CHECK) == WF_CHECK - 1) {
        const uint slot = g.checkpoints % WF_RING;
        if (g.checkpoints >= WF_RING) {                                     // oldest checkpoint of the ring: wait for it, then look at it
          HIPCHK(c, hipEventSynchronize(g.ev[slot]));
          if (g.progress[slot] == 0u) g.finished = true;
        }
        if (!g.finished) {
          HIPCHK(c, hipMemcpyAsync(&g.progress[slot], P.ctr + WF_CTR_WORDS * (wj.iter & 1u), sizeof(uint), hipMemcpyDeviceToHost, g.stream));
          HIPCHK(c, hipEventRecord(g.ev[slot], g.stream));
          g.checkpoints++;
          for (uint k = 1; k < WF_RING && k < g.checkpoints; k++) {         // newer checkpoints that have already landed
            const uint sl = (g.checkpoints - 1 - k) % WF_RING;
            if (hipEventQuery(g.ev[sl]) == hipSuccess && g.progress[sl] == 0u) { g.finished = true; break; }
          }
        }
      }
      if (!g.finished) {
        uint* ovf = c->dStackOvf.p + gi * ovfPerGroup;
        if (stats) launchWfTrace<true>(c, Sw, P, wj.iter, traceBlocks, g.stream, deep, ovf); else launchWfTrace<false>(c, Sw, P, wj.iter, traceBlocks, g.stream, deep, ovf);
        g.it++;
        if (gi == 0) c->lastWfIters++;
        if (g.it >= iterCap) {
          // The safety net tripped. One more shade pass tells whether anything is left: it queues a ray for every path still alive and the
          // rays the last trace pass suspended are already counted in the same word. Work left = an incomplete frame: say so.
          wj.iter = (uint)g.it;
          launchShade(sg, g.stream, P, wj);
          uint left = 0;
          HIPCHK(c, hipMemcpyAsync(&left, P.ctr + WF_CTR_WORDS * (wj.iter & 1u), sizeof(uint), hipMemcpyDeviceToHost, g.stream));
          HIPCHK(c, hipStreamSynchronize(g.stream));
          if (left != 0u) capLeft += left;
          g.finished = true;
        }
      }
      if (g.finished) {
        live--;
        if (drLoss) wfLossReduceKernel<<<dim3(std::min((g.itemCount + 255u) / 256u, 1024u)), dim3(256), 0, g.stream>>>(pools[gi].lossSlot, g.itemCount, c->dLossAcc.p);
        HIPCHK(c, hipEventRecord(g.done, g.stream));
        HIPCHK(c, hipStreamWaitEvent(st, g.done, 0));
      }
    }
    HIPCHK(c, hipGetLastError());
  }
  if (drLoss) wfLossFinishKernel<<<dim3(1), dim3(1), 0, st>>>(c->dLossAcc.p, job.lossAccum);
  HIPCHK(c, hipEventRecord(c->ev1, st));
  if (capLeft != 0ull)
    return c->fail(HPT_ERR_STATE, "wavefront schedule: stopped after " + std::to_string(iterCap) + " rounds with " + std::to_string(capLeft) +
                   " rays still queued - the frame is incomplete (render it with hpt_set_schedule(ctx, 1, ...) or hpt_set_option(\"wf_grace\", 0))");
  return HPT_OK;
}

// ---- schedule 4: block-owned streaming (hpt_stream.hip) -----------------------------------------------------------------------------------
static int launch_stream(hpt_ctx* c, const Job& job, hipStream_t st)
{
  while (c->wfGroups.size() < 1) {
    hpt_ctx::WfGroup* g = new hpt_ctx::WfGroup();
    c->wfGroups.push_back(g);
    HIPCHK(c, hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    HIPCHK(c, hipHostMalloc((void**)&g->progress, WF_RING * sizeof(uint)));
    for (auto& e : g->ev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
  }
  hpt_ctx::WfGroup& g = *c->wfGroups[0];
  const int bpc = c->wfBlocksPerCU > 0 ? c->wfBlocksPerCU : HPT_STREAM_WAVES;
  const uint blocks = (uint)std::max(1, std::min(c->numCUs * bpc, (int)((job.tidCount + 255u) / 256u)));
  uint spb = (job.tidCount + blocks - 1u) / blocks;
  spb = (spb + 255u) & ~255u;                                   // slots per block: whole 256-slot steps of the shade loop
  const uint n = job.tidCount;
  for (int i = 0; i < 8; i++) HIPCHK(c, g.f4[i].alloc(n));
  for (int i = 0; i < 3; i++) HIPCHK(c, g.u[i].alloc(n));
  HIPCHK(c, g.u[6].alloc(n));
  HIPCHK(c, g.u[3].alloc((size_t)blocks * 2u * spb));            // the blocks' ray queues
  WfPool P; std::memset(&P, 0, sizeof(P));
  P.rayO = g.f4[0].p; P.rayD = g.f4[1].p; P.thr = g.f4[2].p; P.acc = g.f4[3].p;
  P.shO = g.f4[4].p; P.shD = g.f4[5].p; P.contrib = g.f4[6].p; P.hit = g.f4[7].p;
  P.hitInst = g.u[0].p; P.occl = g.u[1].p; P.status = g.u[2].p; P.inflight = g.u[6].p;
  WfJob wj; std::memset(&wj, 0, sizeof(wj));
  wj.itemBase = 0; wj.itemCount = n; wj.tidBegin = job.tidBegin; wj.tidChunk = job.tidChunk; wj.tidStride = job.tidStride; wj.tidEnd = job.tidEnd;
  wj.passNum = job.passNum; wj.channels = job.channels; wj.outColor = job.outColor; wj.gens = job.gens; wj.packedXY = job.packedXY;
  const int rc = launchFrame(c, (size_t)blocks * 256, st, [&]() {
    wfInitKernel<<<dim3((n + 255u) / 256u), dim3(256), 0, st>>>(P, n, job.passNum);
    if (c->stackNeeded4 > (uint)LDS_STACK) streamKernel<true><<<dim3(blocks), dim3(256), 0, st>>>(c->S, P, wj, spb, c->wfRefillBelow, g.u[3].p, c->dStackOvf.p, blocks * 256u);
    else                                   streamKernel<false><<<dim3(blocks), dim3(256), 0, st>>>(c->S, P, wj, spb, c->wfRefillBelow, g.u[3].p, c->dStackOvf.p, blocks * 256u);
  });
  if (rc == HPT_OK) c->lastWfIters = 0;
  return rc;
}

// Pass slices: a lane of an earlier sliced launch gave up waiting for the slice before its own (Job::slicePollLimit). Called where the host
// has waited for that launch anyway, and before the next one; the word is sticky until it has been reported once.
static int sliceErrorCheck(hpt_ctx* c)
{
  if (!c->sliceError || *(volatile uint*)c->sliceError == 0u) return HPT_OK;
  *(volatile uint*)c->sliceError = 0u;
  return c->fail(HPT_ERR_STATE, "PathTraceBlock with pass slices: a lane waited for the slice before its own beyond the poll limit; the frame of that call is incomplete");
}

// Where wfShadeSpecKernel applies at all: PathTraceBlock from the camera on static, non-sweep scenes with a trace depth (no naive / input-ray /
// moving-instance variant: those keep their kernels). An adaptive call under "adaptive_wavefront" can take the wavefront form only where this holds.
static bool spectralWaveApplies(const hpt_ctx* c, bool naive, bool inRays)
{ return !inRays && !naive && c->S.motion == 0u && c->S.sweep == 0u && c->S.traceDepth > 0u && !c->instrument; }
// ... and whether any adaptive call of this context can be sent to the wavefront schedule (the 24-bit limit of the loop holds only there)
static bool adaptiveWaveReachable(hpt_ctx* c, uint tidCount)
{ return c->adaptiveWavefront && useWavefront(c, false, false, false, tidCount) && (c->S.spectralMode == 0u || spectralWaveApplies(c, false, false)); }

// Adaptive sampling serves forward RGB calls from the camera on the megakernel's ADAPT instantiations and, under "adaptive_wavefront", on the wavefront
// schedule's (wfShadeKernel<.., ADAPT>); under "adaptive_spectral" also contexts in spectral mode, thin films among them, on the ADAPT instantiations of
// pathTraceSpectralKernel and wfShadeSpecKernel - but not their wavelength layers (channels > 4), over which a moment has no definition. What has
// no kernel is refused by this one check, whichever form would run:
// launch_path_trace makes it for every adaptive call, and the loop makes it once more before it touches the caller's records.
static int adaptiveRefusal(hpt_ctx* c, bool naive, bool inRays, uint channels)
{
  const bool spec = c->S.spectralMode != 0u;
  const char* why = (spec && !c->adaptiveSpectral) ? "m_spectral_mode" : ((c->hasFilm && !spec) ? "scenes with thin films" : (naive ? "the naive integrator" :
                    (inRays ? "input rays" : (c->instrument ? "the instrumented probe" : ((spec && channels > 4u) ? "wavelength layers (channels > 4)" : nullptr)))));
  if (why) return c->fail(HPT_ERR_UNSUPPORTED, std::string("adaptive sampling (per-pixel pass counts): not served for ") + why + " (DESIGN.md 2.13)");
  return HPT_OK;
}

// The wavefront form of an adaptive call ("adaptive_wavefront") is chosen, sized and refused on three numbers of its counts. The
// loop knows them from its own plan; the bare counts entry has them counted on the device and reads the 12 bytes back on `st` - before anything
// of the caller's is written, and in a schedule that synchronises with the host throughout anyway (its progress ring).
static int adaptiveCountsSummary(hpt_ctx* c, const Job& job, hipStream_t st, WfCountsSummary& sum)
{
  if (job.passCounts == nullptr) { sum.maxCount = job.passNum; sum.active = job.passNum != 0u ? job.tidCount : 0u; sum.over = job.passNum > WF_MAX_PASSES ? 1u : 0u; return HPT_OK; }
  WfJob wj; std::memset(&wj, 0, sizeof(wj));
  wj.itemBase = 0u; wj.itemCount = job.tidCount; wj.tidBegin = job.tidBegin; wj.tidChunk = job.tidChunk; wj.tidStride = job.tidStride; wj.tidEnd = job.tidEnd;
  wj.passCounts = job.passCounts;
  HIPCHK(c, c->dAdSummary.alloc(1));
  HIPCHK(c, hipMemsetAsync(c->dAdSummary.p, 0, sizeof(WfCountsSummary), st));
  wfCountsSummaryKernel<<<dim3((job.tidCount + 255u) / 256u), dim3(256), 0, st>>>(wj, c->dAdSummary.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(&sum, c->dAdSummary.p, sizeof(WfCountsSummary), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return HPT_OK;
}

// Whether an adaptive call takes the wavefront form ("adaptive_wavefront"): where a PathTraceBlock of as many pixels as it has counts above 0 would. The
// counts are only looked at where the answer can be yes, i.e. where it is yes for the whole window.
static int adaptiveWaveChoice(hpt_ctx* c, const Job& job, hipStream_t st, const WfCountsSummary* known, WfCountsSummary& sum, bool& wave)
{
  wave = false;
  if (!c->adaptiveWavefront || !useWavefront(c, false, false, false, job.tidCount)) return HPT_OK;
  if (known) sum = *known; else if (int rc = adaptiveCountsSummary(c, job, st, sum)) return rc;
  wave = useWavefront(c, false, false, false, sum.active);
  return HPT_OK;
}
static int adaptiveOverRefusal(hpt_ctx* c, const WfCountsSummary& sum)     // (nothing of the caller's has been written: frame, generators and moments keep every bit)
{
  return c->fail(HPT_ERR_ARG, "adaptive sampling under the wavefront schedule: " + std::to_string(sum.over) + " pass count(s) above 16777215 (0xFFFFFF), all that a pool slot's "
                              "status word holds; split the call, or render it with hpt_set_option(\"adaptive_wavefront\", 0)");
}

// adapt: Job::passCounts / moments are set (the ADAPT kernels); adaptKnown: the loop's summary of its counts (null: counted here when it is needed)
static int launch_path_trace(hpt_ctx* c, Job& job, bool naive, bool dr, hipStream_t st, bool adapt = false, const WfCountsSummary* adaptKnown = nullptr)
{
  const bool inRays = job.inRayPos != nullptr;
  c->lastPassSlice = 0u;
  if (int rc = sliceErrorCheck(c)) return rc;
  if (adapt) { if (int rc = adaptiveRefusal(c, naive, inRays, job.channels)) return rc; }
  if (!c->sceneUploaded || !c->paramsSet) return c->fail(HPT_ERR_STATE, "PathTraceBlock before CommitDeviceData / UpdateMembersPlainData");
  if (!inRays && c->packedCount != (uint)(c->S.winWidth * c->S.winHeight)) return c->fail(HPT_ERR_STATE, "PathTraceBlock before PackXYBlock");
  job.tidStride = c->tidStride > 1 ? c->tidStride : 1u;
  job.tidChunk = (job.tidStride > 1 && c->tidChunk > 0) ? c->tidChunk : 0x40000000u;
  job.tidEnd = inRays ? job.tidBegin + job.tidCount : c->packedCount;
  if (inRays) { job.tidStride = 1; job.tidChunk = 0x40000000u; }
  if (!inRays && job.tidStride == 1 && (size_t)job.tidBegin + job.tidCount > c->packedCount) return c->fail(HPT_ERR_ARG, "PathTraceBlock: tid range exceeds the viewport");
  if (c->dGens.n < (inRays ? (size_t)job.tidEnd : (size_t)c->packedCount)) return c->fail(HPT_ERR_STATE, "PathTraceBlock: m_randomGens smaller than the thread range (InitRandomGens)");
  if (job.channels < 1 || (job.channels > 4 && c->S.spectralMode == 0u)) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlock: channels must be 1..4 (more are the wavelength layers of spectral rendering)");
  // two channels: kernel_ContributeToImage writes three components at pixel * channels (integrator_pt.cpp:636-641), i.e. into the next pixel and,
  // for the last one, past the buffer - refused rather than restated
  if (job.channels == 2) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlock: a two-channel framebuffer cannot hold the three components written per pixel (1, 3 or 4 channels)");
  if (dr && (c->S.traceDepth == 0 || c->S.traceDepth > 16)) return c->fail(HPT_ERR_ARG, "PathTraceDR: trace depth must be 1..16");
  if (dr && c->S.lensCount) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the lens simulation is not differentiated");
  if (dr && c->S.motion) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: motion blur is not differentiated");
  // the DR kernels add the constant m_envColor unweighted; the reference's replay evaluates EnvironmentColor() with the map and the
  // env-sampling MIS weight (integrator_dr.cpp:1077-1098): such scenes are refused rather than differentiated differently
  // hpt_set_option("dr_environment", 1) serves the map and its sampling (the ENV kernels); the replay has no back plate at all
  if (dr && !c->drEnvironment && (c->S.envTexId != 0xFFFFFFFFu || c->S.envEnableSam != 0u || c->S.envCamBackId != 0xFFFFFFFFu))
    return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: environment maps, their sampling and camera back plates are not differentiated (constant m_envColor only)");
  if (dr && c->S.envCamBackId != 0xFFFFFFFFu)
    return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: a camera back plate (m_envCamBackId) is not differentiated: the reference's replay has none");
  if (dr && !c->leanMaterials) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: gltf and emissive materials without normal maps only (what the reference's replay differentiates, integrator_dr.cpp:461-612)");
  // light-colour gradients (hpt_put_diff_lights): served by the megakernel and the wavefront schedule
  const bool drLights = dr && c->diffLightCount != 0u;
  if (drLights && (uint64_t)c->diffLightFirst + c->diffLightCount > c->S.numLights)
    return c->fail(HPT_ERR_ARG, "PathTraceDR: the scene has fewer lights than hpt_put_diff_lights registered");
  if (drLights && c->schedule == 3)
    return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the block-local schedule has no light-gradient variant (its kernel spills at four waves per SIMD as it is); hpt_set_schedule 0, 1 or 2");
  if (drLights && c->instrument) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the instrumented probe has no light-gradient variant");
  // environment maps: served by the megakernel and the wavefront schedule, and not together with registered lights (one more kernel cross product)
  const bool drEnv = dr && drEnvironmentCall(c);
  if (drEnv && drLights)
    return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the light-gradient variant has no environment-map form (hpt_put_diff_lights and an environment scene under dr_environment on one context)");
  if (drEnv && c->schedule == 3)
    return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the block-local schedule has no environment-map variant; hpt_set_schedule 0, 1 or 2");
  if (drEnv && c->instrument) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceDR: the instrumented probe has no environment-map variant");
  if (drEnv)                                                   // (the env sweep scatters rgb: a one-channel registration of a map it reads has no meaning)
    for (uint t = 0; t < (uint)c->hTextures.size(); t++)
      if (c->hTextures[t].diffOffset != ~0ull && c->hTextures[t].diffChannels != 4u && drEnvReads(c, t))
        return c->fail(HPT_ERR_ARG, "PathTraceDR: the environment map is registered with one channel (hpt_put_diff_tex2d: an environment map takes 4)");
  const bool drEnvPlane = drEnv && drEnvMapRegistered(c);
  // never more lanes than pixels: with fewer, the hardware's round-robin block placement spreads them evenly over the CUs, whereas a
  // full grid would let whichever waves ask first take all the work (a small multi-GPU share of a frame)
  if (c->S.spectralMode != 0u) {                               // four wavelengths per path: its own (plain) kernel
    if (dr) return c->fail(HPT_ERR_UNSUPPORTED, "spectral rendering: not the differentiable integrator");
    if (inRays && job.channels != 1u && job.channels != 4u) return c->fail(HPT_ERR_ARG, "PathTraceFromInputRays in spectral mode: 1 or 4 channels (kernel_CopyColorToOutput)");
    job.naive = naive ? 1u : 0u;
    if (c->hasFilm && !c->filmTablesSpectral) return c->fail(HPT_ERR_ARG, "thin film: m_precomp_thin_films was precomputed for RGB rendering (LoadScene sizes the tables by m_spectral_mode)");
    job.gens = c->dGens.p; job.packedXY = c->dPackedXY.p; job.packedCount = c->packedCount;
    // the scope the scene needs (hpt_spectral.hip: SCOPE): the narrowest instantiations that hold it
    bool heavy = c->S.lensCount != 0u || c->S.envTexId != 0xFFFFFFFFu || c->S.envCamBackId != 0xFFFFFFFFu || c->spectralHeavyMats;
    for (const uint g : c->hLightGeom) heavy = heavy || g == LIGHT_GEOM_ENV;
    const int scope = (heavy && c->fewMaterialTypes) ? 3 : (heavy ? 2 : (c->spectralGltfMats ? 1 : 0));
    // Schedule: scenes whose rays walk a real tree (SAH estimate >= 8: the reference's spectral fixture, interiors) run the block-local kernel -
    // persistent blocks on the work queue, rays repacked per block, the 4-wide tree on heavy scenes; the others, input-ray batches, moving
    // instances and sweep scenes keep the one-thread-per-pixel kernel. hpt_set_schedule(1) / (3) force either.
    const bool specBlock = !adapt && !inRays && c->S.motion == 0u && c->S.sweep == 0u && (c->S.traceDepth > 0u || naive) &&
                           (c->schedule == 3 || (c->schedule == 0 && c->sahVisits >= BLOCK_SAH_VISITS));
    // ... and heavy scenes in calls with enough pixels the wavefront schedule (wfShadeSpecKernel + the shared trace kernel), as their RGB rendering does
    // An adaptive call ("adaptive_spectral") keeps the one-thread-per-pixel kernel unless "adaptive_wavefront" sends it to the wavefront schedule under the
    // RGB form's rule (adaptiveWaveChoice), where wfShadeSpecKernel applies at all
    const bool specWaveApplies = spectralWaveApplies(c, naive, inRays);
    WfCountsSummary adSum = { 0u, 0u, 0u };
    bool adaptWave = false;
    if (adapt && specWaveApplies) { if (int rc = adaptiveWaveChoice(c, job, st, adaptKnown, adSum, adaptWave)) return rc; }
    const bool specWave = adapt ? adaptWave : (specWaveApplies &&
                          (c->schedule == 2 || (c->schedule == 0 && c->sahVisits >= HEAVY_SAH_VISITS && job.tidCount >= WF_AUTO_PIXELS)));
    if (specWave) {
      if (adapt && adSum.over != 0u) return adaptiveOverRefusal(c, adSum);
      c->lastSchedule = 2; c->lastWide = wfWide(c) ? 1u : 0u; c->lastDeep = (c->lastWide ? c->stackNeeded4 : c->stackNeeded) > (uint)LDS_STACK ? 1u : 0u; c->lastShadeRecords = 0u;
      if (adapt && adSum.maxCount == 0u) {                      // every count is 0: no round, nothing written
        c->lastWfIters = 0;
        HIPCHK(c, hipEventRecord(c->ev0, st)); HIPCHK(c, hipEventRecord(c->ev1, st));
        return HPT_OK;
      }
      return launch_wavefront(c, job, st, false, scope == 0 ? 1 : scope, adapt ? &adSum.maxCount : nullptr);
    }
    if (specBlock) {
      const bool bwide = c->S.megaWide != 0u && c->S.flatMode != 0u && c->nodes4Count != 0u;
      const bool bdeep = (bwide ? std::max(c->stackNeeded, c->stackNeeded4) : c->stackNeeded) > (uint)LDS_STACK;
      const int bpc = c->blocksPerCU > 0 ? c->blocksPerCU : (scope == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES);
      const int blocks = (int)std::min<size_t>((size_t)c->numCUs * bpc, ((size_t)job.tidCount + 255) / 256);
      HIPCHK(c, c->dQueue.alloc(1));
      HIPCHK(c, hipMemsetAsync(c->dQueue.p, 0, 4, st));
      job.queue = c->dQueue.p;
      const uint bNodeMin = bwide ? std::max(c->bwNodeMin, 16u) : c->bwNodeMin;
      return launchFrame(c, (size_t)blocks * 256, st, [&]() {
        c->lastSchedule = 3; c->lastWide = bwide ? 1u : 0u; c->lastDeep = bdeep ? 1u : 0u; c->lastShadeRecords = 0u;
        job.stackOverflow = c->dStackOvf.p; job.gridLanes = (uint)blocks * 256u;
        if (scope == 3) launchSpectralBlock<3>(c->S, job, blocks, st, bdeep, bwide, c->bwRefillBelow, bNodeMin);
        else if (scope == 2) launchSpectralBlock<2>(c->S, job, blocks, st, bdeep, bwide, c->bwRefillBelow, bNodeMin);
        else if (scope == 1) launchSpectralBlock<1>(c->S, job, blocks, st, bdeep, bwide, c->bwRefillBelow, bNodeMin);
        else launchSpectralBlock<0>(c->S, job, blocks, st, bdeep, bwide, c->bwRefillBelow, bNodeMin);
      });
    }
    const int sblocks = (int)(((size_t)job.tidCount + 255) / 256);
    const bool sdeep = megaStackNeeded(c) > (uint)LDS_STACK;
    return launchFrame(c, (size_t)sblocks * 256, st, [&]() {
      c->lastSchedule = 1; c->lastWide = (c->S.megaWide != 0u && c->S.flatMode != 0u && c->nodes4Count != 0u && c->S.motion == 0u) ? 1u : 0u; c->lastDeep = sdeep ? 1u : 0u; c->lastShadeRecords = 0u;
      job.stackOverflow = c->dStackOvf.p; job.gridLanes = (uint)sblocks * 256u;
      if (adapt) launchSpectralScope<true>(scope, c->S, job, sblocks, st, sdeep); else launchSpectralScope<false>(scope, c->S, job, sblocks, st, sdeep);
    });
  }
  { const int rcS = ensureShadeTris(c, st); if (rcS != HPT_OK) return rcS; }
  const bool motion = c->S.motion != 0;
  const bool film = c->hasFilm;                                // MODE 4 / 5 / 6 kernels, wfShadeKernel<.., FILM>
  if (film && !c->filmTablesRGB) return c->fail(HPT_ERR_ARG, "thin film: m_precomp_thin_films holds no RGB table for a film (LoadScene precomputes every film in RGB mode, sized by its thickness map)");
  if (film && c->instrument && !dr) return c->fail(HPT_ERR_UNSUPPORTED, "thin films: the instrumented probe has no film variant");
  const bool fullMaterials = film || motion || !dr && !(c->leanMaterials && !c->forceFull && c->S.lensCount == 0u && !naive && !inRays && !(c->instrument && !dr));   // MODE 0 / 1 / 2 / STATS kernels
  // MODE 7: the kernel with every BSDF branch built for one more wave per SIMD, for scenes with few material types (hpt_decl.h)
  const bool mode7 = fullMaterials && c->fewMaterialTypes && !c->forceFull && !film && !motion && !dr && !inRays && !naive && !(c->instrument && !dr);
  // Pass slices: the forward megakernel only (PathTraceDR's per-lane loss sum would change its summation order across items; input rays keep
  // one item per ray), and not its instrumented probe nor the block-local schedule, which have their own loops. The slice doubles until the
  // item count fits the queue's 32-bit head with room for every lane's last draw.
  const bool stats = c->instrument;                            // (the DR probe exists as a megakernel only: hpt_kernels.hip, group 15)
  const bool streamCall = !adapt && c->schedule == 4 && !inRays && !naive && !dr && !stats && !motion && !film && c->leanMaterials && !c->forceFull && c->S.lensCount == 0u && wfWide(c) && c->S.traceDepth > 0u;
  // An adaptive call stays on the megakernel unless "adaptive_wavefront" is set; then it goes where a PathTraceBlock of as many pixels as it has
  // counts above 0 would (under schedule 4, whose kernel does not serve it, the automatic rule): adaptiveWaveChoice.
  WfCountsSummary adSum = { 0u, 0u, 0u };
  bool adaptWave = false;
  if (adapt) { if (int rc = adaptiveWaveChoice(c, job, st, adaptKnown, adSum, adaptWave)) return rc; }
  const bool waveCall = adapt ? adaptWave : (!streamCall && !inRays && useWavefront(c, naive, dr, stats && c->schedule != 2, job.tidCount));
  // schedule 3: the megakernel with block-local ray repacking (hpt_block.hip) - PathTrace and PathTraceDR on the BVH2 of either layout
  // automatic: gltf / emissive scenes (and PathTraceDR) whose rays walk a real tree - the test_228 class (SAH estimate 10: 696 -> 735 Mpaths/s at 1024^2,
  // 527 -> 630 at 512^2, PathTraceDR 428 -> 453) and heavy scenes in calls too small for the wavefront schedule (1 M triangles at 640 x 360: 145 -> 160);
  // the light fixtures with every BSDF branch stay on the plain megakernel (typed_materials, estimate 4.8: 1186 vs 1133) - profiles/bw_check.py, bw_heavy.py
  const bool bwLean = dr || (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u);
  const bool bwAuto = c->schedule == 0 && bwLean && c->sahVisits >= BLOCK_SAH_VISITS && !drLights && !drEnv;   // (no block-local kernel with light gradients or environment maps)
  const bool blockLocal = !adapt && (c->schedule == 3 || bwAuto) && !naive && !inRays && !motion && !film && !stats && c->S.sweep == 0u;
  const size_t fullGrid = (size_t)gridBlocks(c, dr, fullMaterials && !mode7) * 256;
  const uint sliceWanted = c->passSlice >= 0 ? (uint)c->passSlice : passSliceAuto(job.tidCount, fullGrid, job.passNum);
  uint slice = (adapt || dr || inRays || naive || film || stats || blockLocal || streamCall || waveCall) ? 0u : sliceWanted;   // (adaptive calls: whole pixels)
  while (slice != 0u && (uint64_t)job.tidCount * passSliceCount(job.passNum, slice) > (1ull << 31)) slice *= 2u;
  if (slice >= job.passNum) slice = 0u;                           // one item per pixel either way: the plain form
  const size_t items = (size_t)job.tidCount * passSliceCount(job.passNum, slice);
  const int blocks = (int)std::min<size_t>((size_t)gridBlocks(c, dr, fullMaterials && !mode7), (items + 255) / 256);
  HIPCHK(c, c->dQueue.alloc(1));
  HIPCHK(c, hipMemsetAsync(c->dQueue.p, 0, 4, st));
  job.queue = c->dQueue.p;
  if (slice != 0u) {                                           // (the slice fields share storage with PathTraceDR's: hpt_decl.h)
    job.passSlice = slice;
    if (!c->sliceError) { HIPCHK(c, hipHostMalloc((void**)&c->sliceError, sizeof(uint), hipHostMallocMapped)); *c->sliceError = 0u; }
    HIPCHK(c, c->dSliceMail.alloc((size_t)job.tidEnd * SLICE_MAIL_WORDS));
    HIPCHK(c, hipMemsetAsync(c->dSliceMail.p, 0, (size_t)job.tidEnd * SLICE_MAIL_WORDS * sizeof(unsigned long long), st));   // tag 0: empty, so no tag of an earlier call is ever taken
    job.sliceMail = c->dSliceMail.p; job.sliceError = c->sliceError;
    // A waiting lane polls once per trip of its wave, or once per sleep (>= one trip's time) when the whole wave waits. What it waits for is at
    // most the pixel's earlier passes, each at most traceDepth + 2 trips: 64 times that, and never less than 2^20 polls.
    job.slicePollLimit = (uint)std::min<uint64_t>(0x7FFFFFFFull, std::max<uint64_t>(1ull << 20, 64ull * job.passNum * (c->S.traceDepth + 2u)));
  }
  job.gens = c->dGens.p; job.packedXY = c->dPackedXY.p; job.packedCount = c->packedCount;
  job.counters = nullptr;
  job.drSkipNonFinite = c->drSkipNonFinite ? 1u : 0u;
  if (drLights) { job.drLightFirst = c->diffLightFirst; job.drLightCount = c->diffLightCount; job.drLightOff = (uint)c->diffLightOff; job.drLightPad = 0u; }   // (share the input-ray pointers' storage)
  if (drEnv) { job.drEnvPad = 0u; job.drEnvPlaneOn = drEnvPlane ? 1u : 0u; }
  c->lastSchedule = 1;
  c->lastShadeRecords = c->S.shadeTris != nullptr ? 1u : 0u;
  // schedule 4 (experimental, never chosen automatically): the block-owned streaming form of the wavefront schedule - heavy static scenes with gltf / emissive materials
  if (streamCall) {
    c->lastSchedule = 4; c->lastWide = 1u; c->lastDeep = c->stackNeeded4 > (uint)LDS_STACK ? 1u : 0u;
    return launch_stream(c, job, st);
  }
  if (waveCall) {
    if (adapt && adSum.over != 0u) return adaptiveOverRefusal(c, adSum);
    c->lastSchedule = 2; c->lastWide = (wfWide(c) && !c->instrument) ? 1u : 0u; c->lastDeep = (c->lastWide ? c->stackNeeded4 : c->stackNeeded) > (uint)LDS_STACK ? 1u : 0u;
    if (adapt && adSum.maxCount == 0u) {                        // every count is 0: no round, nothing written
      c->lastWfIters = 0;
      HIPCHK(c, hipEventRecord(c->ev0, st)); HIPCHK(c, hipEventRecord(c->ev1, st));
      return HPT_OK;
    }
    return launch_wavefront(c, job, st, dr, -1, adapt ? &adSum.maxCount : nullptr);
  }
  c->lastWide = (!stats && !motion && (HPT_FLAT_WIDE || c->S.megaWide != 0u) && c->S.flatMode != 0u && c->nodes4Count != 0u) ? 1u : 0u;
  c->lastDeep = megaStackNeeded(c) > (uint)LDS_STACK ? 1u : 0u;
  if (stats) { HIPCHK(c, c->dCounters.alloc(1)); HIPCHK(c, hipMemsetAsync(c->dCounters.p, 0, sizeof(Counters), st)); job.counters = c->dCounters.p; }
  if (dr) {
    job.recordLanes = (uint)blocks * 256u;
    HIPCHK(c, c->dRecord.alloc((size_t)job.recordLanes * REC_FIELDS * (c->S.traceDepth + 1) + (drLights ? drLightPlaneFloats(job.recordLanes, c->S.traceDepth) : 0) +
                                (drEnvPlane ? drEnvPlaneFloats(job.recordLanes, c->S.traceDepth) : 0)));
    job.record = c->dRecord.p;
  }
  c->lastPassSlice = slice;
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    job.stackOverflow = c->dStackOvf.p; job.gridLanes = (uint)blocks * 256u;
    const bool deep = megaStackNeeded(c) > (uint)LDS_STACK;
    if (blockLocal) {
      const bool lean = dr || (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u);
      const bool bwide = lean && (c->bwWide == 1 || (c->bwWide < 0 && c->S.megaWide != 0u)) && c->S.flatMode != 0u && c->nodes4Count != 0u && c->wideEnabled;      // heavy scenes: the 4-wide compressed tree, as the megakernel walks it
      const bool bdeep = (bwide ? std::max(c->stackNeeded, c->stackNeeded4) : c->stackNeeded) > (uint)LDS_STACK;
      const uint bNodeMin = bwide ? std::max(c->bwNodeMin, 16u) : c->bwNodeMin;                           // (a 4-wide visit is three times the work: the vote pays earlier)
      c->lastSchedule = 3; c->lastWide = bwide ? 1u : 0u; c->lastDeep = bdeep ? 1u : 0u;
      if (dr && job.vjp != 0u) launchBlock<true, true, true>(c->S, job, blocks, st, bdeep, c->bwRefillBelow, bNodeMin, bwide);   // (a template parameter in this kernel: hpt_decl.h)
      else if (dr) launchBlock<true, true>(c->S, job, blocks, st, bdeep, c->bwRefillBelow, bNodeMin, bwide);
      else if (lean) launchBlock<false, true>(c->S, job, blocks, st, bdeep, c->bwRefillBelow, bNodeMin, bwide);
      else launchBlock<false, false>(c->S, job, std::min(blocks, c->numCUs * (c->blocksPerCU > 0 ? c->blocksPerCU : HPT_BW_FULL_WAVES)), st, bdeep, c->bwRefillBelow, c->bwNodeMin);
    }
    else if (motion && film) {
      if (inRays) launchPTMotion<6>(c->S, job, blocks, st, deep); else if (naive) launchPTMotion<5>(c->S, job, blocks, st, deep); else launchPTMotion<4>(c->S, job, blocks, st, deep);
    }
    else if (motion) {
      if (inRays) launchPTMotion<2>(c->S, job, blocks, st, deep); else if (naive) launchPTMotion<1>(c->S, job, blocks, st, deep);
      else if (adapt) launchPTMotion<0, false, true>(c->S, job, blocks, st, deep);
      else if (slice != 0u) launchPTMotion<0, true>(c->S, job, blocks, st, deep); else launchPTMotion<0>(c->S, job, blocks, st, deep);
    }
    else if (dr) {
      // the DR kernel's waves are emptier than the forward kernel's (lane utilisation 0.25), so leaving the inner-node loop when fewer than four
      // lanes still walk pays even on light scenes: test_228 class 346 -> 364 Mpaths/s (forward: 698 -> 699; profiles/vote_medium.sh)
      DevScene Sd = c->S;
      if (c->nodeMinOverride < 0 && Sd.nodeMin < 4u) Sd.nodeMin = 4u;
      if (stats) {                                                 // the counting probe follows the walk an uninstrumented call would do (see the forward probe below)
        Sd.statsWide = (wfWide(c) && (c->statsWide || useWavefront(c, naive, dr, false, job.tidCount))) ? 1u : 0u;
        launchPT<true, true, 0>(Sd, job, blocks, st, deep || (Sd.statsWide && c->stackNeeded4 > (uint)LDS_STACK));
      } else if (drLights) launchPT<false, true, 0, false, true>(Sd, job, blocks, st, deep);
      else if (drEnv) launchPT<false, true, 0, false, false, true>(Sd, job, blocks, st, deep);
      else launchPT<false, true, 0>(Sd, job, blocks, st, deep);
    }
    else if (film) {
      if (inRays) launchPT<false, false, 6>(c->S, job, blocks, st, deep); else if (naive) launchPT<false, false, 5>(c->S, job, blocks, st, deep); else launchPT<false, false, 4>(c->S, job, blocks, st, deep);
    }
    else if (inRays) launchPT<false, false, 2>(c->S, job, blocks, st, deep);
    else if (naive)  launchPT<false, false, 1>(c->S, job, blocks, st, deep);
    else if (stats) {
      // the counting probe follows the walk an uninstrumented call would do: where that is the wavefront trace kernel on the 4-wide tree, the
      // probe's single-level traversal walks that tree too (node visits = 64-byte lines of the tree actually used)
      DevScene Sp = c->S;
      Sp.statsWide = (wfWide(c) && (c->statsWide || useWavefront(c, naive, dr, false, job.tidCount))) ? 1u : 0u;   // "stats_wide": the caller says the measured call ran there
      launchPT<true, false, 0>(Sp, job, blocks, st, deep || (Sp.statsWide && c->stackNeeded4 > (uint)LDS_STACK));
    }
    else if (adapt) {
      if (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u) launchPT<false, false, 3, false, false, false, true>(c->S, job, blocks, st, deep);
      else if (mode7) launchPT<false, false, 7, false, false, false, true>(c->S, job, blocks, st, deep);
      else launchPT<false, false, 0, false, false, false, true>(c->S, job, blocks, st, deep);
    }
    else if (c->leanMaterials && !c->forceFull && c->S.lensCount == 0u) { if (slice != 0u) launchPT<false, false, 3, true>(c->S, job, blocks, st, deep); else launchPT<false, false, 3>(c->S, job, blocks, st, deep); }
    else if (mode7)  { if (slice != 0u) launchPT<false, false, 7, true>(c->S, job, blocks, st, deep); else launchPT<false, false, 7>(c->S, job, blocks, st, deep); }
    else             { if (slice != 0u) launchPT<false, false, 0, true>(c->S, job, blocks, st, deep); else launchPT<false, false, 0>(c->S, job, blocks, st, deep); }
  });
}

extern "C" int hpt_path_trace_block_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, uint32_t passNum, int naive, void* stream)
try {
  if (!c || !outDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (tidCount == 0 || passNum == 0) return HPT_OK;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidBegin = tidBegin; job.tidCount = tidCount; job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  return launch_path_trace(c, job, naive != 0, false, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_path_trace_block_dev"); }

// The round trip of the host-pointer entry points: up() copies the caller's buffers to the device, launch() runs the device-pointer form,
// down() copies the results back; each returns an HPT_ code. The kernel time is the event pair the device-pointer form recorded; it goes to
// hpt_last_kernel_ms and, with the copy times, to the four GetExecutionTime slots: kernel, copy in, copy out, overhead (main.cpp:417-419).
enum KernelTime { KERNEL_EVENTS,       // read the event pair
                  KERNEL_NONE,         // nothing was launched (a zero-size call that still makes its copies): the kernel time is 0
                  KERNEL_UNTIMED };    // the device-pointer form records no events: hpt_last_kernel_ms and the slots stay as they are
template <class Up, class Launch, class Down>
static int roundTrip(hpt_ctx* c, float* slots, KernelTime kt, Up up, Launch launch, Down down)
{
  const double t0 = now_ms();
  if (int rc = up()) return rc;
  const double t1 = now_ms();
  if (int rc = launch()) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  if (int rc = sliceErrorCheck(c)) return rc;
  const double t2 = now_ms();
  if (int rc = down()) return rc;
  const double t3 = now_ms();
  if (kt == KERNEL_UNTIMED) return HPT_OK;
  float kms = 0.0f;
  if (kt == KERNEL_EVENTS) (void)hipEventElapsedTime(&kms, c->ev0, c->ev1);
  c->lastKernelMs = kms;
  if (slots) { slots[0] = kms; slots[1] = float(t1 - t0); slots[2] = float(t3 - t2); slots[3] = float((t2 - t1) - kms); }
  return HPT_OK;
}
// ... with one call-local device copy of one host buffer of n elements: up (unless `upload` is false: every element is written), launch(device pointer), down
template <class T, class Launch>
static int roundTrip(hpt_ctx* c, float* slots, T* host, size_t n, bool upload, Launch launch)
{
  DevBuf<T> d;
  return roundTrip(c, slots, KERNEL_EVENTS,
                   [&]() -> int { HIPCHK(c, d.alloc(n)); if (upload) HIPCHK(c, hipMemcpy(d.p, host, n * sizeof(T), hipMemcpyHostToDevice)); return HPT_OK; },
                   [&]() -> int { return launch(d.p); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(host, d.p, n * sizeof(T), hipMemcpyDeviceToHost)); return HPT_OK; });
}

static int path_trace_host(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum, int naive)
{
  if (!c || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, "PathTraceBlock before UpdateMembersPlainData");
  const size_t n = (size_t)c->S.winWidth * c->S.winHeight * channels;
  return roundTrip(c, naive ? c->tSlots[T_NAIVE] : c->tSlots[T_PATH_TRACE], (tidCount && passNum) ? KERNEL_EVENTS : KERNEL_NONE,
                   [&]() -> int { HIPCHK(c, c->dFrame.alloc(n)); HIPCHK(c, hipMemcpy(c->dFrame.p, out, n * 4, hipMemcpyHostToDevice)); return HPT_OK; },   // the callee ACCUMULATES into the caller's buffer
                   [&]() -> int { return hpt_path_trace_block_dev(c, tidBegin, tidCount, channels, c->dFrame.p, passNum, naive, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, c->dFrame.p, n * 4, hipMemcpyDeviceToHost)); return HPT_OK; });
}

// PathTraceFromInputRaysBlock (integrator_pt.h:261, integrator_pt_host.cpp:92-103): device and host-pointer forms
extern "C" int hpt_path_trace_from_input_rays_block_dev(hpt_ctx* c, uint32_t tid, uint32_t channels, const float* rayPosDev, const float* rayDirDev, float* outDev, uint32_t passNum, void* stream)
try {
  if (!c || !rayPosDev || !rayDirDev || !outDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (tid == 0 || passNum == 0) return HPT_OK;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidBegin = 0; job.tidCount = tid; job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  job.inRayPos = (const float4*)rayPosDev; job.inRayDir = (const float4*)rayDirDev;
  return launch_path_trace(c, job, false, false, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_path_trace_from_input_rays_block_dev"); }
extern "C" int hpt_path_trace_from_input_rays_block(hpt_ctx* c, uint32_t tid, uint32_t channels, const float* rayPos, const float* rayDir, float* out, uint32_t passNum)
try {
  if (!c || !rayPos || !rayDir || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (tid == 0 || passNum == 0) return HPT_OK;
  DevBuf<float> dp, dd, dout;
  const size_t n = (size_t)tid * channels;
  return roundTrip(c, c->tSlots[T_FROM_RAYS], KERNEL_EVENTS,                        // fromRaysPtTime (integrator_pt_host.cpp:92-103) in GetExecutionTime's four slots
                   [&]() -> int { HIPCHK(c, dp.upload(rayPos, (size_t)tid * 4)); HIPCHK(c, dd.upload(rayDir, (size_t)tid * 4)); HIPCHK(c, dout.upload(out, n)); return HPT_OK; },
                   [&]() -> int { return hpt_path_trace_from_input_rays_block_dev(c, tid, channels, dp.p, dd.p, dout.p, passNum, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, dout.p, n * sizeof(float), hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_path_trace_from_input_rays_block"); }

extern "C" int hpt_path_trace_block(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum)
try { return path_trace_host(c, tidBegin, tidCount, channels, out, passNum, 0); }
catch (...) { return hptGuard(c, "hpt_path_trace_block"); }
extern "C" int hpt_naive_path_trace_block(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum)
try { return path_trace_host(c, tidBegin, tidCount, channels, out, passNum, 1); }
catch (...) { return hptGuard(c, "hpt_naive_path_trace_block"); }

// ---- adaptive sampling (hpt_adaptive.hip, the ADAPT instantiations of pathTraceKernel) ----------------------------------------
static_assert(sizeof(hpt_pixel_moments) == sizeof(PixelMoments) && sizeof(hpt_adaptive_params) == sizeof(AdaptiveParams) && sizeof(hpt_adaptive_info) == sizeof(AdaptiveInfo),
              "the public records of adaptive sampling are the kernels' records");
// known: what the caller knows of the counts - their largest (or a bound of it), how many are above 0, how many exceed WF_MAX_PASSES (the loop); null: nothing
static int adaptiveCountsLaunch(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, uint32_t passNum, int naive,
                                const uint32_t* passCountsDev, hpt_pixel_moments* momentsDev, void* stream, const WfCountsSummary* known)
{
  if (tidCount == 0 || (passNum == 0 && !passCountsDev)) return HPT_OK;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidBegin = tidBegin; job.tidCount = tidCount; job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  job.passCounts = passCountsDev; job.moments = (PixelMoments*)momentsDev;
  return launch_path_trace(c, job, naive != 0, false, (hipStream_t)stream, true, known);
}
extern "C" int hpt_path_trace_block_counts_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, uint32_t passNum, int naive,
                                               const uint32_t* passCountsDev, hpt_pixel_moments* momentsDev, void* stream)
try {
  if (!c || !outDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  return adaptiveCountsLaunch(c, tidBegin, tidCount, channels, outDev, passNum, naive, passCountsDev, momentsDev, stream, nullptr);
}
catch (...) { return hptGuard(c, "hpt_path_trace_block_counts_dev"); }

// the planner's and the resolve's window: tids [tidBegin, tidBegin + tidCount) of the packed viewport
static int adaptiveWindowCheck(hpt_ctx* c, const char* what, uint32_t tidBegin, uint32_t tidCount)
{
  const std::string w(what);
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, w + " before UpdateMembersPlainData");
  if (c->packedCount == 0u || c->packedCount != (uint)(c->S.winWidth * c->S.winHeight)) return c->fail(HPT_ERR_STATE, w + " before PackXYBlock");
  if ((uint64_t)tidBegin + tidCount > c->packedCount) return c->fail(HPT_ERR_ARG, w + ": tid range exceeds the viewport");
  return HPT_OK;
}
static int adaptiveParamsCheck(hpt_ctx* c, const char* what, const hpt_adaptive_params* p)
{
  const std::string w(what);
  if (!p) return c->fail(HPT_ERR_ARG, w + ": params is null");
  if (!std::isfinite(p->tol) || !(p->tol > 0.0f)) return c->fail(HPT_ERR_ARG, w + ": tol must be finite and above 0");
  if (!std::isfinite(p->lumFloor) || !(p->lumFloor > 0.0f)) return c->fail(HPT_ERR_ARG, w + ": lumFloor must be finite and above 0");
  if (p->minPasses < 1u || p->minPasses > p->maxPasses) return c->fail(HPT_ERR_ARG, w + ": 1 <= minPasses <= maxPasses is required");
  if (p->step < 1u) return c->fail(HPT_ERR_ARG, w + ": step must be at least 1");
  if (p->dilate > 1u) return c->fail(HPT_ERR_ARG, w + ": dilate is 0 or 1");
  return HPT_OK;
}
// one planning step on st: zero the need image and *infoDev, every pixel's own need, then the counts and the totals (checks made by the callers)
static int adaptivePlanLaunch(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const AdaptiveParams& p, const PixelMoments* momentsDev, uint* countsDev, AdaptiveInfo* infoDev, hipStream_t st)
{
  const size_t pixels = (size_t)c->packedCount;
  HIPCHK(c, c->dAdNeed.alloc(pixels));
  HIPCHK(c, hipMemsetAsync(c->dAdNeed.p, 0, pixels * sizeof(uint), st));
  HIPCHK(c, hipMemsetAsync(infoDev, 0, sizeof(AdaptiveInfo), st));
  const dim3 g((tidCount + 255u) / 256u), b(256);
  adaptiveNeedKernel<<<g, b, 0, st>>>(momentsDev, c->dPackedXY.p, tidBegin, tidCount, (uint)c->S.winWidth, p, c->dAdNeed.p);
  adaptivePlanKernel<<<g, b, 0, st>>>(momentsDev, c->dPackedXY.p, tidBegin, tidCount, (uint)c->S.winWidth, (uint)c->S.winHeight, p, c->dAdNeed.p, countsDev, infoDev);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
// What the loop refuses before it touches anything: the loop zeroes, plans and counts the contiguous window [tidBegin, tidBegin + tidCount), while a
// render under hpt_set_tid_interleave with stride > 1 visits every stride-th chunk, far outside it - its counts would be read from words no planner wrote.
// With "adaptive_wavefront" a round's counts must fit a pool slot's status word (WF_MAX_PASSES) wherever the schedule setting could send a round of this
// window to the wavefront form; a round's largest count is bounded by minPasses (round 0) and min(step, maxPasses) (the planner's clip).
static uint adaptiveRoundBound(const hpt_adaptive_params* p) { return std::min(p->step, p->maxPasses); }
static int adaptiveLoopCheck(hpt_ctx* c, uint32_t channels, const hpt_adaptive_params* p, uint32_t tidCount)
{
  if (adaptiveWaveReachable(c, tidCount) && (p->minPasses > WF_MAX_PASSES || adaptiveRoundBound(p) > WF_MAX_PASSES))
    return c->fail(HPT_ERR_ARG, "PathTraceBlockAdaptive under the wavefront schedule: minPasses and min(step, maxPasses) must not exceed 16777215 (0xFFFFFF), all that a pool "
                                "slot's status word holds; lower them, or render with hpt_set_option(\"adaptive_wavefront\", 0)");
  if (c->tidStride > 1) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlockAdaptive: the loop plans one contiguous tid window; under hpt_set_tid_interleave with stride > 1 drive "
                                                            "hpt_path_trace_block_counts_dev and hpt_adaptive_plan_dev yourself, or reset the interleave");
  if (int rc = adaptiveRefusal(c, false, false, channels)) return rc;
  if (c->S.spectralMode != 0u && c->hasFilm && !c->filmTablesSpectral)      // (launch_path_trace's check, made here before the records are zeroed)
    return c->fail(HPT_ERR_ARG, "thin film: m_precomp_thin_films was precomputed for RGB rendering (LoadScene sizes the tables by m_spectral_mode)");
  if (!c->sceneUploaded) return c->fail(HPT_ERR_STATE, "PathTraceBlockAdaptive before CommitDeviceData");
  if (c->dGens.n < (size_t)c->packedCount) return c->fail(HPT_ERR_STATE, "PathTraceBlockAdaptive: m_randomGens smaller than the thread range (InitRandomGens)");
  if (channels != 1u && channels != 3u && channels != 4u) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlockAdaptive: 1, 3 or 4 channels");
  return HPT_OK;
}
static AdaptiveParams adaptiveParamsOf(const hpt_adaptive_params* p) { AdaptiveParams q; std::memcpy(&q, p, sizeof(q)); return q; }

extern "C" int hpt_adaptive_plan_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const hpt_adaptive_params* params, const hpt_pixel_moments* momentsDev,
                                     uint32_t* passCountsDev, hpt_adaptive_info* infoDev, void* stream)
try {
  if (!c || !momentsDev || !passCountsDev || !infoDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveParamsCheck(c, "AdaptivePlan", params)) return rc;
  if (int rc = adaptiveWindowCheck(c, "AdaptivePlan", tidBegin, tidCount)) return rc;
  if (tidCount == 0) { HIPCHK(c, hipMemsetAsync(infoDev, 0, sizeof(AdaptiveInfo), (hipStream_t)stream)); return HPT_OK; }
  return adaptivePlanLaunch(c, tidBegin, tidCount, adaptiveParamsOf(params), (const PixelMoments*)momentsDev, passCountsDev, (AdaptiveInfo*)infoDev, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_adaptive_plan_dev"); }

extern "C" int hpt_adaptive_resolve_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, const float* frameDev, const hpt_pixel_moments* momentsDev,
                                        float* outDev, void* stream)
try {
  if (!c || !frameDev || !momentsDev || !outDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (channels != 1u && channels != 3u && channels != 4u) return c->fail(HPT_ERR_ARG, "AdaptiveResolve: channels must be 1, 3 or 4");
  if (int rc = adaptiveWindowCheck(c, "AdaptiveResolve", tidBegin, tidCount)) return rc;
  if (tidCount == 0) return HPT_OK;
  adaptiveResolveKernel<<<dim3((tidCount + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>(frameDev, (const PixelMoments*)momentsDev, c->dPackedXY.p, tidBegin, tidCount,
                                                                                                (uint)c->S.winWidth, channels, outDev);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_adaptive_resolve_dev"); }

extern "C" int hpt_path_trace_block_adaptive_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, const hpt_adaptive_params* params,
                                                 uint32_t maxRounds, hpt_pixel_moments* momentsDev, hpt_adaptive_info* info, void* stream)
try {
  if (!c || !outDev || !info) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveParamsCheck(c, "PathTraceBlockAdaptive", params)) return rc;
  if (int rc = adaptiveWindowCheck(c, "PathTraceBlockAdaptive", tidBegin, tidCount)) return rc;
  if (int rc = adaptiveLoopCheck(c, channels, params, tidCount)) return rc;
  hipStream_t st = (hipStream_t)stream;
  AdaptiveInfo res; std::memset(&res, 0, sizeof(res));
  if (tidCount == 0) { std::memcpy(info, &res, sizeof(res)); return HPT_OK; }
  const AdaptiveParams p = adaptiveParamsOf(params);
  if (!momentsDev) { HIPCHK(c, c->dAdMoments.alloc(c->packedCount)); momentsDev = (hpt_pixel_moments*)c->dAdMoments.p; }
  HIPCHK(c, c->dAdCounts.alloc(c->packedCount));
  HIPCHK(c, c->dAdInfo.alloc(1));
  HIPCHK(c, hipMemsetAsync(momentsDev + tidBegin, 0, (size_t)tidCount * sizeof(PixelMoments), st));
  float ms = 0.0f, kms = 0.0f;
  // round 0: minPasses everywhere. The schedule is chosen per round ("adaptive_wavefront"; the two forms are bit-identical) on the round's active
  // pixels: the window here, later the plan's pixels above 0 - read back below anyway - with min(step, maxPasses) bounding the largest count
  WfCountsSummary known = { p.minPasses, tidCount, 0u };
  if (int rc = adaptiveCountsLaunch(c, tidBegin, tidCount, channels, outDev, p.minPasses, 0, nullptr, momentsDev, stream, &known)) return rc;
  res.rounds = 1u; res.passes = (unsigned long long)p.minPasses * tidCount;
  AdaptiveInfo plan; std::memset(&plan, 0, sizeof(plan));
  for (uint32_t round = 0; ; round++) {
    if (int rc = adaptivePlanLaunch(c, tidBegin, tidCount, p, (const PixelMoments*)momentsDev, c->dAdCounts.p, c->dAdInfo.p, st)) return rc;
    HIPCHK(c, hipMemcpyAsync(&plan, c->dAdInfo.p, sizeof(plan), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));                         // (the render launch before this plan has finished: its event pair can be read)
    if (int rc = sliceErrorCheck(c)) return rc;
    (void)hipEventElapsedTime(&kms, c->ev0, c->ev1); ms += kms;
    if (plan.passes == 0ull || round >= maxRounds) break;
    known.maxCount = adaptiveRoundBound(params); known.active = plan.pixels;
    if (int rc = adaptiveCountsLaunch(c, tidBegin, tidCount, channels, outDev, 0u, 0, c->dAdCounts.p, momentsDev, stream, &known)) return rc;
    res.rounds++; res.passes += plan.passes;
  }
  res.pixels = plan.pixels; res.maxPasses = plan.maxPasses; res.nonfinite = plan.nonfinite; res.deviceMs = ms;
  c->lastKernelMs = ms;
  std::memcpy(info, &res, sizeof(res));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_path_trace_block_adaptive_dev"); }

// the host-pointer forms: the caller's arrays are indexed by absolute tid; their window goes to context-owned device arrays at the same offsets
static int adaptiveUploadWindow(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const uint32_t* counts, const hpt_pixel_moments* moments)
{
  if (counts) { HIPCHK(c, c->dAdCountsIn.alloc(c->packedCount)); HIPCHK(c, hipMemcpy(c->dAdCountsIn.p + tidBegin, counts + tidBegin, (size_t)tidCount * sizeof(uint), hipMemcpyHostToDevice)); }
  if (moments) { HIPCHK(c, c->dAdMomentsIn.alloc(c->packedCount)); HIPCHK(c, hipMemcpy(c->dAdMomentsIn.p + tidBegin, moments + tidBegin, (size_t)tidCount * sizeof(PixelMoments), hipMemcpyHostToDevice)); }
  return HPT_OK;
}
extern "C" int hpt_path_trace_block_counts(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum,
                                           const uint32_t* passCounts, hpt_pixel_moments* moments)
try {
  if (!c || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveWindowCheck(c, "PathTraceBlockCounts", tidBegin, tidCount)) return rc;
  if (c->tidStride > 1) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlockCounts: the host-pointer form copies one contiguous tid window (use the device form with hpt_set_tid_interleave)");
  const size_t n = (size_t)c->S.winWidth * c->S.winHeight * channels;
  const bool runs = tidCount != 0 && (passNum != 0 || passCounts);
  return roundTrip(c, c->tSlots[T_PATH_TRACE], runs ? KERNEL_EVENTS : KERNEL_NONE,
                   [&]() -> int { HIPCHK(c, c->dFrame.alloc(n)); HIPCHK(c, hipMemcpy(c->dFrame.p, out, n * 4, hipMemcpyHostToDevice)); return adaptiveUploadWindow(c, tidBegin, tidCount, passCounts, moments); },
                   [&]() -> int { return hpt_path_trace_block_counts_dev(c, tidBegin, tidCount, channels, c->dFrame.p, passNum, 0, passCounts ? c->dAdCountsIn.p : nullptr,
                                                                         moments ? (hpt_pixel_moments*)c->dAdMomentsIn.p : nullptr, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, c->dFrame.p, n * 4, hipMemcpyDeviceToHost));
                                  if (moments && runs) HIPCHK(c, hipMemcpy(moments + tidBegin, c->dAdMomentsIn.p + tidBegin, (size_t)tidCount * sizeof(PixelMoments), hipMemcpyDeviceToHost));
                                  return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_path_trace_block_counts"); }

extern "C" int hpt_adaptive_plan(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const hpt_adaptive_params* params, const hpt_pixel_moments* moments,
                                 uint32_t* passCounts, hpt_adaptive_info* info)
try {
  if (!c || !moments || !passCounts || !info) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveParamsCheck(c, "AdaptivePlan", params)) return rc;
  if (int rc = adaptiveWindowCheck(c, "AdaptivePlan", tidBegin, tidCount)) return rc;
  if (int rc = adaptiveUploadWindow(c, tidBegin, tidCount, nullptr, moments)) return rc;
  HIPCHK(c, c->dAdCountsIn.alloc(c->packedCount));
  HIPCHK(c, c->dAdInfo.alloc(1));
  if (int rc = hpt_adaptive_plan_dev(c, tidBegin, tidCount, params, (const hpt_pixel_moments*)c->dAdMomentsIn.p, c->dAdCountsIn.p, (hpt_adaptive_info*)c->dAdInfo.p, nullptr)) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(passCounts + tidBegin, c->dAdCountsIn.p + tidBegin, (size_t)tidCount * sizeof(uint), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(info, c->dAdInfo.p, sizeof(AdaptiveInfo), hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_adaptive_plan"); }

extern "C" int hpt_adaptive_resolve(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, const float* frame, const hpt_pixel_moments* moments, float* out)
try {
  if (!c || !frame || !moments || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (channels != 1u && channels != 3u && channels != 4u) return c->fail(HPT_ERR_ARG, "AdaptiveResolve: channels must be 1, 3 or 4");
  if (int rc = adaptiveWindowCheck(c, "AdaptiveResolve", tidBegin, tidCount)) return rc;
  const size_t n = (size_t)c->packedCount * channels;
  DevBuf<float> dOut;                                            // (out may be frame: the caller's out is uploaded first so that pixels outside the window keep their contents)
  HIPCHK(c, dOut.upload(out, n));
  HIPCHK(c, c->dFrame.upload(frame, n));
  if (int rc = adaptiveUploadWindow(c, tidBegin, tidCount, nullptr, moments)) return rc;
  if (int rc = hpt_adaptive_resolve_dev(c, tidBegin, tidCount, channels, c->dFrame.p, (const hpt_pixel_moments*)c->dAdMomentsIn.p, dOut.p, nullptr)) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, dOut.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_adaptive_resolve"); }

// The variance plane of DenoiseFrameVar from the records: one float per pixel of the window, in pixel order
static int adaptiveVarianceCheck(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const void* moments, const void* outVar)
{
  if (!moments) return c->fail(HPT_ERR_ARG, "AdaptiveVariance: moments is null");
  if (!outVar) return c->fail(HPT_ERR_ARG, "AdaptiveVariance: outVar is null");
  return adaptiveWindowCheck(c, "AdaptiveVariance", tidBegin, tidCount);
}
extern "C" int hpt_adaptive_variance_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const hpt_pixel_moments* momentsDev, float* outVarDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveVarianceCheck(c, tidBegin, tidCount, momentsDev, outVarDev)) return rc;
  if (tidCount == 0) return HPT_OK;
  adaptiveVarianceKernel<<<dim3((tidCount + 255u) / 256u), dim3(256), 0, (hipStream_t)stream>>>((const PixelMoments*)momentsDev, c->dPackedXY.p, tidBegin, tidCount,
                                                                                                 (uint)c->S.winWidth, outVarDev);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_adaptive_variance_dev"); }
extern "C" int hpt_adaptive_variance(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, const hpt_pixel_moments* moments, float* outVar)
try {
  if (!c) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveVarianceCheck(c, tidBegin, tidCount, moments, outVar)) return rc;
  const size_t n = (size_t)c->packedCount;
  DevBuf<float> dOut;                                            // (the caller's plane goes up first: pixels outside the window keep their contents)
  return roundTrip(c, nullptr, KERNEL_UNTIMED,
                   [&]() -> int { HIPCHK(c, dOut.upload(outVar, n)); return adaptiveUploadWindow(c, tidBegin, tidCount, nullptr, moments); },
                   [&]() -> int { return hpt_adaptive_variance_dev(c, tidBegin, tidCount, (const hpt_pixel_moments*)c->dAdMomentsIn.p, dOut.p, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(outVar, dOut.p, n * sizeof(float), hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_adaptive_variance"); }

extern "C" int hpt_path_trace_block_adaptive(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, const hpt_adaptive_params* params,
                                             uint32_t maxRounds, hpt_pixel_moments* moments, hpt_adaptive_info* info)
try {
  if (!c || !out || !info) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (int rc = adaptiveParamsCheck(c, "PathTraceBlockAdaptive", params)) return rc;
  if (int rc = adaptiveWindowCheck(c, "PathTraceBlockAdaptive", tidBegin, tidCount)) return rc;
  if (int rc = adaptiveLoopCheck(c, channels, params, tidCount)) return rc;
  const size_t n = (size_t)c->packedCount * channels;
  HIPCHK(c, c->dFrame.upload(out, n));
  if (moments) HIPCHK(c, c->dAdMomentsIn.alloc(c->packedCount));
  if (int rc = hpt_path_trace_block_adaptive_dev(c, tidBegin, tidCount, channels, c->dFrame.p, params, maxRounds, moments ? (hpt_pixel_moments*)c->dAdMomentsIn.p : nullptr, info, nullptr)) return rc;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, c->dFrame.p, n * sizeof(float), hipMemcpyDeviceToHost));
  if (moments && tidCount) HIPCHK(c, hipMemcpy(moments + tidBegin, c->dAdMomentsIn.p + tidBegin, (size_t)tidCount * sizeof(PixelMoments), hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_path_trace_block_adaptive"); }

// ---- EvalGBuffer (integrator_pt.h:251, integrator_gbuffer.cpp:264-267) ------------------------------------------------------------------------
static_assert(sizeof(hpt_gbuffer_pixel) == 60 && sizeof(hpt_gbuffer_pixel) == sizeof(GBufferPixel), "GBufferPixel is 15 dwords (integrator_pt.h:187-198)");
// What a per-pixel pass (EvalGBuffer, CastSingleRayBlock, RayTraceBlock) needs before it can run, in the order the reference's driver makes its
// calls. `what` names the reference's method, `outName` its output argument, `countName` its pixel count.
static int pixelPassCheck(hpt_ctx* c, const char* what, const char* outName, const void* out, const char* countName, uint32_t count)
{
  const std::string w(what);
  if (!out) return c->fail(HPT_ERR_ARG, w + ": " + outName + " is null");
  if (!c->sceneUploaded) return c->fail(HPT_ERR_STATE, w + " before CommitDeviceData");
  if (!c->accelCommitted) return c->fail(HPT_ERR_STATE, w + " before CommitScene");
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, w + " before UpdateMembersPlainData");
  if (c->packedCount == 0u || c->packedCount != (uint)(c->S.winWidth * c->S.winHeight)) return c->fail(HPT_ERR_STATE, w + " before PackXYBlock");
  if (count > c->packedCount) return c->fail(HPT_ERR_ARG, w + ": " + countName + " exceeds the packed pixel count");
  return HPT_OK;
}
// Device-pointer form: 16 lanes per pixel through the traversal variant of the committed layout (hpt_gbuffer.hip). The pass draws no random
// numbers and changes no state of the context; it reads only RGB base colours, so m_spectral_mode does not matter. Asynchronous.
extern "C" int hpt_eval_gbuffer_dev(hpt_ctx* c, uint32_t blockNum, hpt_gbuffer_pixel* outDev, hpt_gbuffer_pixel* samplesDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = pixelPassCheck(c, "EvalGBuffer", "out_gbuffer", outDev, "blockNum", blockNum)) return rc;
  if (blockNum == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const uint blocks = (uint)(((size_t)blockNum * 16u + 255u) / 256u);
  GBufferPixel* o = (GBufferPixel*)outDev; GBufferPixel* sm = (GBufferPixel*)samplesDev;
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    traversalDispatch(c, [&](auto flat, auto motion, auto sweep) {
      gbufferKernel<flat(), motion(), sweep()><<<dim3(blocks), dim3(256), 0, st>>>(c->S, c->dPackedXY.p, blockNum, o, sm, c->dStackOvf.p);
    });
  });
}
catch (...) { return hptGuard(c, "hpt_eval_gbuffer_dev"); }
// Integrator::EvalGBuffer(blockNum, out_gbuffer) (integrator_pt.h:251; main.cpp:269-277): host pointer to winWidth * winHeight records. The
// reference writes only the records of pixels packedXY[0 .. blockNum); so does this: the caller's buffer goes up (when some record is not
// written) and comes back. No GetExecutionTime slot.
extern "C" int hpt_eval_gbuffer(hpt_ctx* c, uint32_t blockNum, hpt_gbuffer_pixel* out)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = pixelPassCheck(c, "EvalGBuffer", "out_gbuffer", out, "blockNum", blockNum)) return rc;   // (before packedCount below means anything)
  if (blockNum == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  return roundTrip(c, nullptr, out, (size_t)c->packedCount, blockNum < c->packedCount,
                   [&](hpt_gbuffer_pixel* d) { return hpt_eval_gbuffer_dev(c, blockNum, d, nullptr, nullptr); });
}
catch (...) { return hptGuard(c, "hpt_eval_gbuffer"); }

// ---- DenoiseFrame (no counterpart in the reference; DESIGN.md 2.12, hpt_denoise.hip) -------------------------------------------------------------
static_assert(sizeof(hpt_denoise_params) == 28, "hpt_denoise_params is 7 dwords");
// The refusals both forms share; each names its argument. `a`, `b`: the two frames of n pixels that must not overlap.
static int denoiseCheck(hpt_ctx* c, uint32_t width, uint32_t height, const float* color, const hpt_gbuffer_pixel* gbuffer, const hpt_denoise_params* p, const float* out,
                        const char* what = "DenoiseFrame")
{
  const std::string w = std::string(what) + ": ";
  if (!color) return c->fail(HPT_ERR_ARG, w + "color is null");
  if (!gbuffer) return c->fail(HPT_ERR_ARG, w + "gbuffer is null");
  if (!p) return c->fail(HPT_ERR_ARG, w + "params is null");
  if (!out) return c->fail(HPT_ERR_ARG, w + "out is null");
  if (width == 0u || width > 32768u) return c->fail(HPT_ERR_ARG, w + "width must be 1 .. 32768");
  if (height == 0u || height > 32768u) return c->fail(HPT_ERR_ARG, w + "height must be 1 .. 32768");
  if (p->iterations < 1u || p->iterations > 8u) return c->fail(HPT_ERR_ARG, w + "iterations must be 1 .. 8");
  if (p->normalSquarings > 8u) return c->fail(HPT_ERR_ARG, w + "normalSquarings must be 0 .. 8");
  if (p->flags & ~HPT_DENOISE_DEMODULATE) return c->fail(HPT_ERR_ARG, w + "flags has unknown bits (bit 0: demodulate albedo)");
  const struct { const char* name; float v; } f[] = { { "normConst", p->normConst }, { "sigmaColor", p->sigmaColor }, { "sigmaDepth", p->sigmaDepth }, { "sigmaAlbedo", p->sigmaAlbedo } };
  for (const auto& a : f) if (!(a.v >= 0.0f) || !(a.v <= 3.402823466e38f)) return c->fail(HPT_ERR_ARG, w + a.name + " must be finite and not negative");
  const size_t bytes = (size_t)width * height * 4 * sizeof(float);
  const char* a = (const char*)color; const char* b = (const char*)out;
  if (a < b + bytes && b < a + bytes) return c->fail(HPT_ERR_ARG, w + "out aliases color");
  return HPT_OK;
}
// Device-pointer form: the pack kernel, then `iterations` passes between the two colour planes, the last one into the caller's frame; one event
// pair around them. Asynchronous on stream (growing the scratch planes frees the old ones, which waits for the device).
extern "C" int hpt_denoise_frame_dev(hpt_ctx* c, uint32_t width, uint32_t height, const float* colorDev, const hpt_gbuffer_pixel* gbufferDev,
                                     const hpt_denoise_params* p, float* outDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = denoiseCheck(c, width, height, colorDev, gbufferDev, p, outDev)) return rc;
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)width * height;
  HIPCHK(c, c->dDenoiseN.alloc(n)); HIPCHK(c, c->dDenoiseA.alloc(n)); HIPCHK(c, c->dDenoiseC[0].alloc(n));
  if (p->iterations > 1u) HIPCHK(c, c->dDenoiseC[1].alloc(n));
  DenoiseJob job; std::memset(&job, 0, sizeof(job));
  job.color = (const float4*)colorDev; job.gbuffer = (const GBufferPixel*)gbufferDev;
  job.planeN = c->dDenoiseN.p; job.planeA = c->dDenoiseA.p;
  job.pixels = n; job.width = width; job.height = height;
  job.normalSquarings = p->normalSquarings; job.flags = p->flags; job.normConst = p->normConst;
  job.terms = (p->sigmaDepth != 0.0f ? 1u : 0u) | (p->sigmaColor != 0.0f ? 2u : 0u) | (p->sigmaAlbedo != 0.0f ? 4u : 0u);
  job.sigmaAlbedo2 = p->sigmaAlbedo * p->sigmaAlbedo;
  HIPCHK(c, hipEventRecord(c->ev0, st));
  job.cin = c->dDenoiseC[0].p;
  denoisePackKernel<<<dim3((uint)((n + 255u) / 256u)), dim3(256), 0, st>>>(job);
  const dim3 grid((width + 31u) / 32u, (height + 7u) / 8u);
  for (uint32_t i = 0; i < p->iterations; i++) {
    const bool last = i + 1u == p->iterations;
    job.step = 1u << i;
    job.sigmaDepthStep = p->sigmaDepth * float(job.step);
    const float sc = p->sigmaColor * (1.0f / float(job.step));                // 2^-i: an exact scaling
    job.sigmaColor2 = sc * sc;
    job.cin = c->dDenoiseC[i & 1u].p;
    job.cout = last ? (float4*)outDev : c->dDenoiseC[(i & 1u) ^ 1u].p;
#if HPT_DENOISE_LDS                                                          // steps 1 and 2 read their taps from an LDS tile (hpt_decl.h)
    if (job.step == 1u) { if (last) denoisePassKernel<true, 1><<<grid, dim3(256), 0, st>>>(job); else denoisePassKernel<false, 1><<<grid, dim3(256), 0, st>>>(job); continue; }
    if (job.step == 2u) { if (last) denoisePassKernel<true, 2><<<grid, dim3(256), 0, st>>>(job); else denoisePassKernel<false, 2><<<grid, dim3(256), 0, st>>>(job); continue; }
#endif
    if (last) denoisePassKernel<true><<<grid, dim3(256), 0, st>>>(job);
    else      denoisePassKernel<false><<<grid, dim3(256), 0, st>>>(job);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev1, st));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_denoise_frame_dev"); }
// Host-pointer form: the frame and the records go up, the filtered frame comes back
extern "C" int hpt_denoise_frame(hpt_ctx* c, uint32_t width, uint32_t height, const float* color, const hpt_gbuffer_pixel* gbuffer,
                                 const hpt_denoise_params* p, float* out)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = denoiseCheck(c, width, height, color, gbuffer, p, out)) return rc;
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)width * height;
  DevBuf<float> dColor, dOut; DevBuf<hpt_gbuffer_pixel> dGb;
  return roundTrip(c, c->tSlots[T_DENOISE], KERNEL_EVENTS,
                   [&]() -> int { HIPCHK(c, dColor.upload(color, n * 4)); HIPCHK(c, dGb.upload(gbuffer, n)); HIPCHK(c, dOut.alloc(n * 4)); return HPT_OK; },
                   [&]() -> int { return hpt_denoise_frame_dev(c, width, height, dColor.p, dGb.p, p, dOut.p, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, dOut.p, n * 4 * sizeof(float), hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_denoise_frame"); }

// ---- DenoiseFrameVar: the variance-guided form; it shares the scratch planes N, A, C with DenoiseFrame and adds V ---------------------
static_assert(sizeof(hpt_denoise_var_params) == 16, "hpt_denoise_var_params is 4 dwords");
static bool overlaps(const void* a, size_t na, const void* b, size_t nb) { const char* x = (const char*)a; const char* y = (const char*)b; return x < y + nb && y < x + na; }
static int denoiseVarCheck(hpt_ctx* c, uint32_t width, uint32_t height, const float* color, const hpt_gbuffer_pixel* gbuffer, const float* variance,
                           const hpt_denoise_params* p, const hpt_denoise_var_params* vp, const float* out, const float* outVar)
{
  if (int rc = denoiseCheck(c, width, height, color, gbuffer, p, out, "DenoiseFrameVar")) return rc;
  const std::string w("DenoiseFrameVar: ");
  if (!variance) return c->fail(HPT_ERR_ARG, w + "variance is null");
  if (!vp) return c->fail(HPT_ERR_ARG, w + "var_params is null");
  if (!(vp->sigmaLum >= 0.0f) || !(vp->sigmaLum <= 3.402823466e38f)) return c->fail(HPT_ERR_ARG, w + "sigmaLum must be finite and not negative");
  if (!(vp->varFloor > 0.0f) || !(vp->varFloor <= 3.402823466e38f)) return c->fail(HPT_ERR_ARG, w + "varFloor must be finite and above 0 (it keeps the stop's denominator away from 0)");
  if (vp->reserved != 0u) return c->fail(HPT_ERR_ARG, w + "reserved must be 0");
  if (p->sigmaColor != 0.0f) return c->fail(HPT_ERR_ARG, w + "sigmaColor must be 0 (the luminance stop of sigmaLum stands in its place)");
  const size_t n = (size_t)width * height;
  if (overlaps(out, n * 16, variance, n * 4)) return c->fail(HPT_ERR_ARG, w + "out aliases variance");
  if (outVar) {
    if (overlaps(outVar, n * 4, color, n * 16)) return c->fail(HPT_ERR_ARG, w + "outVar aliases color");
    if (overlaps(outVar, n * 4, gbuffer, n * sizeof(hpt_gbuffer_pixel))) return c->fail(HPT_ERR_ARG, w + "outVar aliases gbuffer");
    if (overlaps(outVar, n * 4, variance, n * 4)) return c->fail(HPT_ERR_ARG, w + "outVar aliases variance");
    if (overlaps(outVar, n * 4, out, n * 16)) return c->fail(HPT_ERR_ARG, w + "outVar aliases out");
  }
  return HPT_OK;
}
template <bool LAST> static void denoiseVarPass(const DenoiseVarJob& job, dim3 grid, hipStream_t st)
{
  if (job.d.step == 1u) denoiseVarPassKernel<LAST, 1><<<grid, dim3(256), 0, st>>>(job);          // steps 1 and 2 read their taps from an LDS tile
  else if (job.d.step == 2u) denoiseVarPassKernel<LAST, 2><<<grid, dim3(256), 0, st>>>(job);
  else denoiseVarPassKernel<LAST, 0><<<grid, dim3(256), 0, st>>>(job);
}
// Device-pointer form: pack, then `iterations` passes between the ping-pong planes of colour and variance; one event pair around them. Asynchronous on stream.
extern "C" int hpt_denoise_frame_var_dev(hpt_ctx* c, uint32_t width, uint32_t height, const float* colorDev, const hpt_gbuffer_pixel* gbufferDev, const float* varianceDev,
                                         const hpt_denoise_params* p, const hpt_denoise_var_params* vp, float* outDev, float* outVarDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = denoiseVarCheck(c, width, height, colorDev, gbufferDev, varianceDev, p, vp, outDev, outVarDev)) return rc;
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)width * height;
  HIPCHK(c, c->dDenoiseN.alloc(n)); HIPCHK(c, c->dDenoiseA.alloc(n)); HIPCHK(c, c->dDenoiseC[0].alloc(n)); HIPCHK(c, c->dDenoiseV[0].alloc(n));
  if (p->iterations > 1u) { HIPCHK(c, c->dDenoiseC[1].alloc(n)); HIPCHK(c, c->dDenoiseV[1].alloc(n)); }
  DenoiseVarJob job; std::memset(&job, 0, sizeof(job));
  job.d.color = (const float4*)colorDev; job.d.gbuffer = (const GBufferPixel*)gbufferDev;
  job.d.planeN = c->dDenoiseN.p; job.d.planeA = c->dDenoiseA.p;
  job.d.pixels = n; job.d.width = width; job.d.height = height;
  job.d.normalSquarings = p->normalSquarings; job.d.flags = p->flags; job.d.normConst = p->normConst;
  job.d.terms = (p->sigmaDepth != 0.0f ? 1u : 0u) | (p->sigmaAlbedo != 0.0f ? 4u : 0u);
  job.d.sigmaAlbedo2 = p->sigmaAlbedo * p->sigmaAlbedo;
  job.variance = varianceDev; job.outVar = outVarDev;
  job.sigmaLum2 = vp->sigmaLum * vp->sigmaLum; job.varFloor = vp->varFloor; job.prefilter = vp->prefilter; job.useLum = vp->sigmaLum != 0.0f ? 1u : 0u;
  HIPCHK(c, hipEventRecord(c->ev0, st));
  job.d.cin = c->dDenoiseC[0].p; job.vin = c->dDenoiseV[0].p;
  denoiseVarPackKernel<<<dim3((uint)((n + 255u) / 256u)), dim3(256), 0, st>>>(job);
  const dim3 grid((width + 31u) / 32u, (height + 7u) / 8u);
  for (uint32_t i = 0; i < p->iterations; i++) {
    const bool last = i + 1u == p->iterations;
    job.d.step = 1u << i;
    job.d.sigmaDepthStep = p->sigmaDepth * float(job.d.step);
    job.d.cin = c->dDenoiseC[i & 1u].p; job.vin = c->dDenoiseV[i & 1u].p;
    job.d.cout = last ? (float4*)outDev : c->dDenoiseC[(i & 1u) ^ 1u].p;
    job.vout = last ? nullptr : c->dDenoiseV[(i & 1u) ^ 1u].p;
    if (last) denoiseVarPass<true>(job, grid, st); else denoiseVarPass<false>(job, grid, st);
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev1, st));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_denoise_frame_var_dev"); }
// Host-pointer form: the frame, the records and the variances go up, the filtered frame (and variance) come back
extern "C" int hpt_denoise_frame_var(hpt_ctx* c, uint32_t width, uint32_t height, const float* color, const hpt_gbuffer_pixel* gbuffer, const float* variance,
                                     const hpt_denoise_params* p, const hpt_denoise_var_params* vp, float* out, float* outVar)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = denoiseVarCheck(c, width, height, color, gbuffer, variance, p, vp, out, outVar)) return rc;
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)width * height;
  DevBuf<float> dColor, dVar, dOut, dOutVar; DevBuf<hpt_gbuffer_pixel> dGb;
  return roundTrip(c, c->tSlots[T_DENOISE_VAR], KERNEL_EVENTS,
                   [&]() -> int { HIPCHK(c, dColor.upload(color, n * 4)); HIPCHK(c, dGb.upload(gbuffer, n)); HIPCHK(c, dVar.upload(variance, n)); HIPCHK(c, dOut.alloc(n * 4));
                                  if (outVar) HIPCHK(c, dOutVar.alloc(n)); return HPT_OK; },
                   [&]() -> int { return hpt_denoise_frame_var_dev(c, width, height, dColor.p, dGb.p, dVar.p, p, vp, dOut.p, outVar ? dOutVar.p : nullptr, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, dOut.p, n * 4 * sizeof(float), hipMemcpyDeviceToHost));
                                  if (outVar) HIPCHK(c, hipMemcpy(outVar, dOutVar.p, n * sizeof(float), hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_denoise_frame_var"); }

// ---- CastSingleRayBlock / RayTraceBlock (integrator_pt.h:254, 263; integrator_rt.cpp:420-461; integrator_pt_host.cpp:29-36, 75-90) ----------------
// channels of RayTraceBlock: 1 and 2 are refused (the reference writes three floats at that stride: over the next pixel and, for the last
// one, past the buffer - DESIGN.md 7); above 4 its kernel_ContributeToImage3 writes nothing, so there is nothing to launch
static int rt_check_channels(hpt_ctx* c, uint32_t channels)
{
  if (channels < 3u) return c->fail(HPT_ERR_ARG, "RayTraceBlock: channels must be 3 or 4 (1 and 2 make the reference write outside the pixel; above 4 nothing is written)");
  return HPT_OK;
}
// one lane per pixel through the traversal variant of the committed layout (hpt_raytrace.hip); channels = 0: CastSingleRay
static int rt_launch(hpt_ctx* c, uint32_t tid, uint32_t channels, float* outDev, hipStream_t st)
{
  (void)hipSetDevice(c->device);
  const uint blocks = (tid + 255u) / 256u;
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    traversalDispatch(c, [&](auto flat, auto motion, auto sweep) {
      if (channels == 0u) castSingleRayKernel<flat(), motion(), sweep()><<<dim3(blocks), dim3(256), 0, st>>>(c->S, c->dPackedXY.p, tid, outDev, c->dStackOvf.p);
      else                rayTraceKernel<flat(), motion(), sweep()><<<dim3(blocks), dim3(256), 0, st>>>(c->S, c->dPackedXY.p, tid, channels, outDev, c->dStackOvf.p);
    });
  });
}
// Host-pointer form of either pass: the caller's frame goes up (RayTraceBlock adds to it; CastSingleRayBlock leaves the pixels past tid as
// they are) and comes back
static int rt_host(hpt_ctx* c, uint32_t tid, uint32_t channels, float* out, float slots[4])
{
  (void)hipSetDevice(c->device);
  return roundTrip(c, slots, out, (size_t)c->packedCount * (channels == 0u ? 4u : channels), true,
                   [&](float* d) { return rt_launch(c, tid, channels, d, nullptr); });
}

// Integrator::CastSingleRayBlock(tid, out_color, a_passNum) (integrator_pt.h:254, integrator_pt_host.cpp:29-36): a_passNum is unused there and here
extern "C" int hpt_cast_single_ray_block_dev(hpt_ctx* c, uint32_t tid, float* outDev, uint32_t passNum, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  (void)passNum;
  if (int rc = pixelPassCheck(c, "CastSingleRayBlock", "out_color", outDev, "tid", tid)) return rc;
  if (tid == 0u) return HPT_OK;
  return rt_launch(c, tid, 0u, outDev, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_cast_single_ray_block_dev"); }
extern "C" int hpt_cast_single_ray_block(hpt_ctx* c, uint32_t tid, float* out, uint32_t passNum)
try {
  if (!c) return HPT_ERR_ARG;
  (void)passNum;
  if (int rc = pixelPassCheck(c, "CastSingleRayBlock", "out_color", out, "tid", tid)) return rc;
  if (tid == 0u) return HPT_OK;
  return rt_host(c, tid, 0u, out, c->tSlots[T_CAST_SINGLE_RAY]);
}
catch (...) { return hptGuard(c, "hpt_cast_single_ray_block"); }

// Integrator::RayTraceBlock(tid, channels, out_color, a_passNum) (integrator_pt.h:263, integrator_pt_host.cpp:75-90): a_passNum is unused there and here
extern "C" int hpt_ray_trace_block_dev(hpt_ctx* c, uint32_t tid, uint32_t channels, float* outDev, uint32_t passNum, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  (void)passNum;
  if (int rc = pixelPassCheck(c, "RayTraceBlock", "out_color", outDev, "tid", tid)) return rc;
  if (int rc = rt_check_channels(c, channels)) return rc;
  if (tid == 0u || channels > 4u) return HPT_OK;
  return rt_launch(c, tid, channels, outDev, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_ray_trace_block_dev"); }
extern "C" int hpt_ray_trace_block(hpt_ctx* c, uint32_t tid, uint32_t channels, float* out, uint32_t passNum)
try {
  if (!c) return HPT_ERR_ARG;
  (void)passNum;
  if (int rc = pixelPassCheck(c, "RayTraceBlock", "out_color", out, "tid", tid)) return rc;
  if (int rc = rt_check_channels(c, channels)) return rc;
  if (tid == 0u || channels > 4u) return HPT_OK;
  return rt_host(c, tid, channels, out, c->tSlots[T_RAY_TRACE]);
}
catch (...) { return hptGuard(c, "hpt_ray_trace_block"); }

// ---- camera plug-in: CamPinHole / CamTableLens (cam_plugin/CamPluginAPI.h:39-77; hpt_camrays.hip) ---------------------------------------------
// The camera's state lives on the context's device; its failures go to the context's error text.
static const uint32_t CAM_TIMED_TILES = 256;                  // tiles of a hpt_cam_render_dev loop that get per-stage events
struct hpt_cam
{
  hpt_ctx* ctx = nullptr; int kind = 0;
  bool paramsSet = false; uint width = 0, height = 0; int spectral = 0; float projInv[16] = {0};
  uint batch = 0, lensCount = 0; float physSize[2] = {0, 0};
  DevBuf<Rng> dGens; DevBuf<float> dWaves, dCos4, dColors; DevBuf<float4> dLines, dRayPos, dRayDir, dCie;   // per-lane arrays, lens lines, tile buffers, own m_cie_xyz
  float tMake[4] = {0, 0, 0, 0}, tContrib[4] = {0, 0, 0, 0}, tTrace[4] = {0, 0, 0, 0}, tRender[4] = {0, 0, 0, 0};
  std::vector<hipEvent_t> ev;                                 // 4 per timed tile of the last render loop, then its first and last event
  uint32_t evTiles = 0; bool renderPending = false;
  ~hpt_cam() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

// what a tile call needs: both set-up calls made, the tile inside the batch and inside the frame
static int camTileCheck(hpt_cam* cam, const char* what, uint32_t n, int subPassId)
{
  hpt_ctx* c = cam->ctx;
  const std::string w(what);
  if (!cam->paramsSet) return c->fail(HPT_ERR_ARG, w + " before SetParameters");
  if (cam->batch == 0u) return c->fail(HPT_ERR_ARG, w + " before SetBatchSize");
  if (subPassId < 0) return c->fail(HPT_ERR_ARG, w + ": negative subPassId");
  if (n > cam->batch) return c->fail(HPT_ERR_ARG, w + ": in_blockSize exceeds the batch size");
  if ((uint64_t)subPassId * cam->batch + n > (uint64_t)cam->width * cam->height) return c->fail(HPT_ERR_ARG, w + ": the tile reaches past width * height");
  return HPT_OK;
}
static void camFillJob(const hpt_cam* cam, CamJob& job, uint32_t n, int subPassId)
{
  std::memset(&job, 0, sizeof(job));
  job.n = n; job.firstPixel = (uint)subPassId * cam->batch; job.width = cam->width; job.height = cam->height;
  std::memcpy(job.projInv, cam->projInv, sizeof(job.projInv));
  job.physSize[0] = cam->physSize[0]; job.physSize[1] = cam->physSize[1];
  job.lensCount = cam->lensCount; job.lensLines = cam->dLines.p;
  job.gens = cam->dGens.p; job.waves = cam->dWaves.p; job.cos4 = cam->dCos4.p;
}
// m_cie_xyz of the camera: the table the context uploaded with a spectral scene, else an own copy of the loaders' table
static int camEnsureCie(hpt_cam* cam)
{
  hpt_ctx* c = cam->ctx;
  if ((c->S.cieXYZ && c->S.numCieXYZ) || cam->dCie.p) return HPT_OK;
  const std::vector<float> t = hydra_hip::cieXyzFit();
  std::vector<float4> cie(t.size() / 4);
  for (size_t i = 0; i < cie.size(); i++) cie[i] = make_float4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
  HIPCHK(c, cam->dCie.upload(cie.data(), cie.size()));
  return HPT_OK;
}
// the two launches; e0 / e1 (may be null) are recorded around the kernel
static int camLaunchMake(hpt_cam* cam, float4* pos, float4* dir, uint32_t n, int subPassId, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
  hpt_ctx* c = cam->ctx;
  if (cam->kind == CAM_TABLE_LENS && cam->lensCount == 0u) return c->fail(HPT_ERR_ARG, "MakeRaysBlock: the table-lens camera has no lens lines (hpt_cam_set_lens)");
  CamJob job; camFillJob(cam, job, n, subPassId);
  job.rayPos = pos; job.rayDir = dir;
  const dim3 g((n + 255u) / 256u), b(256);
  if (e0) HIPCHK(c, hipEventRecord(e0, st));
  if (cam->kind == CAM_PINHOLE) { if (cam->spectral) camMakeRaysKernel<CAM_PINHOLE, true><<<g, b, 0, st>>>(job); else camMakeRaysKernel<CAM_PINHOLE, false><<<g, b, 0, st>>>(job); }
  else                          { if (cam->spectral) camMakeRaysKernel<CAM_TABLE_LENS, true><<<g, b, 0, st>>>(job); else camMakeRaysKernel<CAM_TABLE_LENS, false><<<g, b, 0, st>>>(job); }
  HIPCHK(c, hipGetLastError());
  if (e1) HIPCHK(c, hipEventRecord(e1, st));
  return HPT_OK;
}
static int camLaunchContrib(hpt_cam* cam, float4* frame, const float* colors, uint32_t n, int subPassId, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
  hpt_ctx* c = cam->ctx;
  CamJob job; camFillJob(cam, job, n, subPassId);
  job.frame = frame; job.colors = colors;
  if (cam->spectral) {
    if (int rc = camEnsureCie(cam)) return rc;
    const bool own = !(c->S.cieXYZ && c->S.numCieXYZ);
    job.cie = own ? cam->dCie.p : c->S.cieXYZ; job.numCie = own ? (uint)cam->dCie.n : c->S.numCieXYZ;
  }
  const dim3 g((n + 255u) / 256u), b(256);
  if (e0) HIPCHK(c, hipEventRecord(e0, st));
  if (cam->kind == CAM_PINHOLE) { if (cam->spectral) camContribKernel<CAM_PINHOLE, true><<<g, b, 0, st>>>(job); else camContribKernel<CAM_PINHOLE, false><<<g, b, 0, st>>>(job); }
  else                          { if (cam->spectral) camContribKernel<CAM_TABLE_LENS, true><<<g, b, 0, st>>>(job); else camContribKernel<CAM_TABLE_LENS, false><<<g, b, 0, st>>>(job); }
  HIPCHK(c, hipGetLastError());
  if (e1) HIPCHK(c, hipEventRecord(e1, st));
  return HPT_OK;
}

extern "C" int hpt_cam_create(hpt_ctx* c, int kind, hpt_cam** out)
try {
  if (!c || !out) return HPT_ERR_ARG;
  *out = nullptr;
  if (kind != CAM_PINHOLE && kind != CAM_TABLE_LENS) return c->fail(HPT_ERR_ARG, "hpt_cam_create: kind must be 0 (pinhole) or 1 (table lens)");
  hpt_cam* cam = new hpt_cam();
  cam->ctx = c; cam->kind = kind;
  *out = cam;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_cam_create"); }
extern "C" void hpt_cam_destroy(hpt_cam* cam)
try {
  if (!cam) return;
  (void)hipSetDevice(cam->ctx->device);
  (void)hipDeviceSynchronize();
  delete cam;                                                  // (its DevBuf members free the device arrays)
}
catch (...) { (void)hptGuard(nullptr, "hpt_cam_destroy"); }

extern "C" int hpt_cam_set_parameters(hpt_cam* cam, uint32_t width, uint32_t height, const float* projInv16, int spectralMode)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (!projInv16) return c->fail(HPT_ERR_ARG, "SetParameters: projInv16 is null");
  if (width == 0u || height == 0u || (uint64_t)width * height > 0x7FFFFFFFull) return c->fail(HPT_ERR_ARG, "SetParameters: width * height must be 1 .. 2^31 - 1");
  (void)hipSetDevice(c->device);
  cam->width = width; cam->height = height; cam->spectral = spectralMode != 0 ? 1 : 0;
  std::memcpy(cam->projInv, projInv16, sizeof(cam->projInv));
  cam->paramsSet = true;
  if (cam->spectral) { if (int rc = camEnsureCie(cam)) return rc; }
  else if (cam->dWaves.p) HIPCHK(c, hipMemset(cam->dWaves.p, 0, (size_t)cam->batch * 4));   // RGB rays carry wavelength 0: the pinhole's RGB kernel does not write it again
  return HPT_OK;
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_set_parameters"); }

extern "C" int hpt_cam_set_lens(hpt_cam* cam, const float* lines4, uint32_t n, float physSizeX, float physSizeY)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (cam->kind != CAM_TABLE_LENS) return c->fail(HPT_ERR_ARG, "hpt_cam_set_lens: a pinhole camera has no lens table");
  if (!lines4) return c->fail(HPT_ERR_ARG, "hpt_cam_set_lens: lines4 is null");
  if (n == 0u || n > 64u) return c->fail(HPT_ERR_ARG, "hpt_cam_set_lens: 1 .. 64 lens interfaces");
  for (uint32_t i = 0; i < n; i++) if (!(lines4[4 * i + 3] >= 0.0f)) return c->fail(HPT_ERR_ARG, "hpt_cam_set_lens: negative aperture radius");
  (void)hipSetDevice(c->device);
  std::vector<float4> l(n);
  for (uint32_t i = 0; i < n; i++) l[i] = make_float4(lines4[4 * i], lines4[4 * i + 1], lines4[4 * i + 2], lines4[4 * i + 3]);
  HIPCHK(c, hipDeviceSynchronize());                           // (a tile in flight may still read the old lines)
  HIPCHK(c, cam->dLines.upload(l.data(), l.size()));
  cam->lensCount = n; cam->physSize[0] = physSizeX; cam->physSize[1] = physSizeY;
  return HPT_OK;
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_set_lens"); }

extern "C" int hpt_cam_set_batch_size(hpt_cam* cam, uint32_t tile)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (tile == 0u || tile > (1u << 28)) return c->fail(HPT_ERR_ARG, "SetBatchSize: the tile must hold 1 .. 2^28 rays");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, cam->dGens.alloc(tile)); HIPCHK(c, cam->dWaves.alloc(tile)); HIPCHK(c, cam->dCos4.alloc(tile));
  HIPCHK(c, cam->dRayPos.alloc(tile)); HIPCHK(c, cam->dRayDir.alloc(tile)); HIPCHK(c, cam->dColors.alloc((size_t)tile * 4));
  cam->batch = tile;
  camInitGensKernel<<<dim3((tile + 255u) / 256u), dim3(256), 0, 0>>>(cam->dGens.p, tile);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemset(cam->dWaves.p, 0, (size_t)tile * 4));
  HIPCHK(c, hipMemset(cam->dCos4.p, 0, (size_t)tile * 4));
  return HPT_OK;
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_set_batch_size"); }

extern "C" int hpt_cam_make_rays_block_dev(hpt_cam* cam, float* rayPosDev, float* rayDirDev, uint32_t n, int subPassId, void* stream)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (!rayPosDev || !rayDirDev) return c->fail(HPT_ERR_ARG, "MakeRaysBlock: a ray array is null");
  if (int rc = camTileCheck(cam, "MakeRaysBlock", n, subPassId)) return rc;
  if (cam->kind == CAM_TABLE_LENS && cam->lensCount == 0u) return c->fail(HPT_ERR_ARG, "MakeRaysBlock: the table-lens camera has no lens lines (hpt_cam_set_lens)");
  if (n == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  cam->renderPending = false;
  return camLaunchMake(cam, (float4*)rayPosDev, (float4*)rayDirDev, n, subPassId, (hipStream_t)stream, c->ev0, c->ev1);
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_make_rays_block_dev"); }
extern "C" int hpt_cam_make_rays_block(hpt_cam* cam, float* rayPos, float* rayDir, uint32_t n, int subPassId)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (!rayPos || !rayDir) return c->fail(HPT_ERR_ARG, "MakeRaysBlock: a ray array is null");
  if (int rc = camTileCheck(cam, "MakeRaysBlock", n, subPassId)) return rc;
  if (cam->kind == CAM_TABLE_LENS && cam->lensCount == 0u) return c->fail(HPT_ERR_ARG, "MakeRaysBlock: the table-lens camera has no lens lines (hpt_cam_set_lens)");
  if (n == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  return roundTrip(c, cam->tMake, KERNEL_EVENTS,                // every ray record is written: nothing goes up; the tile buffers serve as the device copies
                   [&]() -> int { return HPT_OK; },
                   [&]() -> int { return hpt_cam_make_rays_block_dev(cam, (float*)cam->dRayPos.p, (float*)cam->dRayDir.p, n, subPassId, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(rayPos, cam->dRayPos.p, (size_t)n * 16, hipMemcpyDeviceToHost)); HIPCHK(c, hipMemcpy(rayDir, cam->dRayDir.p, (size_t)n * 16, hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_make_rays_block"); }

static int camContribCheck(hpt_cam* cam, const void* out, const void* colors, uint32_t n, uint32_t width, uint32_t height, int subPassId)
{
  hpt_ctx* c = cam->ctx;
  if (!out) return c->fail(HPT_ERR_ARG, "AddSamplesContributionBlock: out_color4f is null");
  if (!colors) return c->fail(HPT_ERR_ARG, "AddSamplesContributionBlock: colors is null");
  if (int rc = camTileCheck(cam, "AddSamplesContributionBlock", n, subPassId)) return rc;
  if (width != cam->width || height != cam->height) return c->fail(HPT_ERR_ARG, "AddSamplesContributionBlock: a_width / a_height differ from SetParameters");
  return HPT_OK;
}
extern "C" int hpt_cam_add_samples_contribution_block_dev(hpt_cam* cam, float* outDev, const float* colorsDev, uint32_t n, uint32_t width, uint32_t height, int subPassId, void* stream)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (int rc = camContribCheck(cam, outDev, colorsDev, n, width, height, subPassId)) return rc;
  if (n == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  cam->renderPending = false;
  return camLaunchContrib(cam, (float4*)outDev, colorsDev, n, subPassId, (hipStream_t)stream, c->ev0, c->ev1);
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_add_samples_contribution_block_dev"); }
extern "C" int hpt_cam_add_samples_contribution_block(hpt_cam* cam, float* out, const float* colors, uint32_t n, uint32_t width, uint32_t height, int subPassId)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (int rc = camContribCheck(cam, out, colors, n, width, height, subPassId)) return rc;
  if (n == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  DevBuf<float> dOut;                                          // the frame goes up (it is added to) and comes back, as in RayTraceBlock's host form
  const size_t nf = (size_t)width * height * 4, nc = (size_t)n * (cam->spectral ? 1u : 4u);
  return roundTrip(c, cam->tContrib, KERNEL_EVENTS,
                   [&]() -> int { HIPCHK(c, dOut.upload(out, nf)); HIPCHK(c, hipMemcpy(cam->dColors.p, colors, nc * 4, hipMemcpyHostToDevice)); return HPT_OK; },
                   [&]() -> int { return hpt_cam_add_samples_contribution_block_dev(cam, dOut.p, cam->dColors.p, n, width, height, subPassId, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(out, dOut.p, nf * 4, hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_add_samples_contribution_block"); }

extern "C" int hpt_cam_read_state(hpt_cam* cam, uint32_t* gens, float* waves, float* cos4, uint32_t n)
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (n > cam->batch) return c->fail(HPT_ERR_ARG, "hpt_cam_read_state: n exceeds the batch size");
  if (n == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize());
  if (gens)  HIPCHK(c, hipMemcpy(gens, cam->dGens.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (waves) HIPCHK(c, hipMemcpy(waves, cam->dWaves.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (cos4)  HIPCHK(c, hipMemcpy(cos4, cam->dCos4.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_read_state"); }

// main_with_cam_gpu.cpp:230-266: per pass and tile vkCmdFillBuffer(rayCol), MakeRaysBlockCmd, PathTraceFromInputRaysCmd, AddSamplesContributionBlockCmd,
// all on one stream; the host waits for nothing (the tile count rounds up: a short last tile instead of the reference's dropped remainder)
extern "C" int hpt_cam_render_dev(hpt_ctx* c, hpt_cam* cam, float* frameDev, uint32_t passes, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (!cam || cam->ctx != c) return c->fail(HPT_ERR_ARG, "hpt_cam_render_dev: the camera is null or belongs to another context");
  if (!frameDev) return c->fail(HPT_ERR_ARG, "hpt_cam_render_dev: the frame is null");
  if (int rc = camTileCheck(cam, "hpt_cam_render_dev", 0u, 0)) return rc;
  if (cam->kind == CAM_TABLE_LENS && cam->lensCount == 0u) return c->fail(HPT_ERR_ARG, "hpt_cam_render_dev: the table-lens camera has no lens lines (hpt_cam_set_lens)");
  if (!c->sceneUploaded || !c->paramsSet) return c->fail(HPT_ERR_STATE, "hpt_cam_render_dev before CommitDeviceData / UpdateMembersPlainData");
  if ((c->S.spectralMode != 0u) != (cam->spectral != 0)) return c->fail(HPT_ERR_ARG, "hpt_cam_render_dev: the camera's spectralMode and the integrator's m_spectral_mode differ");
  if (c->dGens.n < cam->batch || c->gensCount < cam->batch) return c->fail(HPT_ERR_STATE, "hpt_cam_render_dev: m_randomGens smaller than the batch size (InitRandomGens)");
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t channels = cam->spectral ? 1u : 4u;
  const uint64_t pixels = (uint64_t)cam->width * cam->height;
  const uint32_t tiles = (uint32_t)((pixels + cam->batch - 1u) / cam->batch);
  const uint64_t total = (uint64_t)tiles * passes;
  const uint32_t timed = (uint32_t)std::min<uint64_t>(total, CAM_TIMED_TILES);
  while (cam->ev.size() < (size_t)timed * 4 + 2) { hipEvent_t e = nullptr; HIPCHK(c, hipEventCreate(&e)); cam->ev.push_back(e); }
  cam->evTiles = timed; cam->renderPending = false;
  cam->tRender[1] = (float)total; cam->tRender[2] = (float)timed;
  if (total == 0u) return HPT_OK;
  hipEvent_t evFirst = cam->ev[(size_t)timed * 4], evLast = cam->ev[(size_t)timed * 4 + 1];
  HIPCHK(c, hipEventRecord(evFirst, st));
  uint64_t k = 0;
  for (uint32_t pass = 0; pass < passes; pass++)
    for (uint32_t sp = 0; sp < tiles; sp++, k++) {
      const uint32_t n = (uint32_t)std::min<uint64_t>(cam->batch, pixels - (uint64_t)sp * cam->batch);
      hipEvent_t* e = k < timed ? &cam->ev[(size_t)k * 4] : nullptr;
      HIPCHK(c, hipMemsetAsync(cam->dColors.p, 0, (size_t)n * channels * 4, st));
      if (int rc = camLaunchMake(cam, cam->dRayPos.p, cam->dRayDir.p, n, (int)sp, st, e ? e[0] : nullptr, e ? e[1] : nullptr)) return rc;
      if (int rc = hpt_path_trace_from_input_rays_block_dev(c, n, channels, (const float*)cam->dRayPos.p, (const float*)cam->dRayDir.p, cam->dColors.p, 1u, st)) return rc;
      if (e) HIPCHK(c, hipEventRecord(e[2], st));
      if (int rc = camLaunchContrib(cam, (float4*)frameDev, cam->dColors.p, n, (int)sp, st, nullptr, e ? e[3] : nullptr)) return rc;
    }
  HIPCHK(c, hipEventRecord(evLast, st));
  cam->renderPending = true;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_cam_render_dev"); }

extern "C" int hpt_cam_get_execution_time(hpt_cam* cam, const char* name, float out[4])
try {
  if (!cam) return HPT_ERR_ARG;
  hpt_ctx* c = cam->ctx;
  if (!name || !out) return c->fail(HPT_ERR_ARG, "GetExecutionTime: a null argument");
  if (cam->renderPending) {                                    // the last loop's events: make = e0..e1, trace = e1..e2 (with its queue reset), contribute = e2..e3
    (void)hipSetDevice(c->device);
    const size_t t4 = (size_t)cam->evTiles * 4;
    HIPCHK(c, hipEventSynchronize(cam->ev[t4 + 1]));
    double make = 0.0, trace = 0.0, contrib = 0.0;
    for (uint32_t k = 0; k < cam->evTiles; k++) {
      float a = 0.0f, b = 0.0f, d = 0.0f; hipEvent_t* e = &cam->ev[(size_t)k * 4];
      (void)hipEventElapsedTime(&a, e[0], e[1]); (void)hipEventElapsedTime(&b, e[1], e[2]); (void)hipEventElapsedTime(&d, e[2], e[3]);
      make += a; trace += b; contrib += d;
    }
    float whole = 0.0f; (void)hipEventElapsedTime(&whole, cam->ev[t4], cam->ev[t4 + 1]);
    cam->tMake[0] = (float)make; cam->tTrace[0] = (float)trace; cam->tContrib[0] = (float)contrib; cam->tRender[0] = whole;
    for (int i = 1; i < 4; i++) cam->tMake[i] = cam->tTrace[i] = cam->tContrib[i] = 0.0f;
    cam->renderPending = false;
  }
  const std::string n(name);
  const float* src = nullptr;
  if (n == "MakeRaysBlock" || n == "MakeRays") src = cam->tMake;
  else if (n == "AddSamplesContributionBlock" || n == "AddSamplesContribution") src = cam->tContrib;
  else if (n == "PathTraceFromInputRays" || n == "PathTraceFromInputRaysBlock") src = cam->tTrace;
  else if (n == "Render") src = cam->tRender;
  if (!src) return HPT_OK;
  for (int i = 0; i < 4; i++) out[i] = src[i];
  return HPT_OK;
}
catch (...) { return hptGuard(cam ? cam->ctx : nullptr, "hpt_cam_get_execution_time"); }

// ---- IntegratorQMC::PathTraceBlock (mlt/integrator_qmc.cpp:284-315; hpt_qmc.hip) -----------------------------------------------------------------
extern "C" int hpt_qmc_table(uint32_t out[341])
try {
  if (!out) return HPT_ERR_ARG;
  static_assert(hpt_qmc::DIMENSIONS * hpt_qmc::RESOLUTION == 341 && hpt_qmc::DIMENSIONS == (int)QMC_DIMENSIONS && hpt_qmc::RESOLUTION == (int)QMC_RESOLUTION, "11 x 31 table");
  hpt_qmc::buildTable(out);
  return HPT_OK;
}
catch (...) { return hptGuard(nullptr, "hpt_qmc_table"); }
extern "C" int hpt_qmc_layout(int dof, int spectral, int motion, uint32_t out[5])
try {
  if (!out) return HPT_ERR_ARG;
  hpt_qmc::layout(dof != 0, spectral != 0, motion != 0, out);
  return HPT_OK;
}
catch (...) { return hptGuard(nullptr, "hpt_qmc_layout"); }
// m_maxThreadId = min(numeric_limits<unsigned>::max(), pixelsNum * a_passNum) (integrator_qmc.cpp:293-294)
extern "C" uint32_t hpt_qmc_sample_count(uint32_t pixelsNum, uint32_t passNum)
try {
  const unsigned long long n = (unsigned long long)pixelsNum * (unsigned long long)passNum;
  return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}
catch (...) { (void)hptGuard(nullptr, "hpt_qmc_sample_count"); return 0u; }
// what the call needs, in the order the reference's driver makes its calls; `out` / records: at least one destination
// The state refusals the QMC and KMLT entries share, one condition each, so that both say the same thing in the same words
static int needCommitted(hpt_ctx* c, const std::string& who)
{ return (!c->sceneUploaded || !c->paramsSet) ? c->fail(HPT_ERR_STATE, who + " before CommitDeviceData / UpdateMembersPlainData") : HPT_OK; }
static int refuseSpectral(hpt_ctx* c, const std::string& who, const char* note)
{ return c->S.spectralMode != 0u ? c->fail(HPT_ERR_UNSUPPORTED, who + ": m_spectral_mode is not served (" + note + ")") : HPT_OK; }
static int needPacked(hpt_ctx* c, const std::string& who)
{ return c->packedCount != (uint)(c->S.winWidth * c->S.winHeight) ? c->fail(HPT_ERR_STATE, who + " before PackXYBlock") : HPT_OK; }
static int needFilmTablesRGB(hpt_ctx* c)
{ return (c->hasFilm && !c->filmTablesRGB) ? c->fail(HPT_ERR_ARG, "thin film: m_precomp_thin_films holds no RGB table for a film (LoadScene precomputes every film in RGB mode, sized by its thickness map)") : HPT_OK; }
static int needFilmTablesSpectral(hpt_ctx* c)
{ return (c->hasFilm && !c->filmTablesSpectral) ? c->fail(HPT_ERR_ARG, "thin film: m_precomp_thin_films was precomputed for RGB rendering (LoadScene sizes the tables by m_spectral_mode)") : HPT_OK; }
// The scope of the spectral kernels the scene needs, chosen as PathTraceBlock chooses it (0 .. 3: hpt_decl.h), and the resident grid of a
// persistent spectral kernel of that scope: what spectral QMC and spectral MLT both launch with
static int spectralScope(const hpt_ctx* c)
{
  bool heavy = c->S.lensCount != 0u || c->S.envTexId != 0xFFFFFFFFu || c->S.envCamBackId != 0xFFFFFFFFu || c->spectralHeavyMats;
  for (const uint lg : c->hLightGeom) heavy = heavy || lg == LIGHT_GEOM_ENV;
  return (heavy && c->fewMaterialTypes) ? 3 : (heavy ? 2 : (c->spectralGltfMats ? 1 : 0));
}
static int spectralGridBlocks(const hpt_ctx* c, int scope)
{ return c->numCUs * (c->blocksPerCU > 0 ? c->blocksPerCU : (scope == 2 ? HPT_SPEC_WIDE_WAVES : HPT_SPEC_WAVES)); }
static uint spectralLastWide(const hpt_ctx* c)
{ return (c->S.megaWide != 0u && c->S.flatMode != 0u && c->nodes4Count != 0u && c->S.motion == 0u) ? 1u : 0u; }
static int qmc_check(hpt_ctx* c, uint32_t channels, const void* out, const void* sampleColor, const void* samplePixel, const void* sampleWaves = nullptr)
{
  const std::string who("PathTraceBlockQMC");
  if (!out && !sampleColor && !samplePixel && !sampleWaves) return c->fail(HPT_ERR_ARG, "PathTraceBlockQMC: no frame and no sample records to write");
  if ((sampleColor == nullptr) != (samplePixel == nullptr)) return c->fail(HPT_ERR_ARG, "PathTraceBlockQMC: the sample records come as a pair (colours and pixel indices)");
  if (sampleWaves != nullptr && sampleColor == nullptr) return c->fail(HPT_ERR_ARG, "PathTraceBlockQMC: the wavelength records come with the colour and pixel records, not alone");
  if (int rc = needCommitted(c, who)) return rc;
  const bool spectral = c->qmcSpectral && c->S.spectralMode != 0u;        // hpt_set_option("qmc_spectral", 1): pathTraceQmcSpectralKernel
  if (!spectral) {
    if (int rc = refuseSpectral(c, who, "the spectral kernels are a separate family; hpt_qmc_layout still answers for it, hpt_set_option(\"qmc_spectral\", 1) turns spectral QMC on")) return rc;
    if (channels > 4u) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlockQMC: channels above 4 are the wavelength layers of spectral rendering");
  }
  if (channels == 2u || channels == 0u) return c->fail(HPT_ERR_UNSUPPORTED, "PathTraceBlockQMC: a framebuffer of 1, 3 or 4 channels (three components are written per pixel)");
  if (int rc = needPacked(c, who)) return rc;
  if (c->gensCount == 0u) return c->fail(HPT_ERR_ARG, "PathTraceBlockQMC before InitRandomGens: sample s runs on generator s % m_randomGens.size()");
  if (spectral) return needFilmTablesSpectral(c);
  return needFilmTablesRGB(c);
}
// pathTraceQmcSpectralKernel<.., SCOPE> over the traversal variants of launchSpectral
template <int SCOPE>
static void launchQmcSpectral(const DevScene& S, const Job& job, const QmcJob& q, int blocks, hipStream_t st, bool deep)
{
  const dim3 g(blocks), b(256);
  if (S.motion) {
    if (S.flatMode) { if (deep) pathTraceQmcSpectralKernel<true, true, false, true, SCOPE><<<g, b, 0, st>>>(S, job, q); else pathTraceQmcSpectralKernel<false, true, false, true, SCOPE><<<g, b, 0, st>>>(S, job, q); }
    else            { if (deep) pathTraceQmcSpectralKernel<true, false, false, true, SCOPE><<<g, b, 0, st>>>(S, job, q); else pathTraceQmcSpectralKernel<false, false, false, true, SCOPE><<<g, b, 0, st>>>(S, job, q); }
  }
  else if (S.sweep)     pathTraceQmcSpectralKernel<false, false, true, false, SCOPE><<<g, b, 0, st>>>(S, job, q);
  else if (S.flatMode)  { if (deep) pathTraceQmcSpectralKernel<true, true, false, false, SCOPE><<<g, b, 0, st>>>(S, job, q); else pathTraceQmcSpectralKernel<false, true, false, false, SCOPE><<<g, b, 0, st>>>(S, job, q); }
  else                  { if (deep) pathTraceQmcSpectralKernel<true, false, false, false, SCOPE><<<g, b, 0, st>>>(S, job, q); else pathTraceQmcSpectralKernel<false, false, false, false, SCOPE><<<g, b, 0, st>>>(S, job, q); }
}
extern "C" int hpt_path_trace_qmc_block_dev2(hpt_ctx* c, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                             float* sampleColorDev, uint32_t* samplePixelDev, float* sampleWavesDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = qmc_check(c, channels, outDev, sampleColorDev, samplePixelDev, sampleWavesDev)) return rc;
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t samples = hpt_qmc_sample_count(pixelsNum, passNum);
  if (samples == 0u) return HPT_OK;
  // "qmc_wavefront" ("Wavefront form"): the generator slots with work are the pool's slots, so the call goes where a PathTraceBlock of
  // that many pixels would; what wfShadeQmcKernel does not serve keeps the megakernel. A slot's samples are its pass count in the status word: more
  // than that holds is refused here, before the table, the queue, the frame, the records or a generator is touched.
  const uint slots = std::min(c->gensCount, samples);
  const bool wave = c->qmcWavefront && c->S.spectralMode == 0u && c->S.sweep == 0u && !c->hasFilm && c->S.traceDepth > 0u && !c->instrument &&
                    useWavefront(c, false, false, false, slots);
  if (wave && (samples - 1u) / c->gensCount + 1u > WF_MAX_PASSES)
    return c->fail(HPT_ERR_ARG, "PathTraceBlockQMC under the wavefront schedule: generator slot 0 would run " + std::to_string((samples - 1u) / c->gensCount + 1u) +
                                " samples, above 16777215 (0xFFFFFF), all that a pool slot's status word holds; use more generators, split the call, or render it with "
                                "hpt_set_option(\"qmc_wavefront\", 0)");
  if (c->dQmcTable.n == 0) {                                               // qmc::init in IntegratorQMC's constructor
    uint32_t table[341];
    hpt_qmc::buildTable(table);
    HIPCHK(c, c->dQmcTable.upload(table, 341));
  }
  DevScene Sq = c->S; Sq.shadeTris = nullptr;                             // every BSDF branch gathers through the index chain: the walk reports primitive ids
  const uint n = c->gensCount;
  uint32_t lay[5];
  const bool spectral = c->S.spectralMode != 0u;                          // (qmc_check let it through: the option is on)
  hpt_qmc::layout(c->S.camLensRadius > 0.0f || c->S.lensCount != 0u, spectral, c->S.motion != 0u, lay);       // EnableQMC
  QmcJob q; std::memset(&q, 0, sizeof(q));
  q.table = c->dQmcTable.p; q.samples = samples; q.gensCount = n;
  q.dofDim = lay[0]; q.spdDim = lay[1]; q.motionDim = lay[2]; q.matDim = lay[3]; q.lgtDim = lay[4];
  q.sampleColor = (float4*)sampleColorDev; q.samplePixel = samplePixelDev; q.sampleWaves = (float4*)sampleWavesDev;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidCount = std::min(n, samples); job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  job.gens = c->dGens.p; job.packedXY = c->dPackedXY.p; job.packedCount = c->packedCount;
  if (wave) {                                                              // work item k is generator slot k: one contiguous window
    job.tidBegin = 0u; job.tidChunk = 0x40000000u; job.tidStride = 1u; job.tidEnd = job.tidCount;
    c->lastSchedule = 2; c->lastShadeRecords = 0u; c->lastWide = wfWide(c) ? 1u : 0u;
    c->lastDeep = (c->lastWide ? c->stackNeeded4 : c->stackNeeded) > (uint)LDS_STACK ? 1u : 0u;
    return launch_wavefront(c, job, st, false, -1, nullptr, &q);
  }
  const int scope = spectral ? spectralScope(c) : 0;
  const int grid = !spectral ? gridBlocks(c, false, true) : spectralGridBlocks(c, scope);
  const int blocks = (int)std::min<size_t>((size_t)grid, ((size_t)job.tidCount + 255) / 256);
  HIPCHK(c, c->dQueue.alloc(1));
  HIPCHK(c, hipMemsetAsync(c->dQueue.p, 0, 4, st));
  job.queue = c->dQueue.p;
  const bool deep = megaStackNeeded(c) > (uint)LDS_STACK;
  const dim3 g(blocks), b(256);
  if (spectral) {
    return launchFrame(c, (size_t)blocks * 256, st, [&]() {
      c->lastSchedule = 1; c->lastShadeRecords = 0u; c->lastDeep = deep ? 1u : 0u;
      c->lastWide = spectralLastWide(c);
      job.stackOverflow = c->dStackOvf.p; job.gridLanes = (uint)blocks * 256u;
      if (scope == 3) launchQmcSpectral<3>(c->S, job, q, blocks, st, deep);
      else if (scope == 2) launchQmcSpectral<2>(c->S, job, q, blocks, st, deep);
      else if (scope == 1) launchQmcSpectral<1>(c->S, job, q, blocks, st, deep);
      else launchQmcSpectral<0>(c->S, job, q, blocks, st, deep);
    });
  }
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    c->lastSchedule = 1; c->lastShadeRecords = 0u; c->lastDeep = deep ? 1u : 0u;
    c->lastWide = (c->S.motion == 0u && (HPT_FLAT_WIDE || c->S.megaWide != 0u) && c->S.flatMode != 0u && c->nodes4Count != 0u) ? 1u : 0u;
    job.stackOverflow = c->dStackOvf.p; job.gridLanes = (uint)blocks * 256u;
    if (c->S.motion != 0u) {
      if (c->S.flatMode) { if (deep) pathTraceQmcKernel<true, true, true, false><<<g, b, 0, st>>>(Sq, job, q); else pathTraceQmcKernel<false, true, true, false><<<g, b, 0, st>>>(Sq, job, q); }
      else               { if (deep) pathTraceQmcKernel<true, false, true, false><<<g, b, 0, st>>>(Sq, job, q); else pathTraceQmcKernel<false, false, true, false><<<g, b, 0, st>>>(Sq, job, q); }
    }
    else if (c->S.sweep)    pathTraceQmcKernel<false, false, false, true><<<g, b, 0, st>>>(Sq, job, q);
    else if (c->S.flatMode) { if (deep) pathTraceQmcKernel<true, true, false, false><<<g, b, 0, st>>>(Sq, job, q); else pathTraceQmcKernel<false, true, false, false><<<g, b, 0, st>>>(Sq, job, q); }
    else                    { if (deep) pathTraceQmcKernel<true, false, false, false><<<g, b, 0, st>>>(Sq, job, q); else pathTraceQmcKernel<false, false, false, false><<<g, b, 0, st>>>(Sq, job, q); }
  });
}
catch (...) { return hptGuard(c, "hpt_path_trace_qmc_block_dev2"); }
extern "C" int hpt_path_trace_qmc_block_dev(hpt_ctx* c, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                            float* sampleColorDev, uint32_t* samplePixelDev, void* stream)
{ return hpt_path_trace_qmc_block_dev2(c, pixelsNum, channels, outDev, passNum, sampleColorDev, samplePixelDev, nullptr, stream); }
// host-pointer form: the caller's frame goes up, is added to and comes back; slots as path_trace_host fills them
extern "C" int hpt_path_trace_qmc_block(hpt_ctx* c, uint32_t pixelsNum, uint32_t channels, float* out, uint32_t passNum)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = qmc_check(c, channels, out, nullptr, nullptr)) return rc;
  (void)hipSetDevice(c->device);
  if (hpt_qmc_sample_count(pixelsNum, passNum) == 0u) return HPT_OK;
  return roundTrip(c, c->tSlots[T_PATH_TRACE_QMC], out, (size_t)c->packedCount * channels, true,
                   [&](float* d) { return hpt_path_trace_qmc_block_dev(c, pixelsNum, channels, d, passNum, nullptr, nullptr, nullptr); });
}
catch (...) { return hptGuard(c, "hpt_path_trace_qmc_block"); }

// ---- IntegratorKMLT (mlt/integrator_kmlt.cpp; hpt_kmlt.hip) ---------------------------------------------------------------------------------
// m_randsPerThread = AlignedSize(PER_BOUNCE * m_traceDepth + BOUNCE_START, 16) (:33-40, 235-244, 262)
extern "C" uint32_t hpt_kmlt_state_size(uint32_t traceDepth)
try {
  const unsigned long long n = 10ull * traceDepth + 6ull;
  return (uint32_t)((n + 15ull) / 16ull * 16ull);
}
catch (...) { (void)hptGuard(nullptr, "hpt_kmlt_state_size"); return 0u; }

// what both entries need of the context, in the order of qmc_check
static int kmlt_check(hpt_ctx* c, const char* who)
{
  const std::string w(who);
  if (int rc = needCommitted(c, w)) return rc;
  const bool spectral = c->kmltSpectral && c->S.spectralMode != 0u;       // hpt_set_option("kmlt_spectral", 1): the spectral MLT kernels
  if (!spectral) { if (int rc = refuseSpectral(c, w, "spectral MLT is opt-in: hpt_set_option(\"kmlt_spectral\", 1) turns it on")) return rc; }
  if (int rc = needPacked(c, w)) return rc;
  return spectral ? needFilmTablesSpectral(c) : needFilmTablesRGB(c);
}
// f gets the spectral scope (0 .. 3) as a compile-time constant
template <class F>
static void spectralScopeDispatch(int scope, F f)
{
  if (scope == 3) f(std::integral_constant<int, 3>());
  else if (scope == 2) f(std::integral_constant<int, 2>());
  else if (scope == 1) f(std::integral_constant<int, 1>());
  else f(std::integral_constant<int, 0>());
}
// the traversal variants pathTraceQmcKernel is dispatched over; f gets (DEEP, FLAT, MOTION, SWEEP) as compile-time constants
template <class F>
static void kmltDispatch(const hpt_ctx* c, bool deep, F f)
{
  const std::true_type T; const std::false_type N;
  if (c->S.motion != 0u) {
    if (c->S.flatMode) { if (deep) f(T, T, T, N); else f(N, T, T, N); }
    else               { if (deep) f(T, N, T, N); else f(N, N, T, N); }
  }
  else if (c->S.sweep)    f(N, N, N, T);
  else if (c->S.flatMode) { if (deep) f(T, T, N, N); else f(N, T, N, N); }
  else                    { if (deep) f(T, N, N, N); else f(N, N, N, N); }
}
static void kmltNoteLaunch(hpt_ctx* c, bool deep)
{
  c->lastSchedule = 1; c->lastShadeRecords = 0u; c->lastDeep = deep ? 1u : 0u;
  c->lastWide = (c->S.motion == 0u && (HPT_FLAT_WIDE || c->S.megaWide != 0u) && c->S.flatMode != 0u && c->nodes4Count != 0u) ? 1u : 0u;
}

extern "C" int hpt_path_trace_pss_dev2(hpt_ctx* c, const float* xDev, uint32_t n, uint32_t strideFloats, float* color4fDev, uint32_t* pixelDev,
                                       float* waves4fDev, float* accum4fDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (!xDev || !color4fDev || !pixelDev) return c->fail(HPT_ERR_ARG, "PathTracePSS: null pointer (the vectors, the colours and the pixel indices are all needed)");
  if (int rc = kmlt_check(c, "PathTracePSS")) return rc;
  const bool spectral = c->S.spectralMode != 0u;                          // (kmlt_check let it through: the option is on)
  if (!spectral && (waves4fDev || accum4fDev)) return c->fail(HPT_ERR_ARG, "PathTracePSS: the wavelength and raw-radiance records exist under m_spectral_mode only (an RGB path has no wavelengths)");
  const uint32_t stateSize = hpt_kmlt_state_size(c->S.traceDepth);
  if (strideFloats < stateSize) return c->fail(HPT_ERR_ARG, "PathTracePSS: strideFloats is below hpt_kmlt_state_size(traceDepth) = " + std::to_string(stateSize));
  (void)hipSetDevice(c->device);
  if (n == 0u) return HPT_OK;
  hipStream_t st = (hipStream_t)stream;
  DevScene Sq = c->S; Sq.shadeTris = nullptr;                             // every BSDF branch gathers through the index chain
  PssJob job; std::memset(&job, 0, sizeof(job));
  job.x = xDev; job.n = n; job.vecStride = strideFloats; job.stateSize = stateSize;
  job.color = (float4*)color4fDev; job.pixel = pixelDev; job.packedXY = c->dPackedXY.p; job.packedCount = c->packedCount;
  const uint blocks = (uint)(((size_t)n + 255) / 256);
  const bool deep = megaStackNeeded(c) > (uint)LDS_STACK;
  const dim3 g(blocks), b(256);
  if (spectral) {
    job.waves = (float4*)waves4fDev; job.accum = (float4*)accum4fDev;
    return launchFrame(c, (size_t)blocks * 256, st, [&]() {
      kmltNoteLaunch(c, deep); c->lastWide = spectralLastWide(c);
      job.stackOverflow = c->dStackOvf.p; job.gridLanes = blocks * 256u;
      spectralScopeDispatch(spectralScope(c), [&](auto sc) {
        constexpr int SC = decltype(sc)::value;
        kmltDispatch(c, deep, [&](auto dp, auto flat, auto motion, auto sweep) { pathTracePssSpectralKernel<dp(), flat(), sweep(), motion(), SC><<<g, b, 0, st>>>(c->S, job); });
      });
    });
  }
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    kmltNoteLaunch(c, deep);
    job.stackOverflow = c->dStackOvf.p; job.gridLanes = blocks * 256u;
    kmltDispatch(c, deep, [&](auto dp, auto flat, auto motion, auto sweep) { pathTracePssKernel<dp(), flat(), motion(), sweep()><<<g, b, 0, st>>>(Sq, job); });
  });
}
catch (...) { return hptGuard(c, "hpt_path_trace_pss_dev2"); }
extern "C" int hpt_path_trace_pss_dev(hpt_ctx* c, const float* xDev, uint32_t n, uint32_t strideFloats, float* color4fDev, uint32_t* pixelDev, void* stream)
{ return hpt_path_trace_pss_dev2(c, xDev, n, strideFloats, color4fDev, pixelDev, nullptr, nullptr, stream); }

// C of a call: the option, or one chain per lane of the resident grid, reduced until every chain has a step
static int kmlt_chain_count(hpt_ctx* c, unsigned long long total, uint& chains)
{
  if (c->kmltChains != 0u) {
    if ((unsigned long long)c->kmltChains > total) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: kmlt_chains exceeds pixelsNum * a_passNum (a chain would have no step)");
    chains = c->kmltChains;
  } else {
    const bool spectral = c->kmltSpectral && c->S.spectralMode != 0u;     // the spectral chain kernel's resident grid is its scope's
    const int grid = spectral ? spectralGridBlocks(c, spectralScope(c)) : gridBlocks(c, false, true);
    chains = (uint)std::min<unsigned long long>((unsigned long long)grid * 256ull, total);
  }
  return HPT_OK;
}

extern "C" int hpt_kmlt_chain_count(hpt_ctx* c, uint32_t pixelsNum, uint32_t passNum, uint32_t* chainsOut, uint32_t* stepsOut)
try {
  if (!c || !chainsOut || !stepsOut) return HPT_ERR_ARG;
  *chainsOut = *stepsOut = 0u;
  const unsigned long long total = (unsigned long long)pixelsNum * (unsigned long long)passNum;
  if (total == 0ull) return HPT_OK;
  uint chains = 0;
  if (int rc = kmlt_chain_count(c, total, chains)) return rc;
  if (total / chains > 0xFFFFFFFEull) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: more than 2^32 - 2 steps per chain: raise kmlt_chains");
  *chainsOut = chains; *stepsOut = (uint32_t)(total / chains);
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_kmlt_chain_count"); }

extern "C" int hpt_path_trace_kmlt_block_dev(hpt_ctx* c, uint32_t pixelsNum, uint32_t channels, float* outDev, uint32_t passNum,
                                             int normalize, hpt_kmlt_records* rec, double* stats4Dev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (c->paramsSet && c->S.renderLayer == FB_DIRECT)                       // :250-251
    return hpt_path_trace_qmc_block_dev(c, pixelsNum, channels, outDev, passNum, nullptr, nullptr, stream);
  if (!outDev) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: null frame");
  if (channels != 4u) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: channels must be 4 (the contributions are written at pixel * 4 whatever it is)");
  if (normalize < 0 || normalize > 2) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: normalize is 0 (chains only), 1 (chains, then the normalisation) or 2 (the normalisation of the last call's chains only)");
  if (int rc = kmlt_check(c, "PathTraceBlockKMLT")) return rc;
  if (pixelsNum > c->packedCount) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: pixelsNum exceeds winWidth * winHeight");
  (void)hipSetDevice(c->device);
  const unsigned long long total = (unsigned long long)pixelsNum * (unsigned long long)passNum;
  if (total == 0ull) return HPT_OK;
  hipStream_t st = (hipStream_t)stream;
  uint chains = 0;
  if (normalize == 2) {
    if (c->kmltLastChains == 0u) return c->fail(HPT_ERR_STATE, "PathTraceBlockKMLT: normalize = 2 before any chains were run on this context");
    chains = c->kmltLastChains;
  } else if (int rc = kmlt_chain_count(c, total, chains)) return rc;
  const unsigned long long steps64 = total / chains;                       // samplesPerPass: the integer quotient, the remainder is dropped (:268)
  if (steps64 > 0xFFFFFFFEull) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: more than 2^32 - 2 steps per chain: raise kmlt_chains");
  const uint steps = (uint)steps64;
  HIPCHK(c, c->dKmltStats.alloc(4));
  double* stats = stats4Dev ? stats4Dev : c->dKmltStats.p;
  auto normalise = [&]() {
    kmltStatsKernel<<<dim3(1), dim3(256), 0, st>>>((const float4*)outDev, pixelsNum, passNum, chains, c->dKmltAccum.p, c->dKmltLarge.p, c->dKmltAccept.p, stats);
    const size_t n = (size_t)pixelsNum * 4u;
    if (normalize != 0) kmltScaleKernel<<<dim3((uint)((n + 255) / 256)), dim3(256), 0, st>>>(outDev, n, stats);
  };
  if (normalize != 2) {
    const uint32_t stateSize = hpt_kmlt_state_size(c->S.traceDepth);
    HIPCHK(c, c->dKmltCur.alloc((size_t)stateSize * chains)); HIPCHK(c, c->dKmltProp.alloc((size_t)stateSize * chains));
    HIPCHK(c, c->dKmltAccum.alloc(chains)); HIPCHK(c, c->dKmltLarge.alloc(chains)); HIPCHK(c, c->dKmltAccept.alloc(chains));
    DevScene Sq = c->S; Sq.shadeTris = nullptr;
    KmltJob job; std::memset(&job, 0, sizeof(job));
    job.chains = chains; job.steps = steps; job.stateSize = stateSize; job.cur = c->dKmltCur.p; job.prop = c->dKmltProp.p; job.outColor = outDev;
    job.packedXY = c->dPackedXY.p; job.packedCount = c->packedCount;
    job.accumBrightness = c->dKmltAccum.p; job.largeSteps = c->dKmltLarge.p; job.accept = c->dKmltAccept.p;
    if (rec) {
      job.recLarge = rec->isLarge; job.recAccepted = rec->accepted; job.recA = rec->a; job.recColor = (float4*)rec->color; job.recPixel = rec->pixel;
      job.recOldPixel = rec->oldPixel; job.recInitColor = (float4*)rec->initColor; job.recInitPixel = rec->initPixel; job.recProposals = rec->proposals;
      job.recContribX = (float4*)rec->contribAtX; job.recContribY = (float4*)rec->contribAtY;
    }
    const uint blocks = (chains + 255u) / 256u;
    const bool deep = megaStackNeeded(c) > (uint)LDS_STACK;
    const dim3 g(blocks), b(256);
    if (int rc = launchFrame(c, (size_t)blocks * 256, st, [&]() {           // the event pair spans the chains and the normalisation
      kmltNoteLaunch(c, deep);
      job.stackOverflow = c->dStackOvf.p; job.gridLanes = blocks * 256u;
      if (c->S.spectralMode != 0u) {                                        // (kmlt_check let it through: the option is on)
        c->lastWide = spectralLastWide(c);
        spectralScopeDispatch(spectralScope(c), [&](auto sc) {
          constexpr int SC = decltype(sc)::value;
          kmltDispatch(c, deep, [&](auto dp, auto flat, auto motion, auto sweep) { kmltChainSpectralKernel<dp(), flat(), sweep(), motion(), SC><<<g, b, 0, st>>>(c->S, job); });
        });
      }
      else kmltDispatch(c, deep, [&](auto dp, auto flat, auto motion, auto sweep) { kmltChainKernel<dp(), flat(), motion(), sweep()><<<g, b, 0, st>>>(Sq, job); });
      normalise();
    })) return rc;
    c->kmltLastChains = chains;
    return HPT_OK;
  }
  return launchFrame(c, 256, st, normalise);
}
catch (...) { return hptGuard(c, "hpt_path_trace_kmlt_block_dev"); }
// host-pointer form: the caller's frame (zero-filled, as main.cpp has it) goes up, is added to and scaled, and comes back
extern "C" int hpt_path_trace_kmlt_block(hpt_ctx* c, uint32_t pixelsNum, uint32_t channels, float* out, uint32_t passNum)
try {
  if (!c) return HPT_ERR_ARG;
  if (c->paramsSet && c->S.renderLayer == FB_DIRECT) return hpt_path_trace_qmc_block(c, pixelsNum, channels, out, passNum);
  if (!out) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: null frame");
  if (channels != 4u) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: channels must be 4 (the contributions are written at pixel * 4 whatever it is)");
  if (int rc = kmlt_check(c, "PathTraceBlockKMLT")) return rc;
  if (pixelsNum > c->packedCount) return c->fail(HPT_ERR_ARG, "PathTraceBlockKMLT: pixelsNum exceeds winWidth * winHeight");
  (void)hipSetDevice(c->device);
  if ((unsigned long long)pixelsNum * passNum == 0ull) return HPT_OK;
  uint chains = 0;
  if (int rc = kmlt_chain_count(c, (unsigned long long)pixelsNum * passNum, chains)) return rc;   // (refused before the frame is copied)
  return roundTrip(c, c->tSlots[T_KMLT], out, (size_t)c->packedCount * 4u, true,
                   [&](float* d) { return hpt_path_trace_kmlt_block_dev(c, pixelsNum, channels, d, passNum, 1, nullptr, nullptr, nullptr); });
}
catch (...) { return hptGuard(c, "hpt_path_trace_kmlt_block"); }

// ---- differentiable rendering ---------------------------------------------------------------------------------------------------------
extern "C" int hpt_reset_diff_tex(hpt_ctx* c)
try {
  if (!c) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  for (TexRec& t : c->hTextures) { t.diffOffset = ~0ull; t.diffW = t.diffH = t.diffChannels = 0; }
  c->gradSize = 0; c->diffLightFirst = c->diffLightCount = 0; c->diffLightOff = 0;
  if (!c->hTextures.empty()) HIPCHK(c, c->dTextures.upload(c->hTextures.data(), c->hTextures.size()));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_reset_diff_tex"); }

extern "C" int hpt_put_diff_tex2d(hpt_ctx* c, uint32_t texId, uint32_t w, uint32_t h, uint32_t channels, uint64_t* outOffset, uint64_t* outSize)
try {
  if (!c || !outOffset || !outSize) return HPT_ERR_ARG;
  if (texId >= c->hTextures.size()) {                                     // reference: prints and returns (size_t(-1), 0) (integrator_dr.cpp:35-39)
    *outOffset = ~0ull; *outSize = 0;
    return c->fail(HPT_ERR_ARG, "[IntegratorDR::PutDiffTex2D]: bad tex id = " + std::to_string(texId));
  }
  if (channels != 1 && channels != 4) return c->fail(HPT_ERR_ARG, "PutDiffTex2D: channels must be 1 or 4");
  if (channels == 4 && (c->gradSize % 4) != 0) return c->fail(HPT_ERR_ARG, "PutDiffTex2D: 4-channel textures must start at a multiple of 4 floats");
  if (channels != 4 && c->drEnvironment && ((c->paramsSet && texId == c->S.envTexId) || (c->S.envLightId < c->hLightTex.size() && texId == c->hLightTex[c->S.envLightId])))
    return c->fail(HPT_ERR_ARG, "PutDiffTex2D: the environment map takes 4 channels (dr_environment reads its rgb)");
  (void)hipSetDevice(c->device);
  TexRec& t = c->hTextures[texId];
  t.diffOffset = c->gradSize; t.diffW = w; t.diffH = h; t.diffChannels = channels;
  const uint64_t sz = (uint64_t)w * h * channels;
  if (c->gradSize + sz > (uint64_t(1) << 31)) return c->fail(HPT_ERR_UNSUPPORTED, "PutDiffTex2D: more than 2^31 parameters (the gradient scatter indexes a_dataGrad with 31 bits)");
  *outOffset = c->gradSize; *outSize = sz;
  c->gradSize += sz;
  HIPCHK(c, c->dTextures.upload(c->hTextures.data(), c->hTextures.size()));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_put_diff_tex2d"); }

// Light-colour gradients (no counterpart in the reference): lights [firstLight, firstLight + count) of the uploaded m_lights get an RGB gain each,
// four floats per light appended to the parameter vector as hpt_put_diff_tex2d appends a texture (the fourth is padding: never read, its gradient
// stays 0). PathTraceDR / PathTraceVJP then evaluate such a light from intensity * gain and return d loss / d gain in a_dataGrad.
extern "C" int hpt_put_diff_lights(hpt_ctx* c, uint32_t firstLight, uint32_t count, uint64_t* outOffset, uint64_t* outSize)
try {
  if (!c) return HPT_ERR_ARG;
  if (!outOffset || !outSize) return c->fail(HPT_ERR_ARG, "PutDiffLights: null out-pointer");
  if (count == 0) return c->fail(HPT_ERR_ARG, "PutDiffLights: count is 0");
  if (!c->sceneUploaded || (uint64_t)firstLight + count > c->S.numLights)
    return c->fail(HPT_ERR_ARG, "PutDiffLights: lights [" + std::to_string(firstLight) + ", " + std::to_string((uint64_t)firstLight + count) + ") reach past the " + std::to_string(c->sceneUploaded ? c->S.numLights : 0u) + " uploaded lights");
  if (c->diffLightCount != 0u) return c->fail(HPT_ERR_ARG, "PutDiffLights: lights are already registered on this context (hpt_reset_diff_tex clears the registration)");
  if ((c->gradSize % 4) != 0) return c->fail(HPT_ERR_ARG, "PutDiffLights: the gains must start at a multiple of 4 floats (as 4-channel textures)");
  const uint64_t sz = 4ull * count;
  if (c->gradSize + sz > (uint64_t(1) << 31)) return c->fail(HPT_ERR_UNSUPPORTED, "PutDiffLights: more than 2^31 parameters (the gradient scatter indexes a_dataGrad with 31 bits)");
  c->diffLightFirst = firstLight; c->diffLightCount = count; c->diffLightOff = c->gradSize;
  *outOffset = c->gradSize; *outSize = sz;
  c->gradSize += sz;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_put_diff_lights"); }

extern "C" int hpt_path_trace_dr_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, uint32_t passNum,
                                     const float* refDev, const float* dataDev, float* gradDev, size_t gradSize, float* lossDev, void* stream)
try {
  if (!c || !outDev || !refDev || !dataDev || !gradDev || !lossDev) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (gradSize < c->gradSize) return c->fail(HPT_ERR_ARG, "PathTraceDR: a_gradSize smaller than the registered differentiable textures");
  if (channels < 3) return c->fail(HPT_ERR_ARG, "PathTraceDR: channels must be 3 or 4");
  if (tidCount == 0 || passNum == 0) return HPT_OK;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidBegin = tidBegin; job.tidCount = tidCount; job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  job.refImg = refDev; job.data = dataDev; job.grad = gradDev; job.lossAccum = lossDev;
  return launch_path_trace(c, job, false, true, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_path_trace_dr_dev"); }

extern "C" int hpt_path_trace_dr(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum,
                                 const float* refImg, const float* data, float* dataGrad, size_t gradSize, float* outLoss)
try {
  if (!c || !out || !refImg || !data || !dataGrad) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, "PathTraceDR before UpdateMembersPlainData");
  const size_t n = (size_t)c->S.winWidth * c->S.winHeight * channels;
  float lossSum = 0.0f;
  const int rc = roundTrip(c, c->tSlots[T_DR], (tidCount && passNum) ? KERNEL_EVENTS : KERNEL_NONE,
    [&]() -> int {
      HIPCHK(c, c->dFrame.alloc(n)); HIPCHK(c, c->dRef.alloc(n)); HIPCHK(c, c->dData.alloc(gradSize)); HIPCHK(c, c->dGrad.alloc(gradSize)); HIPCHK(c, c->dLoss.alloc(1));
      HIPCHK(c, hipMemcpy(c->dFrame.p, out, n * 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(c->dRef.p, refImg, n * 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(c->dData.p, data, gradSize * 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemset(c->dGrad.p, 0, gradSize * 4));                   // memset(a_dataGrad, 0, ...) (integrator_dr.cpp:1139)
      HIPCHK(c, hipMemset(c->dLoss.p, 0, 4));
      return HPT_OK;
    },
    [&]() -> int { return hpt_path_trace_dr_dev(c, tidBegin, tidCount, channels, c->dFrame.p, passNum, c->dRef.p, c->dData.p, c->dGrad.p, gradSize, c->dLoss.p, nullptr); },
    [&]() -> int {
      HIPCHK(c, hipMemcpy(out, c->dFrame.p, n * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(dataGrad, c->dGrad.p, gradSize * 4, hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(&lossSum, c->dLoss.p, 4, hipMemcpyDeviceToHost));
      return HPT_OK;
    });
  if (rc == HPT_OK && outLoss) *outLoss = lossSum / float(c->S.winWidth * c->S.winHeight);   // avgLoss /= W*H (integrator_dr.cpp:1206)
  return rc;
}
catch (...) { return hptGuard(c, "hpt_path_trace_dr"); }

// ---- PathTraceVJP: PathTraceDR's paths with the caller's image adjoint as the seed of the reverse sweep (no counterpart in the reference) ------------
// dataGrad[j] += sum over pixels, samples, c of adjImg[pixel][c] * d C_s[c] / d data[j], C_s the sample's colour as it is added to out_color (not
// divided by a_passNum). What either form refuses before anything is launched or copied; launch_path_trace then refuses what PathTraceDR refuses.
static int vjp_check(hpt_ctx* c, uint32_t channels, const void* out, const void* adj, const void* data, const void* grad, size_t gradSize)
{
  if (!out || !data) return c->fail(HPT_ERR_ARG, "PathTraceVJP: out_color or a_data is null");
  if (gradSize < c->gradSize) return c->fail(HPT_ERR_ARG, "PathTraceDR: a_gradSize smaller than the registered differentiable textures");
  if (channels != 3u && channels != 4u) return c->fail(HPT_ERR_ARG, "PathTraceVJP: channels must be 3 or 4 (the stride of out_color and of the adjoint image)");
  if (adj && (!grad || gradSize == 0)) return c->fail(HPT_ERR_ARG, "PathTraceVJP: an adjoint image needs a_dataGrad and a non-zero a_gradSize");
  return HPT_OK;
}
extern "C" int hpt_path_trace_vjp_dev(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* outDev, uint32_t passNum,
                                      const float* adjDev, const float* dataDev, float* gradDev, size_t gradSize, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = vjp_check(c, channels, outDev, adjDev, dataDev, gradDev, gradSize)) return rc;
  (void)hipSetDevice(c->device);
  if (tidCount == 0 || passNum == 0) return HPT_OK;
  Job job; std::memset(&job, 0, sizeof(job));
  job.tidBegin = tidBegin; job.tidCount = tidCount; job.passNum = passNum; job.channels = channels; job.outColor = outDev;
  job.vjp = 1u; job.adjImg = adjDev; job.data = dataDev; job.grad = adjDev ? gradDev : nullptr;   // (no adjoint: nothing is swept, a_dataGrad is not touched)
  return launch_path_trace(c, job, false, true, (hipStream_t)stream);
}
catch (...) { return hptGuard(c, "hpt_path_trace_vjp_dev"); }

// host-pointer form: out_color goes up, is added to and comes back; with an adjoint image a_dataGrad is zeroed on the device and comes back whole
extern "C" int hpt_path_trace_vjp(hpt_ctx* c, uint32_t tidBegin, uint32_t tidCount, uint32_t channels, float* out, uint32_t passNum,
                                  const float* adjImg, const float* data, float* dataGrad, size_t gradSize)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = vjp_check(c, channels, out, adjImg, data, dataGrad, gradSize)) return rc;
  (void)hipSetDevice(c->device);
  if (!c->paramsSet) return c->fail(HPT_ERR_STATE, "PathTraceVJP before UpdateMembersPlainData");
  const size_t n = (size_t)c->S.winWidth * c->S.winHeight * channels;
  return roundTrip(c, c->tSlots[T_VJP], (tidCount && passNum) ? KERNEL_EVENTS : KERNEL_NONE,
    [&]() -> int {
      HIPCHK(c, c->dFrame.alloc(n)); HIPCHK(c, c->dData.alloc(std::max<size_t>(gradSize, 1)));
      HIPCHK(c, hipMemcpy(c->dFrame.p, out, n * 4, hipMemcpyHostToDevice));
      HIPCHK(c, hipMemcpy(c->dData.p, data, gradSize * 4, hipMemcpyHostToDevice));
      if (adjImg) {
        HIPCHK(c, c->dRef.alloc(n)); HIPCHK(c, c->dGrad.alloc(gradSize));
        HIPCHK(c, hipMemcpy(c->dRef.p, adjImg, n * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemset(c->dGrad.p, 0, gradSize * 4));
      }
      return HPT_OK;
    },
    [&]() -> int { return hpt_path_trace_vjp_dev(c, tidBegin, tidCount, channels, c->dFrame.p, passNum, adjImg ? c->dRef.p : nullptr, c->dData.p, adjImg ? c->dGrad.p : nullptr, gradSize, nullptr); },
    [&]() -> int {
      HIPCHK(c, hipMemcpy(out, c->dFrame.p, n * 4, hipMemcpyDeviceToHost));
      if (adjImg) HIPCHK(c, hipMemcpy(dataGrad, c->dGrad.p, gradSize * 4, hipMemcpyDeviceToHost));
      return HPT_OK;
    });
}
catch (...) { return hptGuard(c, "hpt_path_trace_vjp"); }

// ---- IntegratorDR::RayTraceDR (integrator_dr.cpp:396-459; hpt_raytrace_dr.hip) ------------------------------------------------------------------------
// what either form refuses, in the order the neighbouring entry points check: pointers, the calls made so far, tid, then the arguments of its own
static int rtdr_check(hpt_ctx* c, uint32_t tid, uint32_t channels, const void* out, const void* ref, const void* grad, size_t gradSize)
{
  if (int rc = pixelPassCheck(c, "RayTraceDR", "out_color", out, "tid", tid)) return rc;
  if (!ref) return c->fail(HPT_ERR_ARG, "RayTraceDR: a_refImg is null");
  if (channels != 3u && channels != 4u) return c->fail(HPT_ERR_ARG, "RayTraceDR: channels must be 3 or 4 (three floats of a_refImg are read per pixel at that stride)");
  if (gradSize < c->gradSize) return c->fail(HPT_ERR_ARG, "RayTraceDR: a_gradSize smaller than the registered differentiable textures");
  if (!grad && gradSize != 0) return c->fail(HPT_ERR_ARG, "RayTraceDR: a_dataGrad is null");
  return HPT_OK;
}
extern "C" int hpt_ray_trace_dr_dev(hpt_ctx* c, uint32_t tid, uint32_t channels, float* outDev, uint32_t passNum, const float* refDev, const float* dataDev,
                                    float* gradDev, size_t gradSize, float* lossPerPixelDev, float* lossAccumDev, void* stream)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = rtdr_check(c, tid, channels, outDev, refDev, gradDev, gradSize)) return rc;
  if (tid == 0u) return HPT_OK;
  (void)hipSetDevice(c->device);
  hipStream_t st = (hipStream_t)stream;
  const uint blocks = (tid + 255u) / 256u;
  const bool withGrad = c->drGradMode && dataDev != nullptr && gradDev != nullptr;   // Tex2DFetchAD's condition (integrator_dr.cpp:99) but for the texture's registration
  const float fPass = float(passNum);
  return launchFrame(c, (size_t)blocks * 256, st, [&]() {
    traversalDispatch(c, [&](auto flat, auto motion, auto sweep) {
      if (withGrad) rayTraceDrKernel<flat(), motion(), sweep(), true><<<dim3(blocks), dim3(256), 0, st>>>(c->S, c->dPackedXY.p, tid, channels, fPass, outDev, refDev, dataDev, gradDev, lossPerPixelDev, lossAccumDev, c->dStackOvf.p);
      else          rayTraceDrKernel<flat(), motion(), sweep(), false><<<dim3(blocks), dim3(256), 0, st>>>(c->S, c->dPackedXY.p, tid, channels, fPass, outDev, refDev, nullptr, nullptr, lossPerPixelDev, lossAccumDev, c->dStackOvf.p);
    });
  });
}
catch (...) { return hptGuard(c, "hpt_ray_trace_dr_dev"); }
// Host-pointer form: the frame goes up and comes back (missed pixels and pixels past tid keep the caller's floats), the gradient is zeroed on the
// device and comes back whole, and the per-pixel losses come back to be summed here as the reference sums them: in tid order, in float, each divided
// by a_passNum first (integrator_dr.cpp:417-430)
extern "C" int hpt_ray_trace_dr(hpt_ctx* c, uint32_t tid, uint32_t channels, float* out, uint32_t passNum,
                                const float* refImg, const float* data, float* dataGrad, size_t gradSize, float* outLoss)
try {
  if (!c) return HPT_ERR_ARG;
  if (int rc = rtdr_check(c, tid, channels, out, refImg, dataGrad, gradSize)) return rc;
  (void)hipSetDevice(c->device);
  if (outLoss) *outLoss = 0.0f;
  if (tid == 0u) { if (gradSize) std::memset(dataGrad, 0, gradSize * sizeof(float)); return HPT_OK; }   // memset(a_dataGrad, 0, ...) (integrator_dr.cpp:399), no pixel
  const size_t nOut = (size_t)c->packedCount * 4u, nRef = (size_t)c->packedCount * channels;
  DevBuf<float> dOut, dRefImg, dDat, dGr, dPix;
  std::vector<float> pix(tid);
  const int rc = roundTrip(c, c->tSlots[T_RAY_TRACE_DR], KERNEL_EVENTS,
    [&]() -> int {
      HIPCHK(c, dOut.upload(out, nOut)); HIPCHK(c, dRefImg.upload(refImg, nRef)); HIPCHK(c, dPix.alloc(tid));
      if (data && gradSize) HIPCHK(c, dDat.upload(data, gradSize));
      if (gradSize) { HIPCHK(c, dGr.alloc(gradSize)); HIPCHK(c, hipMemset(dGr.p, 0, gradSize * sizeof(float))); }
      return HPT_OK;
    },
    [&]() -> int { return hpt_ray_trace_dr_dev(c, tid, channels, dOut.p, passNum, dRefImg.p, (data && gradSize) ? dDat.p : nullptr, gradSize ? dGr.p : nullptr, gradSize, dPix.p, nullptr, nullptr); },
    [&]() -> int {
      HIPCHK(c, hipMemcpy(out, dOut.p, nOut * sizeof(float), hipMemcpyDeviceToHost));
      if (gradSize) HIPCHK(c, hipMemcpy(dataGrad, dGr.p, gradSize * sizeof(float), hipMemcpyDeviceToHost));
      HIPCHK(c, hipMemcpy(pix.data(), dPix.p, (size_t)tid * sizeof(float), hipMemcpyDeviceToHost));
      return HPT_OK;
    });
  if (rc != HPT_OK) return rc;
  float avgLoss = 0.0f;
  const float fPass = float(passNum);
  for (uint32_t i = 0; i < tid; i++) { const float share = pix[i] / fPass; avgLoss += share; }
  if (outLoss) *outLoss = avgLoss;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_ray_trace_dr"); }

extern "C" int hpt_adam_step_dev(hpt_ctx* c, float* state, const float* grad, float* momentum, float* gsq, size_t n, int iter, void* stream)
try {
  if (!c || !state || !grad || !momentum || !gsq) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (n == 0) return HPT_OK;
  const float gamma = 0.25f / float(iter / 100 + 1);
  const int blocks = (int)std::min<size_t>((n + 255) / 256, (size_t)c->numCUs * 8);
  adamStepKernel<<<dim3(blocks), dim3(256), 0, (hipStream_t)stream>>>(state, grad, momentum, gsq, n, gamma);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_adam_step_dev"); }

extern "C" int hpt_image2d4f_regularizer_dev(hpt_ctx* c, int w, int h, const float* data, float* grad, void* stream)
try {
  if (!c || !data || !grad || w < 0 || h < 0) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (w < 3 || h < 3) return HPT_OK;                                  // no interior pixel: the loss is identically zero
  image2D4fRegularizerKernel<<<dim3((w + 15) / 16, (h + 15) / 16), dim3(16, 16), 0, (hipStream_t)stream>>>(w, h, (const float4*)data, (float4*)grad);
  HIPCHK(c, hipGetLastError());
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_image2d4f_regularizer_dev"); }

extern "C" int hpt_image2d4f_regularizer(hpt_ctx* c, int w, int h, const float* data, float* grad)
try {
  if (!c || !data || !grad || w < 0 || h < 0) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  const size_t n = (size_t)w * h * 4;
  if (n == 0) return HPT_OK;
  DevBuf<float> dd, dg;
  return roundTrip(c, nullptr, KERNEL_UNTIMED,
                   [&]() -> int { HIPCHK(c, dd.upload(data, n)); HIPCHK(c, dg.upload(grad, n)); return HPT_OK; },
                   [&]() -> int { return hpt_image2d4f_regularizer_dev(c, w, h, dd.p, dg.p, nullptr); },
                   [&]() -> int { HIPCHK(c, hipMemcpy(grad, dg.p, n * sizeof(float), hipMemcpyDeviceToHost)); return HPT_OK; });
}
catch (...) { return hptGuard(c, "hpt_image2d4f_regularizer"); }

// ---- multi-GPU: RCCL collectives behind the C ABI (one context = one GPU = one rank) ---------------------------------------------------
// The path shards without any data-path exchange; what has to cross xGMI is one reduce(SUM) of the framebuffer per frame and,
// for PathTraceDR, one all_reduce(SUM) of a_dataGrad (and the loss) per optimisation iteration. librccl is dlopen'ed here instead of being
// linked, so that a process which already carries an RCCL (PyTorch bundles one) keeps using that copy.
namespace {
struct Id128 { char internal[128]; };         // ncclUniqueId (rccl.h:40-43), passed by value
struct RcclApi
{
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, Id128, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*Reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
RcclApi g_rccl;
const int RCCL_FLOAT32 = 7, RCCL_SUM = 0;       // ncclFloat32, ncclSum (rccl.h:448-466)

int loadRccl(hpt_ctx* c)
{
  if (g_rccl.AllReduce) return HPT_OK;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return c->fail(HPT_ERR_UNSUPPORTED, std::string("hpt_comm: cannot load librccl: ") + dlerror());
  c->rcclLib = lib;
  *(void**)&g_rccl.GetUniqueId = dlsym(lib, "ncclGetUniqueId");
  *(void**)&g_rccl.CommInitRank = dlsym(lib, "ncclCommInitRank");
  *(void**)&g_rccl.CommDestroy = dlsym(lib, "ncclCommDestroy");
  *(void**)&g_rccl.Reduce = dlsym(lib, "ncclReduce");
  *(void**)&g_rccl.AllReduce = dlsym(lib, "ncclAllReduce");
  *(void**)&g_rccl.GetErrorString = dlsym(lib, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.CommDestroy || !g_rccl.Reduce || !g_rccl.AllReduce) { g_rccl = RcclApi(); return c->fail(HPT_ERR_UNSUPPORTED, "hpt_comm: librccl lacks the expected entry points"); }
  return HPT_OK;
}
int rcclFail(hpt_ctx* c, int r, const char* what) { return c->fail(HPT_ERR_HIP, std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error")); }
} // namespace

extern "C" int hpt_comm_get_unique_id(hpt_ctx* c, void* id128)
try {
  if (!c || !id128) return HPT_ERR_ARG;
  int rc = loadRccl(c); if (rc) return rc;
  const int r = g_rccl.GetUniqueId(id128);
  return r ? rcclFail(c, r, "ncclGetUniqueId") : HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_comm_get_unique_id"); }
extern "C" int hpt_comm_init(hpt_ctx* c, int nranks, int rank, const void* id128)
try {
  if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return HPT_ERR_ARG;
  if (c->comm) return c->fail(HPT_ERR_STATE, "hpt_comm_init: communicator already initialised");
  int rc = loadRccl(c); if (rc) return rc;
  (void)hipSetDevice(c->device);
  Id128 id; std::memcpy(&id, id128, sizeof(id));
  const int r = g_rccl.CommInitRank(&c->comm, nranks, id, rank);
  if (r) { c->comm = nullptr; return rcclFail(c, r, "ncclCommInitRank"); }
  c->commRanks = nranks; c->commRank = rank;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_comm_init"); }
extern "C" int hpt_comm_destroy(hpt_ctx* c)
try {
  if (!c) return HPT_ERR_ARG;
  if (c->comm) { (void)hipSetDevice(c->device); (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; c->commRanks = 0; }
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_comm_destroy"); }
extern "C" int hpt_reduce_framebuffer(hpt_ctx* c, float* frameDev, size_t count, int root, void* stream)
try {
  if (!c || !frameDev) return HPT_ERR_ARG;
  if (!c->comm) return c->fail(HPT_ERR_STATE, "hpt_reduce_framebuffer before hpt_comm_init");
  (void)hipSetDevice(c->device);
  const int r = g_rccl.Reduce(frameDev, frameDev, count, RCCL_FLOAT32, RCCL_SUM, root, c->comm, (hipStream_t)stream);
  return r ? rcclFail(c, r, "ncclReduce") : HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_reduce_framebuffer"); }
extern "C" int hpt_allreduce_grad(hpt_ctx* c, float* gradDev, size_t count, void* stream)
try {
  if (!c || !gradDev) return HPT_ERR_ARG;
  if (!c->comm) return c->fail(HPT_ERR_STATE, "hpt_allreduce_grad before hpt_comm_init");
  (void)hipSetDevice(c->device);
  const int r = g_rccl.AllReduce(gradDev, gradDev, count, RCCL_FLOAT32, RCCL_SUM, c->comm, (hipStream_t)stream);
  return r ? rcclFail(c, r, "ncclAllReduce") : HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_allreduce_grad"); }

// ---- timing / instrumentation --------------------------------------------------------------------------------------------------------
static const struct { const char* name; const char* alias; TimeSlot slot; } TIME_NAMES[] = {   // all the names GetExecutionTime answers to
  { "PathTrace", "PathTraceBlock", T_PATH_TRACE },                        // integrator_pt_lgt.cpp:241-251
  { "NaivePathTrace", "NaivePathTraceBlock", T_NAIVE },
  { "PathTraceFromInputRays", "PathTraceFromInputRaysBlock", T_FROM_RAYS },
  { "PathTraceDR", "PathTraceDRBlock", T_DR },                            // integrator_dr2.cpp:82-88
  { "CastSingleRay", "CastSingleRayBlock", T_CAST_SINGLE_RAY },           // main.cpp:443
  { "PathTraceQMC", "PathTraceBlockQMC", T_PATH_TRACE_QMC },              // IntegratorQMC::PathTraceBlock's shadowPtTime (integrator_qmc.cpp:314)
  { "PathTraceKMLT", "PathTraceBlockKMLT", T_KMLT },                      // IntegratorKMLT::PathTraceBlock's shadowPtTime (integrator_kmlt.cpp:477)
  { "RayTrace", "RayTraceBlock", T_RAY_TRACE },                           // raytraceTime (integrator_pt_host.cpp:75-90)
  { "PathTraceVJP", nullptr, T_VJP },                                     // no counterpart: PathTraceDR's slots for the VJP form
  { "RayTraceDR", nullptr, T_RAY_TRACE_DR },                              // shadowPtTime (integrator_dr.cpp:441)
  { "DenoiseFrame", nullptr, T_DENOISE },                                 // no counterpart
  { "DenoiseFrameVar", nullptr, T_DENOISE_VAR },
};
extern "C" int hpt_get_execution_time(hpt_ctx* c, const char* name, float out[4])
try {
  if (!c || !name || !out) return HPT_ERR_ARG;
  for (const auto& t : TIME_NAMES)                                                           // unknown names leave `out` untouched, as the reference does
    if (std::strcmp(name, t.name) == 0 || (t.alias && std::strcmp(name, t.alias) == 0)) { for (int i = 0; i < 4; i++) out[i] = c->tSlots[t.slot][i]; break; }
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_execution_time"); }
extern "C" int hpt_set_instrumentation(hpt_ctx* c, int enabled) try { if (!c) return HPT_ERR_ARG; c->instrument = enabled != 0; return HPT_OK; }
catch (...) { return hptGuard(c, "hpt_set_instrumentation"); }
extern "C" int hpt_get_counters(hpt_ctx* c, uint64_t out[16])
try {
  if (!c || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (!c->dCounters.p) { for (int i = 0; i < 16; i++) out[i] = 0; return HPT_OK; }
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, c->dCounters.p, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_counters"); }
extern "C" int hpt_get_dr_counters(hpt_ctx* c, uint64_t out[16])
try {
  if (!c || !out) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  if (!c->dCounters.p) { for (int i = 0; i < 16; i++) out[i] = 0; return HPT_OK; }
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(out, (const uint64_t*)c->dCounters.p + 16, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_dr_counters"); }
extern "C" int hpt_set_tid_interleave(hpt_ctx* c, uint32_t chunk, uint32_t stride)
try {
  if (!c || (stride > 1 && (chunk == 0 || chunk % 64 != 0))) return HPT_ERR_ARG;
  c->tidChunk = chunk; c->tidStride = stride ? stride : 1;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_tid_interleave"); }
extern "C" int hpt_set_launch_config(hpt_ctx* c, int blocksPerCU) try { if (!c || blocksPerCU < 0 || blocksPerCU > 8) return HPT_ERR_ARG; c->blocksPerCU = blocksPerCU; return HPT_OK; }
catch (...) { return hptGuard(c, "hpt_set_launch_config"); }
extern "C" int hpt_set_schedule(hpt_ctx* c, int schedule, int refillBelow, int traceBlocksPerCU, int groups)
try {
  if (!c || schedule < 0 || schedule > 4 || refillBelow < 0 || refillBelow > 64 || traceBlocksPerCU < 0 || traceBlocksPerCU > 8 || groups < 0 || groups > 64) return HPT_ERR_ARG;
  c->wfGroupCount = groups;
  c->schedule = schedule;
  if (refillBelow > 0) c->wfRefillBelow = (uint)refillBelow;
  c->wfBlocksPerCU = traceBlocksPerCU;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_schedule"); }
extern "C" int hpt_set_option(hpt_ctx* c, const char* name, int value)
try {
  if (!c || !name || value < 0) return HPT_ERR_ARG;
  const std::string k(name);
  if (k == "wf_grace") c->wfGrace = (uint)value;                                      // trips after the queue ran dry before a trace wave suspends its rays (0: never)
  else if (k == "node_min") { c->nodeMinOverride = value & 63; c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; }
  else if (k == "refit") c->refitEnabled = value != 0;                                  // 0: UpdateInstance / UpdateGeom + CommitScene always rebuild the tree on the host   // voted exit of the inner-node loop; takes effect at the next CommitScene
  else if (k == "device_refit") { if (value > 1) return c->fail(HPT_ERR_ARG, "device_refit: 0 an update of a device-built tree is another device build, 1 it is a refit"); c->deviceRefit = value != 0; }
  else if (k == "refit_max_sah_pct") { if (value != 0 && value < 100) return c->fail(HPT_ERR_ARG, "refit_max_sah_pct: 0 never, else >= 100 (per cent of the estimate at build time)"); c->refitMaxSahPct = value; }
  else if (k == "dbg_no_normal_lerp") { if (c->S.motion) c->S.motion = value ? 3u : 1u; }   // diagnostic: moving instances without the reference's normal interpolation (bit 1 of DevScene::motion)
  else if (k == "dbg_wf_iter_cap") c->wfIterCap = (uint)value;                         // diagnostic: make the wavefront loop's safety net reachable in a test
  else if (k == "dr_grad_mode") { if (value > 1) return c->fail(HPT_ERR_ARG, "dr_grad_mode: 0 forward only, 1 with the gradient"); c->drGradMode = value != 0; }   // IntegratorDR's a_gradMode: RayTraceDR only
  else if (k == "pass_slice") c->passSlice = value;                              // forward megakernel: passes of a pixel per work item (0: the whole pixel; hpt_kernels.hip)
  else if (k == "dr_skip_nonfinite") c->drSkipNonFinite = value != 0;                  // PathTraceDR: drop samples whose radiance is not finite (default 0: PixelLossPT as in the reference)
  else if (k == "shade_records") c->shadeTrisEnabled = value != 0;                     // 0: no DevScene::shadeTris (A/B, diagnosis)
  else if (k == "build_threads") c->buildThreads = std::min(value, 64);                // host threads CommitScene builds its trees with (0: the usable cores, at most 16)
  else if (k == "stats_wide") c->statsWide = value != 0;
  else if (k == "sweep_cull") { if (value > 1) return c->fail(HPT_ERR_ARG, "sweep_cull: 0 off, 1 on"); c->sweepCull = (uint)value; if (c->S.sweep) c->S.sweepCull = c->sweepCull; }
  else if (k == "sweep_lanes") { if (value < 0 || value > 1) return c->fail(HPT_ERR_ARG, "sweep_lanes: 0 off, 1 on"); c->sweepLanes = (uint)value; if (c->S.sweep) c->S.sweepLanes = c->sweepLanes; }
  else if (k == "bw_refill_below") { if (value < 1 || value > 64) return c->fail(HPT_ERR_ARG, "bw_refill_below: 1..64"); c->bwRefillBelow = (uint)value; }
  else if (k == "bw_wide") { if (value < -1 || value > 1) return c->fail(HPT_ERR_ARG, "bw_wide: -1 automatic, 0, 1"); c->bwWide = value; }
  else if (k == "bw_node_min") { if (value < 0 || value > 64) return c->fail(HPT_ERR_ARG, "bw_node_min: 0..64"); c->bwNodeMin = (uint)value; }
  else if (k == "device_build") { if (value < -1 || value > 1) return c->fail(HPT_ERR_ARG, "device_build: -1 by CommitScene's options, 0 never, 1 always"); c->deviceBuild = value; c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; }
  else if (k == "device_build_two_level") { if (value < 0 || value > 1) return c->fail(HPT_ERR_ARG, "device_build_two_level: 0 two-level scenes are built on the host, 1 on the device when a device build is asked for"); c->deviceBuildTwoLevel = value; c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; }
  else if (k == "device_build_quality") { if (value > 4) return c->fail(HPT_ERR_ARG, "device_build_quality: 0 the plain linear BVH, 1..4 treelet restructuring passes of every device build"); c->deviceBuildQuality = value; c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false; }
  else if (k == "wide_nodes") { c->wideEnabled = value != 0; c->S.megaWide = (c->wideEnabled && c->nodes4Count != 0u && c->S.flatMode != 0u && c->sahVisits >= HEAVY_SAH_VISITS) ? 1u : 0u; }   // both users of the tree, at once                             // 0: the wavefront trace kernel walks the BVH2 instead of the 4-wide compressed tree (A/B, diagnosis)
  else if (k == "qmc_spectral") { if (value > 1) return c->fail(HPT_ERR_ARG, "qmc_spectral: 0 PathTraceBlockQMC refuses m_spectral_mode, 1 it runs the spectral QMC kernel"); c->qmcSpectral = value != 0; }
  else if (k == "qmc_wavefront") { if (value < 0 || value > 1) return c->fail(HPT_ERR_ARG, "qmc_wavefront: 0 PathTraceBlockQMC runs the megakernel, 1 it takes the wavefront schedule where a PathTraceBlock of as many pixels as it has generator slots would"); c->qmcWavefront = value != 0; }
  else if (k == "dr_environment") { if (value > 1) return c->fail(HPT_ERR_ARG, "dr_environment: 0 PathTraceDR / PathTraceVJP refuse scenes with an environment map or its sampling, 1 they render and differentiate them"); c->drEnvironment = value != 0; }
  else if (k == "adaptive_wavefront") { if (value > 1) return c->fail(HPT_ERR_ARG, "adaptive_wavefront: 0 adaptive calls run the megakernel, 1 they take the wavefront schedule where a PathTraceBlock of their active pixels would"); c->adaptiveWavefront = value != 0; }
  else if (k == "adaptive_spectral") { if (value > 1) return c->fail(HPT_ERR_ARG, "adaptive_spectral: 0 the adaptive calls refuse m_spectral_mode, 1 they run the spectral ADAPT kernels"); c->adaptiveSpectral = value != 0; }
  else if (k == "kmlt_spectral") { if (value > 1) return c->fail(HPT_ERR_ARG, "kmlt_spectral: 0 PathTraceBlockKMLT and the primary-sample-space pass refuse m_spectral_mode, 1 they run the spectral MLT kernels"); c->kmltSpectral = value != 0; }
  else if (k == "kmlt_chains") { if (value < 1 || value > (1 << 28)) return c->fail(HPT_ERR_ARG, "kmlt_chains: 1 .. 2^28 Markov chains (chain c seeds RandomGenInit(7 c + 1))"); c->kmltChains = (uint)value; }
  else if (k == "force_full_materials") c->forceFull = value != 0;                     // diagnostic: never pick the lean (gltf + emissive) kernels
  else if (k == "dbg_stack_witness") { c->stackWitness = value != 0; c->witnessWords = 0; }   // diagnostic: sentinel fill of the stacks' HBM part before every launch (hpt_get_stack_witness)
  else return c->fail(HPT_ERR_ARG, "hpt_set_option: unknown option " + k);
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_option"); }
extern "C" int hpt_get_accel_info(hpt_ctx* c, float out[4])
try {
  if (!c || !out) return HPT_ERR_ARG;
  out[0] = c->sahVisits; out[1] = (float)c->instTris; out[2] = (float)c->insts.size(); out[3] = c->S.sweep ? 2.0f : (c->S.flatMode ? 1.0f : 0.0f);
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_accel_info"); }
extern "C" int hpt_get_commit_time(hpt_ctx* c, float out[4])
try {
  if (!c || !out) return HPT_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = c->tCommit[i];
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_commit_time"); }
extern "C" int hpt_get_build_info(hpt_ctx* c, float out[4])
try {
  if (!c || !out) return HPT_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = c->buildInfo[i];
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_build_info"); }
extern "C" int hpt_get_refit_info(hpt_ctx* c, float out[4])
try {
  if (!c || !out) return HPT_ERR_ARG;
  out[0] = c->sahVisits; out[1] = c->tCommit[3] == 1.0f ? c->sahRefit : c->sahVisits;
  out[2] = (c->S.flatMode == 1u && !c->S.sweep && c->flatRefittable) ? (float)(c->levelOffsets.size() - 1) : 0.0f;
  out[3] = c->refitRejected ? 1.0f : 0.0f;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_refit_info"); }
extern "C" int hpt_read_accel(hpt_ctx* c, int what, void* dst, uint64_t capacityBytes, uint64_t* outBytes, uint32_t* outRootRef)
try {
  if (!c) return HPT_ERR_ARG;
  if (what < 0 || what > 1) return c->fail(HPT_ERR_ARG, "hpt_read_accel: what = 0 (BvhNode array) or 1 (BvhTri array)");
  if (!c->accelCommitted || c->S.flatMode != 1u || c->S.sweep) return c->fail(HPT_ERR_STATE, "hpt_read_accel: no single-level tree is committed");
  const uint64_t bytes = what == 0 ? (uint64_t)std::min(c->flatNodes, c->dNodes.n) * sizeof(BvhNode) : (uint64_t)std::min(c->instTris, c->dTris.n) * sizeof(BvhTri);
  if (outBytes) *outBytes = bytes;
  if (outRootRef) *outRootRef = c->S.rootRef;
  if (!dst) return HPT_OK;
  if (capacityBytes < bytes) return c->fail(HPT_ERR_ARG, "hpt_read_accel: the destination is too small");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize());
  if (bytes) HIPCHK(c, hipMemcpy(dst, what == 0 ? (const void*)c->dNodes.p : (const void*)c->dTris.p, bytes, hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_read_accel"); }
extern "C" int hpt_get_two_level_info(hpt_ctx* c, float out[8])
try {
  if (!c || !out) return HPT_ERR_ARG;
  for (int i = 0; i < 8; i++) out[i] = c->tlInfo[i];
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_two_level_info"); }
extern "C" int hpt_read_accel_two_level(hpt_ctx* c, int what, void* dst, uint64_t capacityBytes, uint64_t* outBytes, uint32_t* outRootRef)
try {
  if (!c) return HPT_ERR_ARG;
  if (what < 0 || what > 2) return c->fail(HPT_ERR_ARG, "hpt_read_accel_two_level: what = 0 (BvhNode array), 1 (BvhTri array) or 2 (BvhInst array)");
  if (!c->accelCommitted || c->S.flatMode != 0u) return c->fail(HPT_ERR_STATE, "hpt_read_accel_two_level: no two-level tree is committed");
  const uint64_t bytes = what == 0 ? (uint64_t)std::min(c->tlNodes, c->dNodes.n) * sizeof(BvhNode) : what == 1 ? (uint64_t)std::min(c->tlTris, c->dTris.n) * sizeof(BvhTri)
                                   : (uint64_t)std::min(c->insts.size(), c->dInsts.n) * sizeof(BvhInst);
  if (outBytes) *outBytes = bytes;
  if (outRootRef) *outRootRef = c->S.rootRef;
  if (!dst) return HPT_OK;
  if (capacityBytes < bytes) return c->fail(HPT_ERR_ARG, "hpt_read_accel_two_level: the destination is too small");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize());
  if (bytes) HIPCHK(c, hipMemcpy(dst, what == 0 ? (const void*)c->dNodes.p : what == 1 ? (const void*)c->dTris.p : (const void*)c->dInsts.p, bytes, hipMemcpyDeviceToHost));
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_read_accel_two_level"); }
extern "C" int hpt_get_schedule(hpt_ctx* c, int* lastSchedule, uint32_t* lastIterations)
try {
  if (!c) return HPT_ERR_ARG;
  if (lastSchedule) *lastSchedule = (int)c->lastSchedule;
  if (lastIterations) *lastIterations = c->lastWfIters;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_schedule"); }
extern "C" int hpt_get_last_launch(hpt_ctx* c, uint32_t out[5])
try {
  if (!c || !out) return HPT_ERR_ARG;
  out[0] = c->lastSchedule; out[1] = c->lastWide; out[2] = c->lastShadeRecords; out[3] = c->lastDeep; out[4] = c->lastPassSlice;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_last_launch"); }
extern "C" int hpt_get_stack_witness(hpt_ctx* c, uint64_t out[2])
try {
  if (!c || !out) return HPT_ERR_ARG;
  out[0] = 0; out[1] = c->witnessWords;
  if (c->witnessWords == 0 || !c->dStackOvf.p) return HPT_OK;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<uint> h(std::min(c->witnessWords, c->dStackOvf.n));
  HIPCHK(c, hipMemcpy(h.data(), c->dStackOvf.p, h.size() * sizeof(uint), hipMemcpyDeviceToHost));
  uint64_t written = 0;
  for (const uint w : h) written += w != STACK_SENTINEL ? 1u : 0u;
  out[0] = written;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_get_stack_witness"); }
extern "C" int hpt_set_accel_layout(hpt_ctx* c, int layout)
try {
  if (!c || layout < 0 || layout > 3) return HPT_ERR_ARG;
  c->accelLayout = layout; c->accelCommitted = false; c->flatRefittable = c->tlUpdatable = false;
  return HPT_OK;
}
catch (...) { return hptGuard(c, "hpt_set_accel_layout"); }
extern "C" int hpt_last_kernel_ms(hpt_ctx* c, float* ms)
try {
  if (!c || !ms) return HPT_ERR_ARG;
  (void)hipSetDevice(c->device);
  float k = 0.0f;
  hipError_t e = hipEventSynchronize(c->ev1);
  if (e == hipSuccess) e = hipEventElapsedTime(&k, c->ev0, c->ev1);
  if (e != hipSuccess) { *ms = c->lastKernelMs; return HPT_OK; }
  *ms = c->lastKernelMs = k;
  return sliceErrorCheck(c);
}
catch (...) { return hptGuard(c, "hpt_last_kernel_ms"); }
