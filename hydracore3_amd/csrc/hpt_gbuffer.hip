// Integrator::EvalGBuffer (integrator_gbuffer.cpp, integrator_pt.h:187-255): the guide layers a denoiser reads next to the beauty frame.
// Per pixel GBUFFER_SAMPLES = 16 primary rays at the Hammersley points of the pixel, one GBufferPixel record per ray, and a reduction that
// keeps the record most similar to the other 15 together with the mean colour and a coverage estimate.
//
// Mapping: one sample per lane, one pixel per 16-lane row of the wave64 (4 pixels per wave, 16 per 256-thread block). The 16 rays of a row
// differ by sub-pixel offsets only, so the traversal stays coherent. After shading its sample a lane publishes what the comparison reads
// (12 dwords) to LDS; lane i then walks j = 0 .. 15 over its row's records (row-uniform addresses: broadcast reads), which IS the
// reference's summation order. The argmin over (diff_i, i) is a 4-step butterfly over the row.
//
// Every f32 operation below is written in the reference's order and the unit is built with -ffp-contract=off; '/' and sqrtf are the
// compiler's correctly rounded forms. No reciprocal / rsqrt intrinsic may be used here: tests/gbuffer_reference.py restates the same
// arithmetic in numpy float32 and the GPU tests ask for equal bits.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"
#include "hpt_primary.h"

namespace hpt {

static const uint GBUFFER_SAMPLES = 16u;                                 // integrator_pt.h: GBUFFER_SAMPLES

// projectedPixelSize (integrator_gbuffer.cpp:36-45)
HPT_DEV float gbProjectedPixelSize(float dist, float FOV, float w, float h)
{
  const float ppx = (FOV / w) * dist;
  const float ppy = (FOV / h) * dist;
  if (dist > 0.0f) return 2.0f * smax(ppx, ppy);
  return 1000.0f;
}

// surfaceSimilarity (integrator_gbuffer.cpp:47-68); data = {norm.xyz, depth}
HPT_DEV float gbSurfaceSimilarity(float4 data1, float4 data2, const float MADXDIFF)
{
  const float MANXDIFF = 0.15f;
  const float dist = length(v3(data1.x - data2.x, data1.y - data2.y, data1.z - data2.z));
  if (dist >= MANXDIFF) return 0.0f;
  const float d1 = data1.w, d2 = data2.w;
  if (absf(d1 - d2) >= MADXDIFF) return 0.0f;
  const float normalSimilar = __builtin_sqrtf(1.0f - (dist / MANXDIFF));
  const float depthSimilar = __builtin_sqrtf(1.0f - absf(d1 - d2) / MADXDIFF);
  return normalSimilar * depthSimilar;
}

// gbuffDiff (integrator_gbuffer.cpp:70-82); ids = {instId, objId, matId, rgba[3]}. Not symmetric: the pixel size comes from s1's depth.
HPT_DEV float gbDiff(float4 s1, float4 id1, float ppSize, float4 s2, float4 id2)
{
  const float surfaceSimilar = gbSurfaceSimilarity(s1, s2, ppSize * 2.0f);
  const float surfaceDiff = 1.0f - surfaceSimilar;
  const float objDiff = (__float_as_uint(id1.x) == __float_as_uint(id2.x) && __float_as_uint(id1.y) == __float_as_uint(id2.y)) ? 0.0f : 1.0f;
  const float matDiff = (__float_as_uint(id1.z) == __float_as_uint(id2.z)) ? 0.0f : 1.0f;
  const float alphaDiff = absf(id1.w - id2.w);
  return surfaceDiff + objDiff + matDiff + alphaDiff;
}

// kernelBE1D_EvalGBuffer (integrator_gbuffer.cpp:243-258): lane = (pixel blockId, sample localId)
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) gbufferKernel(const DevScene S, const uint* packedXY, uint blockNum, GBufferPixel* out, GBufferPixel* samples, uint* stackOverflow)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  // {norm.xyz, depth}, {instId, objId, matId, rgba[3]}, rgba; a row's 16 records are followed by one spare: the four rows a wave reads at once
  // then start 17 float4 apart, on different banks (16 apart they would share them: a ds_read_b128 lane group spans two rows)
  __shared__ float4 pubSurf[256 + 16], pubIds[256 + 16], pubRgba[256 + 16];
  const uint g = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = stackOverflow + g; stk.ovfStride = gridDim.x * 256u;
  // Lanes past the last pixel trace that pixel again and store nothing: every lane reaches the barrier and the row shuffles below.
  const bool live = (g >> 4) < blockNum;
  const uint blockId = live ? (g >> 4) : blockNum - 1u;
  const uint k = g & 15u;

  // -- kernel_InitEyeRayGB (integrator_gbuffer.cpp:91-108); PlaneHammersley (:8-24): u = radical inverse of k in base 2, v = (k + 0.5) / 16 --
  float hu = 0.0f;
  { uint kk = k; for (float p = 0.5f; kk; p *= 0.5f, kk >>= 1) if (kk & 1u) hu += p; }
  const float hv = (float(k) + 0.5f) / float(GBUFFER_SAMPLES);
  uint x, y; V3 rayPos, rayDir;
  pinholeEyeRay(S, packedXY[blockId], hu, hv, x, y, rayPos, rayDir);

  // -- kernel_RayTrace: RayQuery_NearestHit, tnear 0, tfar FLT_MAX; moving instances at time 0 --
  HitRec h; TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const bool found = traceAny<false, false, true, FLAT, MOTION, SWEEP>(S, rayPos, rayDir, 0.0f, HPT_FLT_MAX, h, stk, st, 0.0f);

  // -- kernel_GetRayGBuff (integrator_gbuffer.cpp:110-200) --
  GBufferPixel r;
  r.depth = 0.0f; r.norm[0] = 0.0f; r.norm[1] = 0.0f; r.norm[2] = 1.0f; r.texc[0] = 0.0f; r.texc[1] = 0.0f;
  r.rgba[0] = 0.0f; r.rgba[1] = 0.0f; r.rgba[2] = 0.0f; r.rgba[3] = 0.0f; r.shadow = 0.0f; r.coverage = 0.0f;
  r.matId = -1; r.objId = -1; r.instId = -1;
  if (found) {
    const uint instId = h.inst, geomId = S.insts[instId].geomId;
    V3 nrmO; V2 uv; uint matId;
    gatherHitVertex(S, h, nrmO, uv, matId);                              // no remap list, no blend resolution: as the reference
    const MaterialRec& m = S.materials[matId & 0x00FFFFFFu];            // (the upload checks the id under this mask)
    const V3 hitNorm = normalize(mulNormMat(S.normMat + 12 * instId, nrmO));   // mul3x3(m_normMatrices[instId], hitNorm), normalised, NOT flipped towards the ray
    const V2 texCoordT = mulRows2x4(m.row0[0], m.row1[0], uv);
    V3 color = v3(0, 0, 0);
    if (m.mtype != MAT_TYPE_LIGHT_SOURCE) {                              // colors[GLTF_COLOR_BASE] whatever mtype is; a light source gives 0 (its texture tap is dead)
      const V4 texColor = texSampleRounded(S.textures, m.texid[0], texCoordT);
      color = v3(m.colors[GLTF_COLOR_BASE][0] * texColor.x, m.colors[GLTF_COLOR_BASE][1] * texColor.y, m.colors[GLTF_COLOR_BASE][2] * texColor.z);
    }
    r.depth = h.t; r.norm[0] = hitNorm.x; r.norm[1] = hitNorm.y; r.norm[2] = hitNorm.z; r.texc[0] = texCoordT.x; r.texc[1] = texCoordT.y;
    r.rgba[0] = color.x; r.rgba[1] = color.y; r.rgba[2] = color.z;
    r.rgba[3] = 1.0f;                                                    // the reference reads color[3] of a float3 (:190): undefined there, DEFINED as 1 here
    r.objId = (int)geomId; r.instId = (int)instId; r.matId = (int)matId;
    r.coverage = 1.0f;
  }
  if (samples != nullptr && live) samples[(size_t)blockId * GBUFFER_SAMPLES + k] = r;

  // -- GBufferReduction (integrator_gbuffer.cpp:213-262) --
  const float4 mySurf = make_float4(r.norm[0], r.norm[1], r.norm[2], r.depth);
  const float4 myIds = make_float4(__int_as_float(r.instId), __int_as_float(r.objId), __int_as_float(r.matId), r.rgba[3]);
  const uint row = (threadIdx.x >> 4) * 17u, slot = row + k;
  pubSurf[slot] = mySurf; pubIds[slot] = myIds; pubRgba[slot] = make_float4(r.rgba[0], r.rgba[1], r.rgba[2], r.rgba[3]);
  __syncthreads();
  const float DEG_TO_RAD = 3.14159265358979323846f / 180.0f;             // LiteMath's constant: float(pi) / 180 in f32
  const float ppSize = gbProjectedPixelSize(r.depth, DEG_TO_RAD * 90.0f, float(S.winWidth), float(S.winHeight));
  float diff = 0.0f, coverage = 0.0f;
  float4 summColor = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (uint j = 0; j < GBUFFER_SAMPLES; j++) {                           // j ascending in f32: the order is part of the contract (the winner is an argmin over near-ties)
    const float thisDiff = gbDiff(mySurf, myIds, ppSize, pubSurf[row + j], pubIds[row + j]);
    diff += thisDiff;
    if (thisDiff < 1.0f) coverage += 1.0f;
    const float4 c = pubRgba[row + j];                                   // summColor += samples[i].rgba, i ascending (every lane of the row holds the same sum)
    summColor.x += c.x; summColor.y += c.y; summColor.z += c.z; summColor.w += c.w;
  }
  coverage *= (1.0f / (float)GBUFFER_SAMPLES);
  // the first i with the strictly smallest diff_i, from minDiff = 1e8 and minDiffId = 0: a diff that is not below 1e8 (NaN from a zero-length
  // normal) never wins, which the clamp states for the butterfly; (value, index) compared lexicographically, so every lane of the row agrees
  float best = (diff < 100000000.0f) ? diff : 100000000.0f;
  uint bestId = k;
  for (int m2 = 8; m2 >= 1; m2 >>= 1) {
    const float od = __shfl_xor(best, m2, 16);
    const uint oi = (uint)__shfl_xor((int)bestId, m2, 16);
    if (od < best || (od == best && oi < bestId)) { best = od; bestId = oi; }
  }
  if (live && bestId == k) {
    const float inv = 1.0f / (float)GBUFFER_SAMPLES;
    r.coverage = coverage;
    r.rgba[0] = summColor.x * inv; r.rgba[1] = summColor.y * inv; r.rgba[2] = summColor.z * inv; r.rgba[3] = summColor.w * inv;
    out[(size_t)y * (uint)S.winWidth + x] = r;
  }
}

#define HPT_GB_INST(FLAT, MOTION, SWEEP) template __global__ void gbufferKernel<FLAT, MOTION, SWEEP>(const DevScene, const uint*, uint, GBufferPixel*, GBufferPixel*, uint*);
HPT_GB_INST(false, false, true)     // the traversal variants traversalDispatch() picks (hpt_host.hip): sweep, single-level, single-level with motion,
HPT_GB_INST(true, true, false)      // two-level, two-level with motion
HPT_GB_INST(true, false, false)
HPT_GB_INST(false, true, false)
HPT_GB_INST(false, false, false)

} // namespace hpt
