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

// texSample (hpt_device.h: the same taps, weights and texel decode) with the sRGB decode rgb^2.2 CORRECTLY ROUNDED: the power is taken in double
// and rounded to float once. The device's powf is faithful but off by one in the last bit for about 3 % of its arguments; a host's powf is
// correctly rounded for all but a few in 10^4. The albedo is averaged over 16 samples and compared across implementations bit by bit, so the
// pass does not add the library's rounding to it (profiles/gbuffer.md).
HPT_DEV float gbSrgbDecode(float v) { return (float)pow((double)v, (double)2.2f); }
HPT_DEV V4 gbTexSample(const TexRec* texs, uint texId, V2 uv)
{
  const TexRec t = texs[texId];
  V4 res;
  if (t.filter == 0) {
    int px = (int)floorf(uv.x * float(t.w)), py = (int)floorf(uv.y * float(t.h));
    px = (t.addrU == 2) ? min(max(px, 0), (int)t.w - 1) : wrapi(px, (int)t.w);
    py = (t.addrV == 2) ? min(max(py, 0), (int)t.h - 1) : wrapi(py, (int)t.h);
    res = texel(t, py * (int)t.w + px);
  } else {
    const Taps k = bilinearTaps(t.w, t.h, t.addrU, t.addrV, uv);
    const V4 a = texel(t, k.off[0]), b = texel(t, k.off[1]), c = texel(t, k.off[2]), d = texel(t, k.off[3]);
    res.x = a.x * k.w[0] + b.x * k.w[1] + c.x * k.w[2] + d.x * k.w[3];
    res.y = a.y * k.w[0] + b.y * k.w[1] + c.y * k.w[2] + d.y * k.w[3];
    res.z = a.z * k.w[0] + b.z * k.w[1] + c.z * k.w[2] + d.z * k.w[3];
    res.w = a.w * k.w[0] + b.w * k.w[1] + c.w * k.w[2] + d.w * k.w[3];
  }
  if (t.flags & 1u) { res.x = gbSrgbDecode(res.x); res.y = gbSrgbDecode(res.y); res.z = gbSrgbDecode(res.z); }
  return res;
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
  const uint XY = packedXY[blockId];
  const uint x = XY & 0x0000FFFFu, y = (XY & 0xFFFF0000u) >> 16;
  float hu = 0.0f;
  { uint kk = k; for (float p = 0.5f; kk; p *= 0.5f, kk >>= 1) if (kk & 1u) hu += p; }
  const float hv = (float(k) + 0.5f) / float(GBUFFER_SAMPLES);
  const float xn = (float(x + (uint)S.winStartX) + hu) / float(S.fbWidth);     // the integer add first: not cameraRay's order (hpt_shade.h)
  const float yn = (float(y + (uint)S.winStartY) + hv) / float(S.fbHeight);
  V4 pos = v4(2.0f * xn - 1.0f, 2.0f * yn - 1.0f, 0.0f, 1.0f);                   // EyeRayDirNormalized (cglobals.h:49-55)
  pos = mul4x4(S.projInv, pos);
  const V3 dir = normalize(v3(pos.x / pos.w, pos.y / pos.w, pos.z / pos.w));
  const V3 p1 = mul4x3(S.worldViewInv, v3(0, 0, 0));                             // transform_ray3f (cglobals.h:254-263); always a pinhole
  const V3 p2 = mul4x3(S.worldViewInv, v3(0, 0, 0) + 100.0f * dir);
  const V3 rayPos = p1, rayDir = normalize(p2 - p1);

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
    const uint triOffset = S.matVertOffset[2 * geomId + 0], vertOffset = S.matVertOffset[2 * geomId + 1];
    const uint matId = S.matIdByPrimId[triOffset + h.prim];              // no remap list, no blend resolution: as the reference
    const MaterialRec& m = S.materials[matId & 0x00FFFFFFu];            // (the upload checks the id under this mask)
    const float uvx = h.v, uvy = h.u;                                    // coords[0] = v, coords[1] = u (EmbreeRT.cpp:350-352)
    const uint A = S.triIndices[(triOffset + h.prim) * 3 + 0];
    const uint B = S.triIndices[(triOffset + h.prim) * 3 + 1];
    const uint C = S.triIndices[(triOffset + h.prim) * 3 + 2];
    const float4 nA = ((const float4*)S.vData8f)[2 * (A + vertOffset)], nB = ((const float4*)S.vData8f)[2 * (B + vertOffset)], nC = ((const float4*)S.vData8f)[2 * (C + vertOffset)];
    const float tyA = S.vData8f[8 * (A + vertOffset) + 7], tyB = S.vData8f[8 * (B + vertOffset) + 7], tyC = S.vData8f[8 * (C + vertOffset) + 7];
    const float wA = 1.0f - uvx - uvy;
    const V3 nrmO = v3(wA * nA.x + uvy * nB.x + uvx * nC.x, wA * nA.y + uvy * nB.y + uvx * nC.y, wA * nA.z + uvy * nB.z + uvx * nC.z);
    const V2 uv = v2(wA * nA.w + uvy * nB.w + uvx * nC.w, wA * tyA + uvy * tyB + uvx * tyC);
    const float* nm = S.normMat + 12 * instId;                           // mul3x3(m_normMatrices[instId], hitNorm), normalised, NOT flipped towards the ray
    const V3 hitNorm = normalize(v3(nm[0] * nrmO.x + nm[1] * nrmO.y + nm[2] * nrmO.z,
                                    nm[4] * nrmO.x + nm[5] * nrmO.y + nm[6] * nrmO.z,
                                    nm[8] * nrmO.x + nm[9] * nrmO.y + nm[10] * nrmO.z));
    const V2 texCoordT = mulRows2x4(m.row0[0], m.row1[0], uv);
    V3 color = v3(0, 0, 0);
    if (m.mtype != MAT_TYPE_LIGHT_SOURCE) {                              // colors[GLTF_COLOR_BASE] whatever mtype is; a light source gives 0 (its texture tap is dead)
      const V4 texColor = gbTexSample(S.textures, m.texid[0], texCoordT);
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
HPT_GB_INST(false, false, true)     // the traversal variants ray_query() dispatches (hpt_host.hip): sweep, single-level, single-level with motion,
HPT_GB_INST(true, true, false)      // two-level, two-level with motion
HPT_GB_INST(true, false, false)
HPT_GB_INST(false, true, false)
HPT_GB_INST(false, false, false)

} // namespace hpt
