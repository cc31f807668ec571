// What the two primary-ray units share (hpt_gbuffer.hip, hpt_raytrace.hip): the pinhole eye ray, the vertex gather at a hit and the normal
// matrix product. Both units are compared bit for bit with numpy float32 restatements (tests/gbuffer_reference.py, tests/raytrace_reference.py):
// every f32 operation below is written in the reference's order, '/' and sqrt are the compiler's correctly rounded forms, and no reciprocal,
// rsqrt or fma may appear. The similar gathers of the path-tracing kernels (hpt_shade.h, hpt_spectral.hip) are their own.
#pragma once
#include "hpt_device.h"

namespace hpt {

// kernel_InitEyeRay / kernel_InitEyeRay3 (integrator_rt.cpp:33-82) and kernel_InitEyeRayGB (integrator_gbuffer.cpp:91-108): the ray through
// pixel XY at the sub-pixel offset (du, dv); the integer add first (not cameraRay's order, hpt_shade.h), always a pinhole
HPT_DEV void pinholeEyeRay(const DevScene& S, uint XY, float du, float dv, uint& x, uint& y, V3& rayPos, V3& rayDir)
{
  x = XY & 0x0000FFFFu; y = (XY & 0xFFFF0000u) >> 16;
  const float xn = (float(x + (uint)S.winStartX) + du) / float(S.fbWidth);
  const float yn = (float(y + (uint)S.winStartY) + dv) / float(S.fbHeight);
  V4 pos = v4(2.0f * xn - 1.0f, 2.0f * yn - 1.0f, 0.0f, 1.0f);                   // EyeRayDirNormalized (cglobals.h:49-55)
  pos = mul4x4(S.projInv, pos);
  const V3 dir = normalize(v3(pos.x / pos.w, pos.y / pos.w, pos.z / pos.w));
  const V3 p1 = mul4x3(S.worldViewInv, v3(0, 0, 0));                             // transform_ray3f (cglobals.h:254-263)
  const V3 p2 = mul4x3(S.worldViewInv, v3(0, 0, 0) + 100.0f * dir);
  rayPos = p1; rayDir = normalize(p2 - p1);
}

// The vertex gather of kernel_GetRayGBuff (integrator_gbuffer.cpp:110-200), kernel_GetRayColor (integrator_rt.cpp:128-145) and kernel_RayTrace2
// (integrator_pt.cpp:263-272), as shadeVertex does it: the interpolated object-space normal, the texture coordinate and the primitive's
// material id before any remap
HPT_DEV void gatherHitVertex(const DevScene& S, const HitRec& h, V3& nrmO, V2& uv, uint& matIdOriginal)
{
  const uint geomId = S.insts[h.inst].geomId;
  const uint triOffset = S.matVertOffset[2 * geomId + 0], vertOffset = S.matVertOffset[2 * geomId + 1];
  const float uvx = h.v, uvy = h.u;                                      // coords[0] = v, coords[1] = u (EmbreeRT.cpp:350-352)
  const uint A = S.triIndices[(triOffset + h.prim) * 3 + 0];
  const uint B = S.triIndices[(triOffset + h.prim) * 3 + 1];
  const uint C = S.triIndices[(triOffset + h.prim) * 3 + 2];
  const float4 nA = ((const float4*)S.vData8f)[2 * (A + vertOffset)], nB = ((const float4*)S.vData8f)[2 * (B + vertOffset)], nC = ((const float4*)S.vData8f)[2 * (C + vertOffset)];
  const float tyA = S.vData8f[8 * (A + vertOffset) + 7], tyB = S.vData8f[8 * (B + vertOffset) + 7], tyC = S.vData8f[8 * (C + vertOffset) + 7];
  const float wA = 1.0f - uvx - uvy;
  nrmO = v3(wA * nA.x + uvy * nB.x + uvx * nC.x, wA * nA.y + uvy * nB.y + uvx * nC.y, wA * nA.z + uvy * nB.z + uvx * nC.z);
  uv = v2(wA * nA.w + uvy * nB.w + uvx * nC.w, wA * tyA + uvy * tyB + uvx * tyC);
  matIdOriginal = S.matIdByPrimId[triOffset + h.prim];
}

// mul3x3(m_normMatrices[inst], n): nm = the instance's 12 floats of DevScene::normMat / normMat2 (rows of the upper 3x3, padded to float4)
HPT_DEV V3 mulNormMat(const float* nm, V3 n)
{
  return v3(nm[0] * n.x + nm[1] * n.y + nm[2] * n.z, nm[4] * n.x + nm[5] * n.y + nm[6] * n.z, nm[8] * n.x + nm[9] * n.y + nm[10] * n.z);
}

} // namespace hpt
