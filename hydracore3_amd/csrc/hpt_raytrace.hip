// Integrator::CastSingleRayBlock and Integrator::RayTraceBlock (integrator_rt.cpp; integrator_pt_host.cpp:29-36, 75-90): the primary-ray
// preview and the deterministic Whitted pass. One lane per pixel in m_packedXY order, wave64, 256-thread blocks; no random numbers, no
// state of the context read or written but the scene and the camera.
//
// Both kernels go through the traversal entry point of the committed layout (traceAny: two-level, single-level, triangle sweep; moving
// instances at time 0) and the texture sampler with the correctly rounded sRGB decode (texSampleRounded). Every f32 operation is written in
// the reference's order and the unit is built with -ffp-contract=off; '/' and sqrt are the compiler's correctly rounded forms, no reciprocal
// or rsqrt intrinsic: tests/raytrace_reference.py restates the same arithmetic in numpy float32 and the GPU tests ask for equal bits.
//
// Three places of the reference are DEFINED here because they cannot be restated:
//  1. a miss in CastSingleRay writes out_color[tid] = 0, ONE float at the thread index, racing with the hit pixel that owns it
//     (integrator_rt.cpp:124). Here a miss assigns 0 to the four floats of its own pixel.
//  2. RayTraceBlock with channels 1 or 2 writes three floats at a stride of one or two, over the neighbouring pixel and past the buffer
//     (integrator_rt.cpp:293-298). The host refuses them; the kernel sees 3 or 4 only (above 4 the reference writes nothing: no launch).
//  3. reflect() is LiteMath's, which is not in the tree: the one definition this project already uses for the gltf / conductor mirror,
//     on the device and in its CPU checker alike, is used (hpt_device.h: reflect): i - 2 * dot(n, i) * n.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"
#include "hpt_primary.h"

namespace hpt {

// colors[GLTF_COLOR_BASE].xyz * texture(texid[0]) at the material's transformed coordinate: kernel_GetRayColor, MaterialEvalWhitted and the
// light branch of kernel_RayBounce all read it (integrator_rt.cpp:147-151, 166-169, 225-229)
HPT_DEV V3 rtBaseTimesTex(const DevScene& S, const MaterialRec& m, V2 uv)
{
  const V4 texColor = texSampleRounded(S.textures, m.texid[0], mulRows2x4(m.row0[0], m.row1[0], uv));
  return v3(m.colors[GLTF_COLOR_BASE][0] * texColor.x, m.colors[GLTF_COLOR_BASE][1] * texColor.y, m.colors[GLTF_COLOR_BASE][2] * texColor.z);
}

// CastSingleRay (integrator_rt.cpp:420-430): kernel_InitEyeRay, kernel_RayTrace (RayQuery_NearestHit; moving instances at time 0), kernel_GetRayColor
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) castSingleRayKernel(const DevScene S, const uint* packedXY, uint tidCount, float* outColor, uint* stackOverflow)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint g = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = stackOverflow + g; stk.ovfStride = gridDim.x * 256u;
  if (g >= tidCount) return;
  uint x, y; V3 rayPos, rayDir;
  pinholeEyeRay(S, packedXY[g], 0.5f, 0.5f, x, y, rayPos, rayDir);      // kernel_InitEyeRay: the pixel centre
  HitRec h; TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const bool found = traceAny<false, false, true, FLAT, MOTION, SWEEP>(S, rayPos, rayDir, 0.0f, HPT_FLT_MAX, h, stk, st, 0.0f);
  V3 color = v3(0.0f, 0.0f, 0.0f);                                       // a miss: 0 to the four floats of its own pixel (decision 1 above)
  if (found) {
    V3 nrmO; V2 uv; uint matId;
    gatherHitVertex(S, h, nrmO, uv, matId);                              // no remap list: m_matIdByPrimId straight (the upload checks the id under this mask)
    const MaterialRec& m = S.materials[matId & 0x00FFFFFFu];
    const float w = m.colors[GLTF_COLOR_BASE][3];
    color = (w > 0.0f) ? v3s(clampf(w, 0.0f, 1.0f)) : rtBaseTimesTex(S, m, uv);
  }
  float* o = outColor + ((size_t)y * (uint)S.winWidth + x) * 4u;         // assigned, not accumulated; the fourth float is 0
  o[0] = color.x; o[1] = color.y; o[2] = color.z; o[3] = 0.0f;
}

// RayTrace (integrator_rt.cpp:432-461): kernel_InitEyeRay3, m_traceDepth times kernel_RayTrace2 + kernel_RayBounce, kernel_ContributeToImage3.
// Every bounce is walked until the path dies (a miss or an emitter). A path whose throughput has become zero - every diffuse material after
// its first bounce, colors[METAL] and colors[COAT] being 0 there - is NOT cut short: its later vertices add throughput * shade = 0 * shade,
// which is +-0 only while shade is finite, and a light at distance 0 makes it inf and the product NaN. Nothing cheap shows the sums finite
// ahead of the walk, so the walk is done; depth and light count are small.
template <bool FLAT, bool MOTION, bool SWEEP>
__global__ void __launch_bounds__(256) rayTraceKernel(const DevScene S, const uint* packedXY, uint tidCount, uint channels, float* outColor, uint* stackOverflow)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint g = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = stackOverflow + g; stk.ovfStride = gridDim.x * 256u;
  if (g >= tidCount) return;
  uint x, y; V3 rpos, rdir;
  pinholeEyeRay(S, packedXY[g], 0.5f, 0.5f, x, y, rpos, rdir);          // kernel_InitEyeRay3: the pixel centre
  V3 accum = v3(0.0f, 0.0f, 0.0f), thr = v3(1.0f, 1.0f, 1.0f);
  TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
  const float time = 0.0f;                                               // RayTrace passes time 0 to kernel_RayTrace2 (integrator_rt.cpp:444)
  for (uint depth = 0; depth < S.traceDepth; depth++) {
    // -- kernel_RayTrace2 (integrator_pt.cpp:214-312): RayQuery_NearestHitMotion at time 0; a miss kills the ray --
    HitRec h;
    if (!traceAny<false, false, true, FLAT, MOTION, SWEEP>(S, rpos, rdir, 0.0f, HPT_FLT_MAX, h, stk, st, time)) break;
    const uint instId = h.inst;
    const V3 hitPos = rpos + h.t * (1.f - 1e-6f) * rdir;
    V3 nrmO; V2 uv; uint midOriginal;
    gatherHitVertex(S, h, nrmO, uv, midOriginal);
    V3 hitNorm = mulNormMat(S.normMat + 12 * instId, nrmO);
    if (MOTION && (S.motion & 2u) == 0u) {                               // integrator_pt.cpp:285-292 as shadeVertex has it: lerp(hitNorm, hitNorm2, time) written out, time = 0
      const V3 n2 = mulNormMat(S.normMat2 + 12 * instId, hitNorm);
      hitNorm = hitNorm + time * (n2 - hitNorm);
    }
    hitNorm = normalize(hitNorm);
    const float flipNorm = dot(rdir, hitNorm) > 0.001f ? -1.0f : 1.0f;
    hitNorm = flipNorm * hitNorm;
    const uint matId = remapMaterialId(S, midOriginal, instId) & 0x00FFFFFFu;   // packMatId / extractMatId keep 24 bits
    const MaterialRec& m = S.materials[matId];

    // -- kernel_RayBounce (integrator_rt.cpp:196-281) --
    const V3 color = rtBaseTimesTex(S, m, uv);
    if (m.mtype == MAT_TYPE_LIGHT_SOURCE) {
      const float atten = (m.lightId == 0xFFFFFFFFu) ? 1.0f : (dot(rdir, v3(0.0f, -1.0f, 0.0f)) < 0.0f ? 1.0f : 0.0f);
      accum.x += thr.x * color.x * atten; accum.y += thr.y * color.y * atten; accum.z += thr.z * color.z * atten;
      break;
    }
    V3 shade = v3(0.0f, 0.0f, 0.0f);
    for (uint l = 0; l < S.numLights; l++) {                             // EVERY entry of m_lights, whatever its type, as a point at lights[l].pos
      const LightRec& L = S.lights[l];
      const V3 lightPos = ld3(L.pos);
      const V3 dlt = hitPos - lightPos;
      const float hitDist = sqrtf_(dot(dlt, dlt));
      const V3 shadowRayDir = normalize(lightPos - hitPos);
      const V3 shadowRayPos = hitPos + hitNorm * smax(maxcomp(hitPos), 1.0f) * 5e-6f;
      HitRec sh;                                                         // RayQuery_AnyHit: no time; a moving instance is met at its first key, which is what time 0 gives
      const bool inShadow = traceAny<true, false, true, FLAT, MOTION, SWEEP>(S, shadowRayPos, shadowRayDir, 0.0f, hitDist * 0.9995f, sh, stk, st, 0.0f);
      if (!inShadow && dot(shadowRayDir, ld3(L.norm)) < 0.0f) {
        const V3 matSamColor = HPT_INV_PI * color;                       // MaterialEvalWhitted: lambertEvalBSDF(l, v, n) * (base * tex)
        const float cosThetaOut = smax(dot(shadowRayDir, hitNorm), 0.0f);
        shade = shade + ld3(L.intensity) * matSamColor * cosThetaOut / (hitDist * hitDist);
      }
    }
    // MaterialSampleWhitted: a perfect mirror for every material
    const float alpha = m.data[GLTF_FLOAT_ALPHA];
    const V3 dir = reflect((-1.0f) * ((-1.0f) * rdir), hitNorm);
    const V3 reflColor = alpha * ld3(m.colors[GLTF_COLOR_METAL]) + (1.0f - alpha) * ld3(m.colors[GLTF_COLOR_COAT]);
    const float cosTheta = dot(dir, hitNorm);
    accum.x += thr.x * shade.x; accum.y += thr.y * shade.y; accum.z += thr.z * shade.z;
    thr = thr * cosTheta * reflColor;
    rpos = offsRayPos(hitPos, hitNorm, dir);
    rdir = dir;
  }
  // kernel_ContributeToImage3 (integrator_rt.cpp:283-299): channels is 3 or 4 here
  float* o = outColor + ((size_t)y * (uint)S.winWidth + x) * channels;
  o[0] += accum.x; o[1] += accum.y; o[2] += accum.z;
}

#define HPT_RT_INST(FLAT, MOTION, SWEEP) \
  template __global__ void castSingleRayKernel<FLAT, MOTION, SWEEP>(const DevScene, const uint*, uint, float*, uint*); \
  template __global__ void rayTraceKernel<FLAT, MOTION, SWEEP>(const DevScene, const uint*, uint, uint, float*, uint*);
HPT_RT_INST(false, false, true)     // the traversal variants traversalDispatch() picks (hpt_host.hip): sweep, single-level with motion, single-level,
HPT_RT_INST(true, true, false)      // two-level with motion, two-level
HPT_RT_INST(true, false, false)
HPT_RT_INST(false, true, false)
HPT_RT_INST(false, false, false)

} // namespace hpt
