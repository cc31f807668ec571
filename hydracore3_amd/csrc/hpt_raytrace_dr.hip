// IntegratorDR::RayTraceDR (diff_render/integrator_dr.cpp:168-273, 372-459): the differentiable form of CastSingleRayBlock. One pinhole ray per
// pixel, base colour x texture at the hit, the squared difference to a reference image, and the derivative of that loss scattered into the
// registered parameter textures. One lane per pixel in m_packedXY order, wave64, 256-thread blocks; no random numbers, no state of the context
// read or written but the scene and the camera.
//
// The forward values follow the rules of hpt_raytrace.hip: every f32 operation in the reference's order, -ffp-contract=off, correctly rounded
// '/', no reciprocal or fma; tests/raytrace_dr_reference.py restates them in numpy float32 and the GPU tests ask for equal bits of the colours
// and of the per-pixel losses.
//
// Three places are DEFINED here:
//  4. a miss returns before kernel_CalcRayColor runs (integrator_dr.cpp:267-268): the pixel of out_color is left UNTOUCHED, the rendered colour
//     is 0 and the loss is |ref|^2. (CastSingleRayBlock assigns four zeros there - definition 1 - because its reference races; this one does not.)
//  5. dot3(diff, diff) is LiteMath's, which is not in the tree: (diff.x * diff.x + diff.y * diff.y) + diff.z * diff.z.
//  6. the reference takes the gradient from Enzyme, which fixes no order of the products. Here, per tap k with weight w_k:
//     four channels: ((2 * diff_c) * base_c) * w_k to element base + off_k * 4 + c, c = 0, 1, 2 (alpha gets nothing);
//     one channel:   ((2 * diff_0 * base_0 + 2 * diff_1 * base_1) + 2 * diff_2 * base_2) * w_k to element base + off_k.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"
#include "hpt_primary.h"
#include "hpt_shade.h"

namespace hpt {

// GRAD: m_gradMode != 0 and a_data != nullptr (the host picks the instantiation): registered textures go through texFetchAD and get gradient.
// Without it - and for every texture that is not registered - the fetch is castSingleRayKernel's sampler (integrator_dr.cpp:99, 160).
// outColor: winWidth * winHeight pixels of FOUR floats whatever `channels` is (integrator_dr.cpp:253-256); refImg: pixels of `channels` = 3 or 4
// floats, rows bottom-up; lossPerPixel (may be null): [tidCount], plain stores; lossAccum (may be null): += sum of loss / passNum, one float
// atomic per wave; grad: accumulated into with no-return float atomics, at most 12 per lane.
template <bool FLAT, bool MOTION, bool SWEEP, bool GRAD>
__global__ void __launch_bounds__(256) rayTraceDrKernel(const DevScene S, const uint* packedXY, uint tidCount, uint channels, float passNum, float* outColor,
                                                        const float* refImg, const float* data, float* grad, float* lossPerPixel, float* lossAccum, uint* stackOverflow)
{
  __shared__ uint stackMem[LDS_STACK * 256];
  const uint g = blockIdx.x * 256u + threadIdx.x;
  TravStack stk; stk.lds = &stackMem[threadIdx.x]; stk.ovf = stackOverflow + g; stk.ovfStride = gridDim.x * 256u;
  float lossShare = 0.0f;                                                  // loss / passNum of this lane's pixel; 0 past tidCount (the wave sum below takes every lane)
  if (g < tidCount) {
    uint x, y; V3 rayPos, rayDir;
    pinholeEyeRay(S, packedXY[g], 0.5f, 0.5f, x, y, rayPos, rayDir);       // kernel_InitEyeRay: the pixel centre
    HitRec h; TravStats st; st.nodes = st.tris = st.insts = st.waveNodeIters = st.waveTriIters = 0;
    const bool found = traceAny<false, false, true, FLAT, MOTION, SWEEP>(S, rayPos, rayDir, 0.0f, HPT_FLT_MAX, h, stk, st, 0.0f);
    V3 color = v3(0.0f, 0.0f, 0.0f);                                       // a miss: CastRayDR returns float4(0) and writes nothing (definition 4)
    V3 base = v3(0.0f, 0.0f, 0.0f);
    Taps taps; bool isParam = false;
    if (found) {
      V3 nrmO; V2 uv; uint matId;
      gatherHitVertex(S, h, nrmO, uv, matId);                              // no remap list: m_matIdByPrimId straight, as kernel_CalcRayColor has it
      const MaterialRec& m = S.materials[matId & 0x00FFFFFFu];
      const float w = m.colors[GLTF_COLOR_BASE][3];
      base = ld3(m.colors[GLTF_COLOR_BASE]);
      const uint texId = m.texid[0];
      const V2 tc = mulRows2x4(m.row0[0], m.row1[0], uv);
      V4 texColor;
      if (GRAD && S.textures[texId].diffOffset != ~0ull) texColor = texFetchAD(S, data, texId, tc, taps, isParam);   // Tex2DFetchAD's first branch
      else texColor = texSampleRounded(S.textures, texId, tc);
      if (w > 0.0f) { color = v3s(clampf(w, 0.0f, 1.0f)); isParam = false; }   // the texel is not part of the colour: no gradient
      else color = v3(base.x * texColor.x, base.y * texColor.y, base.z * texColor.z);
      float* o = outColor + ((size_t)y * (uint)S.winWidth + x) * 4u;       // assigned at a stride of four, the fourth float 0
      o[0] = color.x; o[1] = color.y; o[2] = color.z; o[3] = 0.0f;
    }
    // PixelLossRT (integrator_dr.cpp:372-394): the reference image is stored bottom-up
    const uint yRef = (uint)S.winHeight - y - 1u;
    const float* r = refImg + ((size_t)yRef * (uint)S.winWidth + x) * channels;
    const V3 diff = v3(color.x - r[0], color.y - r[1], color.z - r[2]);
    const float loss = diff.x * diff.x + diff.y * diff.y + diff.z * diff.z;   // dot3, summed left to right (definition 5)
    if (lossPerPixel) lossPerPixel[g] = loss;
    lossShare = loss / passNum;
    if (GRAD && isParam) {                                                 // definition 6
      float* gbase = grad + taps.base;
      if (taps.ch == 4u) {
        const V3 d = v3((2.0f * diff.x) * base.x, (2.0f * diff.y) * base.y, (2.0f * diff.z) * base.z);
        for (int k = 0; k < 4; k++) {
          float* e = gbase + (size_t)taps.off[k] * 4u;
          atomicAdd(e + 0, d.x * taps.w[k]); atomicAdd(e + 1, d.y * taps.w[k]); atomicAdd(e + 2, d.z * taps.w[k]);
        }
      } else {
        const float d = (2.0f * diff.x * base.x + 2.0f * diff.y * base.y) + 2.0f * diff.z * base.z;
        for (int k = 0; k < 4; k++) atomicAdd(gbase + taps.off[k], d * taps.w[k]);
      }
    }
  }
  if (lossAccum) {                                                         // wave-uniform (a kernel argument): every lane of the wave is here
    float s = lossShare;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(lossAccum, s);
  }
}

#define HPT_RTDR_INST(FLAT, MOTION, SWEEP) \
  template __global__ void rayTraceDrKernel<FLAT, MOTION, SWEEP, false>(const DevScene, const uint*, uint, uint, float, float*, const float*, const float*, float*, float*, float*, uint*); \
  template __global__ void rayTraceDrKernel<FLAT, MOTION, SWEEP, true>(const DevScene, const uint*, uint, uint, float, float*, const float*, const float*, float*, float*, float*, uint*);
HPT_RTDR_INST(false, false, true)     // the traversal variants traversalDispatch() picks (hpt_host.hip): sweep, single-level with motion, single-level,
HPT_RTDR_INST(true, true, false)      // two-level with motion, two-level
HPT_RTDR_INST(true, false, false)
HPT_RTDR_INST(false, true, false)
HPT_RTDR_INST(false, false, false)

} // namespace hpt
