// DenoiseFrame (no counterpart in the reference, which writes its G-buffer to images for an external tool): an edge-avoiding a-trous wavelet
// filter (Dammertz et al. 2010) guided by the records of EvalGBuffer. DESIGN.md 2.12 is the definition; tests/denoise_reference.py restates it
// in numpy float32 and the GPU tests ask for equal bits, so every f32 operation below is written in the defined order, the unit is built
// with -ffp-contract=off, '/' is the compiler's correctly rounded division and nothing here may become a reciprocal, an expf or an fma.
//
// Layout: the pack kernel turns the 60-byte records into three planes of one float4 per pixel, so that a tap is three 16-byte loads:
//   C = {r, g, b, instId}   the colours entering a pass (two buffers, ping-pong; the id travels with them)
//   N = {n.x, n.y, n.z, depth}
//   A = {albedo.r, albedo.g, albedo.b, matId}
// Mapping of a pass: one pixel per lane, a 256-thread block covers 32 x 8 pixels, a wave64 two rows of 32 (512 contiguous bytes per row and
// plane). The 25 taps of a pixel are accumulated in the defined order (dy outer, dx inner) whatever the mapping or the tiling.
#include <hip/hip_runtime.h>
#include "hpt_decl.h"

namespace hpt {

HPT_DEV bool dnFinite3(float4 c)
{
  return ((__float_as_uint(c.x) & 0x7F800000u) != 0x7F800000u) && ((__float_as_uint(c.y) & 0x7F800000u) != 0x7F800000u) &&
         ((__float_as_uint(c.z) & 0x7F800000u) != 0x7F800000u);
}
HPT_DEV float dnAlbedoFloor(float a) { return a > 1e-3f ? a : 1e-3f; }   // max(albedo, 1e-3f); a NaN gives the floor

__global__ void __launch_bounds__(256) denoisePackKernel(const DenoiseJob job)
{
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= job.pixels) return;
  const GBufferPixel* g = job.gbuffer + p;
  const float4 col = job.color[p];
  float r = col.x * job.normConst, gr = col.y * job.normConst, b = col.z * job.normConst;
  const float ar = g->rgba[0], ag = g->rgba[1], ab = g->rgba[2];
  if (job.flags & 1u) { r = r / dnAlbedoFloor(ar); gr = gr / dnAlbedoFloor(ag); b = b / dnAlbedoFloor(ab); }
  job.cin[p]  = make_float4(r, gr, b, __int_as_float(g->instId));
  job.planeN[p] = make_float4(g->norm[0], g->norm[1], g->norm[2], g->depth);
  job.planeA[p] = make_float4(ar, ag, ab, __int_as_float(g->matId));
}

// One a-trous iteration. LAST: the re-modulation and the alpha of the frame are folded in and the result goes to the caller's frame.
// TILE = 0: every tap is loaded from memory (steps 4 and up: the taps are strided and a tile with their halo would not fit). TILE = 1 / 2 (step TILE
// only): the block first copies its 32 x 8 pixels and a halo of 2 * TILE pixels of the three planes to LDS (36 x 12 / 40 x 16 entries, 20.7 / 30.7 KB)
// and the taps are read from there; the arithmetic and its order are the same.
template <bool LAST, int TILE>
__global__ void __launch_bounds__(256) denoisePassKernel(const DenoiseJob job)
{
  const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u));
  const int y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
  const int W = (int)job.width, H = (int)job.height;
  constexpr int TW = 32 + 4 * TILE, TH = 8 + 4 * TILE;                     // the tile with its halo
  __shared__ float4 tileC[TILE ? TW * TH : 1], tileN[TILE ? TW * TH : 1], tileA[TILE ? TW * TH : 1];
  if (TILE) {
    const int x0 = (int)(blockIdx.x * 32u) - 2 * TILE, y0 = (int)(blockIdx.y * 8u) - 2 * TILE;
    for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
      const int gx = x0 + t % TW, gy = y0 + t / TW;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {                        // entries outside the frame stay unwritten: their taps are skipped below
        const size_t q = (size_t)gy * (size_t)W + (size_t)gx;
        tileC[t] = job.cin[q]; tileN[t] = job.planeN[q]; tileA[t] = job.planeA[q];
      }
    }
    __syncthreads();
  }
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * (size_t)W + (size_t)x;
  const int lp = ((int)(threadIdx.x >> 5) + 2 * TILE) * TW + (int)(threadIdx.x & 31u) + 2 * TILE;   // this pixel in the tile
  const float4 cp = job.cin[p], np = job.planeN[p], ap = job.planeA[p];
  const bool centreFinite = dnFinite3(cp);
  const uint instP = __float_as_uint(cp.w), matP = __float_as_uint(ap.w);
  const int s = (int)job.step;
  const float absZ = np.w < 0.0f ? -np.w : np.w;
  const float zDen = job.sigmaDepthStep * (absZ > 1e-6f ? absZ : 1e-6f);       // (sigmaDepth * float(s)) * max(|z_p|, 1e-6f)
  const bool useZ = (job.terms & 1u) != 0u, useC = (job.terms & 2u) != 0u && centreFinite, useA = (job.terms & 4u) != 0u;
  const float kern[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
  float sumW = 0.0f, sumR = 0.0f, sumG = 0.0f, sumB = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + s * dy;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + s * dx;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const float h = kern[dy + 2] * kern[dx + 2];
      float w; float4 cq;
      if (dy == 0 && dx == 0) {
        if (!centreFinite) continue;
        w = h; cq = cp;
      } else {
        float4 nq, aq;
        if (TILE) { const int lq = lp + (TILE * dy) * TW + TILE * dx; cq = tileC[lq]; nq = tileN[lq]; aq = tileA[lq]; }
        else      { const size_t q = (size_t)qy * (size_t)W + (size_t)qx; cq = job.cin[q]; nq = job.planeN[q]; aq = job.planeA[q]; }
        if (__float_as_uint(cq.w) != instP || __float_as_uint(aq.w) != matP) continue;
        if (!dnFinite3(cq)) continue;
        const float d = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
        float wn = d > 0.0f ? d : 0.0f;
        for (uint k = 0; k < job.normalSquarings; k++) wn = wn * wn;
        float xz = 0.0f, xc = 0.0f, xa = 0.0f;
        if (useZ) { const float dz = np.w - nq.w; xz = (dz < 0.0f ? -dz : dz) / zDen; }
        if (useC) { const float dr = cp.x - cq.x, dg = cp.y - cq.y, db = cp.z - cq.z; xc = ((dr * dr + dg * dg) + db * db) / job.sigmaColor2; }
        if (useA) { const float dr = ap.x - aq.x, dg = ap.y - aq.y, db = ap.z - aq.z; xa = ((dr * dr + dg * dg) + db * db) / job.sigmaAlbedo2; }
        w = (h * wn) / (((1.0f + xz) * (1.0f + xc)) * (1.0f + xa));
      }
      sumW += w;
      sumR += w * cq.x; sumG += w * cq.y; sumB += w * cq.z;
    }
  }
  float r = 0.0f, g = 0.0f, b = 0.0f;
  if (sumW != 0.0f) { r = sumR / sumW; g = sumG / sumW; b = sumB / sumW; }     // (sumW is a sum of non-negative terms; a NaN guide makes it NaN and so the pixel)
  if (!LAST) { job.cout[p] = make_float4(r, g, b, cp.w); return; }
  if (job.flags & 1u) { r = r * dnAlbedoFloor(ap.x); g = g * dnAlbedoFloor(ap.y); b = b * dnAlbedoFloor(ap.z); }
  job.cout[p] = make_float4(r, g, b, job.color[p].w * job.normConst);
}

template __global__ void denoisePassKernel<false, 0>(const DenoiseJob);
template __global__ void denoisePassKernel<true, 0>(const DenoiseJob);
#if HPT_DENOISE_LDS
template __global__ void denoisePassKernel<false, 1>(const DenoiseJob);
template __global__ void denoisePassKernel<true, 1>(const DenoiseJob);
template __global__ void denoisePassKernel<false, 2>(const DenoiseJob);
template __global__ void denoisePassKernel<true, 2>(const DenoiseJob);
#endif

// ---- DenoiseFrameVar (tests/denoise_var_reference.py) ---------------------------------------------------------------------------
// The filter above with the fixed colour stop replaced by a luminance stop scaled by each pixel's own variance (SVGF, Schied et al. 2017), and a
// fourth plane V = the variance of the prepared pixel that is filtered with the squared weights. Kernels of their own, so that the instantiations
// above hold none of this; what the two share is restated here in the same order.
HPT_DEV float dnLum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
HPT_DEV float dnAlbedoLum(float4 a) { return dnLum(dnAlbedoFloor(a.x), dnAlbedoFloor(a.y), dnAlbedoFloor(a.z)); }

__global__ void __launch_bounds__(256) denoiseVarPackKernel(const DenoiseVarJob job)
{
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= job.d.pixels) return;
  const GBufferPixel* g = job.d.gbuffer + p;
  const float4 col = job.d.color[p];
  const float nc = job.d.normConst;
  float r = col.x * nc, gr = col.y * nc, b = col.z * nc;
  const float ar = g->rgba[0], ag = g->rgba[1], ab = g->rgba[2];
  float v = job.variance[p];
  v = (__builtin_isfinite(v) && v > 0.0f) ? v : 0.0f;
  v = v * (nc * nc);
  if (job.d.flags & 1u) {
    r = r / dnAlbedoFloor(ar); gr = gr / dnAlbedoFloor(ag); b = b / dnAlbedoFloor(ab);
    const float ya = dnAlbedoLum(make_float4(ar, ag, ab, 0.0f));
    v = v / (ya * ya);
  }
  job.d.cin[p]  = make_float4(r, gr, b, __int_as_float(g->instId));
  job.d.planeN[p] = make_float4(g->norm[0], g->norm[1], g->norm[2], g->depth);
  job.d.planeA[p] = make_float4(ar, ag, ab, __int_as_float(g->matId));
  job.vin[p] = v;
}

// One iteration. TILE as in denoisePassKernel; the tile gains TW * TH floats of V, from which the taps and the 3 x 3 prefilter (always at unit
// spacing: inside the halo of 2 * TILE) are read. TILE = 0: V taps and prefilter taps are dword loads, contiguous along a row of lanes.
template <bool LAST, int TILE>
__global__ void __launch_bounds__(256) denoiseVarPassKernel(const DenoiseVarJob job)
{
  const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u));
  const int y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
  const int W = (int)job.d.width, H = (int)job.d.height;
  constexpr int TW = 32 + 4 * TILE, TH = 8 + 4 * TILE;
  __shared__ float4 tileC[TILE ? TW * TH : 1], tileN[TILE ? TW * TH : 1], tileA[TILE ? TW * TH : 1];
  __shared__ float tileV[TILE ? TW * TH : 1];
  if (TILE) {
    const int x0 = (int)(blockIdx.x * 32u) - 2 * TILE, y0 = (int)(blockIdx.y * 8u) - 2 * TILE;
    for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
      const int gx = x0 + t % TW, gy = y0 + t / TW;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {                        // entries outside the frame stay unwritten: their taps are skipped below
        const size_t q = (size_t)gy * (size_t)W + (size_t)gx;
        tileC[t] = job.d.cin[q]; tileN[t] = job.d.planeN[q]; tileA[t] = job.d.planeA[q]; tileV[t] = job.vin[q];
      }
    }
    __syncthreads();
  }
  if (x >= W || y >= H) return;
  const size_t p = (size_t)y * (size_t)W + (size_t)x;
  const int lp = ((int)(threadIdx.x >> 5) + 2 * TILE) * TW + (int)(threadIdx.x & 31u) + 2 * TILE;   // this pixel in the tile
  const float4 cp = job.d.cin[p], np = job.d.planeN[p], ap = job.d.planeA[p];
  const float vp = job.vin[p];
  const bool centreFinite = dnFinite3(cp);
  const uint instP = __float_as_uint(cp.w), matP = __float_as_uint(ap.w);
  const int s = (int)job.d.step;
  const float absZ = np.w < 0.0f ? -np.w : np.w;
  const float zDen = job.d.sigmaDepthStep * (absZ > 1e-6f ? absZ : 1e-6f);
  const bool useZ = (job.d.terms & 1u) != 0u, useL = job.useLum != 0u && centreFinite, useA = (job.d.terms & 4u) != 0u;
  // the stop's denominator: (sigmaLum^2) * vbar + varFloor, vbar the binomial mean of the variances entering this iteration
  float vbar = vp;
  if (job.prefilter != 0u) {
    const float g3[3] = { 0.25f, 0.5f, 0.25f };
    float sumG = 0.0f, sumV = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const int qx = x + dx, qy = y + dy;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const float gw = g3[dy + 1] * g3[dx + 1];
        const float vq = TILE ? tileV[lp + dy * TW + dx] : job.vin[(size_t)qy * (size_t)W + (size_t)qx];
        sumG += gw; sumV += gw * vq;
      }
    }
    vbar = sumV / sumG;
  }
  const float denL = job.sigmaLum2 * vbar + job.varFloor;
  const float yp = dnLum(cp.x, cp.y, cp.z);
  const float kern[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
  float sumW = 0.0f, sumR = 0.0f, sumG = 0.0f, sumB = 0.0f, sumV2 = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + s * dy;
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + s * dx;
      if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
      const float h = kern[dy + 2] * kern[dx + 2];
      float w, vq; float4 cq;
      if (dy == 0 && dx == 0) {
        if (!centreFinite) continue;
        w = h; cq = cp; vq = vp;
      } else {
        float4 nq, aq;
        if (TILE) { const int lq = lp + (TILE * dy) * TW + TILE * dx; cq = tileC[lq]; nq = tileN[lq]; aq = tileA[lq]; vq = tileV[lq]; }
        else      { const size_t q = (size_t)qy * (size_t)W + (size_t)qx; cq = job.d.cin[q]; nq = job.d.planeN[q]; aq = job.d.planeA[q]; vq = job.vin[q]; }
        if (__float_as_uint(cq.w) != instP || __float_as_uint(aq.w) != matP) continue;
        if (!dnFinite3(cq)) continue;
        const float d = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
        float wn = d > 0.0f ? d : 0.0f;
        for (uint k = 0; k < job.d.normalSquarings; k++) wn = wn * wn;
        float xz = 0.0f, xl = 0.0f, xa = 0.0f;
        if (useZ) { const float dz = np.w - nq.w; xz = (dz < 0.0f ? -dz : dz) / zDen; }
        if (useL) { const float dl = yp - dnLum(cq.x, cq.y, cq.z); xl = (dl * dl) / denL; }
        if (useA) { const float dr = ap.x - aq.x, dg = ap.y - aq.y, db = ap.z - aq.z; xa = ((dr * dr + dg * dg) + db * db) / job.d.sigmaAlbedo2; }
        w = (h * wn) / (((1.0f + xz) * (1.0f + xl)) * (1.0f + xa));
      }
      sumW += w;
      sumR += w * cq.x; sumG += w * cq.y; sumB += w * cq.z;
      sumV2 += (w * w) * vq;
    }
  }
  float r = 0.0f, g = 0.0f, b = 0.0f, v = 0.0f;
  if (sumW != 0.0f) { r = sumR / sumW; g = sumG / sumW; b = sumB / sumW; v = sumV2 / (sumW * sumW); }
  if (!LAST) { job.d.cout[p] = make_float4(r, g, b, cp.w); job.vout[p] = v; return; }
  if (job.d.flags & 1u) {
    r = r * dnAlbedoFloor(ap.x); g = g * dnAlbedoFloor(ap.y); b = b * dnAlbedoFloor(ap.z);
    const float ya = dnAlbedoLum(ap);
    v = v * (ya * ya);
  }
  job.d.cout[p] = make_float4(r, g, b, job.d.color[p].w * job.d.normConst);
  if (job.outVar) job.outVar[p] = v;
}

template __global__ void denoiseVarPassKernel<false, 0>(const DenoiseVarJob);
template __global__ void denoiseVarPassKernel<true, 0>(const DenoiseVarJob);
template __global__ void denoiseVarPassKernel<false, 1>(const DenoiseVarJob);
template __global__ void denoiseVarPassKernel<true, 1>(const DenoiseVarJob);
template __global__ void denoiseVarPassKernel<false, 2>(const DenoiseVarJob);
template __global__ void denoiseVarPassKernel<true, 2>(const DenoiseVarJob);

} // namespace hpt
