// Plain-data layouts shared by the host side and the gfx950 kernels.
//
// Material / LightSource keep the reference's 320-byte records (include/cmaterial.h:187-203,
// include/clight.h:19-56) so that Integrator::m_materials / m_lights upload with one memcpy and the
// Update_m_materials / Update_m_lights partial-update hooks stay trivial.
#pragma once
#include <stdint.h>
#include <math.h>

namespace hpt {

typedef unsigned int uint;

struct MaterialRec
{
  uint  mtype, cflags, lightId, nonlinear;
  uint  texid[4], spdid[4], datai[4];
  float colors[4][4];
  float row0[4][4];
  float row1[4][4];
  float data[16];
};
static_assert(sizeof(MaterialRec) == 320, "Material record must stay 320 bytes");

struct LightRec
{
  float matrix[16], iesMatrix[16];               // column-major
  float samplerRow0[4], samplerRow1[4], samplerRow0Inv[4], samplerRow1Inv[4];
  float pos[4], intensity[4], norm[4];
  float size[2]; float pdfA; uint geomType;
  uint  distType, flags, pdfTableOffset, pdfTableSize;
  uint  specId, texId, iesId; float mult;
  uint  pdfTableSizeX, pdfTableSizeY, camBackTexId; float lightCos1;
  float lightCos2; uint matId; float dummy2, dummy3;
};
static_assert(sizeof(LightRec) == 320, "LightSource record must stay 320 bytes");

// ---- BVH2 in HBM ------------------------------------------------------------------------------------------------
// One 64-byte node holds BOTH child boxes, so one visit = four 16-byte loads from one 64-byte line:
//   q0 = (lo0.x lo0.y lo0.z hi0.x)  q1 = (hi0.y hi0.z lo1.x lo1.y)  q2 = (lo1.z hi1.x hi1.y hi1.z)  q3 = (ref0 ref1 - -)
// A child reference is 32 bits:
//   bit 31 clear : inner node, value = node index (TLAS and all BLAS share one array)
//   bit 31 set   : leaf; bits 30..28 = triangle count (1..4) and bits 27..0 = first triangle (global, BVH order);
//                  count 0 = instance leaf, bits 27..0 = instance id; 0xFFFFFFFF = "leave instance" stack marker.
static const uint REF_LEAF    = 0x80000000u;
static const uint REF_RESTORE = 0xFFFFFFFFu;
static const uint REF_NONE    = 0xFFFFFFFEu;   // empty scene
#ifndef HPT_BVH_LEAF_MAX
#define HPT_BVH_LEAF_MAX 2
#endif
static const int  BVH_LEAF_MAX = HPT_BVH_LEAF_MAX;   // measured on MI355X: 4 -> 1371, 2 -> 1800, 1 -> 1676 Mpaths/s (Cornell, round 1); 1M triangles on the 4-wide tree: 1 / 2 / 3 / 4 -> 280 / 288 / 281 / 273

struct BvhNode { float q[12]; uint ref0, ref1, pad0, pad1; };   // q = child 0 {lo.x hi.x lo.y hi.y lo.z hi.z}, child 1 {same}: (lo, hi) pairs feed v_pk_* slab tests
static_assert(sizeof(BvhNode) == 64, "BVH2 node must be one 64-byte line");

// 64-byte 4-wide node for the heavy-scene trace kernel (single-level layout): up to four children, their boxes as 8-bit offsets in the node's
// own frame. org = lower corner of the children's union; per axis a power-of-two scale 2^(b - 127) (b = byte a of `exps`, so the float is b << 23);
// q[0..2] = lower bounds x / y / z, q[3..5] = upper bounds, byte c of each word = child c; a bound decodes as fma(q, scale, org) in float - the
// quantiser (quantizeNode4, below) rounds outwards and CHECKS the decoded value with the same fma, so a decoded box always contains the (padded)
// BVH2 child box it came from. Boxes only cull, hits are decided by the exact triangle test: the compressed tree returns bit for bit what the
// BVH2 returns. One node = one 64-byte line = four 16-byte loads, half the lines and half the dependent steps of the BVH2 walk.
struct BvhNode4 { float org[3]; uint exps; uint q[6]; uint pad[2]; uint ref[4]; };   // exps byte 3: bit c set = child c exists; ref as in BvhNode (inner: BvhNode4 index)
static_assert(sizeof(BvhNode4) == 64, "4-wide node must be one 64-byte line");

#if defined(__HIPCC__)
#define HPT_HD __host__ __device__ inline
#else
#define HPT_HD inline
#endif
HPT_HD float hptBitsToFloat(uint b) { union { uint u; float f; } c; c.u = b; return c.f; }
HPT_HD uint  hptFloatToBits(float f) { union { uint u; float f; } c; c.f = f; return c.u; }
// lo[c][a], hi[c][a]: the boxes of the children with bit c set in `valid` (the others are ignored); refs are not touched
HPT_HD void quantizeNode4(const float lo[4][3], const float hi[4][3], uint valid, BvhNode4& out)
{
  float org[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, top[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
  for (int c = 0; c < 4; c++) if (valid & (1u << c)) for (int a = 0; a < 3; a++) { org[a] = lo[c][a] < org[a] ? lo[c][a] : org[a]; top[a] = hi[c][a] > top[a] ? hi[c][a] : top[a]; }
  uint exps = valid << 24;
  for (int w = 0; w < 6; w++) out.q[w] = 0u;
  for (int a = 0; a < 3; a++) {
    out.org[a] = org[a];
    const float x = (top[a] - org[a]) * (1.0f / 254.0f);              // scale must exceed extent / 255: take the next power of two above extent / 254
    uint b = ((hptFloatToBits(x) >> 23) & 0xFFu) + 1u;
    if (b < 1u) b = 1u;
    if (b > 254u) b = 254u;
    for (int attempt = 0; attempt < 4; attempt++) {
      const float s = hptBitsToFloat(b << 23);
      bool ok = true;
      uint wlo = 0u, whi = 0u;
      for (int c = 0; c < 4; c++) {
        if (!(valid & (1u << c))) continue;
        float fl = floorf((lo[c][a] - org[a]) / s), fh = ceilf((hi[c][a] - org[a]) / s);
        fl = fl < 0.0f ? 0.0f : (fl > 255.0f ? 255.0f : fl);
        fh = fh < 0.0f ? 0.0f : fh;
        while (fl > 0.0f && fmaf(fl, s, org[a]) > lo[c][a]) fl -= 1.0f;        // decoded lower bound must not exceed the true one (org itself never does)
        while (fh <= 255.0f && fmaf(fh, s, org[a]) < hi[c][a]) fh += 1.0f;     // decoded upper bound must reach the true one
        if (fh > 255.0f) { ok = false; break; }
        wlo |= (uint)fl << (8 * c); whi |= (uint)fh << (8 * c);
      }
      if (ok) { out.q[a] = wlo; out.q[3 + a] = whi; break; }
      b = b < 254u ? b + 1u : b;                                         // coarser grid and again (at most a step or two: rounding at the top end)
      if (attempt == 3) { out.q[a] = 0u; out.q[3 + a] = 0xFFFFFFFFu; }   // cannot happen for finite boxes; the whole node range stays conservative
    }
    exps |= b << (8 * a);
  }
  out.exps = exps;
}

// 64 bytes of shading data per triangle record of the single-level layout, in the records' order: what kernel_RayTrace2 gathers through five
// dependent fetches (instance -> mesh offsets -> three indices -> three vertices, primitive -> material id -> remap list) in ONE line:
//   q0 = (nA.xyz, txA)  q1 = (nB.xyz, txB)  q2 = (nC.xyz, txC)  q3 = (tyA, tyB, tyC, material id after the instance's remap list)
// - the values themselves, so the interpolation is the same arithmetic on the same numbers. Built on the device (buildShadeTrisKernel).

// 48-byte triangle: v0, e1 = v1-v0, e2 = v2-v0 (what Moeller-Trumbore consumes), primId in the spare lane
struct BvhTri { float v0[3]; uint primId; float e1[3]; uint instId; float e2[3]; uint pad1; };   // instId: flat (single-level) mode only
static_assert(sizeof(BvhTri) == 48, "triangle record must be 48 bytes");

// 64-byte instance record: world->object rows (3x4), BLAS root reference, mesh id
struct BvhInst { float row0[4], row1[4], row2[4]; uint root, geomId, pad0, pad1; };   // pad0 = 1: a moving instance (DevScene::instMotion)
static_assert(sizeof(BvhInst) == 64, "instance record must be 64 bytes");

// ---- sweep pair planes (traceSweep's per-pair cull) -----------------------------------------------------------------------------------------
// One record per record PAIR of DevScene::sweepTris, in the instance's object space: the pair's plane n.(x - ctr) = c (n unit, c ~ 0), and the
// margins of the cull test below. m0 = +inf is the "may not cull" flag (padding-only pairs, pairs whose triangles are not coplanar).
struct SweepPlane { float n[3], c; float ctr[3], m0; float q[3], pad; };
static_assert(sizeof(SweepPlane) == 48, "pair plane must be three float4");

// The cull must never skip a triangle that the exact test (hpt_device.h: triangleOccludes / triangleTestInOrder, Moeller-Trumbore in float)
// would accept, so its margins bound the rounding of BOTH computations. u = 2^-24. For triangle j of the pair (stored v0 = a, e1, e2; N = e1 x e2,
// n^ = N / |N|, in exact arithmetic the ray meets the plane at t* = -f / g with f = n^.(o - a), g = n^.d), the float test computes
// t = (|N| f + E1) / (-|N| g + E2) (1 + r), |r| <= 2u, where - expanding tvec = o - a, qvec = tvec x e1, dot(e2, qvec) term by term - every
// product e2_i t_j e1_k carries at most 6 roundings: |E1| <= 8u sum_k W_k |t_k| with W_x = |e1_y e2_z| + |e1_z e2_y| (and cyclic), and in the same
// way |E2| <= 8u sum_k W_k |d_k|. The weights are per axis, so an axis-aligned quad (the Cornell walls) leaves only the error of its normal
// component, which is a rounding of f itself: the wall a shadow ray leaves is culled although its origin sits a mere 5e-6 * max(maxcomp(p), 1)
// above it. The cull's own s0 = fma(n, o - ctr, -c), sd = n.d differ from f, g by the fma chains' 3-4u, by |n - n^| (per axis) and by the plane
// residual |n^.(a - ctr) - c|. q collects the per-axis factors (taken over both triangles, 2 % added for the roundings of the margin itself), m0
// the constant ones, and the tests are
//   away:  s0 > m  and  s0 + lim (sd - md) > m + 8u |s0|      below:  s0 < -m  and  s0 + lim (sd + md) < -(m + 8u |s0|)
// with m = q.|o - ctr| + m0, md = q.|d|: the first part gives |N| f + E1 the sign of s0, the second puts the float t beyond lim (the slack 8u |s0|
// covers r and the rounding of the fma). Moving away (t < 0) is out of reach as long as tnear >= 0: the caller passes lim = NaN otherwise.
HPT_HD void sweepPairPlane(const BvhTri& t0, const BvhTri& t1, SweepPlane& p)
{
  const double u = 1.0 / 16777216.0;
  const BvhTri* t[2] = { &t0, &t1 };
  p.n[0] = p.n[1] = p.n[2] = p.c = p.ctr[0] = p.ctr[1] = p.ctr[2] = p.q[0] = p.q[1] = p.q[2] = p.pad = 0.0f;
  p.m0 = INFINITY;
  double N[2][3], len[2], nh[2][3], lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
  bool live[2];
  int first = -1;
  for (int j = 0; j < 2; j++) {
    const float* e1 = t[j]->e1; const float* e2 = t[j]->e2; const float* a = t[j]->v0;
    N[j][0] = (double)e1[1] * e2[2] - (double)e1[2] * e2[1]; N[j][1] = (double)e1[2] * e2[0] - (double)e1[0] * e2[2]; N[j][2] = (double)e1[0] * e2[1] - (double)e1[1] * e2[0];
    len[j] = sqrt(N[j][0] * N[j][0] + N[j][1] * N[j][1] + N[j][2] * N[j][2]);
    live[j] = len[j] > 0.0 && len[j] < 1e300;                // (the padding record is all zero: det == 0, never hit)
    for (int k = 0; k < 3 && live[j]; k++) live[j] = isfinite(a[k]) && isfinite(e1[k]) && isfinite(e2[k]);
    if (!live[j]) continue;
    if (first < 0) first = j;
    for (int k = 0; k < 3; k++) {
      const double v[3] = { (double)a[k], (double)a[k] + e1[k], (double)a[k] + e2[k] };
      for (int w = 0; w < 3; w++) { lo[k] = fmin(lo[k], v[w]); hi[k] = fmax(hi[k], v[w]); }
    }
  }
  if (first < 0) return;
  double n[3] = { 0, 0, 0 };
  for (int j = 0; j < 2; j++) {
    if (!live[j]) continue;
    const double s = (N[j][0] * N[first][0] + N[j][1] * N[first][1] + N[j][2] * N[first][2]) < 0.0 ? -1.0 : 1.0;   // orient like the first one
    for (int k = 0; k < 3; k++) { nh[j][k] = s * N[j][k] / len[j]; n[k] += nh[j][k]; }
  }
  if (live[0] && live[1] && nh[0][0] * nh[1][0] + nh[0][1] * nh[1][1] + nh[0][2] * nh[1][2] < 1.0 - 1e-9) return;   // not coplanar: no cull
  const double nl = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  float nf[3], cf[3];
  double ext = 0.0;
  for (int k = 0; k < 3; k++) { nf[k] = (float)(n[k] / nl); cf[k] = (float)(0.5 * (lo[k] + hi[k])); ext = fmax(ext, hi[k] - lo[k]); }
  double c = 0.0;
  for (int k = 0; k < 3; k++) c += (double)nf[k] * ((double)t[first]->v0[k] - cf[k]);
  const float ccf = (float)c;
  double R = 0.0, dn[3] = { 0, 0, 0 }, q[3] = { 0, 0, 0 }, m0 = 0.0;
  for (int j = 0; j < 2; j++) {
    if (!live[j]) continue;
    const float* e1 = t[j]->e1; const float* e2 = t[j]->e2; const float* a = t[j]->v0;
    double r = -(double)ccf, sa = 0.0;
    for (int k = 0; k < 3; k++) { r += nh[j][k] * ((double)a[k] - cf[k]); sa += fabs((double)a[k]) + fabs((double)cf[k]); }
    R = fmax(R, fabs(r) + 1e-14 * sa);                          // (+ the double arithmetic's own rounding, generously)
    const double W[3] = { fabs((double)e1[1] * e2[2]) + fabs((double)e1[2] * e2[1]), fabs((double)e1[2] * e2[0]) + fabs((double)e1[0] * e2[2]),
                          fabs((double)e1[0] * e2[1]) + fabs((double)e1[1] * e2[0]) };
    double w0 = 0.0;
    for (int k = 0; k < 3; k++) {
      dn[k] = fmax(dn[k], fabs((double)nf[k] - nh[j][k]) + 1e-15);
      q[k] = fmax(q[k], 8.0 * u * W[k] / len[j]);
      w0 += 8.0 * u * W[k] * fabs((double)cf[k] - a[k]) / len[j];
    }
    m0 = fmax(m0, w0);
  }
  if (R > 1e-6 * ext + 1e-30) return;                           // the two triangles do not share a plane: no cull
  for (int k = 0; k < 3; k++) { p.n[k] = nf[k]; p.ctr[k] = cf[k]; p.q[k] = (float)(1.02 * (q[k] + 8.0 * u * fabs((double)nf[k]) + dn[k])); }
  p.c = ccf;
  p.m0 = (float)(1.02 * (m0 + 4.0 * u * fabs((double)ccf) + R) + 1e-30);
}

// May the ray (o, d: the instance's object space) meet the pair at a t in [0, lim]? false only when the exact test provably rejects both
// triangles (see sweepPairPlane). 24 VALU instructions: traceSweep's closest-hit pair costs ~136, the occlusion pair ~126.
HPT_HD bool sweepPairMayReach(const float n0, const float n1, const float n2, const float c, const float c0, const float c1, const float c2, const float m0,
                              const float q0, const float q1, const float q2, const float ox, const float oy, const float oz,
                              const float dx, const float dy, const float dz, const float lim)
{
  const float x = ox - c0, y = oy - c1, z = oz - c2;
  const float s0 = __builtin_fmaf(n0, x, __builtin_fmaf(n1, y, __builtin_fmaf(n2, z, -c)));
  const float m = __builtin_fmaf(q0, fabsf(x), __builtin_fmaf(q1, fabsf(y), __builtin_fmaf(q2, fabsf(z), m0)));
  const float sd = __builtin_fmaf(n0, dx, __builtin_fmaf(n1, dy, n2 * dz));
  const float md = __builtin_fmaf(q0, fabsf(dx), __builtin_fmaf(q1, fabsf(dy), q2 * fabsf(dz)));
  const float mh = __builtin_fmaf(4.76837158203125e-7f, fabsf(s0), m);   // 8u |s0|
  const bool away = (s0 > m) & (__builtin_fmaf(lim, sd - md, s0) > mh);
  const bool below = (s0 < -m) & (__builtin_fmaf(lim, sd + md, s0) < -mh);
  return !(away | below);
}

// ---- sweep pair boxes (traceSweep's per-lane pass) ------------------------------------------------------------------------------------------
// One box per record PAIR of DevScene::sweepTris, in the instance's object space, around the vertices as the exact test sees them (v0, v0 + e1,
// v0 + e2 of both triangles), padded like the BVH's node boxes (bvh_build.h: Aabb::pad), {lo.xyz, k1} {hi.xyz, k0}.
// The padding alone does not make the box conservative against the exact float test: Moeller-Trumbore's u, v and t carry errors that grow with
// the distance |o - v0| and with 1 / cos of the angle between the ray and the plane (det = |N| n^.d), so a far or oblique ray can be accepted
// a little outside the triangle. The point o + t d the test accepts lies within C u |o - v0| / (sin(phi) cos(theta)) of the triangle (phi: the
// triangle's angle at v0, |N| = |e1| |e2| sin(phi); C is EMPIRICAL, not derived: tests/cpp/sweep_lane_box_test.cpp misses 8 999 of 24 M hits
// with C = 0 and none with C = 1; C = 4 keeps a factor 4 over that). Each
// lane therefore widens the box by delta = k1 |o|_1 + k0 (|o - v0| <= |o|_1 + |v0|_1), k1 = C u / (sin(phi) SIGMA), k0 = k1 max |v0|_1, and takes
// the pair whatever the box says when |n.d| < SIGMA |d|_1 (n: the pair's plane, SweepPlane; n = 0 when not coplanar: always taken).
// A padding-only pair gets a point box without widening: it may be taken, and then never hits.
static const float SWEEP_GRAZE = 1.0e-3f;
struct SweepPairBox { float lo[3], k1; float hi[3], k0; };
static_assert(sizeof(SweepPairBox) == 32, "pair box must be two float4");

HPT_HD void sweepPairBox(const BvhTri& t0, const BvhTri& t1, SweepPairBox& b)
{
  const double u = 1.0 / 16777216.0, C = 4.0;
  const BvhTri* t[2] = { &t0, &t1 };
  double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 }, k1 = 0.0, m = 0.0;
  bool any = false, finite = true;
  for (int j = 0; j < 2; j++) {
    const float* a = t[j]->v0; const float* e1 = t[j]->e1; const float* e2 = t[j]->e2;
    bool live = false;                                          // the padding record is all zero: d x e2 = 0, det = 0, never hit
    for (int k = 0; k < 3; k++) live |= e1[k] != 0.0f || e2[k] != 0.0f;
    if (!live) continue;
    any = true;
    double l1 = 0.0, l2 = 0.0, N[3] = { (double)e1[1] * e2[2] - (double)e1[2] * e2[1], (double)e1[2] * e2[0] - (double)e1[0] * e2[2], (double)e1[0] * e2[1] - (double)e1[1] * e2[0] }, av = 0.0;
    for (int k = 0; k < 3; k++) {
      const double v[3] = { (double)a[k], (double)a[k] + e1[k], (double)a[k] + e2[k] };
      for (int w = 0; w < 3; w++) { finite &= isfinite(v[w]) != 0; lo[k] = fmin(lo[k], v[w]); hi[k] = fmax(hi[k], v[w]); }
      l1 += (double)e1[k] * e1[k]; l2 += (double)e2[k] * e2[k]; av += fabs((double)a[k]);
    }
    const double sinphi = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]) / sqrt(l1 * l2);
    k1 = fmax(k1, sinphi > 0.0 ? C * u / (sinphi * SWEEP_GRAZE) : INFINITY);
    m = fmax(m, av);
  }
  if (!any) { for (int k = 0; k < 3; k++) { b.lo[k] = 0.0f; b.hi[k] = 0.0f; } b.k1 = b.k0 = 0.0f; return; }
  if (!finite || !(k1 < 1e30)) { for (int k = 0; k < 3; k++) { b.lo[k] = -INFINITY; b.hi[k] = INFINITY; } b.k1 = b.k0 = 0.0f; return; }   // (never skipped)
  double ex = 0.0, mag = 0.0;
  for (int k = 0; k < 3; k++) { ex = fmax(ex, hi[k] - lo[k]); mag = fmax(mag, fmax(fabs(lo[k]), fabs(hi[k]))); }
  const double p = 1e-5 * fmax(ex, mag) + 1e-30;
  for (int k = 0; k < 3; k++) { b.lo[k] = (float)(lo[k] - p); b.hi[k] = (float)(hi[k] + p); }
  b.k1 = (float)(k1 * 1.01); b.k0 = (float)(k1 * 1.01 * m * 1.01);
}

// May the ray meet the pair at a t in [tnear, lim], tnear >= 0? Object space: o, d, id (slabRay's clamped reciprocal), oSum = |o|_1,
// dSum = |d|_1; the pair's box (lo, hi, k1, k0) and its plane normal n (SweepPlane::n). The slab test of the instance-box skip in traceSweep
// with its widening (as nodeSlabs), on the box widened by delta = k1 oSum + k0, or true for a ray within SWEEP_GRAZE of the plane. false only
// when the exact triangle tests of the pair reject the interval (tests/cpp/sweep_lane_box_test.cpp).
HPT_HD bool sweepBoxMayHit(const float lo0, const float lo1, const float lo2, const float k1, const float hi0, const float hi1, const float hi2, const float k0,
                           const float n0, const float n1, const float n2, const float ox, const float oy, const float oz, const float dx, const float dy, const float dz,
                           const float ix, const float iy, const float iz, const float oSum, const float dSum, const float tnear, const float lim)
{
  const float del = __builtin_fmaf(k1, oSum, k0);
  const float wx = del * fabsf(ix), wy = del * fabsf(iy), wz = del * fabsf(iz);
  const float ax0 = (lo0 - ox) * ix, ax1 = (hi0 - ox) * ix, ay0 = (lo1 - oy) * iy, ay1 = (hi1 - oy) * iy, az0 = (lo2 - oz) * iz, az1 = (hi2 - oz) * iz;
  const float tn = fmaxf(fmaxf(fminf(ax0, ax1) - wx, fminf(ay0, ay1) - wy), fmaxf(fminf(az0, az1) - wz, tnear));
  const float tf = fminf(fminf(fmaxf(ax0, ax1) + wx, fmaxf(ay0, ay1) + wy), fminf(fmaxf(az0, az1) + wz, lim));
  const float sd = __builtin_fmaf(n0, dx, __builtin_fmaf(n1, dy, n2 * dz));
  return (fabsf(sd) < SWEEP_GRAZE * dSum) | (tn * 0.999999f <= tf * 1.000001f);
}

// ---- work items of the persistent megakernel (hpt_kernels.hip: pathTraceKernel; tests/cpp/pass_slice_items_test.cpp) ---------------------
// A launch renders `tidCount` pixels with `passNum` passes each. With a pass slice s > 0 a pixel is handed out in ceil(passNum / s) items
// of s passes (the last one shorter), slice-major: item k is slice k / tidCount of the pixel at index k % tidCount, so the slices of a pixel
// enter the queue in ascending order and an item's predecessor (same index, slice - 1) is item k - tidCount. s = 0: one item per pixel.
struct SliceItem { uint index, slice, first, passes; };     // pixel index in the launch, slice, first pass and number of passes of the slice
HPT_HD uint passSliceCount(uint passNum, uint s) { return (s == 0u || s >= passNum) ? 1u : (passNum + s - 1u) / s; }
HPT_HD uint passSliceFirst(uint slice, uint passNum, uint s) { return slice * ((s == 0u || s >= passNum) ? passNum : s); }
HPT_HD uint passSlicePasses(uint slice, uint passNum, uint s)
{
  const uint len = (s == 0u || s >= passNum) ? passNum : s, first = slice * len;
  return (passNum - first < len) ? passNum - first : len;
}
HPT_HD SliceItem passSliceItem(uint k, uint tidCount, uint passNum, uint s)
{
  SliceItem it;
  it.slice = k / tidCount; it.index = k - it.slice * tidCount;
  it.first = passSliceFirst(it.slice, passNum, s);
  it.passes = passSlicePasses(it.slice, passNum, s);
  return it;
}
// The hand-over of a pixel from slice to slice: a mailbox of one record per tid, SLICE_MAIL_WORDS 64-bit words (one 64-byte line) of which
// the first SLICE_MAIL_USED are {tag : 32, payload : 32} for PIX(0), PIX(1), PIX(2), gen.sx, gen.sy, written and read one word at a time
// with relaxed agent-scope 64-bit atomics. tag = writing slice + 1 and the mailbox is zeroed before the launch, so tag 0 is "empty"; the
// lane that holds slice s > 0 takes a word only when its tag is s, i.e. written by slice s - 1 (tests/cpp/slice_mailbox_test.cpp).
#define SLICE_MAIL_WORDS 8
#define SLICE_MAIL_USED  5
HPT_HD unsigned long long sliceWordPack(uint slice, uint payload) { return ((unsigned long long)(slice + 1u) << 32) | (unsigned long long)payload; }
HPT_HD bool sliceWordFor(unsigned long long w, uint slice) { return slice != 0u && (uint)(w >> 32) == slice; }   // is w what slice `slice` waits for?
HPT_HD uint sliceWordPayload(unsigned long long w) { return (uint)(w & 0xFFFFFFFFull); }
// Adaptive sampling (the ADAPT instantiations of pathTraceKernel, hpt_adaptive.hip): one record per tid = hpt_pixel_moments.
// sumY / sumY2: the sums of the samples' luminance and of its square, in pass order; passes: samples added. Read when a lane loads the
// pixel, written back when it flushes it.
struct PixelMoments { float sumY, sumY2; uint passes, reserved; };
static_assert(sizeof(PixelMoments) == 16, "PixelMoments is one 16-byte record per tid");
// pixel index of a launch -> tid (Job::tidBegin / tidChunk / tidStride: every tidStride-th chunk of tidChunk tids, hpt_set_tid_interleave)
HPT_HD uint tidOfIndex(uint tidBegin, uint tidChunk, uint tidStride, uint index)
{ return tidBegin + (index / tidChunk) * tidChunk * tidStride + (index % tidChunk); }

struct TexRec
{
  uint w, h, format, flags, addrU, addrV, filter, pad;
  const void* data;       // device pointer
  // differentiable-texture binding (IntegratorDR::TexInfo, diff_render/integrator_dr.h:56-64); offset = ~0 when unbound
  unsigned long long diffOffset; uint diffW, diffH, diffChannels, pad2;
};

// Everything a kernel needs, passed by value as the kernel argument (lands in SGPRs via the kernarg segment).
struct DevScene
{
  const BvhNode* nodes;
  const BvhTri*  tris;
  const BvhInst* insts;
  const BvhTri*  sweepTris;       // sweep scenes: triangle records per mesh in PRIMITIVE order (traceSweep's tie rule relies on it), one spare record at the end
  const BvhInst* sweepInsts;      // sweep scenes: the instance records with root = first triangle record, pad1 = triangle count
  uint           rootRef;
  uint           numInsts;
  uint           nodeMin;         // traversal leaves its inner-node loop when fewer lanes than this still hold an inner node (0: never)
  uint           flatMode;        // 1: one world-space BVH2 over all instanced triangles (leaf triangles carry their instance id)
  const BvhNode4* nodes4;         // single-level layout, static scenes: the same tree collapsed to 4-wide compressed nodes (wfTraceKernel<WIDE>), or null
  uint           root4;           // its root (a BvhNode4 index)
  const float4*  shadeTris;       // single-level layout, gltf / emissive scenes: 64 B of shading data per triangle record (same index as `tris`): see ShadeTri
  uint           megaWide;        // the megakernel's single-level traversal walks nodes4 too (heavy scenes: set with nodeMin4)
  uint           statsWide;       // instrumented megakernel only: count the walk over nodes4 (what the wavefront trace kernel does on this scene)
  uint           nodeMin4;        // nodeMin for the walk over nodes4 (a 4-wide visit is three times the work of a BVH2 one: the vote pays earlier)

  const uint*    triIndices;      // m_triIndices
  const float*   vData8f;         // m_vData8f (8 floats per vertex)
  const uint*    matIdByPrimId;   // m_matIdByPrimId
  const uint*    matVertOffset;   // m_matVertOffset (2 per geom)
  const float*   normMat;         // 12 floats per instance: rows of the upper 3x3 of m_normMatrices (padded to float4)
  const int*     remapInst;       // m_remapInst (2 per instance)
  const int*     allRemapLists;   // m_allRemapLists
  uint           allRemapListsSize;
  uint           numLights;
  const MaterialRec* materials;
  const LightRec*    lights;
  const TexRec*      textures;
  const float*       arrays1f;    // m_arrays1f: pdf table of the sampled environment map
  // motion blur (integrator_pt_scene.cpp:848-897, EmbreeRT.cpp:264-292): instances with two key transforms, interpolated per ray at its time
  const float*       instMotion;  // 24 floats per instance: object->world rows (3x4) at time 0, then at time 1 (only read for BvhInst::pad0 != 0)
  const float*       normMat2;    // 12 floats per instance: rows of the upper 3x3 of m_normMatrices[m_normMatrices2Offs + i]
  uint               motion;      // m_normMatrices2Offs != 0: a time is drawn per path and normals are interpolated
  uint               sweep;       // 1: the scene is small enough for the wave-uniform triangle sweep (traceSweep); BvhInst::root = the instance's first triangle record, pad1 = its number of record pairs, pad0 (word 14) = 1: the per-lane pass (sweepLanes)
  // lens simulation (integrator_pt.cpp:78-104, 806-938): m_lines as {curvatureRadius, thickness, eta, apertureRadius}, film side first
  const float4*      lensLines;   // lensCount entries; lensCount = 0: m_enableOpticSim off
  uint               lensCount;
  float              physSize[2]; // m_physSize
  uint               padLens;

  // spectral rendering (m_spectral_mode, hpt_spectral.hip): every spectrum resampled at 1 nm from LAMBDA_MIN (m_spec_values), {offset, size} per spectrum
  // id (m_spec_offset_sz), the CIE 1931 observer at 1 nm (m_cie_xyz), the camera's response spectra (m_camResponseSpectrumId, -1: none)
  const float*       specValues;
  const uint*        specOffsetSz;
  const float4*      cieXYZ;
  uint               numCieXYZ, numSpectra;
  int                camResponseSpectrumId[3];
  uint               camResponseType, spectralMode;

  // plain-data members (UpdateMembersPlainData)
  float projInv[16], worldViewInv[16];
  int   winStartX, winStartY, winWidth, winHeight, fbWidth, fbHeight;
  uint  traceDepth, integratorType, renderLayer, tileSize;
  float exposureMult, camLensRadius, camTargetDist;
  float camRespoceRGB[4], envColor[4];
  uint  envTexId, envLightId, envCamBackId, envEnableSam;   // m_envTexId, m_envLightId, m_envCamBackId, m_envEnableSam (0xFFFFFFFF: none)
  float envSamRow0[4], envSamRow1[4];
  uint  envSpecId; float envSpecMult;                        // m_envSpecId (0xFFFFFFFF: none), m_envSpecMult: the environment's spectrum in spectral mode
  // thin films (integrator_pt.h:588-590, hpt_film.h; last, so that no other member moves): eta then k per layer, their spectrum ids, the loader's reflectance / transmittance tables
  const float*       filmsEtaK;
  const uint*        filmsSpecId;
  const float*       precompThinFilms;
  // spectra given by textures (m_spec_tex_ids_wavelengths, m_spec_tex_offset_sz: uint2 each), read by the spectral kernel's colour lookup
  const uint*        specTexIdsWavelengths;
  const uint*        specTexOffsetSz;
  // sweep scenes: the instances' padded world boxes, {lo.xyz, -} {hi.xyz, -} per instance: a wave skips an instance none of its rays can reach (traceSweep)
  const float4*      sweepBoxes;
  // sweep scenes: one SweepPlane per record pair of sweepTris (same pair index): traceSweep skips a pair none of the wave's rays can reach
  const float4*      sweepPlanes;
  uint               sweepCull;   // 1: traceSweep uses sweepPlanes (hpt_set_option("sweep_cull", 0 / 1)); the occlusion sweep, and the closest-hit one if built with HPT_SWEEP_CULL_CLOSEST=1
  // sweep scenes: one SweepPairBox per record pair of sweepTris (same pair index): traceSweep's per-lane pass
  const float4*      sweepPairBoxes;
  uint               sweepLanes;  // 1: traceSweep takes the instances flagged in sweepInsts (word 14) through the per-lane pass (hpt_set_option("sweep_lanes", 0 / 1))
};

struct Counters { unsigned long long v[32]; };  // rays, nodes, tris, surfaceHits, shadowRays, paths, instEnter, texFetch,
                                                // then wave-cycles (s_memtime) of: queue+regen, closest-hit traversal, shading, shadow traversal, path end; loop trips;
                                                // [16..23] PathTraceDR probe: records stored, records with a parameter texture, wave-cycles of the record stores, of the
                                                // reverse sweeps, wave-trips with a sweep, lanes in those sweeps, atomic wave-instructions, bounces walked by sweeps, [24] records written to HBM

} // namespace hpt
