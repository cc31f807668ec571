// Host check of the sweep's per-pair boxes (hydracore3_amd/csrc/hpt_types.h: sweepPairBox, sweepBoxMayHit; used by hpt_device.h: traceSweep's
// per-lane pass). A lane drops a record pair when its ray misses the pair's box over [tnear, lim]; that is only allowed when the exact float
// triangle tests (hpt_device.h: triangleOccludes, triangleTestInOrder - restated here line by line, built with -ffp-contract=off like the
// library) reject both triangles over that interval. Random quads and lone triangles, split in all four vertex orders, at scales 1e-3 ... 1e4,
// axis-aligned, oblique, long and thin, far from the origin. Rays: aimed at the quad's edges and corners (just inside, on, just outside),
// grazing the plane, leaving the quad from the renderer's offset (hpt_shade.h: hitPos + hitNorm * max(maxcomp(hitPos), 1) * 5e-6), axis-parallel
// directions (a zero component: the clamped reciprocal), and segments whose end (lim) or start (tnear) sits exactly on the exact test's own t.
// The device's reciprocal (v_rcp_f32) is within 1 ulp: the test perturbs 1 / d by -1, 0 or +1 ulp. Plain g++, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cfloat>
#include <array>
#include <random>
#include <algorithm>
struct float4 { float x, y, z, w; };
#include "../../hydracore3_amd/csrc/hpt_types.h"
using namespace hpt;

struct V { float x, y, z; };
static V v(float x, float y, float z) { V r; r.x = x; r.y = y; r.z = z; return r; }
static V sub(V a, V b) { return v(a.x - b.x, a.y - b.y, a.z - b.z); }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return v(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// the exact test's t, u, v and det (hpt_device.h: triangleOccludes / triangleTestInOrder compute them the same way)
struct MT { float det, uu, vv, tt; };
static MT mt(const BvhTri& t, V o, V d)
{
  const V e1 = v(t.e1[0], t.e1[1], t.e1[2]), e2 = v(t.e2[0], t.e2[1], t.e2[2]);
  const V pvec = cross(d, e2);
  const float det = dot(e1, pvec);
  const float inv = 1.0f / det;
  const V tvec = sub(o, v(t.v0[0], t.v0[1], t.v0[2]));
  const float uu = dot(tvec, pvec) * inv;
  const V qvec = cross(tvec, e1);
  const float vv = dot(d, qvec) * inv;
  const float tt = dot(e2, qvec) * inv;
  MT r; r.det = det; r.uu = uu; r.vv = vv; r.tt = tt; return r;
}
static bool inside(const MT& m) { return (m.det != 0.0f) & (m.uu >= 0.0f) & (m.vv >= 0.0f) & (m.uu + m.vv <= 1.0f); }
// triangleOccludes over [tnear, tfar]; triangleTestInOrder accepts at most tt <= bestT (found == false), the wider of its two cases
static bool hitsIn(const BvhTri& t, V o, V d, float tnear, float lim) { const MT m = mt(t, o, d); return inside(m) & (m.tt >= tnear) & (m.tt <= lim); }
static BvhTri tri(V a, V b, V c, uint prim)
{
  BvhTri t; std::memset(&t, 0, sizeof(t));
  t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
  t.e1[0] = b.x - a.x; t.e1[1] = b.y - a.y; t.e1[2] = b.z - a.z;
  t.e2[0] = c.x - a.x; t.e2[1] = c.y - a.y; t.e2[2] = c.z - a.z;
  t.primId = prim;
  return t;
}
static float maxcomp(V p) { return std::max(p.x, std::max(p.y, p.z)); }
// world -> object rows of an instance matrix (column-major 4x4, affine): hpt_host.hip: inverse_rows, line by line
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

int main()
{
  std::mt19937 rng(20261017);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto uni = [&](double a, double b) { return a + (b - a) * U(rng); };
  auto unit = [&]() { double x, y, z, l; do { x = uni(-1, 1); y = uni(-1, 1); z = uni(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                      l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  // the device reciprocal: within 1 ulp of 1 / x, clamped like slabRay
  auto rcpg = [&](std::mt19937& g, float x) {
    float r = 1.0f / x;
    const int k = (int)(g() % 3u);
    if (std::isfinite(r) && k == 1) r = std::nextafter(r, INFINITY); else if (std::isfinite(r) && k == 2) r = std::nextafter(r, -INFINITY);
    return std::min(std::max(r, -1.0e30f), 1.0e30f);
  };
  auto rcp = [&](float x) { return rcpg(rng, x); };
  // the instanced class draws from its own generator, so the rays of the classes above stay what they were
  std::mt19937 rng2(20261018);
  auto uni2 = [&](double a, double b) { return a + (b - a) * U(rng2); };
  auto unit2 = [&]() { double x, y, z, l; do { x = uni2(-1, 1); y = uni2(-1, 1); z = uni2(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                       l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  long long irays = 0, irejected = 0, ihits = 0, ibad = 0;
  long long rays = 0, rejected = 0, bad = 0, hitsSeen = 0, boundary = 0;
  const int QUADS = 40000, RAYS = 120, IRAYS = 40;
  for (int qi = 0; qi < QUADS; qi++) {
    const double scale = std::pow(10.0, uni(-3.0, 4.0));
    const int frame = qi % 3;                                         // 0 axis-aligned, 1 oblique, 2 axis-aligned but rotated about one axis
    std::array<double, 3> nrm, tu, tv;
    if (frame == 0) {
      const int a = qi / 3 % 3; nrm = { 0, 0, 0 }; tu = { 0, 0, 0 }; tv = { 0, 0, 0 };
      nrm[a] = (qi / 9) % 2 ? 1.0 : -1.0; tu[(a + 1) % 3] = 1.0; tv[(a + 2) % 3] = 1.0;
    } else if (frame == 1) {
      nrm = unit(); std::array<double, 3> r = unit();
      tu = { nrm[1] * r[2] - nrm[2] * r[1], nrm[2] * r[0] - nrm[0] * r[2], nrm[0] * r[1] - nrm[1] * r[0] };
      const double l = std::sqrt(tu[0] * tu[0] + tu[1] * tu[1] + tu[2] * tu[2]); for (double& x : tu) x /= l;
      tv = { nrm[1] * tu[2] - nrm[2] * tu[1], nrm[2] * tu[0] - nrm[0] * tu[2], nrm[0] * tu[1] - nrm[1] * tu[0] };
    } else {
      const double ang = uni(0, 6.283185307179586); const int a = qi / 3 % 3;
      tu = { 0, 0, 0 }; tv = { 0, 0, 0 }; tv[a] = 1.0; tu[(a + 1) % 3] = std::cos(ang); tu[(a + 2) % 3] = std::sin(ang);
      nrm = { tu[1] * tv[2] - tu[2] * tv[1], tu[2] * tv[0] - tu[0] * tv[2], tu[0] * tv[1] - tu[1] * tv[0] };
    }
    const double far = qi % 4 == 0 ? scale * uni(10.0, 1000.0) : 0.0;  // some quads far from the origin (large coordinates, small extent)
    const double cx = uni(-1, 1) * scale + far, cy = uni(-1, 1) * scale - far, cz = uni(-1, 1) * scale;
    const double hu = scale * uni(0.05, 1.0), hv = scale * uni(0.05, 1.0) * (qi % 7 == 0 ? 1e-3 : 1.0);   // some long thin quads
    V q[4];
    const double su[4] = { -1, 1, 1, -1 }, sv[4] = { -1, -1, 1, 1 };
    for (int k = 0; k < 4; k++)
      q[k] = v((float)(cx + su[k] * hu * tu[0] + sv[k] * hv * tv[0]), (float)(cy + su[k] * hu * tu[1] + sv[k] * hv * tv[1]), (float)(cz + su[k] * hu * tu[2] + sv[k] * hv * tv[2]));
    const int rot = (qi / 5) % 4;
    const V A = q[rot], B = q[(rot + 1) % 4], C = q[(rot + 2) % 4], D = q[(rot + 3) % 4];
    BvhTri t0 = tri(A, B, C, 0), t1 = tri(A, C, D, 1);
    const bool padded = qi % 11 == 0;                                  // a lone triangle paired with the padding record
    if (padded) { std::memset(&t1, 0, sizeof(t1)); t1.primId = 0xFFFFFFFFu; }
    SweepPairBox bx; sweepPairBox(t0, t1, bx);
    SweepPlane pl; sweepPairPlane(t0, t1, pl);
    const V nf = v((float)nrm[0], (float)nrm[1], (float)nrm[2]);
    auto check = [&](std::mt19937& g, V o, V d, int ri, int kind, long long& nR, long long& nRej, long long& nHit, long long& nBound) {
      const MT m0 = mt(t0, o, d), m1 = mt(t1, o, d);
      // intervals: open, random, and ending or starting exactly on either triangle's own t (and one float beyond it)
      float tn[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, lim[6] = { FLT_MAX, (float)(scale * (4.0 * U(g))), m0.tt, m1.tt, std::nextafter(m0.tt, 0.0f), m0.tt };
      if (ri % 3 == 0) { tn[5] = m0.tt; lim[5] = std::nextafter(m0.tt, INFINITY); } else if (ri % 3 == 1) { tn[5] = m1.tt; lim[5] = m1.tt; }
      const V id = v(rcpg(g, d.x), rcpg(g, d.y), rcpg(g, d.z));
      const float oSum = std::fabs(o.x) + std::fabs(o.y) + std::fabs(o.z), dSum = std::fabs(d.x) + std::fabs(d.y) + std::fabs(d.z);
      for (int j = 0; j < 6; j++) {
        if (!(tn[j] >= 0.0f) || !(lim[j] >= tn[j])) continue;        // the device takes every pair of a lane whose tnear < 0
        nR++;
        const bool reach = sweepBoxMayHit(bx.lo[0], bx.lo[1], bx.lo[2], bx.k1, bx.hi[0], bx.hi[1], bx.hi[2], bx.k0, pl.n[0], pl.n[1], pl.n[2],
                                          o.x, o.y, o.z, d.x, d.y, d.z, id.x, id.y, id.z, oSum, dSum, tn[j], lim[j]);
        const bool hit = hitsIn(t0, o, d, tn[j], lim[j]) || hitsIn(t1, o, d, tn[j], lim[j]);
        nHit += hit;
        nBound += hit && (j >= 2);
        if (reach) continue;
        nRej++;
        if (hit) {
          if (bad < 10) std::printf("MISSED quad %d ray %d kind %d scale %g: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) [%.9g, %.9g]\n", qi, ri, kind, scale, o.x, o.y, o.z, d.x, d.y, d.z, tn[j], lim[j]);
          bad++;
        }
      }
    };
    for (int ri = 0; ri < RAYS; ri++) {
      const int kind = ri % 6;
      // a target on the quad's plane: near an edge or a corner (just inside, on, just outside), or anywhere on it
      double a = uni(-1.1, 1.1), b = uni(-1.1, 1.1);
      if (kind == 0 || kind == 1) { const double e = std::pow(10.0, uni(-8.0, -2.0)) * (rng() & 1 ? 1 : -1); if (rng() & 1) a = (rng() & 1 ? 1.0 : -1.0) + e; else b = (rng() & 1 ? 1.0 : -1.0) + e; }
      if (kind == 1) { a = (rng() & 1 ? 1.0 : -1.0) * (1.0 + std::pow(10.0, uni(-8.0, -3.0)) * uni(-1, 1)); b = (rng() & 1 ? 1.0 : -1.0) * (1.0 + std::pow(10.0, uni(-8.0, -3.0)) * uni(-1, 1)); }
      const V hp = v((float)(cx + a * hu * tu[0] + b * hv * tv[0]), (float)(cy + a * hu * tu[1] + b * hv * tv[1]), (float)(cz + a * hu * tu[2] + b * hv * tv[2]));
      V o, d;
      if (kind == 2) {
        // leaving the quad from the renderer's offset: into the half-space, grazing, or coming back
        const float side = (ri & 1) ? 1.0f : -1.0f, h = std::max(maxcomp(hp), 1.0f) * 5e-6f;
        o = v(hp.x + side * nf.x * h, hp.y + side * nf.y * h, hp.z + side * nf.z * h);
        std::array<double, 3> w = unit();
        const double g = std::pow(10.0, uni(-7.0, 0.0)) * (ri % 4 < 2 ? 1.0 : -1.0) * side;
        const double wn = w[0] * nrm[0] + w[1] * nrm[1] + w[2] * nrm[2];
        for (int k = 0; k < 3; k++) w[k] = w[k] - wn * nrm[k] + g * nrm[k];
        const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        d = v((float)(w[0] / wl), (float)(w[1] / wl), (float)(w[2] / wl));
      } else {
        // from anywhere around the quad (at 1e-6 ... 1e3 of its scale), aimed at the target; kind 3: grazing, 4: axis-parallel
        std::array<double, 3> w = unit();
        if (kind == 3) { const double wn = w[0] * nrm[0] + w[1] * nrm[1] + w[2] * nrm[2], g = std::pow(10.0, uni(-7.0, -1.0));
                         for (int k = 0; k < 3; k++) w[k] = w[k] - wn * nrm[k] + g * nrm[k]; const double l = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); for (double& x : w) x /= l; }
        if (kind == 4) { const int ax = (int)(rng() % 3u); w = { 0, 0, 0 }; w[ax] = rng() & 1 ? 1.0 : -1.0; }
        const double dist = scale * std::pow(10.0, uni(-6.0, 3.0));
        o = v((float)(hp.x - w[0] * dist), (float)(hp.y - w[1] * dist), (float)(hp.z - w[2] * dist));
        if (kind == 4) d = v((float)w[0], (float)w[1], (float)w[2]);
        else { const V dd = sub(hp, o); const float l = std::sqrt(dot(dd, dd)); if (!(l > 0.0f)) continue; d = v(dd.x / l, dd.y / l, dd.z / l); }
        if (ri % 17 == 0) d = v(-d.x, -d.y, -d.z);
      }
      check(rng, o, d, ri, kind, rays, rejected, hitsSeen, boundary);
    }
    // instanced rays: a unit WORLD ray taken to the quad's object space the way the sweep does it - the instance's world -> object rows
    // (hpt_host.hip: inverse_rows, restated below) and traceSweep's toObjectSpace expressions in the same order - so the object-space
    // direction has any length and any orientation. Instances: rotation, scales 1e-2 .. 1e2 per axis, a mirror (one in three), a shear
    // (one in three), translations up to 1e3. World rays: aimed at edges and corners, grazing the world plane, leaving it from the
    // renderer's offset, axis-parallel, from near and far.
    for (int ri = 0; ri < IRAYS; ri++) {
      const int kind = ri % 4;
      double L[3][3], T[3];
      {
        const std::array<double, 3> ax = unit2(); const double an = uni2(0.0, 6.283185307179586), c = std::cos(an), sn = std::sin(an), k = 1.0 - c;
        const double Rm[3][3] = { { c + ax[0] * ax[0] * k, ax[0] * ax[1] * k - ax[2] * sn, ax[0] * ax[2] * k + ax[1] * sn },
                                  { ax[1] * ax[0] * k + ax[2] * sn, c + ax[1] * ax[1] * k, ax[1] * ax[2] * k - ax[0] * sn },
                                  { ax[2] * ax[0] * k - ax[1] * sn, ax[2] * ax[1] * k + ax[0] * sn, c + ax[2] * ax[2] * k } };
        double sc[3]; for (double& x : sc) x = std::pow(10.0, uni2(-2.0, 2.0));
        if (rng2() % 3u == 0u) sc[rng2() % 3u] *= -1.0;                                 // mirror
        double Sh[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
        if (rng2() % 3u == 0u) { Sh[0][1] = uni2(-1.5, 1.5); Sh[1][2] = uni2(-1.5, 1.5); Sh[0][2] = uni2(-1.5, 1.5); }
        for (int r = 0; r < 3; r++) for (int q = 0; q < 3; q++) { double a = 0.0; for (int k2 = 0; k2 < 3; k2++) a += Sh[r][k2] * Rm[k2][q]; L[r][q] = a * sc[q]; }
        for (double& x : T) x = uni2(-1.0, 1.0) * std::pow(10.0, uni2(-1.0, 3.0));
      }
      float m[16];                                                       // column-major 4x4, as the host keeps an instance matrix
      for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) m[4 * q + r] = (float)L[r][q]; m[12 + r] = (float)T[r]; m[3 + 4 * r] = 0.0f; }
      m[15] = 1.0f;
      float row0[4], row1[4], row2[4];
      inverse_rows(m, row0, row1, row2);
      auto toWorld = [&](double x, double y, double z) { std::array<double, 3> w; for (int r = 0; r < 3; r++) w[r] = (double)m[r] * x + (double)m[4 + r] * y + (double)m[8 + r] * z + (double)m[12 + r]; return w; };
      // target on the quad's plane (object space), near an edge or corner or anywhere, and in world space through the float matrix
      double a = uni2(-1.1, 1.1), b = uni2(-1.1, 1.1);
      if (kind == 0) { const double e = std::pow(10.0, uni2(-8.0, -2.0)) * (rng2() & 1 ? 1 : -1); if (rng2() & 1) a = (rng2() & 1 ? 1.0 : -1.0) + e; else b = (rng2() & 1 ? 1.0 : -1.0) + e; }
      const std::array<double, 3> hw = toWorld(cx + a * hu * tu[0] + b * hv * tv[0], cy + a * hu * tu[1] + b * hv * tv[1], cz + a * hu * tu[2] + b * hv * tv[2]);
      // the world plane's normal: the inverse transpose of the object normal (rows of the inverse are its columns)
      std::array<double, 3> nw;
      for (int r = 0; r < 3; r++) nw[r] = (double)row0[r] * nrm[0] + (double)row1[r] * nrm[1] + (double)row2[r] * nrm[2];
      { const double l = std::sqrt(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]); for (double& x : nw) x /= l; }
      double wo[3], wd[3];
      std::array<double, 3> w = unit2();
      if (kind == 1) { const double wn = w[0] * nw[0] + w[1] * nw[1] + w[2] * nw[2], g = std::pow(10.0, uni2(-7.0, -1.0)) * (rng2() & 1 ? 1 : -1);
                       for (int k = 0; k < 3; k++) w[k] = w[k] - wn * nw[k] + g * nw[k]; }
      if (kind == 3) { w = { 0, 0, 0 }; w[rng2() % 3u] = rng2() & 1 ? 1.0 : -1.0; }
      { const double l = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]); for (double& x : w) x /= l; }
      if (kind == 2) {
        // leaving the world surface from the renderer's offset, to either side
        const float hp[3] = { (float)hw[0], (float)hw[1], (float)hw[2] }, side = (ri & 4) ? 1.0f : -1.0f;
        const float h = std::max(std::max(hp[0], std::max(hp[1], hp[2])), 1.0f) * 5e-6f;
        for (int k = 0; k < 3; k++) { wo[k] = (double)(hp[k] + side * (float)nw[k] * h); wd[k] = w[k]; }
      } else {
        const double dist = std::max(scale, 1e-3) * std::pow(10.0, uni2(-3.0, 3.0));
        for (int k = 0; k < 3; k++) { wo[k] = hw[k] - w[k] * dist; wd[k] = w[k]; }
        if (kind != 3) { double dd[3], l = 0.0; for (int k = 0; k < 3; k++) { dd[k] = hw[k] - (double)(float)wo[k]; l += dd[k] * dd[k]; }
                         l = std::sqrt(l); if (!(l > 0.0)) continue; for (int k = 0; k < 3; k++) wd[k] = dd[k] / l; }
      }
      if (ri % 13 == 0) for (double& x : wd) x = -x;
      const V fo = v((float)wo[0], (float)wo[1], (float)wo[2]), fd = v((float)wd[0], (float)wd[1], (float)wd[2]);
      // traceSweep's toObjectSpace, the same expressions in the same order
      const V o = v(row0[0] * fo.x + row0[1] * fo.y + row0[2] * fo.z + row0[3], row1[0] * fo.x + row1[1] * fo.y + row1[2] * fo.z + row1[3], row2[0] * fo.x + row2[1] * fo.y + row2[2] * fo.z + row2[3]);
      const V d = v(row0[0] * fd.x + row0[1] * fd.y + row0[2] * fd.z, row1[0] * fd.x + row1[1] * fd.y + row1[2] * fd.z, row2[0] * fd.x + row2[1] * fd.y + row2[2] * fd.z);
      long long nb = 0;
      check(rng2, o, d, ri, 10 + kind, irays, irejected, ihits, nb);
    }
  }
  std::printf("%lld ray intervals, %lld rejected by the box (%.1f %%), %lld exact hits (%lld at an interval end), %lld missed hits\n",
              rays, rejected, 100.0 * rejected / std::max(1LL, rays), hitsSeen, boundary, bad);
  std::printf("instanced (object-space rays through inverse_rows): %lld ray intervals, %lld rejected by the box (%.1f %%), %lld exact hits\n",
              irays, irejected, 100.0 * irejected / std::max(1LL, irays), ihits);
  if (bad == 0 && rejected > rays / 50 && hitsSeen > rays / 10 && irejected > irays / 50 && ihits > irays / 20) std::printf("all conservative\n");
  return bad == 0 ? 0 : 1;
}
