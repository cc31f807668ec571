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

int main()
{
  std::mt19937 rng(20261017);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto uni = [&](double a, double b) { return a + (b - a) * U(rng); };
  auto unit = [&]() { double x, y, z, l; do { x = uni(-1, 1); y = uni(-1, 1); z = uni(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                      l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  // the device reciprocal: within 1 ulp of 1 / x, clamped like slabRay
  auto rcp = [&](float x) {
    float r = 1.0f / x;
    const int k = (int)(rng() % 3u);
    if (std::isfinite(r) && k == 1) r = std::nextafter(r, INFINITY); else if (std::isfinite(r) && k == 2) r = std::nextafter(r, -INFINITY);
    return std::min(std::max(r, -1.0e30f), 1.0e30f);
  };
  long long rays = 0, rejected = 0, bad = 0, hitsSeen = 0, boundary = 0;
  const int QUADS = 40000, RAYS = 120;
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
      const MT m0 = mt(t0, o, d), m1 = mt(t1, o, d);
      // intervals: open, random, and ending or starting exactly on either triangle's own t (and one float beyond it)
      float tn[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, lim[6] = { FLT_MAX, (float)(scale * uni(0.0, 4.0)), m0.tt, m1.tt, std::nextafter(m0.tt, 0.0f), m0.tt };
      if (ri % 3 == 0) { tn[5] = m0.tt; lim[5] = std::nextafter(m0.tt, INFINITY); } else if (ri % 3 == 1) { tn[5] = m1.tt; lim[5] = m1.tt; }
      const V id = v(rcp(d.x), rcp(d.y), rcp(d.z));
      const float oSum = std::fabs(o.x) + std::fabs(o.y) + std::fabs(o.z), dSum = std::fabs(d.x) + std::fabs(d.y) + std::fabs(d.z);
      for (int j = 0; j < 6; j++) {
        if (!(tn[j] >= 0.0f) || !(lim[j] >= tn[j])) continue;        // the device takes every pair of a lane whose tnear < 0
        rays++;
        const bool reach = sweepBoxMayHit(bx.lo[0], bx.lo[1], bx.lo[2], bx.k1, bx.hi[0], bx.hi[1], bx.hi[2], bx.k0, pl.n[0], pl.n[1], pl.n[2],
                                          o.x, o.y, o.z, d.x, d.y, d.z, id.x, id.y, id.z, oSum, dSum, tn[j], lim[j]);
        const bool hit = hitsIn(t0, o, d, tn[j], lim[j]) || hitsIn(t1, o, d, tn[j], lim[j]);
        hitsSeen += hit;
        boundary += hit && (j >= 2);
        if (reach) continue;
        rejected++;
        if (hit) {
          if (bad < 10) std::printf("MISSED quad %d ray %d kind %d scale %g: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) [%.9g, %.9g]\n", qi, ri, kind, scale, o.x, o.y, o.z, d.x, d.y, d.z, tn[j], lim[j]);
          bad++;
        }
      }
    }
  }
  std::printf("%lld ray intervals, %lld rejected by the box (%.1f %%), %lld exact hits (%lld at an interval end), %lld missed hits\n",
              rays, rejected, 100.0 * rejected / std::max(1LL, rays), hitsSeen, boundary, bad);
  if (bad == 0 && rejected > rays / 50 && hitsSeen > rays / 10) std::printf("all conservative\n");
  return bad == 0 ? 0 : 1;
}
