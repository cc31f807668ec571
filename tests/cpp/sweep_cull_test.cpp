// Host check of the sweep's pair cull (hydracore3_amd/csrc/hpt_types.h: sweepPairPlane, sweepPairMayReach; used by hpt_device.h: traceSweep).
// The cull may only skip a record pair when the exact float triangle tests (hpt_device.h: triangleOccludes, triangleTestInOrder - restated
// here line by line, built with -ffp-contract=off like the library) reject both of its triangles. Random quads, split into two triangles in
// all four vertex orders, at scales 1e-3 ... 1e4, some axis-aligned (exactly coplanar), some in a random orientation (coplanar up to the
// rounding of their float vertices), a few bent out of their plane (the host must refuse to cull those), a few paired with the padding
// record. Rays: origins ON the quad moved off it by the renderer's own rule (hpt_shade.h: hitPos + hitNorm * max(maxcomp(hitPos), 1) * 5e-6)
// leaving it, grazing, or coming back; origins anywhere; segments that end just short of the plane or just past it; lim = FLT_MAX.
// Asserts "culled => both exact tests reject" and reports how often the wall a ray leaves is culled. Plain g++, no GPU.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cfloat>
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

// triangleOccludes (hpt_device.h)
static bool occludes(const BvhTri& t, V o, V d, float tnear, float tfar)
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
  return (det != 0.0f) & (uu >= 0.0f) & (vv >= 0.0f) & (uu + vv <= 1.0f) & (tt >= tnear) & (tt <= tfar);
}
// triangleTestInOrder's acceptance (hpt_device.h), for a best distance bestT and both values of `found`
static bool closerHit(const BvhTri& t, V o, V d, float tnear, float bestT, bool found)
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
  const bool closer = (tt < bestT) | (!found & (tt == bestT));
  return (det != 0.0f) & (uu >= 0.0f) & (vv >= 0.0f) & (uu + vv <= 1.0f) & (tt >= tnear) & closer;
}
static BvhTri tri(V a, V b, V c)
{
  BvhTri t; std::memset(&t, 0, sizeof(t));
  t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
  t.e1[0] = b.x - a.x; t.e1[1] = b.y - a.y; t.e1[2] = b.z - a.z;
  t.e2[0] = c.x - a.x; t.e2[1] = c.y - a.y; t.e2[2] = c.z - a.z;
  return t;
}
static float maxcomp(V p) { return std::max(p.x, std::max(p.y, p.z)); }

int main()
{
  std::mt19937 rng(20261016);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto uni = [&](double a, double b) { return a + (b - a) * U(rng); };
  auto unit = [&]() { double x, y, z, l; do { x = uni(-1, 1); y = uni(-1, 1); z = uni(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                      l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  long long rays = 0, culled = 0, bad = 0, ownWall = 0, ownCulled = 0, bentPairs = 0, bentCulling = 0;
  const int QUADS = 40000, RAYS = 100;
  for (int qi = 0; qi < QUADS; qi++) {
    const double scale = std::pow(10.0, uni(-3.0, 4.0));
    const bool axis = (qi & 1) == 0;
    // frame: axis-aligned (a random axis, the quad in the two others) or random
    std::array<double, 3> nrm, tu, tv;
    if (axis) {
      const int a = qi / 2 % 3; nrm = { 0, 0, 0 }; tu = { 0, 0, 0 }; tv = { 0, 0, 0 };
      nrm[a] = (qi / 6) % 2 ? 1.0 : -1.0; tu[(a + 1) % 3] = 1.0; tv[(a + 2) % 3] = 1.0;
    } else {
      nrm = unit(); std::array<double, 3> r = unit();
      tu = { nrm[1] * r[2] - nrm[2] * r[1], nrm[2] * r[0] - nrm[0] * r[2], nrm[0] * r[1] - nrm[1] * r[0] };
      const double l = std::sqrt(tu[0] * tu[0] + tu[1] * tu[1] + tu[2] * tu[2]); for (double& x : tu) x /= l;
      tv = { nrm[1] * tu[2] - nrm[2] * tu[1], nrm[2] * tu[0] - nrm[0] * tu[2], nrm[0] * tu[1] - nrm[1] * tu[0] };
    }
    const double cx = uni(-1, 1) * scale * (qi % 5 == 0 ? 0.0 : 1.0), cy = uni(-1, 1) * scale, cz = uni(-1, 1) * scale;
    const double hu = scale * uni(0.05, 1.0), hv = scale * uni(0.05, 1.0) * (qi % 7 == 0 ? 1e-3 : 1.0);   // some long thin quads
    V q[4];
    const double su[4] = { -1, 1, 1, -1 }, sv[4] = { -1, -1, 1, 1 };
    for (int k = 0; k < 4; k++)
      q[k] = v((float)(cx + su[k] * hu * tu[0] + sv[k] * hv * tv[0]), (float)(cy + su[k] * hu * tu[1] + sv[k] * hv * tv[1]), (float)(cz + su[k] * hu * tu[2] + sv[k] * hv * tv[2]));
    const bool bent = qi % 13 == 0;
    if (bent) { const double b = scale * 1e-3; q[2] = v(q[2].x + (float)(b * nrm[0]), q[2].y + (float)(b * nrm[1]), q[2].z + (float)(b * nrm[2])); }
    const int rot = (qi / 3) % 4;                                 // vertex order of the split
    const V A = q[rot], B = q[(rot + 1) % 4], C = q[(rot + 2) % 4], D = q[(rot + 3) % 4];
    BvhTri t0 = tri(A, B, C), t1 = tri(A, C, D);
    const bool padded = qi % 11 == 0;
    if (padded) { std::memset(&t1, 0, sizeof(t1)); t1.primId = 0xFFFFFFFFu; }
    SweepPlane p; sweepPairPlane(t0, t1, p);
    if (bent && !padded) bentPairs++;
    if (bent && !padded && std::isfinite(p.m0)) bentCulling++;
    const V nf = v((float)nrm[0], (float)nrm[1], (float)nrm[2]);
    for (int ri = 0; ri < RAYS; ri++) {
      V o, d; float lim;
      const int kind = ri % 5;
      // a point on the quad (or on its plane just outside it)
      const double a = uni(-1.2, 1.2), b = uni(-1.2, 1.2);
      const V hp = v((float)(cx + a * hu * tu[0] + b * hv * tv[0]), (float)(cy + a * hu * tu[1] + b * hv * tv[1]), (float)(cz + a * hu * tu[2] + b * hv * tv[2]));
      const float side = (ri & 1) ? 1.0f : -1.0f;
      const V hn = v(side * nf.x, side * nf.y, side * nf.z);
      if (kind <= 2) {
        // the renderer's offset rule, then a direction leaving (kind 0: anywhere into the half-space, 1: grazing), or coming back (2)
        const float h = std::max(maxcomp(hp), 1.0f) * 5e-6f;
        o = v(hp.x + hn.x * h, hp.y + hn.y * h, hp.z + hn.z * h);
        std::array<double, 3> w = unit();
        double wn = w[0] * nrm[0] + w[1] * nrm[1] + w[2] * nrm[2];
        if (kind == 1) { const double g = std::pow(10.0, uni(-7.0, -1.0)); for (int k = 0; k < 3; k++) w[k] = w[k] - wn * nrm[k] + g * side * nrm[k]; wn = g * side; }
        else if ((wn * side < 0) != (kind == 2)) { for (double& x : w) x = -x; }
        const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        d = v((float)(w[0] / wl), (float)(w[1] / wl), (float)(w[2] / wl));
        lim = ri % 3 == 0 ? FLT_MAX : (float)(scale * uni(0.0, 4.0));
        if (kind != 2 && !padded && !bent && axis) ownWall++;
      } else {
        // anywhere around the quad, aimed so that the plane is met at t* (ray kind 3: the segment ends just short of it or just past it)
        const std::array<double, 3> w = unit();
        const double dist = scale * std::pow(10.0, uni(-6.0, 0.5));
        o = v((float)(hp.x + w[0] * dist), (float)(hp.y + w[1] * dist), (float)(hp.z + w[2] * dist));
        const V tgt = v((float)(cx + uni(-1.2, 1.2) * hu * tu[0] + uni(-1.2, 1.2) * hv * tv[0]), (float)(cy + uni(-1.2, 1.2) * hu * tu[1]), (float)(cz + uni(-1.2, 1.2) * hu * tu[2]));
        V dd = sub(tgt, o);
        const float l = std::sqrt(dot(dd, dd));
        if (!(l > 0.0f)) continue;
        d = v(dd.x / l, dd.y / l, dd.z / l);
        if (kind == 4) d = v(-d.x, -d.y, -d.z);
        // exact plane distance along the ray (double), the segment ends a few ulp short of it or past it
        const double so = (o.x - cx) * nrm[0] + (o.y - cy) * nrm[1] + (o.z - cz) * nrm[2], sd = d.x * nrm[0] + d.y * nrm[1] + d.z * nrm[2];
        const double ts = sd != 0.0 ? -so / sd : 1.0;
        lim = (float)(std::fabs(ts) * (1.0 + uni(-1e-5, 1e-5)));
        if (ri % 7 == 0) lim = FLT_MAX;
      }
      rays++;
      const float tnear = 0.0f;
      const bool reach = sweepPairMayReach(p.n[0], p.n[1], p.n[2], p.c, p.ctr[0], p.ctr[1], p.ctr[2], p.m0, p.q[0], p.q[1], p.q[2], o.x, o.y, o.z, d.x, d.y, d.z, lim + 0.0f);
      if (kind <= 1 && !padded && !bent && axis && !reach) ownCulled++;
      if (reach) continue;
      culled++;
      const bool hit = occludes(t0, o, d, tnear, lim) || occludes(t1, o, d, tnear, lim) || closerHit(t0, o, d, tnear, lim, false) || closerHit(t1, o, d, tnear, lim, false);
      if (hit) {
        if (bad < 10) std::printf("MISSED quad %d ray %d scale %g axis %d: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) lim %.9g\n", qi, ri, scale, (int)axis, o.x, o.y, o.z, d.x, d.y, d.z, lim);
        bad++;
      }
    }
  }
  // a ray with tnear < 0 is never culled (traceSweep passes lim = NaN for it)
  {
    BvhTri t0 = tri(v(-1, 0, -1), v(1, 0, -1), v(1, 0, 1)), t1 = tri(v(-1, 0, -1), v(1, 0, 1), v(-1, 0, 1));
    SweepPlane p; sweepPairPlane(t0, t1, p);
    if (!sweepPairMayReach(p.n[0], p.n[1], p.n[2], p.c, p.ctr[0], p.ctr[1], p.ctr[2], p.m0, p.q[0], p.q[1], p.q[2], 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, std::nanf(""))) { std::printf("NaN limit culled\n"); bad++; }
    if (sweepPairMayReach(p.n[0], p.n[1], p.n[2], p.c, p.ctr[0], p.ctr[1], p.ctr[2], p.m0, p.q[0], p.q[1], p.q[2], 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, 10.0f)) { std::printf("plain miss not culled\n"); bad++; }
  }
  std::printf("%lld rays, %lld culled (%.1f %%), %lld missed hits; own wall (axis-aligned) culled %.2f %% of %lld; bent pairs allowed to cull: %lld of %lld\n",
              rays, culled, 100.0 * culled / rays, bad, 100.0 * ownCulled / std::max(1LL, ownWall), ownWall, bentCulling, bentPairs);
  if (bad == 0 && bentCulling == 0 && ownCulled * 10 > ownWall * 9) std::printf("all conservative\n");
  return bad == 0 ? 0 : 1;
}
