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
  std::mt19937 rng(20261016);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  auto uni = [&](double a, double b) { return a + (b - a) * U(rng); };
  auto unit = [&]() { double x, y, z, l; do { x = uni(-1, 1); y = uni(-1, 1); z = uni(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                      l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  long long rays = 0, culled = 0, bad = 0, ownWall = 0, ownCulled = 0, bentPairs = 0, bentCulling = 0;
  const int QUADS = 40000, RAYS = 100, IRAYS = 30;
  // the instanced class draws from its own generator, so the rays of the classes above stay what they were
  std::mt19937 rng2(20261019);
  auto uni2 = [&](double a, double b) { return a + (b - a) * U(rng2); };
  auto unit2 = [&]() { double x, y, z, l; do { x = uni2(-1, 1); y = uni2(-1, 1); z = uni2(-1, 1); l = x * x + y * y + z * z; } while (l > 1.0 || l < 1e-6);
                       l = std::sqrt(l); return std::array<double, 3>{ x / l, y / l, z / l }; };
  long long irays = 0, iculled = 0, ihits = 0;
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
    // instanced rays: a unit WORLD ray taken to the quad's object space the way the sweep does it - the instance's world -> object rows
    // (inverse_rows above) and traceSweep's toObjectSpace expressions in the same order - so the object-space direction has any length and
    // orientation. Instances: rotation, scales 1e-2 .. 1e2 per axis, a mirror (one in three), a shear (one in three), translations up to 1e3.
    // World rays leave the world surface from the renderer's offset (into the half-space, grazing, or coming back) or come from anywhere
    // with a segment ending a relative 1e-5 short of or past the plane.
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
      const double a = uni2(-1.2, 1.2), b = uni2(-1.2, 1.2);
      const std::array<double, 3> hw = toWorld(cx + a * hu * tu[0] + b * hv * tv[0], cy + a * hu * tu[1] + b * hv * tv[1], cz + a * hu * tu[2] + b * hv * tv[2]);
      std::array<double, 3> nw;                                          // the world plane's normal (inverse transpose)
      for (int r = 0; r < 3; r++) nw[r] = (double)row0[r] * nrm[0] + (double)row1[r] * nrm[1] + (double)row2[r] * nrm[2];
      { const double l = std::sqrt(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]); for (double& x : nw) x /= l; }
      const double side = (ri & 4) ? 1.0 : -1.0;
      double wo[3], wd[3], lim;
      if (kind <= 2) {
        const float hp[3] = { (float)hw[0], (float)hw[1], (float)hw[2] };
        const float h = std::max(std::max(hp[0], std::max(hp[1], hp[2])), 1.0f) * 5e-6f;
        for (int k = 0; k < 3; k++) wo[k] = (double)(hp[k] + (float)(side * nw[k]) * h);
        std::array<double, 3> w = unit2();
        double wn = w[0] * nw[0] + w[1] * nw[1] + w[2] * nw[2];
        if (kind == 1) { const double g = std::pow(10.0, uni2(-7.0, -1.0)); for (int k = 0; k < 3; k++) w[k] = w[k] - wn * nw[k] + g * side * nw[k]; }
        else if ((wn * side < 0) != (kind == 2)) { for (double& x : w) x = -x; }
        const double wl = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        for (int k = 0; k < 3; k++) wd[k] = w[k] / wl;
        lim = ri % 3 == 0 ? FLT_MAX : std::fabs(scale) * uni2(0.0, 4.0) * 10.0;
      } else {
        const std::array<double, 3> w = unit2();
        const double dist = std::max(scale, 1e-3) * std::pow(10.0, uni2(-3.0, 2.0));
        double dd[3], l = 0.0;
        for (int k = 0; k < 3; k++) wo[k] = (double)(float)(hw[k] + w[k] * dist);
        for (int k = 0; k < 3; k++) { dd[k] = hw[k] - wo[k]; l += dd[k] * dd[k]; }
        l = std::sqrt(l); if (!(l > 0.0)) continue;
        for (int k = 0; k < 3; k++) wd[k] = dd[k] / l;
        lim = l * (1.0 + uni2(-1e-5, 1e-5));
        if (ri % 7 == 0) lim = FLT_MAX;
      }
      const V fo = v((float)wo[0], (float)wo[1], (float)wo[2]), fd = v((float)wd[0], (float)wd[1], (float)wd[2]);
      // traceSweep's toObjectSpace, the same expressions in the same order
      const V o = v(row0[0] * fo.x + row0[1] * fo.y + row0[2] * fo.z + row0[3], row1[0] * fo.x + row1[1] * fo.y + row1[2] * fo.z + row1[3], row2[0] * fo.x + row2[1] * fo.y + row2[2] * fo.z + row2[3]);
      const V d = v(row0[0] * fd.x + row0[1] * fd.y + row0[2] * fd.z, row1[0] * fd.x + row1[1] * fd.y + row1[2] * fd.z, row2[0] * fd.x + row2[1] * fd.y + row2[2] * fd.z);
      const float flim = (float)lim, tnear = 0.0f;
      irays++;
      const bool hit = occludes(t0, o, d, tnear, flim) || occludes(t1, o, d, tnear, flim) || closerHit(t0, o, d, tnear, flim, false) || closerHit(t1, o, d, tnear, flim, false);
      ihits += hit;
      if (sweepPairMayReach(p.n[0], p.n[1], p.n[2], p.c, p.ctr[0], p.ctr[1], p.ctr[2], p.m0, p.q[0], p.q[1], p.q[2], o.x, o.y, o.z, d.x, d.y, d.z, flim + 0.0f)) continue;
      iculled++;
      if (hit) {
        if (bad < 10) std::printf("MISSED (instanced) quad %d ray %d scale %g axis %d: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) lim %.9g\n", qi, ri, scale, (int)axis, o.x, o.y, o.z, d.x, d.y, d.z, flim);
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
  std::printf("instanced (object-space rays through inverse_rows): %lld rays, %lld culled (%.1f %%), %lld exact hits\n", irays, iculled,
              100.0 * iculled / std::max(1LL, irays), ihits);
  if (bad == 0 && bentCulling == 0 && ownCulled * 10 > ownWall * 9 && iculled > irays / 10 && ihits > irays / 20) std::printf("all conservative\n");
  return bad == 0 ? 0 : 1;
}
