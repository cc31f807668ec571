// Niederreiter base-2 low-discrepancy sampler of the QMC integrator (mlt/rnd_qmc.{h,cpp}, mlt/integrator_qmc.cpp: EnableQMC), host side.
// Written from the published construction - P. Bratley, B. L. Fox, H. Niederreiter, "Implementation and test of low discrepancy sequences",
// ACM TOMACS 2(3), 1992, section 3 (base 2) - and pinned to the numbers the reference's own program prints
// (tests/golden/qmc/niederreiter_11x31.json, tests/test_qmc_cpu.py).
//
// Dimension d uses the d-th monic irreducible polynomial p over GF(2) in increasing order of its bit pattern, starting from x (they need not
// be primitive): x, x+1, x^2+x+1, x^3+x+1, ... Let e = deg p. For q = 0, 1, 2, ... write q = e*k + u with 0 <= u < e and let b = p^(k+1),
// m = deg b. The sequence v_k satisfies the linear recurrence whose characteristic polynomial is b; its m starting values are 0 below
// deg p^k and 1 from there on. Generator-matrix entry (row q, column i) is v_k[i + u]: column i is the word that sample index bit i
// switches on, row 0 being its most significant bit. 31 rows give the 31-bit words of the table (the upper 31 of the reference's 63 rows).
#pragma once
#include <cstdint>

namespace hpt_qmc {

static const int DIMENSIONS = 11;
static const int RESOLUTION = 31;

// remainder of a modulo b, polynomials over GF(2) as bit patterns
inline uint32_t polyMod(uint32_t a, uint32_t b)
{
  int db = 31; while (!((b >> db) & 1u)) db--;
  for (int da = 31; da >= db; da--) if ((a >> da) & 1u) a ^= b << (da - db);
  return a;
}

// the first DIMENSIONS irreducible polynomials: a candidate is kept when no earlier one divides it (every reducible polynomial below the
// 11th irreducible one, x^5+x^3+x^2+x+1, has an irreducible factor among its predecessors)
inline void irreduciblePolys(uint32_t out[DIMENSIONS])
{
  int n = 0;
  for (uint32_t cand = 2u; n < DIMENSIONS; cand++) {
    bool irreducible = true;
    for (int i = 0; i < n && irreducible; i++) if (polyMod(cand, out[i]) == 0u) irreducible = false;
    if (irreducible) out[n++] = cand;
  }
}

// table[d * RESOLUTION + i]: the 31-bit column of dimension d that bit i of the sample index selects
inline void buildTable(uint32_t table[DIMENSIONS * RESOLUTION])
{
  uint32_t polys[DIMENSIONS];
  irreduciblePolys(polys);
  for (int d = 0; d < DIMENSIONS; d++) {
    const uint32_t p = polys[d];
    int e = 31; while (!((p >> e) & 1u)) e--;
    uint32_t* col = table + d * RESOLUTION;
    for (int i = 0; i < RESOLUTION; i++) col[i] = 0u;
    uint64_t b = 1u;                                   // p^k as a bit pattern; its degree stays below 64 for the 31 rows kept (e <= 5: at most 35)
    int m = 0;
    uint8_t v[RESOLUTION + 8];                         // v_k[0 .. RESOLUTION + e - 2]
    for (int q = 0; q < RESOLUTION; q++) {
      const int u = q % e;
      if (u == 0) {
        const int mPrev = m;
        uint64_t nb = 0u;                              // b *= p
        for (int t = 0; t <= e; t++) if ((p >> t) & 1u) nb ^= b << t;
        b = nb; m += e;
        for (int i = 0; i < RESOLUTION + e - 1; i++) {
          if (i < mPrev) v[i] = 0;
          else if (i < m) v[i] = 1;
          else {                                       // v[i] = sum over t = 1..m of (coefficient of x^(m-t) in b) * v[i - t]
            uint8_t s = 0;
            for (int t = 1; t <= m; t++) s ^= (uint8_t)((b >> (m - t)) & 1u) & v[i - t];
            v[i] = s;
          }
        }
      }
      for (int i = 0; i < RESOLUTION; i++) col[i] |= (uint32_t)v[i + u] << (RESOLUTION - 1 - q);
    }
  }
}

// IntegratorQMC::EnableQMC (mlt/integrator_qmc.cpp:11-86): which dimensions feed which draw. out = { dof, spd, motion, mat, lgt }; 0 = that
// draw stays with the pseudo generator (dimensions 0 and 1 are always the pixel). The layout with all three features leaves the
// first-bounce material and light draws pseudo as well.
inline void layout(bool dof, bool spectral, bool motion, uint32_t out[5])
{
  uint32_t spd = 0, mot = 0, mat = 0, lgt = 0;
  if (dof && spectral && motion) { mot = 5; spd = 4; mat = 0; lgt = 0; }
  else if (dof && spectral)      { spd = 4; mat = 5; lgt = 7; }
  else if (spectral && motion)   { mot = 2; spd = 3; mat = 4; lgt = 6; }
  else if (dof && motion)        { mot = 4; mat = 5; lgt = 7; }
  else if (dof)                  { mat = 4; lgt = 6; }
  else if (spectral)             { spd = 4; mat = 2; lgt = 5; }
  else if (motion)               { mot = 4; mat = 2; lgt = 5; }
  else                           { mat = 2; lgt = 4; }
  out[0] = 2u; out[1] = spd; out[2] = mot; out[3] = mat; out[4] = lgt;
}

} // namespace hpt_qmc
