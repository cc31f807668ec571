// The optimal binary topology over the <= 7 leaves of a treelet (Karras & Aila, "Fast Parallel Construction of High-Quality Bounding Volume
// Hierarchies", HPG 2013, section 3): dynamic programming over the subsets of the leaves. This header is the scalar DEFINITION of the recurrence
// and of its tie rule; hpt_lbvh.hip evaluates the same two functions with the subsets spread over the lanes of a wave, a host test
// (tests/cpp/treelet_opt_test.cpp) runs them against the enumeration of every topology, tests/treelet_reference.py restates them in numpy.
//
//   area(s)  = half-area of the union box of the leaves in s (unpadded min / max unions: exact in float)
//   cost(s)  = 0                                                   for a single leaf (leaf sets never change; their cost is a constant)
//            = area(s) + min over p of (cost(p) + cost(s ^ p))     p a non-empty proper subset of s
//   part(s)  = the LOWEST mask p that attains the minimum (so p never holds s's highest leaf, and s ^ p always does)
//
// Every sum is a float sum in exactly this association and nothing is contracted (the build sets -ffp-contract=off), so the scalar and the
// lane-parallel evaluation choose the same partitions bit for bit. Float addition is monotonic, so cost(full set) never exceeds the cost, summed
// by the same formula, of any particular topology: "strictly lower than the current tree" is a comparison of two such sums.
#pragma once

#ifndef HPT_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define HPT_HD __host__ __device__ inline
#else
#define HPT_HD inline
#endif
#endif

namespace hpt {

static const int TREELET_LEAVES = 7;                       // leaves of a treelet at the most
static const int TREELET_SUBSETS = 1 << TREELET_LEAVES;    // entry s of a table belongs to the leaf set with mask s (entry 0 is unused)

HPT_HD float treeletHalfArea(const float lo[3], const float hi[3])
{
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}

HPT_HD int treeletPopcount(unsigned s) { int c = 0; for (; s; s &= s - 1u) c++; return c; }

// union box of the leaves in s (leafBox[j] = {lo.xyz, hi.xyz} of leaf j) and its half-area
HPT_HD float treeletUnion(unsigned s, const float (*leafBox)[6], float lo[3], float hi[3])
{
  for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
  for (int j = 0; j < TREELET_LEAVES; j++) if ((s >> j) & 1u)
    for (int a = 0; a < 3; a++) { lo[a] = leafBox[j][a] < lo[a] ? leafBox[j][a] : lo[a]; hi[a] = leafBox[j][3 + a] > hi[a] ? leafBox[j][3 + a] : hi[a]; }
  return treeletHalfArea(lo, hi);
}

// The best split of s (two leaves or more) given cost[] of every smaller subset of s: returns min (cost(p) + cost(s ^ p)) and the lowest p that
// attains it. The candidates are the non-empty subsets of s without its highest leaf, each unordered split once, in ascending order of p.
HPT_HD float treeletBestSplit(unsigned s, const float* cost, unsigned& part)
{
  unsigned top = s; while (top & (top - 1u)) top &= top - 1u;           // s's highest bit
  const unsigned rest = s ^ top;
  float best = 3.0e38f; unsigned bestP = 0u;
  // (p - rest) & rest walks the subsets of rest in ascending order, starting from 0
  for (unsigned p = (0u - rest) & rest; p != 0u; p = (p - rest) & rest) {
    const float c = cost[p] + cost[s ^ p];
    if (c < best || bestP == 0u) { best = c; bestP = p; }
  }
  part = bestP;
  return best;
}

// The scalar form: area, cost and part of every subset of the first k leaves (2 <= k <= 7), subsets in order of their size
HPT_HD void treeletOptimize(int k, const float (*leafBox)[6], float* area, float* cost, unsigned char* part)
{
  const unsigned full = (1u << k) - 1u;
  for (unsigned s = 1u; s <= full; s++) { float lo[3], hi[3]; area[s] = treeletUnion(s, leafBox, lo, hi); cost[s] = 0.0f; part[s] = 0; }
  for (int size = 2; size <= k; size++)
    for (unsigned s = 1u; s <= full; s++) if (treeletPopcount(s) == size) {
      unsigned p; const float c = treeletBestSplit(s, cost, p);
      cost[s] = area[s] + c; part[s] = (unsigned char)p;
    }
}

} // namespace hpt
