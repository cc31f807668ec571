// The treelet optimiser's scalar form (hydracore3_amd/csrc/treelet_opt.h) against the explicit enumeration of every binary topology over k = 2 .. 7
// leaf boxes: the optimum equals the minimum over all (2k - 3)!! topologies, and the topology the partitions describe attains it. Random boxes,
// coincident boxes, flat boxes and boxes with one far outlier, from a fixed seed. Every case is printed - the boxes as float bit patterns, the
// chosen partition of every subset, the optimum's bit pattern - so that tests/treelet_reference.py can be held to the same choices.
// Build: g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined treelet_opt_test.cpp   (no device, no library)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../hydracore3_amd/csrc/treelet_opt.h"

using namespace hpt;

static uint32_t rngState = 20130719u;
static float rnd() { rngState = rngState * 1664525u + 1013904223u; return (float)(rngState >> 8) * (1.0f / 16777216.0f); }
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// every topology over the leaves in `leaves`, each once: the last leaf stays on the second side; cost by the recurrence's formula
static void enumerate(const std::vector<int>& leaves, const float* area, std::vector<float>& costs, std::vector<unsigned>& masks)
{
  costs.clear(); masks.clear();
  unsigned all = 0u; for (int l : leaves) all |= 1u << l;
  if (leaves.size() == 1) { costs.push_back(0.0f); return; }
  const size_t r = leaves.size() - 1;
  for (unsigned m = 1u; m < (1u << r); m++) {
    std::vector<int> a, b;
    for (size_t j = 0; j < r; j++) (((m >> j) & 1u) ? a : b).push_back(leaves[j]);
    b.push_back(leaves[r]);
    std::vector<float> ca, cb; std::vector<unsigned> unused;
    enumerate(a, area, ca, unused); enumerate(b, area, cb, unused);
    for (float x : ca) for (float y : cb) costs.push_back(area[all] + (x + y));
  }
}

static float chosenCost(unsigned s, const float* area, const unsigned char* part)
{
  if ((s & (s - 1u)) == 0u) return 0.0f;
  const unsigned p = part[s];
  return area[s] + (chosenCost(p, area, part) + chosenCost(s ^ p, area, part));
}

static int failures = 0;

static void runCase(const char* kind, int k, const float (*box)[6])
{
  float area[TREELET_SUBSETS], cost[TREELET_SUBSETS]; unsigned char part[TREELET_SUBSETS];
  treeletOptimize(k, box, area, cost, part);
  const unsigned full = (1u << k) - 1u;
  std::vector<int> leaves; for (int j = 0; j < k; j++) leaves.push_back(j);
  std::vector<float> costs; std::vector<unsigned> unused;
  enumerate(leaves, area, costs, unused);
  size_t want = 1; for (int j = 3; j <= 2 * k - 3; j += 2) want *= (size_t)j;
  float best = costs[0]; for (float c : costs) best = c < best ? c : best;
  bool ok = costs.size() == want && bits(best) == bits(cost[full]) && bits(chosenCost(full, area, part)) == bits(best);
  for (unsigned s = 1u; s <= full; s++) if (s & (s - 1u)) {                // a partition: non-empty, proper, without s's highest leaf
    const unsigned p = part[s]; unsigned top = s; while (top & (top - 1u)) top &= top - 1u;
    ok = ok && p != 0u && (p & ~s) == 0u && p != s && (p & top) == 0u;
  }
  if (!ok) { failures++; std::printf("FAILED %s k=%d: %zu topologies (want %zu), enumerated minimum %a, optimum %a, chosen %a\n", kind, k, costs.size(), want, best, cost[full], chosenCost(full, area, part)); }
  std::printf("case %s k=%d boxes=", kind, k);
  for (int j = 0; j < k; j++) for (int a = 0; a < 6; a++) std::printf("%08x%s", bits(box[j][a]), (j == k - 1 && a == 5) ? "" : ",");
  std::printf(" parts=");
  for (unsigned s = 1u; s <= full; s++) std::printf("%02x", part[s]);
  std::printf(" cost=%08x topologies=%zu\n", bits(cost[full]), costs.size());
}

int main()
{
  int cases = 0;
  for (int k = 2; k <= TREELET_LEAVES; k++) {
    float box[TREELET_LEAVES][6];
    auto randomBox = [&](int j, float spread, float size) {
      for (int a = 0; a < 3; a++) { const float c = rnd() * spread, e = rnd() * size; box[j][a] = c; box[j][3 + a] = c + e; }
    };
    for (int rep = 0; rep < 3; rep++) { for (int j = 0; j < k; j++) randomBox(j, 10.0f, 3.0f); runCase("random", k, box); cases++; }
    // coincident: every box the same (every topology costs the same up to the rounding of its sums: ties nearly everywhere)
    randomBox(0, 10.0f, 3.0f); for (int j = 1; j < k; j++) std::memcpy(box[j], box[0], sizeof(box[0]));
    runCase("coincident", k, box); cases++;
    // all points in one spot: every half-area is 0
    for (int j = 0; j < k; j++) for (int a = 0; a < 3; a++) box[j][a] = box[j][3 + a] = 1.5f;
    runCase("points", k, box); cases++;
    // flat: no extent in y (half of them) or in z
    for (int j = 0; j < k; j++) { randomBox(j, 10.0f, 3.0f); const int a = (j & 1) ? 1 : 2; box[j][3 + a] = box[j][a]; }
    runCase("flat", k, box); cases++;
    // pairs of coincident boxes among random ones: ties between some subsets only
    for (int j = 0; j < k; j++) { if (j & 1) std::memcpy(box[j], box[j - 1], sizeof(box[0])); else randomBox(j, 10.0f, 3.0f); }
    runCase("pairs", k, box); cases++;
    // one far outlier
    for (int j = 0; j < k; j++) randomBox(j, 1.0f, 0.5f);
    for (int a = 0; a < 3; a++) { box[k / 2][a] += 1.0e4f; box[k / 2][3 + a] += 1.0e4f; }
    runCase("outlier", k, box); cases++;
  }
  if (failures) { std::printf("%d of %d cases FAILED\n", failures, cases); return 1; }
  std::printf("%d cases passed\n", cases);
  return 0;
}
