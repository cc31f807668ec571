// The sort key of the batched BLAS build (lbvh_key.h: lbvhSlotBits, lbvhMortonBits, lbvhPackKey, lbvhKeySlot) on the host: the slot comes back
// out of the key, keys order by slot first and by the truncated Morton code second, the code never reaches into the slot's bits, and the Morton bits
// left per axis are the ones the header states. Built with -fsanitize=address,undefined by tests/test_device_two_level_cpu.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include "../../hydracore3_amd/csrc/lbvh_key.h"

using namespace hpt;
typedef unsigned uint;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); failures++; } } while (0)

int main()
{
  CHECK(lbvhSlotBits(0) == 0 && lbvhSlotBits(1) == 0 && lbvhSlotBits(2) == 1 && lbvhSlotBits(3) == 2 && lbvhSlotBits(256) == 8 && lbvhSlotBits(257) == 9);
  CHECK(lbvhSlotBits(0xFFFFFFFFu) == 32);
  for (uint e = 0; e <= 31; e++) {
    const uint sb = lbvhSlotBits(1u << e);
    CHECK(sb == e);
    std::printf("slots=2^%u morton_bits=%u\n", e, lbvhMortonBits(sb));
    CHECK(3u * lbvhMortonBits(sb) + sb <= 64u);
  }
  std::mt19937_64 rng(7);
  const unsigned long long M63 = 0x7FFFFFFFFFFFFFFFull;
  for (uint slots : { 1u, 2u, 3u, 5u, 256u, 257u, 300u, 4096u, 65536u, 1u << 20, 1u << 22, 0xFFFFFFFFu }) {
    const uint sb = lbvhSlotBits(slots), m = lbvhMortonBits(sb);
    for (int k = 0; k < 2000; k++) {
      const uint s0 = (uint)(rng() % slots), s1 = (uint)(rng() % slots);
      const unsigned long long c0 = k == 0 ? M63 : (k == 1 ? 0ull : rng() & M63), c1 = rng() & M63;
      const unsigned long long k0 = lbvhPackKey(s0, sb, c0), k1 = lbvhPackKey(s1, sb, c1);
      CHECK(lbvhKeySlot(k0, sb) == s0 && lbvhKeySlot(k1, sb) == s1);
      const unsigned long long t0 = c0 >> (3u * (21u - m)), t1 = c1 >> (3u * (21u - m));
      CHECK((k0 & ((m == 21u && sb <= 1u) ? M63 : ((1ull << (3u * m)) - 1ull))) == t0);                 // the code sits below the slot, untouched
      if (s0 != s1) CHECK((k0 < k1) == (s0 < s1));
      else CHECK((k0 < k1) == (t0 < t1) && (k0 == k1) == (t0 == t1));
      if (c0 <= c1) CHECK(lbvhPackKey(s0, sb, c0) <= lbvhPackKey(s0, sb, c1));                            // truncation keeps the order of the codes
    }
  }
  if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
  std::printf("all key checks passed\n");
  return 0;
}
