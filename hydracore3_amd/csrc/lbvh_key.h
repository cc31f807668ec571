// The 64-bit sort key of the batched BLAS build (hpt_lbvh.hip section 9): the mesh's slot in the batch above the Morton code of the centroid.
// Plain integers only, so that host programs (tests/cpp/lbvh_key_test.cpp) compile exactly what the kernels compile.
#pragma once
#if defined(__HIPCC__)
#define LBVH_KEY_HD __host__ __device__ inline
#else
#define LBVH_KEY_HD inline
#endif

namespace hpt {

// bits that hold the slot: ceil(log2(slots)); Morton bits per axis that remain: min(21, (64 - slotBits) / 3) - 21 up to 2 slots, 16 at 2^16, 14 at 2^20
LBVH_KEY_HD unsigned lbvhSlotBits(unsigned slots) { unsigned b = 0; while (b < 32u && (1ull << b) < (unsigned long long)slots) b++; return b; }
LBVH_KEY_HD unsigned lbvhMortonBits(unsigned slotBits) { const unsigned m = (64u - slotBits) / 3u; return m < 21u ? m : 21u; }
// morton63: the interleaved code of three 21-bit coordinates (bit 3 k + 2 - axis); its low 3 (21 - m) bits - the low bits of every axis - are dropped
LBVH_KEY_HD unsigned long long lbvhPackKey(unsigned slot, unsigned slotBits, unsigned long long morton63)
{
  const unsigned m = lbvhMortonBits(slotBits);
  const unsigned long long code = (morton63 & 0x7FFFFFFFFFFFFFFFull) >> (3u * (21u - m));
  return slotBits ? (((unsigned long long)slot << (3u * m)) | code) : code;
}
LBVH_KEY_HD unsigned lbvhKeySlot(unsigned long long key, unsigned slotBits) { return slotBits ? (unsigned)(key >> (3u * lbvhMortonBits(slotBits))) : 0u; }

} // namespace hpt
