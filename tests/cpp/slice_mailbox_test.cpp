// Host check of the tagged words a pixel is handed over in between the pass slices of the megakernel (hydracore3_amd/csrc/hpt_types.h:
// sliceWordPack, sliceWordFor, sliceWordPayload; used by hpt_kernels.hip: pathTraceKernel<.., SLICED>). A word written by slice j is taken by
// slice j + 1 and by no other; the payload comes back bit for bit, whatever float it was (all ones, NaNs with payload bits, -0, denormals);
// an empty word (tag 0: the zeroed mailbox) is taken by no slice, slice 0 included. Plain g++, no GPU; meant to be built with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
struct float4 { float x, y, z, w; };
#include "../../hydracore3_amd/csrc/hpt_types.h"
using namespace hpt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static uint bitsOf(float f) { uint u; std::memcpy(&u, &f, 4); return u; }

int main()
{
  static_assert(sizeof(unsigned long long) == 8, "a mailbox word is 64 bits");
  static_assert(SLICE_MAIL_USED <= SLICE_MAIL_WORDS && SLICE_MAIL_WORDS * 8 == 64, "one 64-byte line per pixel");
  const uint payloads[] = {
    0u, 1u, 0xFFFFFFFFu,                                              // all ones (as a float: a NaN with every payload bit)
    bitsOf(std::numeric_limits<float>::quiet_NaN()), 0x7FC00001u, 0xFFC00000u, 0x7F800001u /* signalling */, 0xFF800001u,
    bitsOf(-0.0f), bitsOf(0.0f), 0x80000000u,                         // negative zero keeps its sign bit
    bitsOf(std::numeric_limits<float>::infinity()), bitsOf(-std::numeric_limits<float>::infinity()),
    bitsOf(std::numeric_limits<float>::denorm_min()), 0x80000001u, bitsOf(1.0f), bitsOf(-123.456f), 0x12345678u, 0x7FFFFFFFu };
  const uint slices[] = { 0u, 1u, 2u, 3u, 255u, 0x7FFFFFFEu, 0xFFFFFFFDu };
  int cases = 0;
  for (uint p : payloads)
    for (uint j : slices) {
      const unsigned long long w = sliceWordPack(j, p);
      CHECK(sliceWordPayload(w) == p, "payload %08x of slice %u came back as %08x", p, j, sliceWordPayload(w));
      CHECK((uint)(w >> 32) == j + 1u && (uint)(w >> 32) != 0u, "slice %u: tag %u", j, (uint)(w >> 32));
      CHECK(sliceWordFor(w, j + 1u), "the word of slice %u is not taken by slice %u (payload %08x)", j, j + 1u, p);
      for (uint t : slices) if (t != j + 1u) CHECK(!sliceWordFor(w, t), "the word of slice %u is taken by slice %u (payload %08x)", j, t, p);
      CHECK(!sliceWordFor(w, j), "the word of slice %u is taken by its own slice", j);
      // through the float the kernel holds: the bits survive the conversion there and back
      CHECK(hptFloatToBits(hptBitsToFloat(sliceWordPayload(w))) == p, "payload %08x changed through a float", p);
      cases++;
    }
  // tag 0 (the zeroed mailbox, whatever its payload bits) matches no slice
  for (uint p : payloads) {
    const unsigned long long empty = (unsigned long long)p;
    for (uint t : slices) CHECK(!sliceWordFor(empty, t), "an empty word (payload %08x) is taken by slice %u", p, t);
    for (uint t = 0u; t < 1024u; t++) CHECK(!sliceWordFor(empty, t), "an empty word (payload %08x) is taken by slice %u", p, t);
    cases++;
  }
  // a payload never leaks into the tag nor the tag into the payload
  CHECK(sliceWordPack(0u, 0xFFFFFFFFu) == 0x00000001FFFFFFFFull, "pack(0, ~0)");
  CHECK(sliceWordPack(4u, 0x80000000u) == 0x0000000580000000ull, "pack(4, -0.0f)");
  if (failures) { std::printf("slice_mailbox_test: %d failure(s)\n", failures); return 1; }
  std::printf("slice_mailbox_test: %d cases passed\n", cases);
  return 0;
}
