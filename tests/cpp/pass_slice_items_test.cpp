// Host check of the megakernel's work-item arithmetic (hydracore3_amd/csrc/hpt_types.h: passSliceCount, passSliceItem, tidOfIndex; used by
// hpt_kernels.hip: pathTraceKernel and by the host's grid sizing). For passNum in {1, 7, 8, 1024} and slices {0, 1, 2, 3, 8, 2000}, with and
// without a tid interleave: every (tid, pass) is covered exactly once, the slices of a tid appear in ascending item order and each starts
// where the one before it ended, and an item's predecessor (the slice before it of the same pixel) has a smaller item index - what the
// kernel's progress argument rests on. Plain g++, no GPU; meant to be built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
struct float4 { float x, y, z, w; };
#include "../../hydracore3_amd/csrc/hpt_types.h"
using namespace hpt;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void run(uint tidBegin, uint tidCount, uint chunk, uint stride, uint tidEnd, uint passNum, uint s)
{
  const uint slices = passSliceCount(passNum, s);
  const size_t items = (size_t)tidCount * slices;
  CHECK(slices >= 1u && (s == 0u || s >= passNum ? slices == 1u : slices == (passNum + s - 1u) / s), "slice count %u for %u passes, slice %u", slices, passNum, s);
  std::vector<unsigned char> covered((size_t)tidEnd * passNum, 0);      // (tid, pass) -> times rendered
  std::vector<uint> nextSlice(tidEnd, 0u), nextPass(tidEnd, 0u);         // per tid: the slice and the pass the next item must bring
  std::vector<long long> lastItem(tidEnd, -1);
  for (size_t k = 0; k < items; k++) {
    const SliceItem it = passSliceItem((uint)k, tidCount, passNum, s);
    CHECK(it.index < tidCount && it.slice < slices, "item %zu: index %u slice %u", k, it.index, it.slice);
    CHECK((size_t)it.slice * tidCount + it.index == k, "item %zu is not slice-major", k);
    CHECK(it.passes >= 1u && it.first + it.passes <= passNum, "item %zu: passes [%u, %u) of %u", k, it.first, it.first + it.passes, passNum);
    CHECK(it.first == passSliceFirst(it.slice, passNum, s) && it.passes == passSlicePasses(it.slice, passNum, s), "item %zu: the parts disagree", k);
    if (s != 0u && s < passNum) CHECK(it.slice + 1u == slices ? it.passes <= s : it.passes == s, "item %zu: %u passes with slice %u", k, it.passes, s);
    if (it.slice + 1u == slices) CHECK(it.first + it.passes == passNum, "item %zu: the last slice ends at %u of %u", k, it.first + it.passes, passNum);
    // the kernel's test for "this slice has a successor"
    CHECK(((s != 0u && (it.slice + 1u) * s < passNum) ? 1 : 0) == (it.slice + 1u < slices ? 1 : 0), "item %zu: successor test", k);
    const uint tid = tidOfIndex(tidBegin, chunk, stride, it.index);
    if (tid >= tidEnd) continue;                                           // dropped by the kernel: in every slice alike
    CHECK(it.slice == nextSlice[tid], "tid %u: slice %u drawn when %u was due", tid, it.slice, nextSlice[tid]);
    CHECK(it.first == nextPass[tid], "tid %u: slice %u starts at pass %u, the one before ended at %u", tid, it.slice, it.first, nextPass[tid]);
    if (it.slice > 0u) {
      CHECK(k >= tidCount && lastItem[tid] == (long long)(k - tidCount), "tid %u: predecessor of item %zu is item %lld", tid, k, lastItem[tid]);
      CHECK(lastItem[tid] < (long long)k, "tid %u: predecessor %lld not before item %zu", tid, lastItem[tid], k);
    }
    lastItem[tid] = (long long)k; nextSlice[tid] = it.slice + 1u; nextPass[tid] = it.first + it.passes;
    for (uint p = it.first; p < it.first + it.passes; p++) covered[(size_t)tid * passNum + p]++;
  }
  // every tid the launch maps to gets every pass once; no other tid gets any
  std::vector<unsigned char> mine(tidEnd, 0);
  for (uint i = 0; i < tidCount; i++) { const uint tid = tidOfIndex(tidBegin, chunk, stride, i); if (tid < tidEnd) { CHECK(!mine[tid], "tid %u mapped twice", tid); mine[tid] = 1; } }
  for (uint tid = 0; tid < tidEnd; tid++)
    for (uint p = 0; p < passNum; p++)
      CHECK(covered[(size_t)tid * passNum + p] == mine[tid], "tid %u pass %u rendered %u times (passNum %u, slice %u)", tid, p, (uint)covered[(size_t)tid * passNum + p], passNum, s);
}

int main()
{
  const uint passNums[] = {1u, 7u, 8u, 1024u}, slicesOf[] = {0u, 1u, 2u, 3u, 8u, 2000u};
  int cases = 0;
  for (uint passNum : passNums)
    for (uint s : slicesOf) {
      run(0u, 300u, 0x40000000u, 1u, 300u, passNum, s);          // one contiguous window
      run(37u, 200u, 0x40000000u, 1u, 300u, passNum, s);         // a window inside the frame
      run(0u, 160u, 16u, 2u, 300u, passNum, s);                  // rank 0 of 2: every other 16-tid chunk, the last ones past the frame's end
      run(16u, 160u, 16u, 2u, 300u, passNum, s);                 // rank 1 of 2
      run(32u, 112u, 16u, 3u, 300u, passNum, s);                 // rank 2 of 3, a partial last chunk
      cases += 5;
    }
  if (failures) { std::printf("pass_slice_items_test: %d failure(s)\n", failures); return 1; }
  std::printf("pass_slice_items_test: %d cases passed\n", cases);
  return 0;
}
