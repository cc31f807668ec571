// rcpIeee / divIeee (hpt_device.h) against the compiler's own 1.0f / x and a / b, bit for bit, on the device.
//
//   exact_div_probe          the device run: one JSON line per set
//     rcp_all      every one of the 2^32 float bit patterns (a wave takes 64 consecutive patterns, so its lanes share an exponent and the
//                  lanes that took the fast path are exactly the patterns inside the guard range: 128 exponents x 2^24 = 2^31)
//     div_edges    the full cross product of an edge set: every exponent x mantissas {0, 1, 0x400000, 0x7FFFFF} x both signs (2048 values:
//                  zeros, denormals, infinities and NaNs among them), 2^22 pairs
//     div_random   2^28 seeded pairs of raw bit patterns
//     div_inrange  2^28 seeded pairs with both exponents inside the guard range [96, 159]: every lane must take the fast path
//   exact_div_probe --host   no device: the guard predicates against the documented ranges for every exponent (the reciprocal seed is a
//                  software stand-in there, so this build proves the predicate and that the helpers compile for the host, not the chain)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "hpt_device.h"

using namespace hpt;

struct Result { unsigned long long mismatches, fast, firstBad; };

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

__host__ __device__ inline uint mix32(uint x) { x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16; return x; }
__host__ __device__ inline uint edgeValue(uint k)   // k < 2048: sign (1 bit), exponent (8 bits), mantissa choice (2 bits)
{
  const uint mant = (k & 3u) == 0u ? 0u : (k & 3u) == 1u ? 1u : (k & 3u) == 2u ? 0x400000u : 0x7FFFFFu;
  return ((k >> 10) << 31) | (((k >> 2) & 255u) << 23) | mant;
}
__host__ __device__ inline uint intoDivRange(uint r) { return (r & 0x807FFFFFu) | ((96u + ((r >> 23) & 63u)) << 23); }

enum { SET_RCP_ALL = 0, SET_DIV_EDGES = 1, SET_DIV_RANDOM = 2, SET_DIV_INRANGE = 3 };

template <int SET>
__global__ void __launch_bounds__(256) probe(const unsigned long long n, const uint seed, Result* out)
{
  unsigned long long bad = 0ull, fast = 0ull, firstBad = ~0ull;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;           // a multiple of 64: a wave's items are consecutive
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint ab, bb = 0u;
    float got, want;
    bool f;
    if (SET == SET_RCP_ALL) {
      ab = (uint)i;
      const float x = __uint_as_float(ab);
      got = rcpIeee(x, f);
      want = 1.0f / x;
    } else {
      if (SET == SET_DIV_EDGES) { ab = edgeValue((uint)(i >> 11)); bb = edgeValue((uint)i & 2047u); }
      else {
        ab = mix32((uint)i * 2u + seed); bb = mix32((uint)i * 2u + 1u + seed * 0x9E3779B9u);
        if (SET == SET_DIV_INRANGE) { ab = intoDivRange(ab); bb = intoDivRange(bb); }
      }
      const float a = __uint_as_float(ab), b = __uint_as_float(bb);
      got = divIeee(a, b, f);
      want = a / b;
    }
    if (__float_as_uint(got) != __float_as_uint(want)) { bad++; const unsigned long long w = ((unsigned long long)ab << 32) | bb; if (w < firstBad) firstBad = w; }
    fast += f ? 1ull : 0ull;
  }
  if (bad != 0ull) { atomicAdd(&out->mismatches, bad); atomicMin(&out->firstBad, firstBad); }
  if (fast != 0ull) atomicAdd(&out->fast, fast);
}

template <int SET>
static int runSet(const char* name, unsigned long long n, uint seed, Result* dres)
{
  Result r = { 0ull, 0ull, ~0ull };
  CHECK(hipMemcpy(dres, &r, sizeof(r), hipMemcpyHostToDevice));
  probe<SET><<<dim3(8192), dim3(256)>>>(n, seed, dres);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(&r, dres, sizeof(r), hipMemcpyDeviceToHost));
  std::printf("{\"set\": \"%s\", \"items\": %llu, \"mismatches\": %llu, \"fast\": %llu, \"first_bad\": \"%016llx\"}\n", name, n, r.mismatches, r.fast, r.firstBad);
  return 0;
}

static int hostCheck()
{
  const uint mants[3] = { 0u, 1u, 0x7FFFFFu };
  int wrong = 0;
  for (uint s = 0; s < 2; s++) for (uint e = 0; e < 256; e++) for (uint m = 0; m < 3; m++) {
    const uint xb = (s << 31) | (e << 23) | mants[m];
    float x; std::memcpy(&x, &xb, 4);
    if (rcpIeeeInRange(x) != (e >= 64u && e <= 191u)) wrong++;
    if (rcpIeeeInRange(x, 1.0f) != (e >= 64u && e <= 191u) || rcpIeeeInRange(1.0f, x) != (e >= 64u && e <= 191u)) wrong++;
    for (uint e2 = 0; e2 < 256; e2++) {
      const uint yb = (e2 << 23) | mants[(m + e2) % 3u];
      float y; std::memcpy(&y, &yb, 4);
      const bool want = e >= 96u && e <= 159u && e2 >= 96u && e2 <= 159u;
      if (divIeeeInRange(x, y) != want || divIeeeInRange(y, x) != want) wrong++;
    }
  }
  for (uint k = 0; k < 4096u; k++) {                                 // intoDivRange lands inside the quotient's range, whatever comes in
    const uint vb = intoDivRange(mix32(k));
    float v; std::memcpy(&v, &vb, 4);
    if (!divIeeeInRange(v, v)) wrong++;
  }
  bool f1, f2, f3;
  const float r = rcpIeee(3.0f, f1), q = divIeee(1.0f, 3.0f, f2), z = rcpIeee(0.0f, f3);
  if (!f1 || !f2 || f3 != false || !(z > 3.0e38f)) wrong++;
  std::printf("{\"set\": \"host\", \"wrong\": %d, \"rcp3\": %.9g, \"div13\": %.9g, \"fast_build\": %d}\n", wrong, r, q, (int)HPT_EXACT_DIV_FAST);
  return wrong == 0 ? 0 : 1;
}

int main(int argc, char** argv)
{
  if (argc > 1 && std::strcmp(argv[1], "--host") == 0) return hostCheck();
  Result* dres = nullptr;
  CHECK(hipMalloc(&dres, sizeof(Result)));
  int rc = runSet<SET_RCP_ALL>("rcp_all", 1ull << 32, 0u, dres);
  if (rc == 0) rc = runSet<SET_DIV_EDGES>("div_edges", 1ull << 22, 0u, dres);
  if (rc == 0) rc = runSet<SET_DIV_RANDOM>("div_random", 1ull << 28, 0x1234567u, dres);
  if (rc == 0) rc = runSet<SET_DIV_INRANGE>("div_inrange", 1ull << 28, 0x89ABCDEu, dres);
  (void)hipFree(dres);
  return rc;
}
