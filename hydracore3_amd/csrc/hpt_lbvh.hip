// CommitScene on the device (CrossRT.h:109 CommitScene, :85-86 UpdateGeom_Triangles3f, :134 UpdateInstance; Embree backend: EmbreeRT.cpp:294-307):
// the single-level tree of hpt_host.hip's flat layout - ONE BVH2 over all instanced triangles, world-space boxes, object-space triangle
// records - and its 4-wide compressed form, built by kernels instead of the host's binned-SAH builder. For scenes whose topology changes
// from frame to frame a quarter of a second of host build against a 0.44 s frame (1 M triangles) is the bottleneck; this build takes a few
// milliseconds. It is a linear BVH: triangles sorted along a 63-bit Morton curve of their world-space centroids (hipCUB radix sort), the
// hierarchy of Karras (HPG 2012: every inner node finds its key range and split from the sorted codes, no dependencies between nodes), boxes
// fitted bottom-up by the second thread to arrive at each node, subtrees of <= BVH_LEAF_MAX triangles folded into leaves, then the same
// collapse to 4-wide nodes the host does (a node adopts its grandchildren, largest surface first) level by level, quantised by the shared
// quantizeNode4. Tree quality is below the SAH build's (hpt_set_option("device_build", ..) / CommitScene's BUILD_LOW | BUILD_MEDIUM choose it,
// BUILD_HIGH keeps the host's SAH tree). Hits do not depend on the tree: the closest hit is min t with ties broken by (instId, primId) and
// triangles are tested in object space by the shared triangleTest, so frames, generators and ray queries are bit-identical to the host-built
// tree's (tests/test_gpu_parity.py::test_device_built_tree_*).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hpt_lbvh.h"
#include "treelet_opt.h"

namespace hpt {

namespace {

struct Scratch
{
  // per instanced triangle (unsorted): world box, Morton key, index; sorted copies
  float* triBox = nullptr;                // [6][n]: lo.xyz, hi.xyz (unpadded), SoA
  unsigned long long *keysIn = nullptr, *keysOut = nullptr;
  uint *valsIn = nullptr, *valsOut = nullptr;
  void* sortTemp = nullptr; size_t sortTempBytes = 0;
  // hierarchy: inner node i in [0, n - 1)
  uint *childL = nullptr, *childR = nullptr, *parent = nullptr, *leafParent = nullptr, *first = nullptr, *last = nullptr, *flags = nullptr, *depth = nullptr;
  uint* height = nullptr;                 // per inner node: its height in the EMITTED tree (0 = both children are leaves), see lbvhFitKernel
  unsigned char* folded = nullptr;        // per inner node: 1 = the emitter folds its subtree into one leaf; decided once, on the Karras tree (lbvhHierarchyKernel)
  uint* passIds = nullptr;                // treelet passes only: the emitted nodes grouped by height (allocated with the first pass)
  float* nodeBox = nullptr;               // [6][n - 1]
  uint2 *frontA = nullptr, *frontB = nullptr;
  uint* counters = nullptr;               // see LbvhCounters
  // inputs mirrored on the device
  float* geomPos = nullptr; uint* geomIdx = nullptr; size_t geomPosCap = 0, geomIdxCap = 0;
  float* instMat = nullptr; uint4* instInfo = nullptr; size_t instCap = 0;
  unsigned char* instDirty = nullptr; size_t instDirtyCap = 0;   // lbvhUpdatePositions: 1 = the instance's mesh moved
  uint ni = 0, n = 0;                     // what the last build was over (valsOut, instInfo and the geometry stay as it left them)
  size_t cap = 0;
  // the two-level layout (section 9): per mesh its slot and the batch's results, per dirty mesh its place in the batch, per instance its mesh, the TLAS stage's result words
  LbvhMeshSlot* meshSlot = nullptr; LbvhMeshOut* meshOut = nullptr; size_t meshCap = 0;
  uint2* batch = nullptr; size_t batchCap = 0;
  uint* instGeom = nullptr; size_t instGeomCap = 0;
  void* tlasResult = nullptr;
  void freeAll()
  {
    void* ps[] = { triBox, keysIn, keysOut, valsIn, valsOut, sortTemp, childL, childR, parent, leafParent, first, last, flags, depth, height, folded, passIds, nodeBox, frontA, frontB, counters, geomPos, geomIdx, instMat, instInfo, instDirty, meshSlot, meshOut, batch, instGeom, tlasResult };
    for (void* p : ps) if (p) (void)hipFree(p);
    *this = Scratch();
  }
};

// device-side result words
struct LbvhCounters
{
  uint sceneLo[3], sceneHi[3]; uint count4; uint frontCount[2]; uint depth4; float sahSum; uint pad;
  uint levelCount[LBVH_MAX_LEVELS], levelFill[LBVH_MAX_LEVELS];       // emitted nodes per height; where the next node of that height goes in the level lists
  uint treelet[2 * 64];                                               // treelet passes: {examined, rewritten}, spread over 64 slots to keep the atomics apart
};

__device__ inline void padBox(float lo[3], float hi[3])      // Aabb::pad (bvh_build.h): the same formula as the host build's
{
  const float ex = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
  float mag = 0.0f;
  for (int a = 0; a < 3; a++) mag = fmaxf(mag, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
  const float p = 1e-5f * fmaxf(ex, mag) + 1e-30f;
  for (int a = 0; a < 3; a++) { lo[a] -= p; hi[a] += p; }
}

// ---- 1. instanced triangles: world box + scene bounds ---------------------------------------------------------------------------------------
// instInfo[i] = {first instanced triangle of instance i, its triangle count, offset of its mesh's positions (floats), offset of its mesh's indices}
__device__ inline uint findInstance(const uint4* info, uint ni, uint k)
{
  uint lo = 0, hi = ni;                       // last i with info[i].x <= k
  while (hi - lo > 1u) { const uint mid = (lo + hi) >> 1; if (info[mid].x <= k) lo = mid; else hi = mid; }
  return lo;
}
__global__ void __launch_bounds__(256) lbvhTriBoxKernel(const float* __restrict__ geomPos, const uint* __restrict__ geomIdx, const float* __restrict__ instMat, const uint4* __restrict__ instInfo,
                                                        uint ni, uint n, float* __restrict__ triBox, LbvhCounters* C)
{
  __shared__ uint sLo[3], sHi[3];
  if (threadIdx.x < 3) { sLo[threadIdx.x] = 0xFFFFFFFFu; sHi[threadIdx.x] = 0u; }
  __syncthreads();
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) {
    const uint i = findInstance(instInfo, ni, k);
    const uint4 inf = instInfo[i];
    const uint t = k - inf.x;
    const float* m = instMat + 12 * (size_t)i;                           // object -> world rows (3 x 4)
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (int v = 0; v < 3; v++) {
      const float* p = geomPos + inf.z + 3 * (size_t)geomIdx[inf.w + 3 * (size_t)t + v];
      // (the host build's expression order: m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12])
      const float q[3] = { m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3], m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7], m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11] };
      for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], q[a]); hi[a] = fmaxf(hi[a], q[a]); }
    }
    for (int a = 0; a < 3; a++) { triBox[(size_t)a * n + k] = lo[a]; triBox[(size_t)(3 + a) * n + k] = hi[a]; atomicMin(&sLo[a], floatKey(lo[a])); atomicMax(&sHi[a], floatKey(hi[a])); }
  }
  __syncthreads();
  if (threadIdx.x < 3) { atomicMin(&C->sceneLo[threadIdx.x], sLo[threadIdx.x]); atomicMax(&C->sceneHi[threadIdx.x], sHi[threadIdx.x]); }
}

// ---- 2. Morton keys of the centroids -----------------------------------------------------------------------------------------------------------
__device__ inline unsigned long long expand21(unsigned long long v)   // bit k of v -> bit 3k
{
  v &= 0x1FFFFFull;
  v = (v | (v << 32)) & 0x1F00000000FFFFull;
  v = (v | (v << 16)) & 0x1F0000FF0000FFull;
  v = (v | (v << 8))  & 0x100F00F00F00F00Full;
  v = (v | (v << 4))  & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2))  & 0x1249249249249249ull;
  return v;
}
// the 63-bit code of box k's centre within the bounds (loKey, hiKey: floatKey words)
__device__ inline unsigned long long mortonOfBox(const float* __restrict__ triBox, size_t n, uint k, const uint* loKey, const uint* hiKey)
{
  unsigned long long key = 0ull;
  // one scale for the three axes (the scene's longest extent): the Morton cells are cubes whatever the scene's proportions, so a split never
  // halves an axis that is already the shortest of its cell (a 10 x 4 x 10 room normalised per axis splits y as often as x and z)
  float ext = 0.0f;
  for (int a = 0; a < 3; a++) ext = fmaxf(ext, keyFloat(hiKey[a]) - keyFloat(loKey[a]));
  for (int a = 0; a < 3; a++) {
    const float lo = keyFloat(loKey[a]);
    const float c = 0.5f * (triBox[(size_t)a * n + k] + triBox[(size_t)(3 + a) * n + k]);
    float u = ext > 0.0f ? (c - lo) / ext : 0.0f;
    u = fminf(fmaxf(u, 0.0f), 1.0f);
    const unsigned long long q = (unsigned long long)fminf(u * 2097152.0f, 2097151.0f);
    key |= expand21(q) << (2 - a);
  }
  return key;
}
__global__ void __launch_bounds__(256) lbvhMortonKernel(const float* __restrict__ triBox, uint n, const LbvhCounters* C, unsigned long long* keys, uint* vals)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  keys[k] = mortonOfBox(triBox, n, k, C->sceneLo, C->sceneHi); vals[k] = k;
}

// ---- 3. hierarchy (Karras 2012) ---------------------------------------------------------------------------------------------------------------------
__device__ inline int delta(const unsigned long long* keys, int n, int i, int j)
{
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = keys[i], b = keys[j];
  if (a != b) return __clzll((long long)(a ^ b));
  return 64 + __clz(i ^ j);                                             // equal keys: the index decides, so every pair differs
}
__global__ void __launch_bounds__(256) lbvhHierarchyKernel(const unsigned long long* __restrict__ keys, int n, uint* childL, uint* childR, uint* parent, uint* leafParent, uint* first, uint* last, unsigned char* folded)
{
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= n - 1) return;
  const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1) if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0;
  for (int t = (l + 1) >> 1; ; t = (t + 1) >> 1) { if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t; if (t == 1) break; }
  const int gamma = i + s * d + (d < 0 ? -1 : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const bool leafL = lo == gamma, leafR = hi == gamma + 1;
  childL[i] = leafL ? (0x80000000u | (uint)gamma) : (uint)gamma;
  childR[i] = leafR ? (0x80000000u | (uint)(gamma + 1)) : (uint)(gamma + 1);
  if (leafL) leafParent[gamma] = (uint)i; else parent[gamma] = (uint)i;
  if (leafR) leafParent[gamma + 1] = (uint)i; else parent[gamma + 1] = (uint)i;
  first[i] = (uint)lo; last[i] = (uint)hi;
  folded[i] = (uint)(hi - lo) + 1u <= (uint)BVH_LEAF_MAX ? 1 : 0;      // a contiguous record range: true of the Karras tree only, so it is decided here for good
  if (i == 0) parent[0] = 0xFFFFFFFFu;
}

// ---- 4. boxes bottom-up: the second thread to arrive at a node fits it ---------------------------------------------------------------------------
// (boxStride: the row length of triBox - n, but for the TLAS of section 9, whose boxes are indexed by instance)
__global__ void __launch_bounds__(256) lbvhFitKernel(const float* __restrict__ triBox, size_t boxStride, const uint* __restrict__ vals, uint n, const uint* __restrict__ childL, const uint* __restrict__ childR,
                                                     const uint* __restrict__ parent, const uint* __restrict__ leafParent, const unsigned char* __restrict__ folded,
                                                     uint* flags, float* nodeBox, uint* depth, uint* height)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n || n < 2u) return;
  const size_t m = n - 1;
  uint node = leafParent[k];
  while (node != 0xFFFFFFFFu) {
    __threadfence();
    if (atomicAdd(&flags[node], 1u) == 0u) return;                       // the first arrival leaves; its sibling's subtree is not ready yet
    __threadfence();
    float lo[3], hi[3]; uint dep = 0, hgt = 0;                           // hgt: the height among the nodes lbvhEmitKernel emits (a child folded into a leaf counts as a leaf)
    const uint cs[2] = { childL[node], childR[node] };
    for (int a = 0; a < 3; a++) { lo[a] = 3.0e38f; hi[a] = -3.0e38f; }
    for (int c = 0; c < 2; c++) {
      const uint ch = cs[c];
      if (ch & 0x80000000u) {
        const uint t = vals[ch & 0x7FFFFFFFu];
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], triBox[(size_t)a * boxStride + t]); hi[a] = fmaxf(hi[a], triBox[(size_t)(3 + a) * boxStride + t]); }
      } else {
        for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], __hip_atomic_load(&nodeBox[(size_t)a * m + ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); hi[a] = fmaxf(hi[a], __hip_atomic_load(&nodeBox[(size_t)(3 + a) * m + ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
        dep = max(dep, __hip_atomic_load(&depth[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (!folded[ch]) hgt = max(hgt, __hip_atomic_load(&height[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u);
      }
    }
    for (int a = 0; a < 3; a++) { __hip_atomic_store(&nodeBox[(size_t)a * m + node], lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(&nodeBox[(size_t)(3 + a) * m + node], hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __hip_atomic_store(&depth[node], dep + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&height[node], hgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    node = parent[node];
  }
}

// ---- 4b. treelet restructuring (Karras & Aila 2013; hpt_set_option("device_build_quality", passes)) ---------------------------------------------------
// One wave = one treelet: the node `root` and up to 7 treelet leaves, grown from the root's two children by expanding, again and again, the leaf
// with the largest half-area that may be expanded (an inner node the emitter does not fold; ties: the lowest leaf slot). The optimal topology over
// the leaves is found by the subset recurrence of treelet_opt.h - the 128 subsets lie two per lane, areas, costs and partitions in LDS, one
// barrier per subset size - and the treelet's inner nodes are rewritten in place (the root keeps its slot, box and parent) only when the optimum
// is strictly below the present topology's cost, summed by the same formula. Boxes are unpadded unions of the leaf boxes: the same floats whatever
// the order, so the pass moves no box of a node it keeps.
// Schedule: one launch per height of the emitted tree as it was BEFORE the pass, ascending (lbvhBuild). Nodes of equal height are never nested and
// a rewrite keeps the set of nodes below its root, so the waves of a launch touch disjoint nodes; kernel boundaries order the launches. No wave
// waits for another.
__device__ inline void treeletLoadLeaf(uint ref, uint n, const unsigned char* folded, const float* triBox, const uint* vals, const float* nodeBox, float box[6], float& area, bool& expandable)
{
  if (ref & 0x80000000u) { const uint t = vals[ref & 0x7FFFFFFFu]; for (int a = 0; a < 6; a++) box[a] = triBox[(size_t)a * n + t]; expandable = false; }
  else { for (int a = 0; a < 6; a++) box[a] = nodeBox[(size_t)a * (n - 1u) + ref]; expandable = !folded[ref]; }
  area = treeletHalfArea(box, box + 3);
}
__global__ void __launch_bounds__(64) lbvhTreeletKernel(const uint* __restrict__ ids, uint count, uint n, uint* childL, uint* childR, uint* parent, uint* leafParent,
                                                        const unsigned char* __restrict__ folded, const float* __restrict__ triBox, const uint* __restrict__ vals, float* nodeBox, LbvhCounters* C)
{
  __shared__ float sLeafBox[TREELET_LEAVES][6];
  __shared__ uint sLeafRef[TREELET_LEAVES], sSlot[TREELET_LEAVES - 1], sSlotMask[TREELET_LEAVES - 1], sSlotLeft[TREELET_LEAVES - 1], sStack[TREELET_LEAVES];
  __shared__ float sArea[TREELET_SUBSETS], sCost[TREELET_SUBSETS], sNow[TREELET_SUBSETS];
  __shared__ unsigned char sPart[TREELET_SUBSETS];
  if (blockIdx.x >= count) return;
  const int lane = (int)threadIdx.x;
  const uint root = ids[blockIdx.x];
  if (root + 1u >= n) return;
  // -- the treelet: leaf j lives in lane j (reference, box, half-area), inner slot e in lane e (the leaves below it, and below its left child)
  uint myRef = 0u; float myBox[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }, myArea = 0.0f; bool myExp = false;
  uint slotMask = lane == 0 ? 3u : 0u, slotLeft = lane == 0 ? 1u : 0u;
  if (lane < 2) { myRef = lane == 0 ? childL[root] : childR[root]; treeletLoadLeaf(myRef, n, folded, triBox, vals, nodeBox, myBox, myArea, myExp); }
  if (lane == 0) sSlot[0] = root;
  int k = 2;
  while (k < TREELET_LEAVES) {
    float a = (lane < k && myExp) ? myArea : -1.0f; int who = lane & 7;
    for (int o = 4; o > 0; o >>= 1) {                                    // the largest half-area among lanes 0..7, ties to the lowest lane
      const float oa = __shfl_xor(a, o); const int ow = __shfl_xor(who, o);
      if (oa > a || (oa == a && ow < who)) { a = oa; who = ow; }
    }
    a = __shfl(a, 0); who = __shfl(who, 0);
    if (a < 0.0f) break;                                                 // nothing left to expand
    const uint node = __shfl(myRef, who);
    if (lane == 0) sSlot[k - 1] = node;
    if (lane < k - 1 && ((slotMask >> who) & 1u)) { slotMask |= 1u << k; if ((slotLeft >> who) & 1u) slotLeft |= 1u << k; }
    if (lane == k - 1) { slotMask = (1u << who) | (1u << k); slotLeft = 1u << who; }
    if (lane == who || lane == k) { myRef = lane == who ? childL[node] : childR[node]; treeletLoadLeaf(myRef, n, folded, triBox, vals, nodeBox, myBox, myArea, myExp); }
    k++;
  }
  if (k < 3) return;                                                     // two leaves have one topology
  if (lane < k) { sLeafRef[lane] = myRef; for (int a = 0; a < 6; a++) sLeafBox[lane][a] = myBox[a]; }
  if (lane < k - 1) { sSlotMask[lane] = slotMask; sSlotLeft[lane] = slotLeft; }
  for (int j = k + lane; j < TREELET_LEAVES; j += 64) for (int a = 0; a < 6; a++) sLeafBox[j][a] = 0.0f;   // (never selected: the subsets stay below 1 << k)
  __syncthreads();
  // -- the recurrence of treelet_opt.h, subsets lane and lane + 64
  const uint full = (1u << k) - 1u;
  for (uint s = (uint)lane; s < (uint)TREELET_SUBSETS; s += 64u) {
    float lo[3], hi[3];
    const float ar = (s != 0u && s <= full) ? treeletUnion(s, sLeafBox, lo, hi) : 0.0f;
    sArea[s] = ar; sCost[s] = 0.0f; sNow[s] = 0.0f; sPart[s] = 0;
  }
  __syncthreads();
  for (int size = 2; size <= k; size++) {
    for (uint s = (uint)lane; s < (uint)TREELET_SUBSETS; s += 64u) if (s <= full && __popc(s) == size) {
      uint p; const float c = treeletBestSplit(s, sCost, p);
      sCost[s] = sArea[s] + c; sPart[s] = (unsigned char)p;
    }
    __syncthreads();
  }
  // -- the present topology's cost by the same formula (children of a slot have greater slot numbers), then the rewrite; one lane
  if (lane == 0) {
    for (int e = k - 2; e >= 0; e--) { const uint s = sSlotMask[e], l = sSlotLeft[e]; sNow[s] = sArea[s] + (sNow[l] + sNow[s ^ l]); }
    const bool better = sCost[full] < sNow[full];
    atomicAdd(&C->treelet[2u * (blockIdx.x & 63u)], 1u);
    if (better) {
      atomicAdd(&C->treelet[2u * (blockIdx.x & 63u) + 1u], 1u);
      const size_t m = n - 1u;
      int next = 1, sp = 1;
      sStack[0] = full;                                                  // entries: inner slot << 8 | leaf set
      while (sp > 0) {
        const uint it = sStack[--sp], s = it & 0xFFu, node = sSlot[it >> 8];
        const uint p = sPart[s];
        for (int c = 0; c < 2; c++) {
          const uint cs = c == 0 ? p : (s ^ p);
          uint child;
          if ((cs & (cs - 1u)) == 0u) {                                  // one leaf
            child = sLeafRef[__ffs((int)cs) - 1];
            if (child & 0x80000000u) leafParent[child & 0x7FFFFFFFu] = node; else parent[child] = node;
          } else {
            const int e = next++;
            child = sSlot[e];
            parent[child] = node;
            float lo[3], hi[3]; treeletUnion(cs, sLeafBox, lo, hi);
            for (int a = 0; a < 3; a++) { nodeBox[(size_t)a * m + child] = lo[a]; nodeBox[(size_t)(3 + a) * m + child] = hi[a]; }
            sStack[sp++] = ((uint)e << 8) | cs;
          }
          if (c == 0) childL[node] = child; else childR[node] = child;
        }
      }
    }
  }
}

// ---- 5. BvhNode records (both child boxes in the parent, hpt_types.h), leaves of <= BVH_LEAF_MAX triangles; triangle records in leaf order ----
__device__ inline uint childRef(uint ch, const uint* first, const uint* last, const unsigned char* folded, uint& leafFirst, uint& leafCount)
{
  if (ch & 0x80000000u) { leafFirst = ch & 0x7FFFFFFFu; leafCount = 1u; return REF_LEAF | (1u << 28) | leafFirst; }
  if (folded[ch]) { const uint cnt = last[ch] - first[ch] + 1u; leafFirst = first[ch]; leafCount = cnt; return REF_LEAF | (cnt << 28) | leafFirst; }   // (a folded subtree is never restructured: its range stays)
  leafCount = 0u; return ch;
}
__global__ void __launch_bounds__(256) lbvhEmitKernel(uint n, const uint* __restrict__ childL, const uint* __restrict__ childR, const uint* __restrict__ first, const uint* __restrict__ last, const unsigned char* __restrict__ folded,
                                                      const float* __restrict__ triBox, const uint* __restrict__ vals, const float* __restrict__ nodeBox, BvhNode* nodes, LbvhCounters* C)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  float sah = 0.0f;
  if (i + 1u < n && !folded[i]) {
    const size_t m = n - 1;
    BvhNode nd;
    const uint cs[2] = { childL[i], childR[i] };
    for (int c = 0; c < 2; c++) {
      uint lf, lc; const uint ref = childRef(cs[c], first, last, folded, lf, lc);
      float lo[3], hi[3];
      if (cs[c] & 0x80000000u) { const uint t = vals[cs[c] & 0x7FFFFFFFu]; for (int a = 0; a < 3; a++) { lo[a] = triBox[(size_t)a * n + t]; hi[a] = triBox[(size_t)(3 + a) * n + t]; } }
      else for (int a = 0; a < 3; a++) { lo[a] = nodeBox[(size_t)a * m + cs[c]]; hi[a] = nodeBox[(size_t)(3 + a) * m + cs[c]]; }
      padBox(lo, hi);
      for (int a = 0; a < 3; a++) { nd.q[6 * c + 2 * a] = lo[a]; nd.q[6 * c + 2 * a + 1] = hi[a]; }
      if (c == 0) nd.ref0 = ref; else nd.ref1 = ref;
      if ((ref & REF_LEAF) == 0u) { const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2]; sah += dx * dy + dy * dz + dz * dx; }
    }
    nd.pad0 = nd.pad1 = 0u;
    nodes[i] = nd;
  }
  // sum of the inner children's half-areas (sah_node_visits' numerator): wave-reduced, one atomic per wave
  for (int o = 32; o > 0; o >>= 1) sah += __shfl_down(sah, o);
  if ((threadIdx.x & 63u) == 0u && sah != 0.0f) atomicAdd(&C->sahSum, sah);
}
__global__ void __launch_bounds__(256) lbvhGatherTrisKernel(const float* __restrict__ geomPos, const uint* __restrict__ geomIdx, const uint4* __restrict__ instInfo, uint ni, uint n,
                                                            const uint* __restrict__ vals, BvhTri* tris)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint src = vals[k];
  const uint i = findInstance(instInfo, ni, src);
  const uint4 inf = instInfo[i];
  const uint p = src - inf.x;
  const uint* ix = geomIdx + inf.w + 3 * (size_t)p;
  const float* A = geomPos + inf.z + 3 * (size_t)ix[0]; const float* B = geomPos + inf.z + 3 * (size_t)ix[1]; const float* Cc = geomPos + inf.z + 3 * (size_t)ix[2];
  BvhTri t;
  for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = Cc[a] - A[a]; }   // the same object-space record as the host build's
  t.primId = p; t.instId = i; t.pad1 = 0u;
  tris[k] = t;
}

// ---- 6. collapse to 4-wide compressed nodes, one level per launch (collapseToWide of bvh_build.h as a frontier kernel) -------------------------------
__global__ void __launch_bounds__(256) lbvhCollapseKernel(const BvhNode* __restrict__ nodes, const uint2* __restrict__ frontIn, uint2* frontOut, uint level, BvhNode4* nodes4, uint cap4, uint* src4, LbvhCounters* C)
{
  const uint e = blockIdx.x * 256u + threadIdx.x;
  const uint cnt = C->frontCount[level & 1u];
  if (e == 0u && cnt != 0u) C->depth4 = level + 1u;
  if (e >= cnt) return;
  const uint2 it = frontIn[e];                                           // {BVH2 node, index of the wide node to fill}
  uint kids[4]; int nk = 2;                                              // each kid = (BVH2 node << 1 | side)
  kids[0] = it.x << 1; kids[1] = (it.x << 1) | 1u;
  auto refOf = [&](uint k) { const BvhNode& nd = nodes[k >> 1]; return (k & 1u) ? nd.ref1 : nd.ref0; };
  auto area = [&](uint k) { const float* q = nodes[k >> 1].q + 6 * (k & 1u); const float dx = q[1] - q[0], dy = q[3] - q[2], dz = q[5] - q[4]; return dx * dy + dy * dz + dz * dx; };
  while (nk < 4) {
    int best = -1; float bestA = -1.0f;
    for (int k = 0; k < nk; k++) { const uint r = refOf(kids[k]); if (r != REF_NONE && !(r & REF_LEAF)) { const float a = area(kids[k]); if (a > bestA) { bestA = a; best = k; } } }
    if (best < 0) break;
    const uint inner = refOf(kids[best]);
    kids[best] = inner << 1; kids[nk++] = (inner << 1) | 1u;
  }
  float lo[4][3], hi[4][3]; uint valid = 0u, refs[4] = { REF_NONE, REF_NONE, REF_NONE, REF_NONE };
  uint nInner = 0u;
  for (int k = 0; k < nk; k++) {
    const uint r = refOf(kids[k]);
    if (r == REF_NONE) continue;
    const float* q = nodes[kids[k] >> 1].q + 6 * (kids[k] & 1u);
    for (int a = 0; a < 3; a++) { lo[k][a] = q[2 * a]; hi[k][a] = q[2 * a + 1]; }
    valid |= 1u << k;
    refs[k] = r;
    if (!(r & REF_LEAF)) nInner++;
  }
  if (nInner) {
    const uint base4 = atomicAdd(&C->count4, nInner);
    const uint baseF = atomicAdd(&C->frontCount[(level + 1u) & 1u], nInner);
    uint j = 0;
    for (int k = 0; k < nk; k++) if (refs[k] != REF_NONE && !(refs[k] & REF_LEAF)) {
      if (base4 + j < cap4) frontOut[baseF + j] = make_uint2(refs[k], base4 + j);
      refs[k] = base4 + j; j++;
    }
  }
  BvhNode4 nd;
  nd.pad[0] = nd.pad[1] = 0u;
  quantizeNode4(lo, hi, valid, nd);
  for (int k = 0; k < 4; k++) nd.ref[k] = refs[k];
  if (it.y < cap4) {
    nodes4[it.y] = nd;
    if (src4) for (int k = 0; k < 4; k++) src4[4u * (size_t)it.y + k] = k < nk ? kids[k] : 0u;     // where child k's box lives: what refitNodes4Kernel requantises from
  }
}
__global__ void lbvhResetFrontKernel(LbvhCounters* C, uint level) { C->frontCount[level & 1u] = 0u; }

// ---- 7. what a refit needs: the emitted nodes grouped by height (a node reads only children of smaller height) ------------------------------------
// Histogram over the heights, a scan over its <= 64 bins, a scatter. Level l of the lists holds the nodes of height (root's height - l): level 0 is
// the root alone and the refit walks the levels from the last to the first, as it does for a host-built tree. The order inside a level is whatever
// the atomics make it. Heights are clamped to the bins: a tree that deep is given back to the host's builder (hpt_host.hip) and its lists are not used.
__device__ inline bool emittedHeight(uint i, uint n, const unsigned char* folded, const uint* height, uint& h)
{
  if (i + 1u >= n || folded[i]) return false;
  h = min(height[i], LBVH_MAX_LEVELS - 1u);
  return true;
}
__global__ void __launch_bounds__(256) lbvhLevelHistKernel(uint n, const unsigned char* __restrict__ folded, const uint* __restrict__ height, LbvhCounters* C)
{
  __shared__ uint cnt[LBVH_MAX_LEVELS];
  if (threadIdx.x < LBVH_MAX_LEVELS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  uint h;
  if (emittedHeight(blockIdx.x * 256u + threadIdx.x, n, folded, height, h)) atomicAdd(&cnt[h], 1u);
  __syncthreads();
  if (threadIdx.x < LBVH_MAX_LEVELS && cnt[threadIdx.x]) atomicAdd(&C->levelCount[threadIdx.x], cnt[threadIdx.x]);
}
__global__ void __launch_bounds__(64) lbvhLevelScanKernel(const uint* __restrict__ height, LbvhCounters* C)       // one wave: lane = height
{
  const uint h = threadIdx.x, top = min(height[0], LBVH_MAX_LEVELS - 1u);
  uint before = 0u;                                                     // nodes of the levels in front of this height's: the greater heights
  for (uint g = h + 1u; g <= top; g++) before += C->levelCount[g];
  C->levelFill[h] = before;
}
__global__ void __launch_bounds__(256) lbvhLevelScatterKernel(uint n, const unsigned char* __restrict__ folded, const uint* __restrict__ height, LbvhCounters* C, uint* levelIds)
{
  __shared__ uint cnt[LBVH_MAX_LEVELS], base[LBVH_MAX_LEVELS];
  if (threadIdx.x < LBVH_MAX_LEVELS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const uint i = blockIdx.x * 256u + threadIdx.x;
  uint h = 0u, rank = 0u;
  const bool emitted = emittedHeight(i, n, folded, height, h);
  if (emitted) rank = atomicAdd(&cnt[h], 1u);
  __syncthreads();
  if (threadIdx.x < LBVH_MAX_LEVELS && cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&C->levelFill[threadIdx.x], cnt[threadIdx.x]);
  __syncthreads();
  if (emitted && base[h] + rank < n - 1u) levelIds[base[h] + rank] = i;  // (fewer than n - 1 nodes are emitted: the lists fit in n - 1 entries)
}

// ---- 8. moved vertices: the records of the flagged instances again, from the meshes' current positions ---------------------------------------------
// One lane per record. The record names its instance and primitive, so the sorted order need not be consulted; the expressions are
// lbvhGatherTrisKernel's, so the records equal a fresh build's bit for bit.
__global__ void __launch_bounds__(256) lbvhRegatherTrisKernel(const float* __restrict__ geomPos, const uint* __restrict__ geomIdx, const uint4* __restrict__ instInfo, const unsigned char* __restrict__ instDirty,
                                                              uint ni, uint n, BvhTri* tris)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint i = tris[k].instId, p = tris[k].primId;
  if (i >= ni || !instDirty[i]) return;
  const uint4 inf = instInfo[i];
  if (p >= inf.y) return;
  const uint* ix = geomIdx + inf.w + 3 * (size_t)p;
  const float* A = geomPos + inf.z + 3 * (size_t)ix[0]; const float* B = geomPos + inf.z + 3 * (size_t)ix[1]; const float* Cc = geomPos + inf.z + 3 * (size_t)ix[2];
  BvhTri t;
  for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = Cc[a] - A[a]; }
  t.primId = p; t.instId = i; t.pad1 = 0u;
  tris[k] = t;
}

// ---- 9. the two-level layout: the BLAS of all dirty meshes in one batch, then the TLAS (interface and key layout: hpt_lbvh.h) -------------------------
// Batch: the dirty meshes' triangles back to back, slot d of the batch = batch[d] {first triangle, mesh}. Sections 3 and 4 run over the whole batch
// unchanged; tlCutKernel, between them, takes every mesh's subtree off the nodes that span several meshes, so the fit stops at the mesh roots.
struct TlasResult { uint lo[3], hi[3]; float a0; uint depth; double sahSum, instSum; };   // bounds of the instance boxes' centres' domain (floatKey), TLAS root half-area and depth, the two sums of the estimate

__device__ inline uint findSlot(const uint2* batch, uint D, uint k)
{
  uint lo = 0, hi = D;                        // last d with batch[d].x <= k
  while (hi - lo > 1u) { const uint mid = (lo + hi) >> 1; if (batch[mid].x <= k) lo = mid; else hi = mid; }
  return lo;
}
__device__ inline float halfAreaOf(const float lo[3], const float hi[3])      // Aabb::halfArea (bvh_build.h)
{
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  return dx < 0.0f ? 0.0f : dx * dy + dy * dz + dz * dx;
}
// object-space triangle boxes; per-mesh bounds by integer-keyed atomics, block-reduced for the mesh the block's first triangle belongs to
__global__ void __launch_bounds__(256) tlTriBoxKernel(const float* __restrict__ geomPos, const uint* __restrict__ geomIdx, const LbvhMeshSlot* __restrict__ slots, const uint2* __restrict__ batch,
                                                      uint D, uint n, float* __restrict__ triBox, LbvhMeshOut* mesh)
{
  __shared__ uint sLo[3], sHi[3], sGeom;
  if (threadIdx.x < 3) { sLo[threadIdx.x] = 0xFFFFFFFFu; sHi[threadIdx.x] = 0u; }
  if (threadIdx.x == 0) sGeom = batch[findSlot(batch, D, min(blockIdx.x * 256u, n - 1u))].y;
  __syncthreads();
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) {
    const uint2 b = batch[findSlot(batch, D, k)];
    const LbvhMeshSlot sl = slots[b.y];
    const uint t = k - b.x;
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (int v = 0; v < 3; v++) {
      const float* p = geomPos + sl.posOff + 3 * (size_t)geomIdx[sl.idxOff + 3 * (size_t)t + v];
      for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], p[a]); hi[a] = fmaxf(hi[a], p[a]); }
    }
    const bool inBlockMesh = b.y == sGeom;
    for (int a = 0; a < 3; a++) {
      triBox[(size_t)a * n + k] = lo[a]; triBox[(size_t)(3 + a) * n + k] = hi[a];
      if (inBlockMesh) { atomicMin(&sLo[a], floatKey(lo[a])); atomicMax(&sHi[a], floatKey(hi[a])); }
      else { atomicMin(&mesh[b.y].lo[a], floatKey(lo[a])); atomicMax(&mesh[b.y].hi[a], floatKey(hi[a])); }
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && sLo[threadIdx.x] <= sHi[threadIdx.x]) { atomicMin(&mesh[sGeom].lo[threadIdx.x], sLo[threadIdx.x]); atomicMax(&mesh[sGeom].hi[threadIdx.x], sHi[threadIdx.x]); }
}
__global__ void __launch_bounds__(256) tlMortonKernel(const float* __restrict__ triBox, const uint2* __restrict__ batch, uint D, uint n, const LbvhMeshOut* __restrict__ mesh, uint slotBits,
                                                      unsigned long long* keys, uint* vals)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint d = findSlot(batch, D, k);
  const LbvhMeshOut* m = mesh + batch[d].y;
  keys[k] = lbvhPackKey(d, slotBits, mortonOfBox(triBox, n, k, m->lo, m->hi)); vals[k] = k;
}
// After the hierarchy: a node whose range lies in one mesh and is that mesh's whole range is the mesh's root - it loses its parent; a node that spans
// several meshes lets go of a leaf child (a mesh of one triangle). Such a node's other children are mesh roots, which let go themselves.
__global__ void __launch_bounds__(256) tlCutKernel(const unsigned long long* __restrict__ keys, uint n, uint slotBits, const uint2* __restrict__ batch, const LbvhMeshSlot* __restrict__ slots,
                                                   const uint* __restrict__ childL, const uint* __restrict__ childR, const uint* __restrict__ first, const uint* __restrict__ last,
                                                   uint* parent, uint* leafParent, LbvhMeshOut* mesh)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i + 1u >= n) return;
  const uint a = first[i], b = last[i];
  const uint sa = lbvhKeySlot(keys[a], slotBits), sb = lbvhKeySlot(keys[b], slotBits);
  if (sa != sb) {
    const uint cs[2] = { childL[i], childR[i] };
    for (int c = 0; c < 2; c++) if (cs[c] & 0x80000000u) leafParent[cs[c] & 0x7FFFFFFFu] = 0xFFFFFFFFu;
    return;
  }
  const uint2 bt = batch[sa];
  if (a == bt.x && b == bt.x + slots[bt.y].nt - 1u) { parent[i] = 0xFFFFFFFFu; mesh[bt.y].karrasRoot = i; }
}
// BvhNode records of every mesh into its slot (lbvhEmitKernel's rules); a mesh's nodes are the Karras nodes of its range but one - the end of the
// range its root does not sit on - so node i lies at nodeBase + i - (the first node of the range that is one)
__device__ inline uint tlFirstNode(uint karrasRoot, uint batchFirst) { return karrasRoot == batchFirst ? batchFirst : batchFirst + 1u; }
__global__ void __launch_bounds__(256) tlEmitBlasKernel(const unsigned long long* __restrict__ keys, uint n, uint slotBits, const uint2* __restrict__ batch, const LbvhMeshSlot* __restrict__ slots,
                                                        const uint* __restrict__ childL, const uint* __restrict__ childR, const uint* __restrict__ first, const uint* __restrict__ last,
                                                        const unsigned char* __restrict__ folded, const float* __restrict__ triBox, const uint* __restrict__ vals, const float* __restrict__ nodeBox,
                                                        BvhNode* nodes, LbvhMeshOut* mesh)
{
  const uint i = blockIdx.x * 256u + threadIdx.x;
  double sah = 0.0; uint geom = 0xFFFFFFFFu;
  if (i + 1u < n && !folded[i]) {
    const uint sa = lbvhKeySlot(keys[first[i]], slotBits);
    if (sa == lbvhKeySlot(keys[last[i]], slotBits)) {
      const uint2 bt = batch[sa];
      const LbvhMeshSlot sl = slots[bt.y];
      const uint node0 = tlFirstNode(mesh[bt.y].karrasRoot, bt.x);
      const size_t m = n - 1;
      if (i - node0 + 1u < sl.nt) {                                      // (always: the mesh's nodes are node0 .. node0 + nt - 2; nothing is written outside the slot)
      geom = bt.y;
      BvhNode nd;
      const uint cs[2] = { childL[i], childR[i] };
      for (int c = 0; c < 2; c++) {
        uint lf, lc; uint ref = childRef(cs[c], first, last, folded, lf, lc);
        ref = lc ? (REF_LEAF | (lc << 28) | (sl.triBase + (lf - bt.x))) : (sl.nodeBase + (ref - node0));
        float lo[3], hi[3];
        if (cs[c] & 0x80000000u) { const uint t = vals[cs[c] & 0x7FFFFFFFu]; for (int a = 0; a < 3; a++) { lo[a] = triBox[(size_t)a * n + t]; hi[a] = triBox[(size_t)(3 + a) * n + t]; } }
        else for (int a = 0; a < 3; a++) { lo[a] = nodeBox[(size_t)a * m + cs[c]]; hi[a] = nodeBox[(size_t)(3 + a) * m + cs[c]]; }
        padBox(lo, hi);
        for (int a = 0; a < 3; a++) { nd.q[6 * c + 2 * a] = lo[a]; nd.q[6 * c + 2 * a + 1] = hi[a]; }
        if (c == 0) nd.ref0 = ref; else nd.ref1 = ref;
        if (lc == 0u) { const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2]; sah += (double)(dx * dy + dy * dz + dz * dx); }
      }
      nd.pad0 = nd.pad1 = 0u;
      nodes[sl.nodeBase + (i - node0)] = nd;
      }
    }
  }
  // per mesh: one atomic per wave when the wave's nodes belong to one mesh (large meshes), else one per lane
  const unsigned long long has = __ballot(geom != 0xFFFFFFFFu);
  if (has == 0ull) return;
  const uint g0 = __shfl(geom, __ffsll((long long)has) - 1);
  if (__all(geom == 0xFFFFFFFFu || geom == g0)) {
    for (int o = 32; o > 0; o >>= 1) sah += __shfl_down(sah, o);
    if ((threadIdx.x & 63u) == 0u && sah != 0.0) atomicAdd(&mesh[g0].sahSum, sah);
  } else if (geom != 0xFFFFFFFFu && sah != 0.0) atomicAdd(&mesh[geom].sahSum, sah);
}
__global__ void __launch_bounds__(256) tlGatherTrisKernel(const float* __restrict__ geomPos, const uint* __restrict__ geomIdx, const LbvhMeshSlot* __restrict__ slots, const uint2* __restrict__ batch,
                                                          const unsigned long long* __restrict__ keys, uint slotBits, uint n, const uint* __restrict__ vals, BvhTri* tris)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint2 bt = batch[lbvhKeySlot(keys[k], slotBits)];               // (sorted by slot first: position k and the triangle it holds belong to the same mesh)
  const LbvhMeshSlot sl = slots[bt.y];
  const uint p = vals[k] - bt.x;
  const uint* ix = geomIdx + sl.idxOff + 3 * (size_t)p;
  const float* A = geomPos + sl.posOff + 3 * (size_t)ix[0]; const float* B = geomPos + sl.posOff + 3 * (size_t)ix[1]; const float* Cc = geomPos + sl.posOff + 3 * (size_t)ix[2];
  BvhTri t;
  for (int a = 0; a < 3; a++) { t.v0[a] = A[a]; t.e1[a] = B[a] - A[a]; t.e2[a] = Cc[a] - A[a]; }   // the host build's object-space record
  t.primId = p; t.instId = 0u; t.pad1 = 0u;
  tris[sl.triBase + (k - bt.x)] = t;
}
// per dirty mesh: its root as the instances will hold it, and the inner levels of its emitted tree
__global__ void __launch_bounds__(256) tlMeshRootKernel(const uint2* __restrict__ batch, uint D, const LbvhMeshSlot* __restrict__ slots, const uint* __restrict__ height, LbvhMeshOut* mesh)
{
  const uint d = blockIdx.x * 256u + threadIdx.x;
  if (d >= D) return;
  const uint2 bt = batch[d];
  const LbvhMeshSlot sl = slots[bt.y];
  LbvhMeshOut* o = mesh + bt.y;
  if (sl.nt <= (uint)BVH_LEAF_MAX) { o->root = REF_LEAF | (sl.nt << 28) | sl.triBase; o->depth = 0u; return; }
  const uint r = o->karrasRoot;
  if (r - bt.x >= sl.nt) return;                                        // (never: the cut found no root; the mesh stays out of the TLAS)
  o->root = sl.nodeBase + (r - tlFirstNode(r, bt.x)); o->depth = height[r] + 1u;
}
// TLAS: the padded world box of every instance of a non-empty mesh - the eight corners of the BLAS bounds through the object -> world rows at both
// keys, the host build's expressions - and the bounds of those boxes; an instance of an empty mesh gets an inverted box
__global__ void __launch_bounds__(256) tlInstBoxKernel(const uint* __restrict__ instGeom, const float* __restrict__ instMotion, const LbvhMeshOut* __restrict__ mesh, uint ni, float* __restrict__ box, TlasResult* R)
{
  __shared__ uint sLo[3], sHi[3];
  if (threadIdx.x < 3) { sLo[threadIdx.x] = 0xFFFFFFFFu; sHi[threadIdx.x] = 0u; }
  __syncthreads();
  const uint i = blockIdx.x * 256u + threadIdx.x;
  if (i < ni) {
    const LbvhMeshOut mo = mesh[instGeom[i]];
    float lo[3] = { 1.0f, 1.0f, 1.0f }, hi[3] = { -1.0f, -1.0f, -1.0f };
    if (mo.root != REF_NONE) {
      float blo[3], bhi[3];
      for (int a = 0; a < 3; a++) { blo[a] = keyFloat(mo.lo[a]); bhi[a] = keyFloat(mo.hi[a]); lo[a] = 3.402823466e+38f; hi[a] = -3.402823466e+38f; }
      for (int key = 0; key < 2; key++) {
        const float* m = instMotion + 24 * (size_t)i + 12 * key;
        for (int k = 0; k < 8; k++) {
          const float p[3] = { (k & 1) ? bhi[0] : blo[0], (k & 2) ? bhi[1] : blo[1], (k & 4) ? bhi[2] : blo[2] };
          const float q[3] = { m[0] * p[0] + m[1] * p[1] + m[2] * p[2] + m[3], m[4] * p[0] + m[5] * p[1] + m[6] * p[2] + m[7], m[8] * p[0] + m[9] * p[1] + m[10] * p[2] + m[11] };
          for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], q[a]); hi[a] = fmaxf(hi[a], q[a]); }
        }
      }
      padBox(lo, hi);
      for (int a = 0; a < 3; a++) { atomicMin(&sLo[a], floatKey(lo[a])); atomicMax(&sHi[a], floatKey(hi[a])); }
    }
    for (int a = 0; a < 3; a++) { box[(size_t)a * ni + i] = lo[a]; box[(size_t)(3 + a) * ni + i] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 3 && sLo[threadIdx.x] <= sHi[threadIdx.x]) { atomicMin(&R->lo[threadIdx.x], sLo[threadIdx.x]); atomicMax(&R->hi[threadIdx.x], sHi[threadIdx.x]); }
}
// an instance of an empty mesh sorts behind every live one: the hierarchy is built over the first nLive entries of the sorted arrays
__global__ void __launch_bounds__(256) tlInstMortonKernel(const float* __restrict__ box, uint ni, const TlasResult* R, unsigned long long* keys, uint* vals)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  if (k >= ni) return;
  keys[k] = box[k] > box[(size_t)3 * ni + k] ? 0xFFFFFFFFFFFFFFFFull : mortonOfBox(box, ni, k, R->lo, R->hi); vals[k] = k;
}
// TLAS nodes (node = Karras node, the TLAS occupies the front of the node array), leaves of exactly one instance with the instance's own padded
// box; the two sums of the estimate: half-areas of the inner children, and per live instance halfArea(box) / halfArea(root) x its BLAS' visits
__global__ void __launch_bounds__(256) tlEmitTlasKernel(uint nLive, uint ni, const uint* __restrict__ childL, const uint* __restrict__ childR, const float* __restrict__ box, const uint* __restrict__ vals,
                                                        const float* __restrict__ nodeBox, const uint* __restrict__ depth, const uint* __restrict__ instGeom, const LbvhMeshOut* __restrict__ mesh,
                                                        BvhNode* nodes, TlasResult* R)
{
  const uint k = blockIdx.x * 256u + threadIdx.x;
  const size_t m = nLive - 1u;
  double sah = 0.0, inst = 0.0;
  float rlo[3], rhi[3];
  for (int a = 0; a < 3; a++) { rlo[a] = nodeBox[(size_t)a * m]; rhi[a] = nodeBox[(size_t)(3 + a) * m]; }   // (node 0 is the root)
  const float a0 = halfAreaOf(rlo, rhi);
  if (k + 1u < nLive) {
    BvhNode nd;
    const uint cs[2] = { childL[k], childR[k] };
    for (int c = 0; c < 2; c++) {
      float lo[3], hi[3]; uint ref;
      if (cs[c] & 0x80000000u) { const uint t = vals[cs[c] & 0x7FFFFFFFu]; ref = REF_LEAF | t; for (int a = 0; a < 3; a++) { lo[a] = box[(size_t)a * ni + t]; hi[a] = box[(size_t)(3 + a) * ni + t]; } }
      else {
        ref = cs[c];
        for (int a = 0; a < 3; a++) { lo[a] = nodeBox[(size_t)a * m + cs[c]]; hi[a] = nodeBox[(size_t)(3 + a) * m + cs[c]]; }
        padBox(lo, hi);
        sah += (double)halfAreaOf(lo, hi);
      }
      for (int a = 0; a < 3; a++) { nd.q[6 * c + 2 * a] = lo[a]; nd.q[6 * c + 2 * a + 1] = hi[a]; }
      if (c == 0) nd.ref0 = ref; else nd.ref1 = ref;
    }
    nd.pad0 = nd.pad1 = 0u;
    nodes[k] = nd;
  }
  if (k < nLive && a0 > 0.0f) {
    const uint t = vals[k];
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) { lo[a] = box[(size_t)a * ni + t]; hi[a] = box[(size_t)(3 + a) * ni + t]; }
    inst = (double)halfAreaOf(lo, hi) / (double)a0 * (double)lbvhBlasVisits(mesh[instGeom[t]]);
  }
  if (k == 0u) { R->a0 = a0; R->depth = depth[0]; }
  for (int o = 32; o > 0; o >>= 1) { sah += __shfl_down(sah, o); inst += __shfl_down(inst, o); }
  if ((threadIdx.x & 63u) == 0u) { if (sah != 0.0) atomicAdd(&R->sahSum, sah); if (inst != 0.0) atomicAdd(&R->instSum, inst); }
}

template <class T> bool ensure(T*& p, size_t count) { if (p) (void)hipFree(p); p = nullptr; return hipMalloc((void**)&p, count * sizeof(T)) == hipSuccess; }

} // namespace

void* lbvhCreate() { return new Scratch(); }
void lbvhDestroy(void* s) { if (s) { ((Scratch*)s)->freeAll(); delete (Scratch*)s; } }

#define LCHK(call) do { hipError_t _e = (call); if (_e != hipSuccess) { err = std::string(#call) + ": " + hipGetErrorString(_e); return false; } } while (0)

// the per-primitive arrays and the sort's temporary storage, for builds over up to n primitives
static bool growScratch(Scratch& S, size_t n, std::string& err)
{
  if (n <= S.cap) return true;
  const size_t c = n;
  bool ok = ensure(S.triBox, 6 * c) && ensure(S.keysIn, c) && ensure(S.keysOut, c) && ensure(S.valsIn, c) && ensure(S.valsOut, c) && ensure(S.childL, c) && ensure(S.childR, c) &&
            ensure(S.parent, c) && ensure(S.leafParent, c) && ensure(S.first, c) && ensure(S.last, c) && ensure(S.flags, c) && ensure(S.depth, c) && ensure(S.height, c) && ensure(S.folded, c) && ensure(S.nodeBox, 6 * c) &&
            ensure(S.frontA, c) && ensure(S.frontB, c);
  if (!ok) { err = "hipMalloc (build scratch)"; S.cap = 0; return false; }
  S.cap = c;
  if (S.passIds) { (void)hipFree(S.passIds); S.passIds = nullptr; }
  size_t bytes = 0, bytes64 = 0;                                       // (the single-level build sorts 63 bits, section 9 all 64)
  LCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, S.keysIn, S.keysOut, S.valsIn, S.valsOut, (int)n, 0, 63, nullptr));
  LCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes64, S.keysIn, S.keysOut, S.valsIn, S.valsOut, (int)n, 0, 64, nullptr));
  if (bytes64 > bytes) bytes = bytes64;
  if (S.sortTemp) (void)hipFree(S.sortTemp);
  S.sortTemp = nullptr;
  LCHK(hipMalloc(&S.sortTemp, bytes + 16)); S.sortTempBytes = bytes;
  return true;
}

bool lbvhUploadGeometry(void* scratch, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<const uint*>& idx, const std::vector<size_t>& idxCount,
                        std::vector<size_t>& posOffset, std::vector<size_t>& idxOffset, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  size_t np = 0, nx = 0;
  posOffset.resize(pos.size()); idxOffset.resize(idx.size());
  for (size_t g = 0; g < pos.size(); g++) { posOffset[g] = np; idxOffset[g] = nx; np += posFloats[g]; nx += idxCount[g]; }
  if (np > S.geomPosCap) { if (!ensure(S.geomPos, np + 1)) { err = "hipMalloc (mesh positions)"; return false; } S.geomPosCap = np; }
  if (nx > S.geomIdxCap) { if (!ensure(S.geomIdx, nx + 1)) { err = "hipMalloc (mesh indices)"; return false; } S.geomIdxCap = nx; }
  for (size_t g = 0; g < pos.size(); g++) {
    if (posFloats[g]) LCHK(hipMemcpyAsync(S.geomPos + posOffset[g], pos[g], posFloats[g] * sizeof(float), hipMemcpyHostToDevice, nullptr));
    if (idxCount[g]) LCHK(hipMemcpyAsync(S.geomIdx + idxOffset[g], idx[g], idxCount[g] * sizeof(uint), hipMemcpyHostToDevice, nullptr));
  }
  return true;
}

bool lbvhBuild(void* scratch, const LbvhInstance* insts, uint ni, uint n, BvhNode* nodes, BvhTri* tris, BvhNode4* nodes4, uint cap4, bool wantWide, const LbvhRefitOut& refit, uint qualityPasses, LbvhResult& out, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  out = LbvhResult();
  S.ni = 0; S.n = 0;
  if (n == 0u) { out.rootRef = REF_NONE; return true; }
  if (!growScratch(S, n, err)) return false;
  if (!S.counters) LCHK(hipMalloc((void**)&S.counters, sizeof(LbvhCounters)));
  if (ni > S.instCap) { if (!ensure(S.instMat, 12 * (size_t)ni) || !ensure(S.instInfo, (size_t)ni)) { err = "hipMalloc (instances)"; return false; } S.instCap = ni; }
  {
    std::vector<float> mats(12 * (size_t)ni); std::vector<uint4> info(ni);
    uint acc = 0;
    for (uint i = 0; i < ni; i++) {
      for (int k = 0; k < 12; k++) mats[12 * (size_t)i + k] = insts[i].objectToWorld[k];
      info[i] = make_uint4(acc, insts[i].triCount, (uint)insts[i].posOffset, (uint)insts[i].idxOffset);
      acc += insts[i].triCount;
    }
    LCHK(hipMemcpyAsync(S.instMat, mats.data(), mats.size() * sizeof(float), hipMemcpyHostToDevice, nullptr));
    LCHK(hipMemcpyAsync(S.instInfo, info.data(), info.size() * sizeof(uint4), hipMemcpyHostToDevice, nullptr));
    LCHK(hipStreamSynchronize(nullptr));                               // (the staging vectors leave scope)
  }
  LbvhCounters init; std::memset(&init, 0, sizeof(init));
  for (int a = 0; a < 3; a++) { init.sceneLo[a] = 0xFFFFFFFFu; init.sceneHi[a] = 0u; }
  init.count4 = 1u; init.frontCount[0] = 1u;
  LCHK(hipMemcpyAsync(S.counters, &init, sizeof(init), hipMemcpyHostToDevice, nullptr));
  LbvhCounters* C = (LbvhCounters*)S.counters;
  const dim3 blk(256), grdN((n + 255u) / 256u);
  lbvhTriBoxKernel<<<grdN, blk>>>(S.geomPos, S.geomIdx, S.instMat, S.instInfo, ni, n, S.triBox, C);
  lbvhMortonKernel<<<grdN, blk>>>(S.triBox, n, C, S.keysIn, S.valsIn);
  size_t bytes = S.sortTempBytes;
  LCHK(hipcub::DeviceRadixSort::SortPairs(S.sortTemp, bytes, S.keysIn, S.keysOut, S.valsIn, S.valsOut, (int)n, 0, 63, nullptr));
  lbvhGatherTrisKernel<<<grdN, blk>>>(S.geomPos, S.geomIdx, S.instInfo, ni, n, S.valsOut, tris);
  S.ni = ni; S.n = n;
  if (n <= (uint)BVH_LEAF_MAX) {                                      // the whole scene is one leaf
    LCHK(hipStreamSynchronize(nullptr));
    out.rootRef = REF_LEAF | (n << 28); out.numNodes = 0; out.depth = 0; out.sahVisits = 1.0f;
    return true;
  }
  LCHK(hipMemsetAsync(S.flags, 0, (size_t)n * sizeof(uint), nullptr));
  LCHK(hipMemsetAsync(S.depth, 0, (size_t)n * sizeof(uint), nullptr));
  LCHK(hipMemsetAsync(S.height, 0, (size_t)n * sizeof(uint), nullptr));
  lbvhHierarchyKernel<<<grdN, blk>>>(S.keysOut, (int)n, S.childL, S.childR, S.parent, S.leafParent, S.first, S.last, S.folded);
  lbvhFitKernel<<<grdN, blk>>>(S.triBox, n, S.valsOut, n, S.childL, S.childR, S.parent, S.leafParent, S.folded, S.flags, S.nodeBox, S.depth, S.height);
  if (qualityPasses) {
    // "device_build_quality": treelet passes over the whole tree. Per pass: the emitted nodes grouped by their present height (the kernels of section 7,
    // into a list of the build's own), one lbvhTreeletKernel launch per height from 1 up, then the fit again for the new heights and depths
    // (the boxes it writes are the ones the pass left: unions are exact). Everything below - records, cost, 4-wide tree, level lists - reads the result.
    if (!S.passIds && !ensure(S.passIds, S.cap)) { err = "hipMalloc (treelet pass lists)"; return false; }
    const size_t levelWords = offsetof(LbvhCounters, levelCount), levelBytes = 2 * LBVH_MAX_LEVELS * sizeof(uint);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    LCHK(hipEventCreate(&ev0));
    if (hipEventCreate(&ev1) != hipSuccess) { (void)hipEventDestroy(ev0); err = "hipEventCreate"; return false; }
    auto passes = [&]() -> bool {
      LCHK(hipEventRecord(ev0, nullptr));
      for (uint pass = 0; pass < qualityPasses; pass++) {
        uint rootHeight = 0;
        LCHK(hipMemcpy(&rootHeight, S.height, sizeof(uint), hipMemcpyDeviceToHost));
        // height 0: no treelet of three leaves. A height in the last bin is clamped there with every greater one (emittedHeight), so its list
        // could hold nested nodes: such a tree is deeper than the traversal stack anyway and stays as it is
        if (rootHeight == 0u || rootHeight >= LBVH_MAX_LEVELS - 1u) break;
        lbvhLevelHistKernel<<<grdN, blk>>>(n, S.folded, S.height, C);
        lbvhLevelScanKernel<<<1, LBVH_MAX_LEVELS>>>(S.height, C);
        lbvhLevelScatterKernel<<<grdN, blk>>>(n, S.folded, S.height, C, S.passIds);
        uint cnt[LBVH_MAX_LEVELS];
        LCHK(hipMemcpy(cnt, (const char*)S.counters + levelWords, sizeof(cnt), hipMemcpyDeviceToHost));
        std::vector<uint> off(rootHeight + 2u, 0u);                      // a height's nodes lie behind those of the greater heights (lbvhLevelScanKernel)
        for (uint h = rootHeight; h-- > 0u;) off[h] = off[h + 1u] + cnt[h + 1u];
        for (uint h = 1u; h <= rootHeight; h++) {
          if (cnt[h] == 0u || (size_t)off[h] + cnt[h] > (size_t)n - 1u) continue;
          lbvhTreeletKernel<<<dim3(cnt[h]), dim3(64)>>>(S.passIds + off[h], cnt[h], n, S.childL, S.childR, S.parent, S.leafParent, S.folded, S.triBox, S.valsOut, S.nodeBox, C);
        }
        LCHK(hipMemsetAsync((char*)S.counters + levelWords, 0, levelBytes, nullptr));
        LCHK(hipMemsetAsync(S.flags, 0, (size_t)n * sizeof(uint), nullptr));
        LCHK(hipMemsetAsync(S.depth, 0, (size_t)n * sizeof(uint), nullptr));
        LCHK(hipMemsetAsync(S.height, 0, (size_t)n * sizeof(uint), nullptr));
        lbvhFitKernel<<<grdN, blk>>>(S.triBox, n, S.valsOut, n, S.childL, S.childR, S.parent, S.leafParent, S.folded, S.flags, S.nodeBox, S.depth, S.height);
        out.passesRun = pass + 1u;
      }
      LCHK(hipEventRecord(ev1, nullptr));
      LCHK(hipEventSynchronize(ev1));
      LCHK(hipEventElapsedTime(&out.passMs, ev0, ev1));
      if (out.passesRun == 0u) out.passMs = 0.0f;                          // (nothing ran: nothing to report)
      return true;
    };
    const bool ok = passes();
    (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
    if (!ok) return false;
  }
  lbvhEmitKernel<<<grdN, blk>>>(n, S.childL, S.childR, S.first, S.last, S.folded, S.triBox, S.valsOut, S.nodeBox, nodes, C);
  const uint MAX_LEVELS = 64u;
  if (wantWide && nodes4 && cap4) {
    const uint2 root = make_uint2(0u, 0u);
    LCHK(hipMemcpyAsync(S.frontA, &root, sizeof(root), hipMemcpyHostToDevice, nullptr));
    for (uint level = 0; level < MAX_LEVELS; level++) {
      lbvhResetFrontKernel<<<1, 1>>>(C, level + 1u);
      lbvhCollapseKernel<<<grdN, blk>>>(nodes, (level & 1u) ? S.frontB : S.frontA, (level & 1u) ? S.frontA : S.frontB, level, nodes4, cap4, refit.src4, C);
    }
  }
  if (refit.levelIds) {
    lbvhLevelHistKernel<<<grdN, blk>>>(n, S.folded, S.height, C);
    lbvhLevelScanKernel<<<1, LBVH_MAX_LEVELS>>>(S.height, C);
    lbvhLevelScatterKernel<<<grdN, blk>>>(n, S.folded, S.height, C, refit.levelIds);
  }
  LCHK(hipGetLastError());
  LbvhCounters res; uint rootDepth = 0, rootHeight = 0; float rootBox[6];
  LCHK(hipMemcpy(&res, S.counters, sizeof(res), hipMemcpyDeviceToHost));
  LCHK(hipMemcpy(&rootDepth, S.depth, sizeof(uint), hipMemcpyDeviceToHost));
  if (refit.levelIds) {
    LCHK(hipMemcpy(&rootHeight, S.height, sizeof(uint), hipMemcpyDeviceToHost));
    if (rootHeight < LBVH_MAX_LEVELS) {                                  // (else: deeper than the traversal stack; the caller rebuilds on the host)
      out.numLevels = rootHeight + 1u;
      for (uint l = 0; l <= rootHeight; l++) out.levelCount[l] = res.levelCount[rootHeight - l];
    }
  }
  for (int a = 0; a < 6; a++) LCHK(hipMemcpy(&rootBox[a], S.nodeBox + (size_t)a * (n - 1), sizeof(float), hipMemcpyDeviceToHost));
  out.rootRef = 0u; out.numNodes = n - 1u; out.depth = rootDepth;
  for (int k = 0; k < 64; k++) { out.treeletsExamined += res.treelet[2 * k]; out.treeletsRewritten += res.treelet[2 * k + 1]; }
  float lo[3] = { rootBox[0], rootBox[1], rootBox[2] }, hi[3] = { rootBox[3], rootBox[4], rootBox[5] };
  const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
  const float a0 = dx * dy + dy * dz + dz * dx;
  out.sahVisits = a0 > 0.0f ? 1.0f + res.sahSum / a0 : 1.0f;
  if (wantWide && nodes4 && cap4) {
    if (res.frontCount[MAX_LEVELS & 1u] != 0u || res.count4 > cap4) { out.nodes4Count = 0; out.depth4 = 0; }     // (deeper than the level loop / more nodes than room: no wide tree)
    else { out.nodes4Count = res.count4; out.depth4 = res.depth4; }
  }
  return true;
}

bool lbvhUpdatePositions(void* scratch, const std::vector<uint>& geoms, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<size_t>& posOffset,
                         const unsigned char* instDirty, uint ni, uint n, BvhTri* tris, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  if (ni != S.ni || n != S.n || !S.geomPos || !S.instInfo) { err = "the scene is not the one the tree was built over"; return false; }
  for (uint g : geoms) {
    if (g >= pos.size() || g >= posOffset.size() || posOffset[g] + posFloats[g] > S.geomPosCap) { err = "a mesh outside the uploaded geometry"; return false; }
    if (posFloats[g]) LCHK(hipMemcpyAsync(S.geomPos + posOffset[g], pos[g], posFloats[g] * sizeof(float), hipMemcpyHostToDevice, nullptr));
  }
  if (ni > S.instDirtyCap) { if (!ensure(S.instDirty, (size_t)ni)) { err = "hipMalloc (instance flags)"; S.instDirtyCap = 0; return false; } S.instDirtyCap = ni; }
  LCHK(hipMemcpyAsync(S.instDirty, instDirty, ni, hipMemcpyHostToDevice, nullptr));
  lbvhRegatherTrisKernel<<<dim3((n + 255u) / 256u), dim3(256)>>>(S.geomPos, S.geomIdx, S.instInfo, S.instDirty, ni, n, tris);
  LCHK(hipGetLastError());
  LCHK(hipStreamSynchronize(nullptr));                                 // (the caller's staging leaves scope)
  return true;
}

// ---- the two-level layout (section 9's kernels). Launches and synchronisations per call do not depend on the number of meshes or instances -------------
namespace {
struct StageTimer                          // device time between two events on the null stream
{
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~StageTimer() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
  bool start() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess && hipEventRecord(e0, nullptr) == hipSuccess; }
  bool stop(float& ms) { return hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess; }
};
}

bool lbvhCopyPositions(void* scratch, const std::vector<uint>& geoms, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<size_t>& posOffset, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  for (uint g : geoms) {
    if (!S.geomPos || g >= pos.size() || g >= posFloats.size() || g >= posOffset.size() || posOffset[g] + posFloats[g] > S.geomPosCap) { err = "a mesh outside the uploaded geometry"; return false; }
    if (posFloats[g]) LCHK(hipMemcpyAsync(S.geomPos + posOffset[g], pos[g], posFloats[g] * sizeof(float), hipMemcpyHostToDevice, nullptr));
  }
  LCHK(hipStreamSynchronize(nullptr));                                 // (the caller's staging leaves scope)
  return true;
}

bool lbvhBuildBlasBatch(void* scratch, const LbvhMeshSlot* slots, uint numGeoms, const uint* dirty, uint numDirty, LbvhMeshOut* meshOut, BvhNode* nodes, BvhTri* tris, float& ms, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  ms = 0.0f;
  S.ni = 0; S.n = 0;                                                   // (the scratch no longer holds a single-level build's order)
  if (numGeoms > S.meshCap) { if (!ensure(S.meshSlot, (size_t)numGeoms) || !ensure(S.meshOut, (size_t)numGeoms)) { err = "hipMalloc (meshes)"; S.meshCap = 0; return false; } S.meshCap = numGeoms; }
  if (numDirty > S.batchCap) { if (!ensure(S.batch, (size_t)numDirty)) { err = "hipMalloc (batch)"; S.batchCap = 0; return false; } S.batchCap = numDirty; }
  std::vector<uint2> batch(numDirty);
  size_t total = 0;
  for (uint d = 0; d < numDirty; d++) {
    if (dirty[d] >= numGeoms || slots[dirty[d]].nt == 0u) { err = "an empty mesh in the batch"; return false; }
    batch[d] = make_uint2((uint)total, dirty[d]); total += slots[dirty[d]].nt;
  }
  if (total >= (size_t(1) << 31)) { err = "more than 2^31 triangles in one batch"; return false; }
  const uint n = (uint)total, D = numDirty;
  if (numGeoms) {
    LCHK(hipMemcpyAsync(S.meshSlot, slots, (size_t)numGeoms * sizeof(LbvhMeshSlot), hipMemcpyHostToDevice, nullptr));
    LCHK(hipMemcpyAsync(S.meshOut, meshOut, (size_t)numGeoms * sizeof(LbvhMeshOut), hipMemcpyHostToDevice, nullptr));
  }
  if (n == 0u) { LCHK(hipStreamSynchronize(nullptr)); return true; }
  if (!growScratch(S, n, err)) return false;
  LCHK(hipMemcpyAsync(S.batch, batch.data(), (size_t)D * sizeof(uint2), hipMemcpyHostToDevice, nullptr));
  StageTimer timer;
  if (!timer.start()) { err = "hipEventCreate / hipEventRecord"; return false; }
  const uint slotBits = lbvhSlotBits(D);
  const dim3 blk(256), grdN((n + 255u) / 256u);
  tlTriBoxKernel<<<grdN, blk>>>(S.geomPos, S.geomIdx, S.meshSlot, S.batch, D, n, S.triBox, S.meshOut);
  tlMortonKernel<<<grdN, blk>>>(S.triBox, S.batch, D, n, S.meshOut, slotBits, S.keysIn, S.valsIn);
  size_t bytes = S.sortTempBytes;
  LCHK(hipcub::DeviceRadixSort::SortPairs(S.sortTemp, bytes, S.keysIn, S.keysOut, S.valsIn, S.valsOut, (int)n, 0, 64, nullptr));
  tlGatherTrisKernel<<<grdN, blk>>>(S.geomPos, S.geomIdx, S.meshSlot, S.batch, S.keysOut, slotBits, n, S.valsOut, tris);
  if (n >= 2u) {
    LCHK(hipMemsetAsync(S.flags, 0, (size_t)n * sizeof(uint), nullptr));
    LCHK(hipMemsetAsync(S.depth, 0, (size_t)n * sizeof(uint), nullptr));
    LCHK(hipMemsetAsync(S.height, 0, (size_t)n * sizeof(uint), nullptr));
    lbvhHierarchyKernel<<<grdN, blk>>>(S.keysOut, (int)n, S.childL, S.childR, S.parent, S.leafParent, S.first, S.last, S.folded);
    tlCutKernel<<<grdN, blk>>>(S.keysOut, n, slotBits, S.batch, S.meshSlot, S.childL, S.childR, S.first, S.last, S.parent, S.leafParent, S.meshOut);
    lbvhFitKernel<<<grdN, blk>>>(S.triBox, n, S.valsOut, n, S.childL, S.childR, S.parent, S.leafParent, S.folded, S.flags, S.nodeBox, S.depth, S.height);
    tlEmitBlasKernel<<<grdN, blk>>>(S.keysOut, n, slotBits, S.batch, S.meshSlot, S.childL, S.childR, S.first, S.last, S.folded, S.triBox, S.valsOut, S.nodeBox, nodes, S.meshOut);
  }
  tlMeshRootKernel<<<dim3((D + 255u) / 256u), blk>>>(S.batch, D, S.meshSlot, S.height, S.meshOut);
  LCHK(hipGetLastError());
  if (!timer.stop(ms)) { err = "hipEventSynchronize"; return false; }
  LCHK(hipMemcpy(meshOut, S.meshOut, (size_t)numGeoms * sizeof(LbvhMeshOut), hipMemcpyDeviceToHost));
  return true;
}

bool lbvhBuildTlas(void* scratch, const uint* instGeom, uint ni, uint nLive, uint firstLive, const float* instMotion, const LbvhMeshOut* meshOut, uint numGeoms, BvhNode* nodes, LbvhTlasResult& out, float& ms, std::string& err)
{
  Scratch& S = *(Scratch*)scratch;
  out = LbvhTlasResult(); ms = 0.0f;
  if (nLive == 0u || firstLive >= ni || instGeom[firstLive] >= numGeoms) return true;
  if (nLive == 1u) {                                                   // the root is the instance's leaf: no node, nothing to launch
    out.rootRef = REF_LEAF | firstLive; out.depth = 0u; out.sahVisits = lbvhBlasVisits(meshOut[instGeom[firstLive]]);
    return true;
  }
  if (numGeoms > S.meshCap || !S.meshOut) { err = "no batch was built for these meshes"; return false; }
  if (!growScratch(S, ni, err)) return false;
  S.ni = 0; S.n = 0;
  if (ni > S.instGeomCap) { if (!ensure(S.instGeom, (size_t)ni)) { err = "hipMalloc (instances)"; S.instGeomCap = 0; return false; } S.instGeomCap = ni; }
  if (!S.tlasResult) LCHK(hipMalloc(&S.tlasResult, sizeof(TlasResult)));
  TlasResult init; std::memset(&init, 0, sizeof(init));
  for (int a = 0; a < 3; a++) { init.lo[a] = 0xFFFFFFFFu; init.hi[a] = 0u; }
  LCHK(hipMemcpyAsync(S.instGeom, instGeom, (size_t)ni * sizeof(uint), hipMemcpyHostToDevice, nullptr));
  LCHK(hipMemcpyAsync(S.tlasResult, &init, sizeof(init), hipMemcpyHostToDevice, nullptr));
  StageTimer timer;
  if (!timer.start()) { err = "hipEventCreate / hipEventRecord"; return false; }
  TlasResult* R = (TlasResult*)S.tlasResult;
  const dim3 blk(256), grdI((ni + 255u) / 256u), grdL((nLive + 255u) / 256u);
  tlInstBoxKernel<<<grdI, blk>>>(S.instGeom, instMotion, S.meshOut, ni, S.triBox, R);
  tlInstMortonKernel<<<grdI, blk>>>(S.triBox, ni, R, S.keysIn, S.valsIn);
  size_t bytes = S.sortTempBytes;
  LCHK(hipcub::DeviceRadixSort::SortPairs(S.sortTemp, bytes, S.keysIn, S.keysOut, S.valsIn, S.valsOut, (int)ni, 0, 64, nullptr));
  LCHK(hipMemsetAsync(S.flags, 0, (size_t)nLive * sizeof(uint), nullptr));
  LCHK(hipMemsetAsync(S.depth, 0, (size_t)nLive * sizeof(uint), nullptr));
  LCHK(hipMemsetAsync(S.height, 0, (size_t)nLive * sizeof(uint), nullptr));
  lbvhHierarchyKernel<<<grdL, blk>>>(S.keysOut, (int)nLive, S.childL, S.childR, S.parent, S.leafParent, S.first, S.last, S.folded);
  lbvhFitKernel<<<grdL, blk>>>(S.triBox, ni, S.valsOut, nLive, S.childL, S.childR, S.parent, S.leafParent, S.folded, S.flags, S.nodeBox, S.depth, S.height);
  tlEmitTlasKernel<<<grdL, blk>>>(nLive, ni, S.childL, S.childR, S.triBox, S.valsOut, S.nodeBox, S.depth, S.instGeom, S.meshOut, nodes, R);
  LCHK(hipGetLastError());
  if (!timer.stop(ms)) { err = "hipEventSynchronize"; return false; }
  TlasResult res;
  LCHK(hipMemcpy(&res, S.tlasResult, sizeof(res), hipMemcpyDeviceToHost));
  out.rootRef = 0u; out.depth = res.depth;
  // TLAS visits + the chance of entering each instance x its BLAS visits (hpt_host.hip's two-level estimate)
  const float tlasVisits = res.a0 > 0.0f ? (float)(1.0 + res.sahSum / (double)res.a0) : 0.0f;
  out.sahVisits = (float)((double)tlasVisits + res.instSum);
  return true;
}

} // namespace hpt
