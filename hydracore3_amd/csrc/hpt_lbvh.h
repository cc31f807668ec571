// Interface of the device-side CommitScene (hpt_lbvh.hip): a linear BVH over the instanced triangles of the single-level layout and its 4-wide
// compressed form, built by kernels. Called by hpt_host.hip's commit path when the caller asks for a fast build (CommitScene(BUILD_LOW / BUILD_MEDIUM),
// CrossRT.h:8-14, 109) or hpt_set_option("device_build", 1).
#pragma once
#include <string>
#include <vector>
#include "hpt_types.h"
#include "lbvh_key.h"

namespace hpt {

static const uint LBVH_MAX_LEVELS = 64;   // (a tree deeper than the 64-entry traversal stack is handed back to the host's builder)

struct LbvhInstance { float objectToWorld[12]; uint triCount; size_t posOffset, idxOffset; };   // rows of the 3x4 matrix; offsets (floats / uints) of its mesh in the uploaded geometry
struct LbvhResult
{
  uint rootRef = REF_NONE, numNodes = 0, depth = 0, nodes4Count = 0, depth4 = 0; float sahVisits = 1.0f;
  // what a refit needs (LbvhRefitOut): levelCount[l] nodes of level l, level 0 = the root's, the last level = the nodes over leaves only
  uint numLevels = 0, levelCount[LBVH_MAX_LEVELS] = {};
  // the treelet passes ("device_build_quality"): passes run, treelets of three leaves or more examined and rewritten over all passes, milliseconds between
  // the device events around the passes
  uint passesRun = 0, treeletsExamined = 0, treeletsRewritten = 0; float passMs = 0.0f;
};
// Caller-owned device arrays the build fills for a later refit (hpt_host.hip: refit_flat), both optional:
// levelIds (n - 1 entries): the emitted nodes grouped by level, a level = the node's height in the emitted tree counted down from the root's, so a
// node's inner children always lie in later levels (what refitLevelKernel needs); src4 (4 * cap4): per 4-wide child the BVH2 (node << 1 | side)
// its box comes from (what refitNodes4Kernel needs)
struct LbvhRefitOut { uint* levelIds = nullptr; uint* src4 = nullptr; };

void* lbvhCreate();
void  lbvhDestroy(void* scratch);
// copies every mesh's positions (3 floats per vertex) and indices to the device; posOffset / idxOffset receive each mesh's place
bool  lbvhUploadGeometry(void* scratch, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<const uint*>& idx, const std::vector<size_t>& idxCount,
                         std::vector<size_t>& posOffset, std::vector<size_t>& idxOffset, std::string& err);
// builds into caller-owned device arrays: nodes (n - 1 entries), tris (n), nodes4 (cap4 entries; skipped when !wantWide).
// qualityPasses: treelet restructuring passes over the hierarchy before anything is emitted (0: the plain Karras tree, nothing else launched)
bool  lbvhBuild(void* scratch, const LbvhInstance* insts, uint ni, uint n, BvhNode* nodes, BvhTri* tris, BvhNode4* nodes4, uint cap4, bool wantWide, const LbvhRefitOut& refit,
                 uint qualityPasses, LbvhResult& out, std::string& err);
// moved vertices of a built tree: copies the positions of the meshes listed in `geoms` to their place in the uploaded geometry (posOffset as
// lbvhUploadGeometry returned it) and rewrites, in the build's expressions, the records in `tris` (n of them) of the instances flagged in
// instDirty (ni bytes); everything else stays. The sorted order of the last build is kept by the scratch until the next one.
bool  lbvhUpdatePositions(void* scratch, const std::vector<uint>& geoms, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<size_t>& posOffset,
                          const unsigned char* instDirty, uint ni, uint n, BvhTri* tris, std::string& err);

// ---- the two-level layout on the device (hpt_set_option("device_build_two_level", 1)) ----------------------------------------------------------------
// One batched build for the BLAS of all dirty meshes, in object space, then a TLAS over the live instances. The batch is ONE sort and ONE Karras
// hierarchy over the dirty meshes' concatenated triangles: the 64-bit sort key carries the mesh's slot in the batch above the Morton code of the
// centroid (normalised to the mesh's own bounds), so every mesh is a subtree and the nodes that span several meshes are simply never fitted or emitted.
// Key layout (lbvh_key.h: lbvhPackKey): slot << 3 m | Morton code of m bits per axis, m = min(21, (64 - slotBits) / 3), slotBits = ceil(log2(slots)).
// Morton bits per axis left: 21 up to 2 meshes, 16 at 2^16 meshes, 14 at 2^20 meshes. Equal keys stay separated by index (delta() of hpt_lbvh.hip).
HPT_HD uint floatKey(float f) { const uint b = hptFloatToBits(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }       // monotonic float -> uint
HPT_HD float keyFloat(uint k) { return hptBitsToFloat((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// a mesh's fixed place in the two-level arrays (host-made): nt - 1 nodes from nodeBase, nt records from triBase; its place in the uploaded geometry
struct LbvhMeshSlot { uint nodeBase, triBase, nt, posOff, idxOff; };
// what the batch leaves per mesh (device-made; the host keeps a mirror): object-space bounds as floatKey words, the patched BLAS root (a leaf for
// meshes of <= BVH_LEAF_MAX triangles, REF_NONE for an empty mesh), the emitted tree's inner levels, the Karras node that is its root, and the sum
// of the half-areas of its emitted inner children
struct LbvhMeshOut { uint lo[3], hi[3]; uint root, depth, karrasRoot, pad; double sahSum; };
HPT_HD void lbvhMeshOutReset(LbvhMeshOut& o) { for (int a = 0; a < 3; a++) { o.lo[a] = 0xFFFFFFFFu; o.hi[a] = 0u; } o.root = REF_NONE; o.depth = 0u; o.karrasRoot = 0xFFFFFFFFu; o.pad = 0u; o.sahSum = 0.0; }
// expected inner-node visits of a BLAS (sah_node_visits of hpt_host.hip on its tree): 0 when the root is no node
HPT_HD float lbvhBlasVisits(const LbvhMeshOut& o)
{
  if (o.root == REF_NONE || (o.root & REF_LEAF)) return 0.0f;
  const float dx = keyFloat(o.hi[0]) - keyFloat(o.lo[0]), dy = keyFloat(o.hi[1]) - keyFloat(o.lo[1]), dz = keyFloat(o.hi[2]) - keyFloat(o.lo[2]);
  const float a0 = dx < 0.0f ? 0.0f : dx * dy + dy * dz + dz * dx;
  return a0 > 0.0f ? (float)(1.0 + o.sahSum / (double)a0) : 0.0f;
}
struct LbvhTlasResult { uint rootRef = REF_NONE, depth = 0; float sahVisits = 0.0f; };

// BLAS of the meshes listed in `dirty` (each with slots[g].nt > 0), every one into its own slot of nodes / tris; meshOut (numGeoms entries, host):
// in - the entries of the dirty meshes reset, the others as the last batch left them; out - the dirty meshes' results. ms: device time of the stage
bool  lbvhBuildBlasBatch(void* scratch, const LbvhMeshSlot* slots, uint numGeoms, const uint* dirty, uint numDirty, LbvhMeshOut* meshOut, BvhNode* nodes, BvhTri* tris, float& ms, std::string& err);
// TLAS over the instances whose mesh is not empty (nLive of the ni; firstLive: the lowest such instance) into nodes[0 .. nLive - 1), instance leaves of
// exactly one instance. instGeom: the mesh of every instance (host); instMotion (device): 2 x 12 object -> world rows per instance, both keys (equal
// for an instance that does not move). Reads the per-mesh results the last batch left on the device. sahVisits: TLAS visits + the sum over the
// instances of halfArea(instance box) / halfArea(TLAS root) x BLAS visits of its mesh
bool  lbvhBuildTlas(void* scratch, const uint* instGeom, uint ni, uint nLive, uint firstLive, const float* instMotion, const LbvhMeshOut* meshOut, uint numGeoms, BvhNode* nodes, LbvhTlasResult& out, float& ms, std::string& err);
// copies the positions of the meshes in `geoms` to their place in the uploaded geometry (posOffset as lbvhUploadGeometry returned it)
bool  lbvhCopyPositions(void* scratch, const std::vector<uint>& geoms, const std::vector<const float*>& pos, const std::vector<size_t>& posFloats, const std::vector<size_t>& posOffset, std::string& err);

} // namespace hpt
