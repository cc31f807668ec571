// Interface of the device-side CommitScene (hpt_lbvh.hip): a linear BVH over the instanced triangles of the single-level layout and its 4-wide
// compressed form, built by kernels. Called by hpt_host.hip's commit path when the caller asks for a fast build (CommitScene(BUILD_LOW / BUILD_MEDIUM),
// CrossRT.h:8-14, 109) or hpt_set_option("device_build", 1).
#pragma once
#include <string>
#include <vector>
#include "hpt_types.h"

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

} // namespace hpt
