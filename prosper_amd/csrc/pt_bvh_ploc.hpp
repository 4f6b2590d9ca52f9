// pt_bvh_ploc.hpp — the PLOC method of the GPU hierarchy build (the rule is stated in prosper_amd/ploc.py and
// pt_bvh_ploc.hip meets it bit for bit): parallel locally-ordered clustering over the Morton order pt_bvh_build.hip has made.
// It leaves the binary tree in the radix tree's own form (first, last, split, plus the cost of every inner node's box) and
// the leaf order, and everything behind the binary tree - collapse, numbering, stack bound, heights, tables - is the
// linear method's code.  The cluster count lives on the device; one scalar per round crosses to the host.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pt_bvh_ploc_rule.hpp"
#include "pt_context.hpp"
#include "pt_scene.hpp"
#include "pt_sync.hpp"

namespace ppt
{

// From this many clusters down, one workgroup runs all remaining rounds in one launch (the same rounds in the same order,
// with barriers between them): the clusters of a round and of the next fit its LDS.  prosper_amd/ploc.py names the same
// number for the tests.
constexpr uint32_t kPlocSingleWorkgroupClusters = 512;

// The scratch arrays of the clustering, one allocation that only grows, made by the first PLOC build.  Lives with the
// linear build's (LbvhState).  112 bytes per triangle.
struct PlocState
{
    DeviceBuffer block;
    size_t capacity = 0;                           // triangles the carved arrays hold
    PlocCluster *clusters[2] = {nullptr, nullptr}; // a round reads one and writes the other
    uint32_t *nearest = nullptr;
    uint64_t *flags = nullptr, *offsets = nullptr; // survivors in the low half, new nodes in the high half
    uint32_t *left = nullptr, *right = nullptr, *size = nullptr, *parent = nullptr; // the binary tree (PlocTree)
    float *nodeCost = nullptr;                     // by merged node
    float *cost = nullptr;                         // by number in the radix tree's form: LbvhRadixTree::cost
    uint32_t *scalars = nullptr;                   // PlocScalars (pt_bvh_ploc.hip)
    void *scanTemp = nullptr;
    size_t scanTempBytes = 0;
};

struct PlocRounds
{
    uint32_t rounds = 0;       // all of them
    uint32_t finishRounds = 0; // those that ran in the single-workgroup launch
};

// The binary tree of `count` >= 2 triangles in Morton order `sorted`, on `stream`: `first`, `last`, `split` and st.cost
// indexed as the radix tree's inner nodes are, and the leaf order in `permutation` (not `sorted` itself).  `readback`
// is pinned memory of at least one word.  The stream has been waited for when this returns.
int ploc_binary_tree(
    PlocState &st, const WorldTriangle *flat, const uint32_t *sorted, uint32_t count, uint32_t radius, uint32_t *first, uint32_t *last,
    uint32_t *split, uint32_t *permutation, uint32_t *readback, hipStream_t stream, PlocRounds &out);

} // namespace ppt
