// pt_bvh_ploc_rule.hpp — the arithmetic of the GPU hierarchy build's PLOC method that has to match prosper_amd/ploc.py bit
// for bit: a cluster's box, the cost of a pair, the packed key and its comparison, the union, one position's part of a
// round, a node's place in the leaf order.  Plain functions for host and device like pt_bvh_rule.hpp, so that
// tests/ploc_rule_main.cpp runs the very code of the kernels (pt_bvh_ploc.hip) on a CPU, under sanitizers.
#pragma once

#include "pt_bvh_rule.hpp"

namespace ppt
{

constexpr uint32_t kPlocDefaultRadius = 8; // (with leaves of 2 the lowest C3 frame time of radii 8, 16, 32 x leaves of 1, 2, 4: DESIGN.md f26)
constexpr uint32_t kPlocMaxRadius = 32;
constexpr uint32_t kPlocNone = 0xFFFFFFFFu;

// one position of the cluster list: the box, the binary node it stands for, that node's triangles
struct alignas(16) PlocCluster
{
    float lo[3];
    uint32_t node;
    float hi[3];
    uint32_t size;
};

PPT_RULE PlocCluster ploc_leaf(const float *tri, uint32_t node)
{
    PlocCluster c;
    for (int k = 0; k < 3; ++k)
    {
        c.lo[k] = rule_min(rule_min(tri[k], tri[4 + k]), tri[8 + k]);
        c.hi[k] = rule_max(rule_max(tri[k], tri[4 + k]), tri[8 + k]);
    }
    c.node = node;
    c.size = 1u;
    return c;
}
// the box is the exact union; node and size are the caller's
PPT_RULE PlocCluster ploc_union(const PlocCluster &a, const PlocCluster &b)
{
    PlocCluster c;
    for (int k = 0; k < 3; ++k)
    {
        c.lo[k] = rule_min(a.lo[k], b.lo[k]);
        c.hi[k] = rule_max(a.hi[k], b.hi[k]);
    }
    c.node = kPlocNone;
    c.size = a.size + b.size;
    return c;
}
PPT_RULE float ploc_box_cost(const PlocCluster &c)
{
    const float ex = c.hi[0] - c.lo[0], ey = c.hi[1] - c.lo[1], ez = c.hi[2] - c.lo[2];
    return (ex * ey + ey * ez) + ez * ex;
}
PPT_RULE float ploc_pair_cost(const PlocCluster &a, const PlocCluster &b) { return ploc_box_cost(ploc_union(a, b)); }
PPT_RULE uint32_t ploc_float_bits(float f)
{
    union
    {
        float f;
        uint32_t u;
    } v;
    v.f = f;
    return v.u;
}
// the key of the pair (i, j) as position i sees it; the least key is the nearest neighbour.  The cost is never negative
// (a zero may carry a sign), so its bits order as the floats do.
PPT_RULE uint64_t ploc_key(float cost, uint32_t i, uint32_t j)
{
    const uint32_t below = j < i ? j : i, distance = j < i ? i - j : j - i;
    return ((uint64_t)(ploc_float_bits(cost) & 0x7FFFFFFFu) << 32) | (uint64_t)(distance << 2) | (uint64_t)((below & 1u) << 1) |
           (uint64_t)(j > i ? 1u : 0u);
}
// nn(i) among the m > 1 clusters of a round; clusters[p - origin] is the cluster at position p, for every p within
// `radius` of i that lies in 0 .. m - 1
PPT_RULE uint32_t ploc_nearest(const PlocCluster *clusters, int64_t origin, uint32_t m, uint32_t i, uint32_t radius)
{
    const PlocCluster self = clusters[(int64_t)i - origin];
    uint64_t best = ~0ull;
    uint32_t nn = kPlocNone;
    for (uint32_t d = 1; d <= radius; ++d)
    {
        if (i >= d)
        {
            const uint64_t key = ploc_key(ploc_pair_cost(self, clusters[(int64_t)(i - d) - origin]), i, i - d);
            if (key < best)
            {
                best = key;
                nn = i - d;
            }
        }
        if (i + d < m)
        {
            const uint64_t key = ploc_key(ploc_pair_cost(self, clusters[(int64_t)(i + d) - origin]), i, i + d);
            if (key < best)
            {
                best = key;
                nn = i + d;
            }
        }
    }
    return nn;
}
// what position i does in a round, from every position's nn: bit 0: it survives (it is not the upper end of a mutual
// pair), bit 32: it is the lower end of one and becomes the merged cluster.  The two halves are what the round's
// exclusive sum counts: survivor positions and new nodes.
PPT_RULE uint64_t ploc_flags(const uint32_t *nearest, uint32_t i)
{
    const uint32_t j = nearest[i];
    const bool mutual = nearest[j] == i;
    return (mutual && j < i ? 0ull : 1ull) | (mutual && i < j ? 1ull << 32 : 0ull);
}

// The binary tree the rounds leave: nodes 0 .. n - 1 are the leaves by ordered position, n .. 2 n - 2 the merged nodes
// (left, right, size indexed from n); parent of every node, kPlocNone at the root.
struct PlocTree
{
    const uint32_t *left, *right, *size, *parent;
    uint32_t n;
};
PPT_RULE uint32_t ploc_size(const PlocTree &t, uint32_t node) { return node < t.n ? 1u : t.size[node - t.n]; }
// first leaf position of a node: walking up, the left sibling's size wherever the walk came up from the right
PPT_RULE uint32_t ploc_first(const PlocTree &t, uint32_t node)
{
    uint32_t first = 0;
    for (uint32_t c = node, p = t.parent[node]; p != kPlocNone; c = p, p = t.parent[p])
        if (t.right[p - t.n] == c) first += ploc_size(t, t.left[p - t.n]);
    return first;
}
// A merged node in the radix tree's form (pt_bvh_rule.hpp LbvhRadixTree), which numbers the root 0, a left child by its
// last position and a right child by its first: its number, range and split
PPT_RULE uint32_t ploc_radix_form(const PlocTree &t, uint32_t node, uint32_t &first, uint32_t &last, uint32_t &split)
{
    first = ploc_first(t, node);
    last = first + ploc_size(t, node) - 1u;
    split = first + ploc_size(t, t.left[node - t.n]) - 1u;
    const uint32_t p = t.parent[node];
    if (p == kPlocNone) return 0u;
    return t.left[p - t.n] == node ? last : first;
}

} // namespace ppt
