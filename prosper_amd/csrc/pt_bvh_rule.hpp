// pt_bvh_rule.hpp — the arithmetic of the GPU hierarchy build that has to match prosper_amd/lbvh.py bit for bit: centroids,
// quantisation, the 63-bit code, a radix-tree node (Karras 2012), the 4-wide collapse.  Plain functions for host and device
// without any include of the runtime, so that tests/lbvh_rule_main.cpp runs the very code of the kernels (pt_bvh_build.hip)
// on a CPU, under sanitizers.  Integer and IEEE fp32 arithmetic only; the library is compiled without contraction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define PPT_RULE __host__ __device__ inline
#else
#define PPT_RULE inline
#endif

namespace ppt
{

PPT_RULE float rule_min(float a, float b) { return b < a ? b : a; }
PPT_RULE float rule_max(float a, float b) { return b > a ? b : a; }

// a world triangle is twelve words: v0.xyz, -, v1.xyz, -, v2.xyz, - (pt_scene.hpp WorldTriangle)
PPT_RULE void lbvh_centroid(const float *tri, float c[3])
{
    for (int k = 0; k < 3; ++k)
    {
        const float lo = rule_min(rule_min(tri[k], tri[4 + k]), tri[8 + k]);
        const float hi = rule_max(rule_max(tri[k], tri[4 + k]), tri[8 + k]);
        c[k] = 0.5f * (lo + hi);
    }
}

// an unsigned key whose order is the floats' own: the centroid bounds are integer minima and maxima of these
PPT_RULE uint32_t float_key(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the cell of c on an axis whose centroid bounds are [lo, hi]: 21 bits, 0 on an axis without extent, the top clamped
PPT_RULE uint32_t lbvh_quantise(float c, float lo, float hi)
{
    const float ext = hi - lo;
    if (!(ext > 0.0f)) return 0u;
    const float v = ((c - lo) / ext) * 2097152.0f;
    if (v >= 2097151.0f) return 2097151u;
    return v > 0.0f ? (uint32_t)v : 0u;
}
// bit i of x -> bit 3 i
PPT_RULE uint64_t lbvh_spread3(uint32_t x)
{
    uint64_t v = x & 0x1FFFFFu;
    v = (v | (v << 32)) & 0x001F00000000FFFFull;
    v = (v | (v << 16)) & 0x001F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}
PPT_RULE uint64_t lbvh_code(const float c[3], const float lo[3], const float hi[3])
{
    return (lbvh_spread3(lbvh_quantise(c[0], lo[0], hi[0])) << 2) | (lbvh_spread3(lbvh_quantise(c[1], lo[1], hi[1])) << 1) |
           lbvh_spread3(lbvh_quantise(c[2], lo[2], hi[2]));
}

// common prefix of the keys at positions i and j != i of the ordered codes; -1 outside the array.  Equal codes differ
// in their position.
PPT_RULE int lbvh_prefix(const uint64_t *codes, uint32_t count, uint32_t i, uint64_t ci, int64_t j)
{
    if (j < 0 || j >= (int64_t)count) return -1;
    const uint64_t x = ci ^ codes[j];
    if (x) return __builtin_clzll(x);
    const uint32_t y = i ^ (uint32_t)j;
    return 64 + (y ? __builtin_clz(y) : 32);
}

// inner node i (0 .. count - 2) of the radix tree over `count` >= 2 ordered codes: its range [first, last] and its split;
// its children are [first, split] and [split + 1, last], and a child of more than one key is inner node `split` (left) or
// `split + 1` (right)
PPT_RULE void lbvh_radix_node(const uint64_t *codes, uint32_t count, uint32_t i, uint32_t &first, uint32_t &last, uint32_t &split)
{
    const uint64_t ci = codes[i];
    const int64_t p = (int64_t)i;
    const int64_t d = lbvh_prefix(codes, count, i, ci, p + 1) > lbvh_prefix(codes, count, i, ci, p - 1) ? 1 : -1;
    const int dmin = lbvh_prefix(codes, count, i, ci, p - d);
    int64_t lmax = 2;
    while (lbvh_prefix(codes, count, i, ci, p + lmax * d) > dmin) lmax *= 2;
    int64_t length = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (lbvh_prefix(codes, count, i, ci, p + (length + t) * d) > dmin) length += t;
    const int64_t j = p + length * d;
    const int dnode = lbvh_prefix(codes, count, i, ci, j);
    int64_t s = 0;
    for (int64_t t = length; t > 1;)
    {
        t = (t + 1) / 2;
        if (lbvh_prefix(codes, count, i, ci, p + (s + t) * d) > dnode) s += t;
    }
    first = (uint32_t)(d > 0 ? p : j);
    last = (uint32_t)(d > 0 ? j : p);
    split = (uint32_t)(p + s * d + (d < 0 ? -1 : 0));
}

// a slot of a node under collapse: the range [a, b] of ordered positions, and the radix node that covers it (a != b)
struct LbvhKid
{
    uint32_t a, b, radix;
};
struct LbvhRadixTree
{
    const uint32_t *first, *last, *split;
    const float *cost; // null: the linear method.  Else the cost of every inner node's own box (pt_bvh_ploc_rule.hpp)
};
PPT_RULE uint32_t lbvh_kid_triangles(const LbvhKid &k) { return k.b - k.a + 1u; }
PPT_RULE void lbvh_children(const LbvhRadixTree &r, uint32_t t, LbvhKid &left, LbvhKid &right)
{
    const uint32_t s = r.split[t];
    left = LbvhKid{r.first[t], s, s};
    right = LbvhKid{s + 1u, r.last[t], s + 1u};
}
// the slots of the 4-wide node made of radix node t: open the largest range (the first one on a tie) until four slots are
// in use or none holds more than leafSize triangles; returns the slots in use.  A tree that carries box costs opens the
// slot of more than leafSize triangles with the largest cost instead (on equal cost the larger range, then the first).
PPT_RULE uint32_t lbvh_collapse(const LbvhRadixTree &r, uint32_t t, uint32_t leafSize, LbvhKid kids[4])
{
    lbvh_children(r, t, kids[0], kids[1]);
    uint32_t k = 2;
    while (k < 4u)
    {
        int best = -1;
        uint32_t bestCount = leafSize;
        float bestCost = 0.0f;
        for (uint32_t c = 0; c < k; ++c)
        {
            const uint32_t triangles = lbvh_kid_triangles(kids[c]);
            if (triangles <= leafSize) continue;
            const float cost = r.cost ? r.cost[kids[c].radix] : 0.0f;
            if (r.cost ? (best < 0 || cost > bestCost || (cost == bestCost && triangles > bestCount)) : triangles > bestCount)
            {
                best = (int)c;
                bestCount = triangles;
                bestCost = cost;
            }
        }
        if (best < 0) break;
        LbvhKid left, right;
        lbvh_children(r, kids[best].radix, left, right);
        kids[best] = left;
        kids[k++] = right;
    }
    return k;
}
// the reference of a leaf slot: ~ref = first << 3 | count - 1
PPT_RULE int32_t lbvh_leaf_reference(const LbvhKid &k) { return ~(int32_t)((k.a << 3) | (lbvh_kid_triangles(k) - 1u)); }

} // namespace ppt
