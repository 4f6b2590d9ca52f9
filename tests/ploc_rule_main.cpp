// ploc_rule_main.cpp — the arithmetic of the GPU hierarchy build's PLOC method (prosper_amd/csrc/pt_bvh_ploc_rule.hpp and
// pt_bvh_rule.hpp: the functions the kernels of pt_bvh_ploc.hip and pt_bvh_build.hip call) run on a CPU, in the kernels'
// order of work: codes, a stable sort, the rounds (every position's search, the flags, their exclusive sum, the scatter),
// every node's place in the leaf order, the collapse and numbering depth by depth.  tests/test_ploc_cpu.py compares what
// it writes with prosper_amd/ploc.py.
//
//   ploc_rule <triangles.bin> <leafSize> <radius> <out.bin>
//
// triangles.bin: n x 12 words (WorldTriangle).  out.bin, uint32 words: n, nodeCount, stackBound, rounds, codes (2 n, low
// word first), permutation (n), and per node child[4], reserved.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "pt_bvh_ploc_rule.hpp"

using namespace ppt;

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    std::vector<float> tris;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        float word;
        while (std::fread(&word, 4, 1, f) == 1) tris.push_back(word);
        std::fclose(f);
    }
    const uint32_t n = (uint32_t)(tris.size() / 12), leafSize = (uint32_t)std::atoi(argv[2]), radius = (uint32_t)std::atoi(argv[3]);
    if (radius < 1 || radius > kPlocMaxRadius) return 2;
    std::vector<float> centroid(3 * (size_t)n);
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i)
    {
        lbvh_centroid(&tris[12 * (size_t)i], &centroid[3 * (size_t)i]);
        for (int k = 0; k < 3; ++k)
        {
            lo[k] = i ? rule_min(lo[k], centroid[3 * (size_t)i + k]) : centroid[3 * (size_t)i + k];
            hi[k] = i ? rule_max(hi[k], centroid[3 * (size_t)i + k]) : centroid[3 * (size_t)i + k];
        }
    }
    std::vector<uint64_t> codes(n);
    for (uint32_t i = 0; i < n; ++i) codes[i] = lbvh_code(&centroid[3 * (size_t)i], lo, hi);
    std::vector<uint32_t> sorted(n), perm(n);
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return codes[a] < codes[b]; });
    perm = sorted;

    struct Node
    {
        int32_t child[4];
        uint32_t reserved;
    };
    std::vector<Node> nodes;
    uint32_t stackNeed = 0, rounds = 0;
    if (n <= leafSize)
        nodes.push_back(Node{{n ? ~(int32_t)(n - 1u) : -1, -1, -1, -1}, n ? 1u : 0u});
    else
    {
        // ---- the rounds ----
        std::vector<PlocCluster> clusters(n), following;
        for (uint32_t p = 0; p < n; ++p) clusters[p] = ploc_leaf(&tris[12 * (size_t)sorted[p]], p);
        std::vector<uint32_t> left(n - 1), right(n - 1), size(n - 1), parent(2 * (size_t)n - 1, kPlocNone);
        std::vector<float> nodeCost(n - 1);
        uint32_t made = 0;
        while (clusters.size() > 1)
        {
            const uint32_t m = (uint32_t)clusters.size();
            std::vector<uint32_t> nearest(m);
            for (uint32_t i = 0; i < m; ++i) nearest[i] = ploc_nearest(clusters.data(), 0, m, i, radius);
            std::vector<uint64_t> flags(m), offsets(m);
            for (uint32_t i = 0; i < m; ++i) flags[i] = ploc_flags(nearest.data(), i);
            uint64_t sum = 0;
            for (uint32_t i = 0; i < m; ++i)
            {
                offsets[i] = sum;
                sum += flags[i];
            }
            following.assign((size_t)(sum & 0xFFFFFFFFu), PlocCluster{});
            for (uint32_t i = 0; i < m; ++i)
            {
                if (!(flags[i] & 1u)) continue;
                PlocCluster c = clusters[i];
                if (flags[i] >> 32)
                {
                    const uint32_t k = made + (uint32_t)(offsets[i] >> 32);
                    const PlocCluster &other = clusters[nearest[i]];
                    left.at(k) = c.node;
                    right.at(k) = other.node;
                    parent.at(c.node) = parent.at(other.node) = n + k;
                    c = ploc_union(c, other);
                    c.node = n + k;
                    size.at(k) = c.size;
                    nodeCost.at(k) = ploc_box_cost(c);
                }
                following.at((size_t)(offsets[i] & 0xFFFFFFFFu)) = c;
            }
            made += (uint32_t)(sum >> 32);
            if (following.size() >= clusters.size()) return 3; // (every round merges a pair)
            clusters.swap(following);
            ++rounds;
        }
        if (made != n - 1 || clusters[0].node != 2 * n - 2 || clusters[0].size != n) return 3;

        // ---- the leaf order and the radix tree's form ----
        const PlocTree binary{left.data(), right.data(), size.data(), parent.data(), n};
        std::vector<uint32_t> first(n - 1), last(n - 1), split(n - 1);
        std::vector<float> cost(n - 1);
        for (uint32_t p = 0; p < n; ++p) perm.at(ploc_first(binary, p)) = sorted[p];
        for (uint32_t node = n; node < 2 * n - 1; ++node)
        {
            uint32_t a, b, s;
            const uint32_t t = ploc_radix_form(binary, node, a, b, s);
            first.at(t) = a;
            last.at(t) = b;
            split.at(t) = s;
            cost.at(t) = nodeCost[node - n];
        }

        // ---- the collapse (as tests/lbvh_rule_main.cpp) ----
        const LbvhRadixTree tree{first.data(), last.data(), split.data(), cost.data()};
        std::vector<uint32_t> radixOf{0u}, pathSum{0u};
        uint32_t firstNode = 0, count = 1;
        while (count)
        {
            uint32_t next = firstNode + count;
            for (uint32_t w = firstNode; w < firstNode + count; ++w)
            {
                LbvhKid kids[4];
                const uint32_t k = lbvh_collapse(tree, radixOf[w], leafSize, kids);
                const uint32_t need = pathSum[w] + k - 1u;
                Node node{{-1, -1, -1, -1}, k};
                for (uint32_t c = 0; c < k; ++c)
                    if (lbvh_kid_triangles(kids[c]) <= leafSize)
                        node.child[c] = lbvh_leaf_reference(kids[c]);
                    else
                    {
                        node.child[c] = (int32_t)next++;
                        radixOf.push_back(kids[c].radix);
                        pathSum.push_back(need);
                    }
                nodes.push_back(node);
                stackNeed = std::max(stackNeed, need);
            }
            const uint32_t following = next - (firstNode + count);
            firstNode += count;
            count = following;
        }
    }

    FILE *out = std::fopen(argv[4], "wb");
    if (!out) return 2;
    const uint32_t header[4] = {n, (uint32_t)nodes.size(), stackNeed + 1u, rounds};
    std::fwrite(header, 4, 4, out);
    if (n) // (an empty vector's data() may be null)
    {
        std::fwrite(codes.data(), 8, n, out);
        std::fwrite(perm.data(), 4, n, out);
    }
    std::fwrite(nodes.data(), sizeof(Node), nodes.size(), out);
    std::fclose(out);
    std::printf("ploc rule ok\n");
    return 0;
}
