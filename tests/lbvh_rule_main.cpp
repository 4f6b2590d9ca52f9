// lbvh_rule_main.cpp — the arithmetic of the GPU hierarchy build (prosper_amd/csrc/pt_bvh_rule.hpp: the functions the
// kernels of pt_bvh_build.hip call) run on a CPU, in the kernels' order of work: codes, a stable sort, every radix node,
// the collapse and numbering depth by depth.  tests/test_lbvh_cpu.py compares what it writes with prosper_amd/lbvh.py.
//
//   lbvh_rule <triangles.bin> <leafSize> <out.bin>
//
// triangles.bin: n x 12 words (WorldTriangle).  out.bin, uint32 words: n, nodeCount, stackBound, codes (2 n, low word
// first), permutation (n), and per node child[4], reserved.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "pt_bvh_rule.hpp"

using namespace ppt;

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    std::vector<float> tris;
    {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        float word;
        while (std::fread(&word, 4, 1, f) == 1) tris.push_back(word);
        std::fclose(f);
    }
    const uint32_t n = (uint32_t)(tris.size() / 12), leafSize = (uint32_t)std::atoi(argv[2]);
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
    std::vector<uint64_t> codes(n), ordered(n);
    for (uint32_t i = 0; i < n; ++i) codes[i] = lbvh_code(&centroid[3 * (size_t)i], lo, hi);
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return codes[a] < codes[b]; });
    for (uint32_t i = 0; i < n; ++i) ordered[i] = codes[perm[i]];

    struct Node
    {
        int32_t child[4];
        uint32_t reserved;
    };
    std::vector<Node> nodes;
    uint32_t stackNeed = 0;
    if (n <= leafSize)
        nodes.push_back(Node{{n ? ~(int32_t)(n - 1u) : -1, -1, -1, -1}, n ? 1u : 0u});
    else
    {
        std::vector<uint32_t> first(n - 1), last(n - 1), split(n - 1);
        for (uint32_t i = 0; i + 1 < n; ++i) lbvh_radix_node(ordered.data(), n, i, first[i], last[i], split[i]);
        const LbvhRadixTree tree{first.data(), last.data(), split.data()};
        std::vector<uint32_t> radixOf{0u}, pathSum{0u};
        uint32_t firstNode = 0, count = 1;
        while (count)
        {
            uint32_t next = firstNode + count; // (the prefix sum over the depth, taken as the loop goes)
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

    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const uint32_t header[3] = {n, (uint32_t)nodes.size(), stackNeed + 1u};
    std::fwrite(header, 4, 3, out);
    if (n) // (an empty vector's data() may be null)
    {
        std::fwrite(codes.data(), 8, n, out);
        std::fwrite(perm.data(), 4, n, out);
    }
    std::fwrite(nodes.data(), sizeof(Node), nodes.size(), out);
    std::fclose(out);
    std::printf("lbvh rule ok\n");
    return 0;
}
