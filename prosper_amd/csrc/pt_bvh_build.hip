// pt_bvh_build.hip — see pt_bvh_build.hpp; the rule every kernel here meets bit for bit is prosper_amd/lbvh.py.
//
//   lbvh_bounds         boxes, centroids, the exact centroid bounds (integer min / max of order-preserving keys)
//   lbvh_codes          21 bits per axis, interleaved to 63-bit codes
//   (hipCUB radix sort) ascending (code, triangle index): the sort is stable and starts from index order
//   lbvh_radix_tree     Karras 2012: every inner node finds its own range and split, no atomics
//                       (the PLOC method makes the binary tree in its place: pt_bvh_ploc.hip, prosper_amd/ploc.py)
//   lbvh_count / _emit  per 4-wide depth: collapse by largest range (PLOC: by largest box cost), children numbered by a
//                       prefix sum over the depth
//   lbvh_heights        per depth, deepest first: node heights, their histogram
//   (hipCUB radix sort) nodes by (height, index)
//   lbvh_nest_boxes     behind every refit of such a tree: inner children's stored boxes grown to contain their own children's
//
// Nothing written here depends on the order in which atomics arrive: the only atomics are integer min / max / add.
#include "pt_bvh_build.hpp"

#include "bvh_encode.hpp"
#include "pt_bvh_rule.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstddef>

namespace ppt
{

namespace
{

struct LbvhScalars
{
    uint32_t centroidLo[3], centroidHi[3]; // order-preserving keys of the floats
    uint32_t nextCount;                    // inner children of the depth emitted last = nodes of the next depth
    uint32_t stackNeed;                    // largest sum of (reserved - 1) along a path
    uint32_t overflow;                     // a node number beyond the arrays (the tree has fewer nodes than triangles)
    uint32_t pad[7];
    uint32_t histogram[kLbvhMaxLevels];    // nodes per height
};

// (float_key, the other direction: pt_bvh_rule.hpp)
__device__ __forceinline__ float key_float(uint32_t k)
{
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ void centroid_of(const WorldTriangle *__restrict__ flat, uint32_t i, float c[3])
{
    const float4 *src = reinterpret_cast<const float4 *>(flat + i);
    const float4 a = src[0], b = src[1], d = src[2];
    const float tri[12] = {a.x, a.y, a.z, 0.0f, b.x, b.y, b.z, 0.0f, d.x, d.y, d.z, 0.0f};
    lbvh_centroid(tri, c);
}

__global__ void lbvh_reset_kernel(LbvhScalars *s)
{
    const uint32_t i = threadIdx.x;
    if (i < 3)
    {
        s->centroidLo[i] = 0xFFFFFFFFu;
        s->centroidHi[i] = 0u;
    }
    if (i == 0) s->nextCount = s->stackNeed = s->overflow = 0u;
    if (i < kLbvhMaxLevels) s->histogram[i] = 0u;
}

__global__ __launch_bounds__(256) void lbvh_bounds_kernel(const WorldTriangle *__restrict__ flat, uint32_t count, LbvhScalars *s)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (g < count)
    {
        float c[3];
        centroid_of(flat, g, c);
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = float_key(c[k]);
    }
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off > 0; off >>= 1)
        {
            lo[k] = min(lo[k], (uint32_t)__shfl_xor((int)lo[k], off, 64));
            hi[k] = max(hi[k], (uint32_t)__shfl_xor((int)hi[k], off, 64));
        }
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 3; ++k)
        {
            atomicMin(&s->centroidLo[k], lo[k]);
            atomicMax(&s->centroidHi[k], hi[k]);
        }
}

__global__ __launch_bounds__(256) void lbvh_codes_kernel(
    const WorldTriangle *__restrict__ flat, uint32_t count, const LbvhScalars *__restrict__ s, uint64_t *__restrict__ codes,
    uint32_t *__restrict__ index)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    float c[3];
    centroid_of(flat, g, c);
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k)
    {
        lo[k] = key_float(s->centroidLo[k]);
        hi[k] = key_float(s->centroidHi[k]);
    }
    codes[g] = lbvh_code(c, lo, hi);
    index[g] = g;
}

__global__ __launch_bounds__(256) void lbvh_radix_tree_kernel(
    const uint64_t *__restrict__ codes, uint32_t count, uint32_t *__restrict__ first, uint32_t *__restrict__ last,
    uint32_t *__restrict__ split)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i + 1u >= count) return;
    uint32_t a, b, s;
    lbvh_radix_node(codes, count, i, a, b, s);
    first[i] = a;
    last[i] = b;
    split[i] = s;
}

__global__ __launch_bounds__(256) void lbvh_count_kernel(
    LbvhRadixTree r, const uint32_t *__restrict__ radixOf, uint32_t firstNode, uint32_t nodes, uint32_t leafSize,
    uint32_t *__restrict__ innerCount)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nodes) return;
    LbvhKid kids[4];
    const uint32_t k = lbvh_collapse(r, radixOf[firstNode + g], leafSize, kids);
    uint32_t inner = 0;
    for (uint32_t c = 0; c < k; ++c) inner += lbvh_kid_triangles(kids[c]) > leafSize ? 1u : 0u;
    innerCount[firstNode + g] = inner;
}

__global__ __launch_bounds__(256) void lbvh_emit_kernel(
    LbvhRadixTree r, uint32_t *__restrict__ radixOf, uint32_t *__restrict__ pathSum, const uint32_t *__restrict__ innerCount,
    const uint32_t *__restrict__ innerOffset, uint32_t firstNode, uint32_t nodes, uint32_t leafSize, uint32_t capacity,
    BvhNode *__restrict__ out, LbvhScalars *s)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nodes) return;
    const uint32_t w = firstNode + g;
    LbvhKid kids[4];
    const uint32_t k = lbvh_collapse(r, radixOf[w], leafSize, kids);
    const uint32_t need = pathSum[w] + k - 1u;
    uint32_t next = firstNode + nodes + innerOffset[w];
    BvhNode n;
    n.origin[0] = n.origin[1] = n.origin[2] = 0.0f;
    n.reserved = k;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 4; ++c) n.lo[a][c] = n.hi[a][c] = 0x7C00u; // (the first refit writes every box)
    for (uint32_t c = 0; c < 4u; ++c)
    {
        n.child[c] = ~0;
        if (c >= k) continue;
        if (lbvh_kid_triangles(kids[c]) <= leafSize)
        {
            n.child[c] = lbvh_leaf_reference(kids[c]);
            continue;
        }
        if (next >= capacity)
        {
            atomicMax(&s->overflow, 1u);
            continue;
        }
        n.child[c] = (int32_t)next;
        radixOf[next] = kids[c].radix;
        pathSum[next] = need;
        ++next;
    }
    out[w] = n;
    atomicMax(&s->stackNeed, need);
    if (g + 1u == nodes) s->nextCount = innerOffset[w] + innerCount[w];
}

__global__ void lbvh_single_leaf_kernel(uint32_t count, BvhNode *__restrict__ out, uint32_t *__restrict__ order, LbvhScalars *s)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    BvhNode n;
    n.origin[0] = n.origin[1] = n.origin[2] = 0.0f;
    n.reserved = 1u;
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 4; ++c) n.lo[a][c] = n.hi[a][c] = 0x7C00u;
    n.child[0] = ~(int32_t)(count - 1u);
    n.child[1] = n.child[2] = n.child[3] = ~0;
    out[0] = n;
    order[0] = 0u;
    s->histogram[0] = 1u;
}

__global__ __launch_bounds__(256) void lbvh_heights_kernel(
    const BvhNode *__restrict__ nodes, uint32_t firstNode, uint32_t count, uint32_t *__restrict__ height,
    uint32_t *__restrict__ nodeIndex, LbvhScalars *s)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const uint32_t w = firstNode + g;
    uint32_t h = 0;
    for (uint32_t c = 0; c < 4u; ++c)
    {
        const int32_t ch = nodes[w].child[c];
        if (ch >= 0) h = max(h, height[ch] + 1u); // (a deeper depth: written by an earlier launch)
    }
    height[w] = h;
    nodeIndex[w] = w;
    atomicAdd(&s->histogram[min(h, kLbvhMaxLevels - 1u)], 1u);
}

__global__ __launch_bounds__(256) void lbvh_leaf_positions_kernel(
    const uint32_t *__restrict__ perm, uint32_t *__restrict__ leafPosition, uint32_t count)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < count) leafPosition[perm[g]] = g; // (perm is a permutation of 0 .. count - 1: the sort's values)
}

// ---- nesting: after the refit has encoded every node of a GPU-built tree, every inner child's stored box is grown to
//      contain the stored boxes of that child's own children.  The encoder pads each stored box from the exact bounds below
//      it and rounds outward on its own node's binary16 grid, so a grandchild's box can stick out of the child's by a
//      fraction of a grid step; here the nodes are visited by height, lowest first, and a node whose children's boxes
//      stick out is re-encoded around the union.  Boxes only grow; a node that already nests keeps its bytes.  Stored
//      corners are origin + offset, exact in double. ----
__device__ __forceinline__ float float_below(double v)
{
    float f = (float)v;
    if ((double)f > v) f = enc_next_down(f);
    return f;
}
__device__ __forceinline__ float float_above(double v)
{
    float f = (float)v;
    if ((double)f < v) f = enc_next_up(f);
    return f;
}

__global__ __launch_bounds__(256) void lbvh_nest_boxes_kernel(
    BvhNode *__restrict__ nodes, const uint32_t *__restrict__ order, uint32_t first, uint32_t count)
{
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count) return;
    const uint32_t i = order[first + g];
    BvhNode n = nodes[i];
    const uint32_t k = n.reserved < 4u ? n.reserved : 4u;
    double lo[4][3], hi[4][3];
    bool grow = false;
    for (uint32_t c = 0; c < k; ++c)
    {
        for (int a = 0; a < 3; ++a)
        {
            lo[c][a] = (double)n.origin[a] + (double)half_value(n.lo[a][c]);
            hi[c][a] = (double)n.origin[a] + (double)half_value(n.hi[a][c]);
        }
        if (n.child[c] < 0) continue;
        const BvhNode m = nodes[n.child[c]]; // (a lower height: final since an earlier launch)
        const uint32_t km = m.reserved < 4u ? m.reserved : 4u;
        for (uint32_t s = 0; s < km; ++s)
            for (int a = 0; a < 3; ++a)
            {
                const double l = (double)m.origin[a] + (double)half_value(m.lo[a][s]);
                const double h = (double)m.origin[a] + (double)half_value(m.hi[a][s]);
                if (l < lo[c][a])
                {
                    lo[c][a] = l;
                    grow = true;
                }
                if (h > hi[c][a])
                {
                    hi[c][a] = h;
                    grow = true;
                }
            }
    }
    if (!grow) return;
    for (int a = 0; a < 3; ++a)
    {
        float origin = n.origin[a]; // (never raised: a slot that did not grow keeps its offsets)
        for (uint32_t c = 0; c < k; ++c) origin = enc_min(origin, float_below(lo[c][a]));
        for (uint32_t c = 0; c < k; ++c)
        {
            n.lo[a][c] = half_floor(enc_max(float_below(lo[c][a] - (double)origin), 0.0f));
            n.hi[a][c] = half_ceil(float_above(hi[c][a] - (double)origin));
        }
        n.origin[a] = origin;
    }
    nodes[i] = n;
}

constexpr size_t kAlign = 256;
size_t aligned(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }

int reserve(LbvhState &st, uint32_t count)
{
    if (const int rc = st.events.create()) return rc;
    if (!st.readback.ptr)
        if (const int rc = st.readback.allocate(sizeof(LbvhScalars))) return rc;
    if (count <= st.capacity && st.block.ptr) return PROSPER_PT_OK;
    const size_t n = (size_t)count + count / 4 + 64;
    size_t sortBytes = 0, sortBytes2 = 0, scanBytes = 0;
    const uint64_t *k64 = nullptr;
    const uint32_t *k32 = nullptr;
    uint64_t *o64 = nullptr;
    uint32_t *o32 = nullptr;
    PPT_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, k64, o64, k32, o32, (int)n, 0, 63));
    PPT_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes2, k32, o32, k32, o32, (int)n, 0, 8));
    PPT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, k32, o32, (int)n));
    const size_t tempBytes = std::max(sortBytes, std::max(sortBytes2, scanBytes)) + kAlign;
    const size_t parts[] = {
        n * 8, n * 8, n * 4, n * 4, n * 4, n * 4, n * 4, n * sizeof(BvhNode), n * 4, n * 4, n * 4, n * 4, n * 4, n * 4, n * 4, n * 4,
        sizeof(LbvhScalars), tempBytes};
    size_t total = 0;
    for (size_t p : parts) total += aligned(p);
    st.capacity = 0;
    if (const int rc = grow_buffer(st.block, GrowWait::Device, nullptr, total, total)) return rc;
    uint8_t *at = st.block.as<uint8_t>();
    size_t part = 0;
    auto take = [&]() {
        uint8_t *p = at;
        at += aligned(parts[part++]);
        return p;
    };
    st.codes = reinterpret_cast<uint64_t *>(take());
    st.codesSorted = reinterpret_cast<uint64_t *>(take());
    st.index = reinterpret_cast<uint32_t *>(take());
    st.perm = reinterpret_cast<uint32_t *>(take());
    st.first = reinterpret_cast<uint32_t *>(take());
    st.last = reinterpret_cast<uint32_t *>(take());
    st.split = reinterpret_cast<uint32_t *>(take());
    st.nodes = reinterpret_cast<BvhNode *>(take());
    st.radixOf = reinterpret_cast<uint32_t *>(take());
    st.pathSum = reinterpret_cast<uint32_t *>(take());
    st.innerCount = reinterpret_cast<uint32_t *>(take());
    st.innerOffset = reinterpret_cast<uint32_t *>(take());
    st.height = reinterpret_cast<uint32_t *>(take());
    st.heightSorted = reinterpret_cast<uint32_t *>(take());
    st.nodeIndex = reinterpret_cast<uint32_t *>(take());
    st.order = reinterpret_cast<uint32_t *>(take());
    st.scalars = reinterpret_cast<uint32_t *>(take());
    st.sortTemp = take();
    st.sortTempBytes = tempBytes;
    st.capacity = n;
    return PROSPER_PT_OK;
}

dim3 grid_for(uint32_t n) { return dim3((n + 255u) / 256u); }

} // namespace

int lbvh_begin(LbvhState &st, uint32_t count, hipStream_t stream, uint32_t **bounds)
{
    static_assert(offsetof(LbvhScalars, centroidLo) == 0 && offsetof(LbvhScalars, centroidHi) == 3 * sizeof(uint32_t), "lo[3], hi[3] lead the scalars");
    if (count == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "GPU hierarchy build: nothing to build");
    if (const int rc = reserve(st, count)) return rc;
    PPT_HIP(hipEventRecord(st.events.events[kLbvhStageBounds], stream));
    hipLaunchKernelGGL(lbvh_reset_kernel, dim3(1), dim3(kLbvhMaxLevels), 0, stream, reinterpret_cast<LbvhScalars *>(st.scalars));
    PPT_HIP(hipGetLastError());
    *bounds = st.scalars;
    return PROSPER_PT_OK;
}

int lbvh_build(
    LbvhState &st, const WorldTriangle *flat, uint32_t count, uint32_t leafSize, const LbvhMethod &method, hipStream_t stream, LbvhResult &out,
    bool boundsReady)
{
    const bool ploc = method.method == PROSPER_PT_GPU_HIERARCHY_PLOC;
    if (count == 0 || leafSize == 0 || leafSize > kMaxLeafTriangles)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "GPU hierarchy build: nothing to build, or a leaf size outside 1 .. 4");
    if (boundsReady && (!st.block.ptr || count > st.capacity))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "GPU hierarchy build: the centroid bounds were not made for this build");
    if (const int rc = reserve(st, count)) return rc; // (boundsReady: lbvh_begin has sized the arrays, nothing moves)
    LbvhScalars *s = reinterpret_cast<LbvhScalars *>(st.scalars);
    const uint32_t capacity = (uint32_t)st.capacity;
    hipEvent_t *ev = st.events.events;
    const dim3 block(256);

    if (!boundsReady)
    {
        PPT_HIP(hipEventRecord(ev[kLbvhStageBounds], stream));
        hipLaunchKernelGGL(lbvh_reset_kernel, dim3(1), dim3(kLbvhMaxLevels), 0, stream, s);
        hipLaunchKernelGGL(lbvh_bounds_kernel, grid_for(count), block, 0, stream, flat, count, s);
    }
    PPT_HIP(hipEventRecord(ev[kLbvhStageCodes], stream));
    hipLaunchKernelGGL(lbvh_codes_kernel, grid_for(count), block, 0, stream, flat, count, s, st.codes, st.index);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(ev[kLbvhStageSort], stream));
    size_t tempBytes = st.sortTempBytes;
    PPT_HIP(hipcub::DeviceRadixSort::SortPairs(
        st.sortTemp, tempBytes, (const uint64_t *)st.codes, st.codesSorted, (const uint32_t *)st.index, st.perm, (int)count, 0, 63, stream));
    PPT_HIP(hipEventRecord(ev[kLbvhStageRadixTree], stream));

    std::vector<uint32_t> depthStart{0u}; // first node of every 4-wide depth, and the node count behind the last
    if (count <= leafSize)
    {
        PPT_HIP(hipEventRecord(ev[kLbvhStageCollapse], stream));
        hipLaunchKernelGGL(lbvh_single_leaf_kernel, dim3(1), dim3(64), 0, stream, count, st.nodes, st.order, s);
        depthStart.push_back(1u);
        PPT_HIP(hipEventRecord(ev[kLbvhStageHeights], stream));
        PPT_HIP(hipEventRecord(ev[kLbvhStageTables], stream));
    }
    else
    {
        if (ploc)
        {
            // the rounds read the Morton order and leave the leaf order in st.index (free since the sort), which then
            // becomes st.perm: everything behind this point reads the same arrays under either method
            if (const int rc = ploc_binary_tree(
                    st.ploc, flat, st.perm, count, method.radius, st.first, st.last, st.split, st.index, st.readback.ptr, stream, out.ploc))
                return rc;
            PPT_HIP(hipMemcpyAsync(st.perm, st.index, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        }
        else
            hipLaunchKernelGGL(lbvh_radix_tree_kernel, grid_for(count - 1u), block, 0, stream, st.codesSorted, count, st.first, st.last, st.split);
        PPT_HIP(hipGetLastError());
        PPT_HIP(hipEventRecord(ev[kLbvhStageCollapse], stream));
        const LbvhRadixTree tree{st.first, st.last, st.split, ploc ? st.ploc.cost : nullptr};
        // the root: radix node 0, nothing above it on its path
        PPT_HIP(hipMemsetAsync(st.radixOf, 0, sizeof(uint32_t), stream));
        PPT_HIP(hipMemsetAsync(st.pathSum, 0, sizeof(uint32_t), stream));
        uint32_t firstNode = 0, nodes = 1;
        while (nodes)
        {
            if (depthStart.size() >= kLbvhMaxLevels) return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build: the tree is deeper than 128 nodes");
            if ((uint64_t)firstNode + nodes > capacity) return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build: more nodes than triangles");
            hipLaunchKernelGGL(lbvh_count_kernel, grid_for(nodes), block, 0, stream, tree, st.radixOf, firstNode, nodes, leafSize, st.innerCount);
            tempBytes = st.sortTempBytes;
            PPT_HIP(hipcub::DeviceScan::ExclusiveSum(
                st.sortTemp, tempBytes, (const uint32_t *)st.innerCount + firstNode, st.innerOffset + firstNode, (int)nodes, stream));
            hipLaunchKernelGGL(
                lbvh_emit_kernel, grid_for(nodes), block, 0, stream, tree, st.radixOf, st.pathSum, st.innerCount, st.innerOffset, firstNode,
                nodes, leafSize, capacity, st.nodes, s);
            PPT_HIP(hipGetLastError());
            // one scalar per depth crosses to the host: how many nodes the next depth has
            PPT_HIP(hipMemcpyAsync(st.readback.ptr, &s->nextCount, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            PPT_HIP(hipStreamSynchronize(stream));
            firstNode += nodes;
            depthStart.push_back(firstNode);
            nodes = st.readback.ptr[0];
        }
        PPT_HIP(hipEventRecord(ev[kLbvhStageHeights], stream));
        for (size_t depth = depthStart.size() - 1; depth-- > 0;)
            hipLaunchKernelGGL(
                lbvh_heights_kernel, grid_for(depthStart[depth + 1] - depthStart[depth]), block, 0, stream, st.nodes, depthStart[depth],
                depthStart[depth + 1] - depthStart[depth], st.height, st.nodeIndex, s);
        PPT_HIP(hipGetLastError());
        PPT_HIP(hipEventRecord(ev[kLbvhStageTables], stream));
        tempBytes = st.sortTempBytes;
        PPT_HIP(hipcub::DeviceRadixSort::SortPairs(
            st.sortTemp, tempBytes, (const uint32_t *)st.height, st.heightSorted, (const uint32_t *)st.nodeIndex, st.order, (int)depthStart.back(), 0, 8,
            stream));
    }
    PPT_HIP(hipEventRecord(ev[kLbvhStageInstall], stream));
    PPT_HIP(hipMemcpyAsync(st.readback.ptr, s, sizeof(LbvhScalars), hipMemcpyDeviceToHost, stream));
    PPT_HIP(hipStreamSynchronize(stream));
    const LbvhScalars *h = reinterpret_cast<const LbvhScalars *>(st.readback.ptr);
    if (h->overflow) return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build: more nodes than triangles");
    out.nodeCount = depthStart.back();
    out.depths = (uint32_t)depthStart.size() - 1u;
    out.stackBound = h->stackNeed + 1u;
    if (out.stackBound > kMaxStackBound)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build: BVH stack bound exceeds the traversal's overflow capacity");
    out.levelOffsets.assign(1, 0u);
    for (uint32_t l = 0; l < kLbvhMaxLevels && out.levelOffsets.back() < out.nodeCount; ++l)
        out.levelOffsets.push_back(out.levelOffsets.back() + h->histogram[l]);
    if (out.levelOffsets.back() != out.nodeCount) return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build: the heights do not cover the nodes");
    return PROSPER_PT_OK;
}

void launch_lbvh_nest_boxes(BvhNode *nodes, const uint32_t *order, const uint32_t *levelOffsets, uint32_t levels, hipStream_t stream)
{
    for (uint32_t l = 1; l < levels; ++l) // (nodes of height 0 have no inner child)
    {
        const uint32_t first = levelOffsets[l], count = levelOffsets[l + 1] - first;
        if (count == 0) continue;
        hipLaunchKernelGGL(lbvh_nest_boxes_kernel, grid_for(count), dim3(256), 0, stream, nodes, order, first, count);
    }
}

void launch_lbvh_leaf_positions(const uint32_t *perm, uint32_t *leafPosition, uint32_t count, hipStream_t stream)
{
    if (count == 0) return;
    hipLaunchKernelGGL(lbvh_leaf_positions_kernel, grid_for(count), dim3(256), 0, stream, perm, leafPosition, count);
}

} // namespace ppt
