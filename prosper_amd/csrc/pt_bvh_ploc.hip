// pt_bvh_ploc.hip — see pt_bvh_ploc.hpp; the rule every kernel here meets bit for bit is prosper_amd/ploc.py, and the
// arithmetic is pt_bvh_ploc_rule.hpp's.
//
//   ploc_init        position p holds leaf p: the box of triangle sorted[p]; no node has a parent yet
//   per round, while more clusters are left than one workgroup holds:
//     ploc_search    a workgroup's clusters plus `radius` positions of halo on each side into LDS; every lane scans its own
//                    2 * radius neighbours for nn
//     ploc_flags     mutual pairs: who survives, who becomes a merged node
//     (hipCUB scan)  exclusive sum of both counts at once: survivor positions, new node numbers
//     ploc_scatter   merged nodes into the tree, the next round's cluster list in order; the new count
//   ploc_finish      all remaining rounds in one workgroup, the cluster lists in LDS
//   ploc_ranges      every node walks up its parent links to its first leaf position: the leaf order, and the tree in the
//                    radix tree's form for the collapse
//
// No atomics; nothing here depends on the order in which anything arrives.
#include "pt_bvh_ploc.hpp"

#include "pt_error.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace ppt
{

namespace
{

constexpr uint32_t kBlock = 256;
constexpr uint32_t kT = kPlocSingleWorkgroupClusters;

struct PlocScalars
{
    uint32_t count[2]; // clusters before a round (by the round's parity) and after it
    uint32_t made[2];  // merged nodes made so far, likewise
    uint32_t rounds, finishRounds;
    uint32_t pad[2];
};

__global__ __launch_bounds__(kBlock) void ploc_init_kernel(
    const WorldTriangle *__restrict__ flat, const uint32_t *__restrict__ sorted, uint32_t count, PlocCluster *__restrict__ out,
    uint32_t *__restrict__ parent, PlocScalars *s)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0)
    {
        s->count[0] = count;
        s->made[0] = 0u;
        s->rounds = s->finishRounds = 0u;
    }
    if (p < 2u * count - 1u) parent[p] = kPlocNone; // (a node that is merged gets its parent then; the root keeps this)
    if (p >= count) return;
    const float4 *src = reinterpret_cast<const float4 *>(flat + sorted[p]);
    const float4 a = src[0], b = src[1], d = src[2];
    const float tri[12] = {a.x, a.y, a.z, 0.0f, b.x, b.y, b.z, 0.0f, d.x, d.y, d.z, 0.0f};
    out[p] = ploc_leaf(tri, p);
}

__global__ __launch_bounds__(kBlock) void ploc_search_kernel(
    const PlocCluster *__restrict__ in, const PlocScalars *__restrict__ s, uint32_t parity, uint32_t radius, uint32_t *__restrict__ nearest)
{
    __shared__ PlocCluster tile[kBlock + 2u * kPlocMaxRadius];
    const uint32_t m = s->count[parity];
    const uint32_t base = blockIdx.x * kBlock;
    if (base >= m) return; // (the grid is sized by the last count the host knows; the whole workgroup leaves)
    const int64_t origin = (int64_t)base - (int64_t)radius;
    for (uint32_t t = threadIdx.x; t < kBlock + 2u * radius; t += kBlock)
    {
        const int64_t p = origin + (int64_t)t;
        if (p >= 0 && p < (int64_t)m) tile[t] = in[p];
    }
    __syncthreads();
    const uint32_t i = base + threadIdx.x;
    if (i < m) nearest[i] = ploc_nearest(tile, origin, m, i, radius);
}

__global__ __launch_bounds__(kBlock) void ploc_flags_kernel(
    const uint32_t *__restrict__ nearest, const PlocScalars *__restrict__ s, uint32_t parity, uint32_t bound, uint64_t *__restrict__ flags)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= bound) return;
    flags[i] = i < s->count[parity] ? ploc_flags(nearest, i) : 0ull; // (the scan runs over `bound` items)
}

// what a surviving position hands to the next round; a merged node goes into the tree
__device__ __forceinline__ PlocCluster ploc_survivor(
    const PlocCluster *in, const uint32_t *nearest, uint32_t i, uint64_t flag, uint64_t offset, uint32_t made, uint32_t n,
    uint32_t *__restrict__ left, uint32_t *__restrict__ right, uint32_t *__restrict__ size, uint32_t *__restrict__ parent,
    float *__restrict__ nodeCost)
{
    PlocCluster c = in[i];
    if (flag >> 32)
    {
        const uint32_t k = made + (uint32_t)(offset >> 32);
        const PlocCluster other = in[nearest[i]];
        left[k] = c.node;
        right[k] = other.node;
        parent[c.node] = parent[other.node] = n + k;
        c = ploc_union(c, other);
        c.node = n + k;
        size[k] = c.size;
        nodeCost[k] = ploc_box_cost(c);
    }
    return c;
}

__global__ __launch_bounds__(kBlock) void ploc_scatter_kernel(
    const PlocCluster *__restrict__ in, PlocCluster *__restrict__ out, const uint32_t *__restrict__ nearest,
    const uint64_t *__restrict__ flags, const uint64_t *__restrict__ offsets, PlocScalars *s, uint32_t parity, uint32_t n,
    uint32_t *__restrict__ left, uint32_t *__restrict__ right, uint32_t *__restrict__ size, uint32_t *__restrict__ parent,
    float *__restrict__ nodeCost)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t m = s->count[parity], made = s->made[parity];
    if (i >= m) return;
    const uint64_t flag = flags[i], offset = offsets[i];
    if (i + 1u == m)
    {
        const uint64_t total = offset + flag;
        s->count[parity ^ 1u] = (uint32_t)total;
        s->made[parity ^ 1u] = made + (uint32_t)(total >> 32);
        s->rounds += 1u;
    }
    if (!(flag & 1ull)) return;
    out[(uint32_t)offset] = ploc_survivor(in, nearest, i, flag, offset, made, n, left, right, size, parent, nodeCost);
}

__global__ __launch_bounds__(kT) void ploc_finish_kernel(
    const PlocCluster *__restrict__ in, PlocScalars *s, uint32_t parity, uint32_t radius, uint32_t n, uint32_t *__restrict__ left,
    uint32_t *__restrict__ right, uint32_t *__restrict__ size, uint32_t *__restrict__ parent, float *__restrict__ nodeCost)
{
    using Scan = hipcub::BlockScan<unsigned long long, (int)kT>;
    __shared__ PlocCluster lists[2][kT];
    __shared__ uint32_t nearest[kT];
    __shared__ typename Scan::TempStorage temp;
    const uint32_t i = threadIdx.x;
    uint32_t m = min(s->count[parity], kT), made = s->made[parity], cur = 0, rounds = 0;
    if (i < m) lists[0][i] = in[i];
    __syncthreads();
    while (m > 1u)
    {
        if (i < m) nearest[i] = ploc_nearest(lists[cur], 0, m, i, radius);
        __syncthreads();
        const unsigned long long flag = i < m ? ploc_flags(nearest, i) : 0ull;
        unsigned long long offset, total;
        Scan(temp).ExclusiveSum(flag, offset, total);
        if (flag & 1ull)
            lists[cur ^ 1u][(uint32_t)offset] = ploc_survivor(lists[cur], nearest, i, flag, offset, made, n, left, right, size, parent, nodeCost);
        __syncthreads();
        m = (uint32_t)total;
        made += (uint32_t)(total >> 32);
        cur ^= 1u;
        ++rounds;
    }
    if (i == 0)
    {
        s->rounds += rounds;
        s->finishRounds = rounds;
    }
}

__global__ __launch_bounds__(kBlock) void ploc_ranges_kernel(
    PlocTree tree, const uint32_t *__restrict__ sorted, const float *__restrict__ nodeCost, uint32_t *__restrict__ permutation,
    uint32_t *__restrict__ first, uint32_t *__restrict__ last, uint32_t *__restrict__ split, float *__restrict__ cost)
{
    const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= 2u * tree.n - 1u) return;
    if (node < tree.n)
    {
        permutation[ploc_first(tree, node)] = sorted[node];
        return;
    }
    uint32_t a, b, sp;
    const uint32_t t = ploc_radix_form(tree, node, a, b, sp);
    first[t] = a;
    last[t] = b;
    split[t] = sp;
    cost[t] = nodeCost[node - tree.n];
}

constexpr size_t kAlign = 256;
size_t aligned(size_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }
dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1u) / kBlock); }

int reserve(PlocState &st, uint32_t count)
{
    if (count <= st.capacity && st.block.ptr) return PROSPER_PT_OK;
    const size_t n = (size_t)count + count / 4 + 64;
    size_t scanBytes = 0;
    const uint64_t *in = nullptr;
    uint64_t *out = nullptr;
    PPT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scanBytes, in, out, (int)n));
    const size_t tempBytes = scanBytes + kAlign;
    const size_t parts[] = {n * sizeof(PlocCluster), n * sizeof(PlocCluster), n * 4, n * 8, n * 8, n * 4, n * 4, n * 4, 2 * n * 4, n * 4, n * 4,
                            sizeof(PlocScalars), tempBytes};
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
    st.clusters[0] = reinterpret_cast<PlocCluster *>(take());
    st.clusters[1] = reinterpret_cast<PlocCluster *>(take());
    st.nearest = reinterpret_cast<uint32_t *>(take());
    st.flags = reinterpret_cast<uint64_t *>(take());
    st.offsets = reinterpret_cast<uint64_t *>(take());
    st.left = reinterpret_cast<uint32_t *>(take());
    st.right = reinterpret_cast<uint32_t *>(take());
    st.size = reinterpret_cast<uint32_t *>(take());
    st.parent = reinterpret_cast<uint32_t *>(take());
    st.nodeCost = reinterpret_cast<float *>(take());
    st.cost = reinterpret_cast<float *>(take());
    st.scalars = reinterpret_cast<uint32_t *>(take());
    st.scanTemp = take();
    st.scanTempBytes = tempBytes;
    st.capacity = n;
    return PROSPER_PT_OK;
}

} // namespace

int ploc_binary_tree(
    PlocState &st, const WorldTriangle *flat, const uint32_t *sorted, uint32_t count, uint32_t radius, uint32_t *first, uint32_t *last,
    uint32_t *split, uint32_t *permutation, uint32_t *readback, hipStream_t stream, PlocRounds &out)
{
    if (count < 2u || radius < 1u || radius > kPlocMaxRadius)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "GPU hierarchy build (PLOC): fewer than two triangles, or a radius outside 1 .. 32");
    if (const int rc = reserve(st, count)) return rc;
    PlocScalars *s = reinterpret_cast<PlocScalars *>(st.scalars);
    const dim3 block(kBlock);
    hipLaunchKernelGGL(ploc_init_kernel, grid_for(2u * count - 1u), block, 0, stream, flat, sorted, count, st.clusters[0], st.parent, s);
    PPT_HIP(hipGetLastError());

    // the rounds one workgroup cannot hold: the count stays on the device, the host learns it once per round to size the
    // next round's grid (never too small: a round only removes clusters)
    uint32_t known = count, parity = 0;
    while (known > kT)
    {
        hipLaunchKernelGGL(ploc_search_kernel, grid_for(known), block, 0, stream, st.clusters[parity], s, parity, radius, st.nearest);
        hipLaunchKernelGGL(ploc_flags_kernel, grid_for(known), block, 0, stream, st.nearest, s, parity, known, st.flags);
        size_t tempBytes = st.scanTempBytes;
        PPT_HIP(hipcub::DeviceScan::ExclusiveSum(st.scanTemp, tempBytes, (const uint64_t *)st.flags, st.offsets, (int)known, stream));
        hipLaunchKernelGGL(
            ploc_scatter_kernel, grid_for(known), block, 0, stream, st.clusters[parity], st.clusters[parity ^ 1u], st.nearest, st.flags,
            st.offsets, s, parity, count, st.left, st.right, st.size, st.parent, st.nodeCost);
        PPT_HIP(hipGetLastError());
        parity ^= 1u;
        PPT_HIP(hipMemcpyAsync(readback, &s->count[parity], sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        PPT_HIP(hipStreamSynchronize(stream));
        if (readback[0] == 0u || readback[0] >= known) return fail(PROSPER_PT_ERR_UNSUPPORTED, "GPU hierarchy build (PLOC): a round merged nothing");
        known = readback[0];
    }
    hipLaunchKernelGGL(
        ploc_finish_kernel, dim3(1), dim3(kT), 0, stream, st.clusters[parity], s, parity, radius, count, st.left, st.right, st.size, st.parent,
        st.nodeCost);
    const PlocTree tree{st.left, st.right, st.size, st.parent, count};
    hipLaunchKernelGGL(ploc_ranges_kernel, grid_for(2u * count - 1u), block, 0, stream, tree, sorted, st.nodeCost, permutation, first, last, split, st.cost);
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipMemcpyAsync(readback, &s->rounds, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    PPT_HIP(hipStreamSynchronize(stream));
    out.rounds = readback[0];
    out.finishRounds = readback[1];
    return PROSPER_PT_OK;
}

} // namespace ppt
