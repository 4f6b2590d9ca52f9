// pt_wavefront.hip — wavefront formulation of the path-tracing reference pass (gfx950).
//
// The megakernel of rt/reference/main.rgen:225-299 runs at ~25 % lane utilisation on 64-wide
// waves (measured: SQ_THREAD_CYCLES_VALU / SQ_INSTS_VALU, profiles/): lanes whose ray missed sit
// through the shading of the others, only the lanes that drew a front-facing light traverse the
// shadow ray, and every traversal loop runs as long as its slowest lane.  Here the loop body is cut
// into stage kernels and each stage only ever sees live work:
//
//   generate_extend   camera rays (ray.glsl:15-78) + first traceClosest, sky on a miss
//   shade             evaluateSurface + evaluateDirectLighting (without visibility) +
//                     importanceSampleBounce + roulette (main.rgen:146-223,90-144,269-276)
//   shadow            shadow() any-hit traversal (main.rgen:49-60), adds the direct term
//   extend            traceClosest of the next bounce (main.rgen:62-81), sky on a miss
//   accumulate        running mean over the batch's frames + history (main.rgen:285-298)
//
// Scheduling is per WAVE: a wave owns one fixed segment of path slots (WavefrontBuffers) through
// all bounces and compacts survivors to the front of its segment with __ballot + popcount.  No
// global queue, no atomics, fully coalesced 16-byte-per-lane state traffic, and the memory layout
// (hence every sum) is identical from run to run.  Results are bit-identical to the megakernel:
// every path keeps its own RNG stream and its contributions are added in the reference's order
// (direct of bounce b, then sky of bounce b+1).
#include "pt_kernels.hpp"

#include "pt_device.hpp"
#include "pt_render_common.hpp"
#include "pt_trace_stream.hpp"

// Register budgets (measured on C2/C3, profiles/r01_occupancy_ab.txt): the traversal kernels (generate,
// trace) run at 5 waves/SIMD (<= 96 VGPRs, no spill), the shade kernel at 4 (120 VGPRs; 5 would spill).
// The LDS stack is 16 or 24 entries x 64 lanes x 4 B per wave, deeper entries go to global memory.
#define PPT_SHADE_WPE 4
#ifndef PPT_GEN_WPE
#define PPT_GEN_WPE 5
#endif
#ifndef PPT_TRACE_WPE
#define PPT_TRACE_WPE(stack) 5
#endif

namespace ppt
{

namespace
{

constexpr uint32_t kSlotMask = 0x0FFFFFFFu;

struct SegmentId
{
    uint32_t seg;
    uint32_t base;
    bool valid;
};

// Workgroup -> 4 consecutive segments of this launch's group range; block ids are remapped so that each
// XCD (blocks b, b+8, ...) works on one contiguous range of segments, i.e. one band of the image
// (speed only).
// SCALAR: the wave's index in its workgroup - the same in all its lanes - is read from the first lane, so that the
// segment's number and base are scalars, and with them the part of every record address that they make up
// (wf_generate_extend 1562 -> 1481 VALU instructions and 94 -> 90 VGPRs, wf_shade 3847 -> 3837 and 128 -> 126).  Not in
// wf_trace: with scalar stream lengths the compiler duplicates the scheduler's loops there (2274 -> 2574 instructions)
// and spills.
template <bool SCALAR>
__device__ __forceinline__ SegmentId my_segment(const WavefrontBuffers &w)
{
    const uint32_t groups = w.groupCount;
    const uint32_t perXcd = (groups + 7u) / 8u;
    const uint32_t local = (blockIdx.x % 8u) * perXcd + (blockIdx.x / 8u);
    uint32_t wave = threadIdx.x >> 6;
    if constexpr (SCALAR) wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    const uint32_t seg = (w.groupBase + local) * 4u + wave;
    SegmentId id;
    id.seg = seg;
    id.base = seg * w.segLen;
    id.valid = local < groups && seg < w.nSeg;
    return id;
}

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }

// Exclusive rank of this lane among the lanes whose predicate is set, and the total.
__device__ __forceinline__ uint32_t wave_rank(bool pred, uint32_t &total)
{
    const unsigned long long m = __ballot(pred);
    total = (uint32_t)__builtin_popcountll(m);
    return lanes_below(m);
}

__device__ __forceinline__ f3 xyz(float4 v) { return f3{v.x, v.y, v.z}; }
__device__ __forceinline__ uint32_t asu(float f) { return __builtin_bit_cast(uint32_t, f); }
__device__ __forceinline__ float asf(uint32_t u) { return __builtin_bit_cast(float, u); }

// The path state between stages (ray, throughput, generator, hit and shadow records) is written by one stage and read by
// the next one or two: 3.3 GB per 8-spp step that passes through the L2 and the Infinity Cache once.  PPT_STREAM_NT marks
// those accesses non-temporal (global_load / global_store ... nt), so that they do not push the scene - nodes, triangles,
// shading records, texels: what IS re-read - out of the caches.  (profiles/r04_stream_nt.txt)
#ifndef PPT_STREAM_NT
#define PPT_STREAM_NT 7 // bit 0: loads, bit 1: stores, bit 2: the radiance slots too (round 4: C3 12.95 -> 12.50 ms, others -0 .. 1 %)
#endif
typedef float ppt_f4v __attribute__((ext_vector_type(4)));
typedef uint32_t ppt_u4v __attribute__((ext_vector_type(4)));
typedef uint32_t ppt_u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 sld(const float4 *p)
{
#if PPT_STREAM_NT & 1
    const ppt_f4v v = __builtin_nontemporal_load(reinterpret_cast<const ppt_f4v *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ uint4 sld(const uint4 *p)
{
#if PPT_STREAM_NT & 1
    const ppt_u4v v = __builtin_nontemporal_load(reinterpret_cast<const ppt_u4v *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}
__device__ __forceinline__ uint2 sld(const uint2 *p)
{
#if PPT_STREAM_NT & 1
    const ppt_u2v v = __builtin_nontemporal_load(reinterpret_cast<const ppt_u2v *>(p));
    return make_uint2(v.x, v.y);
#else
    return *p;
#endif
}
__device__ __forceinline__ uint32_t sld(const uint32_t *p)
{
#if PPT_STREAM_NT & 1
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void sst(float4 *p, float4 v)
{
#if PPT_STREAM_NT & 2
    __builtin_nontemporal_store(ppt_f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<ppt_f4v *>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void sst(uint4 *p, uint4 v)
{
#if PPT_STREAM_NT & 2
    __builtin_nontemporal_store(ppt_u4v{v.x, v.y, v.z, v.w}, reinterpret_cast<ppt_u4v *>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void sst(uint2 *p, uint2 v)
{
#if PPT_STREAM_NT & 2
    __builtin_nontemporal_store(ppt_u2v{v.x, v.y}, reinterpret_cast<ppt_u2v *>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void sst(uint32_t *p, uint32_t v)
{
#if PPT_STREAM_NT & 2
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// Record `i` of a workspace array.  Every index is below nSeg * segLen < 2^28 (ensure_wavefront_workspace refuses more) and
// a record has at most 16 bytes, so the byte offset fits 32 bits: written as one, the access is the array's (uniform)
// address in SGPRs plus a 32-bit VGPR offset - one shift per access instead of a 64-bit shift-and-add (and the zero or
// sign extension of the index that feeds it).
template <class T>
__device__ __forceinline__ T *rec(T *base, uint32_t i)
{
    using Byte = std::conditional_t<std::is_const_v<T>, const char, char>;
    return reinterpret_cast<T *>(reinterpret_cast<Byte *>(base) + (uint32_t)(i * (uint32_t)sizeof(T)));
}

// n / d by the terms make_magic_div(d) made (pt_scene.hpp): exact for every n
__device__ __forceinline__ uint32_t magic_div(uint32_t n, MagicDiv m)
{
    const uint32_t t = __umulhi(m.mul, n);
    return (t + ((n - t) >> (m.shifts & 0xFFu))) >> (m.shifts >> 8);
}

struct SlotPixel
{
    uint32_t lx, py, frame;
    bool valid;
};
__device__ __forceinline__ SlotPixel decode_slot(const WavefrontBuffers &w, const RenderParams &p, uint32_t slot)
{
    SlotPixel r;
    r.frame = magic_div(slot >> 6, w.divTiles); // slot / pixelsPadded: pixelsPadded = 64 x tiles
    const uint32_t rem = slot - r.frame * w.pixelsPadded;
    const uint32_t tile = rem >> 6, inTile = rem & 63u;
    const uint32_t ty = magic_div(tile, w.divTilesX);
    r.lx = (tile - ty * w.tilesX) * 8u + (inTile & 7u);
    r.py = ty * 8u + (inTile >> 3);
    r.valid = r.frame < p.frameCount && r.lx < p.localWidth && r.py < p.height;
    return r;
}

// Which (frame, pixel) lane `lane` of batch `q` of a render's camera rays is.  A batch is 64 paths: NOT one 8x8 tile of one
// frame but a block of 64 / g pixels of a tile in g consecutive frames (g = 64 while that many frames remain, then 32,
// 16, ... 1 - a single frame is the 8x8 tile again).  The g camera rays of a pixel differ by their sub-pixel jitter
// only: they walk the same nodes and mostly hit the same triangle, so the lockstep traversal of the batch diverges far
// less than 64 different pixels do (a dense mesh has a triangle every few pixels), and in wf_shade the hits of a pixel
// sit next to each other - one shading record, one texel footprint for all of them.  Slots keep their meaning (frame *
// pixelsPadded + tile * 64 + pixel in tile): only the order the camera rays are generated in changes.
// (FlightHelmet, 8 spp: wf_generate_extend 1249 -> 918 us; C3 1536 -> 1449 and wf_shade 1004 -> 934; C4 6860 -> 6056.)
struct BatchLane
{
    uint32_t slot, lx, py, frame;
    bool valid;
};
#ifndef PPT_BATCH_MAX_FRAMES
#define PPT_BATCH_MAX_FRAMES 64u
#endif
// `q` counts the batches of the tiles [tileBase, tileBase + tiles) only (the whole image: 0, pixelsPadded >> 6); `divTiles`
// are the division terms of `tiles`.
__device__ __forceinline__ BatchLane batch_lane(
    const WavefrontBuffers &w, const RenderParams &p, uint32_t q, uint32_t lane, uint32_t tileBase, uint32_t tiles,
    MagicDiv divTiles)
{
    constexpr uint32_t kMax = PPT_BATCH_MAX_FRAMES, kMaxShift = kMax == 64u ? 6u : (kMax == 32u ? 5u : (kMax == 16u ? 4u : (kMax == 8u ? 3u : 0u)));
    static_assert(kMaxShift != 0u || kMax == 1u, "PPT_BATCH_MAX_FRAMES is 1, 8, 16, 32 or 64");
    const uint32_t frames = p.frameCount;
    uint32_t shift = kMaxShift, firstFrame = 0u, rem = q;
    const uint32_t fullGroups = frames >> kMaxShift;
    const uint32_t fullBatches = (fullGroups << kMaxShift) * tiles; // batches of the groups of kMax frames
    bool inRange = true;
    if (rem < fullBatches)
    {
        const uint32_t group = magic_div(rem >> kMaxShift, divTiles); // rem / (tiles << kMaxShift)
        firstFrame = group << kMaxShift;
        rem -= group * (tiles << kMaxShift);
    }
    else
    {
        rem -= fullBatches;
        firstFrame = fullGroups << kMaxShift;
        inRange = false;
        for (shift = kMaxShift; shift-- != 0u;)
            if (frames & (1u << shift))
            {
                if (rem < (tiles << shift))
                {
                    inRange = true;
                    break;
                }
                rem -= tiles << shift;
                firstFrame += 1u << shift;
            }
        if (!inRange) shift = 0u;
    }
    // 2^shift batches per tile, each a block of 64 >> shift pixels: 8x8, 8x4, 4x4, 4x2, 2x2, 2x1, 1x1
    const uint32_t rank = rem >> shift, part = rem & ((1u << shift) - 1u);
    const uint32_t tile = tileBase + rank;
    const uint32_t wShift = (7u - shift) >> 1, hShift = (6u - shift) >> 1; // log2 of the block's width and height
    const uint32_t pixel = lane & ((64u >> shift) - 1u);
    const uint32_t bx = part & ((8u >> wShift) - 1u), by = part >> (3u - wShift);
    const uint32_t ix = (bx << wShift) + (pixel & ((1u << wShift) - 1u)), iy = (by << hShift) + (pixel >> wShift);
    BatchLane r;
    r.frame = firstFrame + (lane >> (6u - shift));
    const uint32_t ty = magic_div(tile, w.divTilesX);
    r.lx = (tile - ty * w.tilesX) * 8u + ix;
    r.py = ty * 8u + iy;
    r.slot = r.frame * w.pixelsPadded + tile * 64u + iy * 8u + ix;
    r.valid = inRange && rank < tiles && r.frame < frames && r.lx < p.localWidth && r.py < p.height;
    return r;
}

// addBounce (main.rgen:83-88) into the path's radiance slot
__device__ __forceinline__ void add_to_slot(float4 *color, uint32_t slot, uint32_t flags, f3 value, uint32_t bounce)
{
#if PPT_STREAM_NT & 4
    const ppt_f4v cv = __builtin_nontemporal_load(reinterpret_cast<const ppt_f4v *>(rec(color, slot)));
    float4 c = make_float4(cv.x, cv.y, cv.z, cv.w);
#else
    float4 c = *rec(color, slot);
#endif
    f3 acc = f3{c.x, c.y, c.z};
    add_bounce(flags, acc, value, bounce);
#if PPT_STREAM_NT & 4
    __builtin_nontemporal_store(ppt_f4v{acc.x, acc.y, acc.z, 0.0f}, reinterpret_cast<ppt_f4v *>(rec(color, slot)));
#else
    *rec(color, slot) = make_float4(acc.x, acc.y, acc.z, 0.0f);
#endif
}

// The world triangles into LDS, each followed by its guard box (kLdsTriStride float4s per triangle; pt_device.hpp
// guard_box): what box_guard would rebuild for every candidate, worked out once per triangle and workgroup.
__device__ __forceinline__ void stage_triangles_in_lds(const DeviceScene &s, float4 *lt, uint32_t triCount)
{
    const float4 *gt = reinterpret_cast<const float4 *>(s.triangles);
    for (uint32_t i = threadIdx.x; i < triCount; i += blockDim.x)
    {
        const float4 a = gt[i * 3u], b = gt[i * 3u + 1u], c = gt[i * 3u + 2u];
        const GuardBox box = guard_box(xyz(a), xyz(b), xyz(c));
        float4 *to = lt + i * kLdsTriStride;
        to[0] = a;
        to[1] = b;
        to[2] = c;
        to[3] = make_float4(box.lo.x, box.lo.y, box.lo.z, 0.0f);
        to[4] = make_float4(box.hi.x, box.hi.y, box.hi.z, 0.0f);
    }
}

// Copies the BVH nodes into this workgroup's LDS as they are (LdsGeomHalf), and the world triangles.
__device__ __forceinline__ LdsGeomHalf stage_scene_in_lds_half(const DeviceScene &s, float4 *lds, uint32_t nodeCount, uint32_t triCount)
{
    const float4 *gn = reinterpret_cast<const float4 *>(s.nodes);
    for (uint32_t i = threadIdx.x; i < nodeCount * kLdsNodeStrideHalf; i += blockDim.x) lds[i] = gn[i];
    float4 *lt = lds + nodeCount * kLdsNodeStrideHalf;
    stage_triangles_in_lds(s, lt, triCount);
    __syncthreads();
    return LdsGeomHalf{lds, lt};
}

// The BVH nodes - converted to the fp32 image of LdsGeom (pt_device.hpp) - and the world triangles into this workgroup's LDS.
__device__ __forceinline__ LdsGeom stage_scene_in_lds(const DeviceScene &s, float4 *lds, uint32_t nodeCount, uint32_t triCount)
{
    const BvhNode *gn = s.nodes;
    float *lf = reinterpret_cast<float *>(lds);
    // one thread per (node, float of the 36-float image)
    for (uint32_t i = threadIdx.x; i < nodeCount * (kLdsNodeStride * 4u); i += blockDim.x)
    {
        const uint32_t n = i / (kLdsNodeStride * 4u), k = i - n * (kLdsNodeStride * 4u);
        const uint32_t q = k >> 2, c = k & 3u; // float4 index within the image, component
        float v = 0.0f;
        if (q == 0u)
            v = c < 3u ? gn[n].origin[c] : 0.0f;
        else if (q >= 1u && q <= 3u)
            v = half_to_float(gn[n].lo[q - 1u][c]);
        else if (q == 4u)
            v = __builtin_bit_cast(float, gn[n].child[c]);
        else if (q <= 7u)
            v = half_to_float(gn[n].hi[q - 5u][c]);
        lf[i] = v;
    }
    float4 *lt = lds + nodeCount * kLdsNodeStride;
    stage_triangles_in_lds(s, lt, triCount);
    __syncthreads();
    return LdsGeom{lds, lt};
}

} // namespace

// ------------------------------------------------------------------------------------------
// generate + first extend
// ------------------------------------------------------------------------------------------

template <bool COUNT, int STACK, bool LDS_SCENE>
__global__ __launch_bounds__(256, PPT_GEN_WPE) void wf_generate_extend(
    DeviceScene s, RenderParams p, WavefrontBuffers w, uint32_t nodeCount, uint32_t triCount,
    int32_t *__restrict__ stackOverflow, unsigned long long *__restrict__ counters)
{
    __shared__ int32_t ldsStack[STACK * 256];
    __shared__ float4 ldsScene[LDS_SCENE ? kLdsSceneFloat4s : 1];
    LdsGeomHalf lg = {};
    if constexpr (LDS_SCENE) lg = stage_scene_in_lds_half(s, ldsScene, nodeCount, triCount);
    const GlobalGeom gg{s.nodes, s.triangles};
    const SegmentId id = my_segment<true>(w);
    if (!id.valid) return;
    const uint32_t lane = lane_id();
    const TraversalStack stack{(lds_int32 *)ldsStack + (threadIdx.x >> 6) * (STACK * 64u) + lane,
                               stackOverflow + blockIdx.x * 256u + threadIdx.x, (uint32_t)STACK, gridDim.x * 256u, 64u, LDS_SCENE};
    const bool traceRays = p.pc.maxBounces > 0;

    LaneCounters cnt = {};
    uint32_t nHit = 0;
    if (!traceRays)
    {
        // maxBounces == 0: the loop of main.rgen:241-244 never runs, every path is black
        for (uint32_t k = lane; k < w.segLen; k += 64u)
        {
            const SlotPixel sp = decode_slot(w, p, id.base + k);
            if (sp.valid)
            {
                if constexpr (COUNT) cnt.paths++;
                *rec(w.color, id.base + k) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
    else
    {
        // Batch b of segment s is batch number q = b * nSeg + s of the frame's batch sequence (batch_lane): every segment
        // gets batches from all over the image (and all frame groups), so the waves of a launch carry statistically
        // equal work and finish together; consecutive segments still start on neighbouring batches.
        BatchLane bl = {};
        auto fetch = [&](uint32_t k) {
            const uint32_t at = id.base + k; // where the path's records live in this segment
            StreamRay r;
            if (!bl.valid)
            {
                // slot outside the image / batch: a ray that cannot hit anything
                r.o = f3{0.0f, 0.0f, 0.0f};
                r.d = f3{0.0f, 0.0f, 1.0f};
                r.tMin = 0.0f;
                r.tMax = -1.0f;
                r.seed = 0;
                return r;
            }
            PathState st;
            start_path<COUNT>(p, local_to_global_x(p, bl.lx), bl.py, (p.pc.frameIndex + bl.frame) % PROSPER_RT_FRAME_PERIOD,
                              st, cnt);
            if constexpr (COUNT) cnt.closestRays++;
            // a path's state between stages: direction + one word of the generator, the other two words, and for
            // bounce 0 - no throughput record, it is (1, 1, 1) - the radiance slot as one dword (28 B per camera path)
            sst(rec(w.rayB[0], at), make_float4(st.d.x, st.d.y, st.d.z, asf(st.rng.x)));
            sst(rec(w.pathR[0], at), make_uint2(st.rng.y, st.rng.z));
            sst(rec(w.cameraSlot, at), bl.slot);
            r.o = st.o;
            r.d = st.d;
            r.tMin = 0.0f;
            r.tMax = kInf;
            r.seed = pcg(st.rng.x ^ st.rng.z);
            return r;
        };
        auto commit = [&](bool pred, uint32_t k, bool found, const Hit &hit, const f3 &dir) {
            const bool valid = pred && bl.valid;
            if (valid)
            {
                f3 color = f3{0.0f, 0.0f, 0.0f};
                if (!found && (p.pc.flags & PROSPER_PC_FLAG_IBL))
                {
                    if constexpr (COUNT) cnt.skyLookups++;
                    add_bounce(p.pc.flags, color, sample_skybox(s, dir), 0u); // throughput is (1,1,1)
                }
#if PPT_STREAM_NT & 4
                __builtin_nontemporal_store(ppt_f4v{color.x, color.y, color.z, 0.0f}, reinterpret_cast<ppt_f4v *>(rec(w.color, bl.slot)));
#else
                *rec(w.color, bl.slot) = make_float4(color.x, color.y, color.z, 0.0f);
#endif
            }
            const bool isHit = valid && found;
            uint32_t total;
            const uint32_t pos = nHit + wave_rank(isHit, total);
            if (isHit)
            {
                sst(rec(w.hit, id.base + pos),make_uint4(hit.drawInstance, hit.primitive, asu(hit.bary.x), asu(hit.bary.y)));
                sst(rec(w.hitIdx, id.base + pos), k);
            }
            nHit += total;
        };
        // Camera rays of a batch are coherent: 64 of them in lockstep keep ~96 % of the lanes busy on C2, so they skip the
        // stream scheduler and its bookkeeping.  Running them through trace_stream() instead was measured slower on
        // every configuration (profiles/r02_scheduler_experiments.txt: C2 365 -> 572 us, C3 1551 -> 1922, C4 7119 ->
        // 9805, FlightHelmet 1438 -> 1562).
        // ... or, banded (WavefrontBuffers::bandSegments): batch number b * S + j of the batches of ONE band of tiles, S the
        // segments that share the band and j this segment's place among them - the same striding inside the band.
        uint32_t dealStride = w.nSeg, dealFirst = id.seg, tileBase = 0u, tileCount = w.pixelsPadded >> 6;
        MagicDiv divTileCount = w.divTiles;
        if (w.bandSegments != 0u)
        {
            const uint32_t band = id.seg / w.bandSegments;
            const uint32_t firstSeg = band * w.bandSegments;
            dealStride = w.nSeg - firstSeg < w.bandSegments ? w.nSeg - firstSeg : w.bandSegments;
            dealFirst = id.seg - firstSeg;
            tileBase = w.bandTile[band];
            tileCount = w.bandTile[band + 1u] - tileBase;
            divTileCount = w.divBandTiles[band];
        }
        for (uint32_t k0 = 0; k0 < w.segLen; k0 += 64u)
        {
            const uint32_t k = k0 + lane;
            bl = batch_lane(w, p, (k0 >> 6) * dealStride + dealFirst, lane, tileBase, tileCount, divTileCount);
            const StreamRay r = fetch(k);
            Hit hit;
            bool found;
            if constexpr (LDS_SCENE)
                found = trace_in<false, COUNT>(lg, s, r.o, r.d, r.tMin, r.tMax, r.seed, stack, hit, cnt);
            else
                found = trace_in<false, COUNT>(gg, s, r.o, r.d, r.tMin, r.tMax, r.seed, stack, hit, cnt);
            commit(true, k, found, hit, r.d);
        }
    }
    if (lane == 0) w.segHits[id.seg] = nHit;
    flush_counters<COUNT>(cnt, counters);
}

// ------------------------------------------------------------------------------------------
// extend: traceClosest of bounce >= 1
// ------------------------------------------------------------------------------------------

// One wave's extend work: traces the `n` live rays (buffer set `cur`) of its segment `id` and compacts the hits to the
// segment's front; returns their number.
template <bool COUNT, class Geom>
__device__ __forceinline__ uint32_t extend_segment(
    const Geom &g, const DeviceScene &s, const RenderParams &p, const WavefrontBuffers &w, const SegmentId &id, uint32_t n,
    uint32_t bounce, uint32_t cur, const TraversalStack &stack, LaneCounters &cnt)
{
    const float4 *__restrict__ rayA = w.rayA[cur];
    const float4 *__restrict__ rayB = w.rayB[cur];
    uint32_t nHit = 0;
    auto fetch = [&](uint32_t k) {
        const float4 a = sld(rec(rayA, id.base + k));
        const float4 b = sld(rec(rayB, id.base + k));
        if constexpr (COUNT) cnt.closestRays++;
        StreamRay r;
        r.o = xyz(a);
        r.d = xyz(b);
        r.tMin = 0.0f;
        r.tMax = kInf;
        r.seed = asu(a.w);
        return r;
    };
    auto commit = [&](bool pred, uint32_t k, bool found, const Hit &hit, const f3 &dir) {
        if (pred && !found && (p.pc.flags & PROSPER_PC_FLAG_IBL))
        {
            if constexpr (COUNT) cnt.skyLookups++;
            const float4 t = sld(rec(w.pathT[cur], id.base + k));
            add_to_slot(w.color, asu(t.w) & kSlotMask, p.pc.flags, xyz(t) * sample_skybox(s, dir), bounce);
        }
        const bool isHit = pred && found;
        uint32_t total;
        const uint32_t pos = nHit + wave_rank(isHit, total);
        if (isHit)
        {
            sst(rec(w.hit, id.base + pos),make_uint4(hit.drawInstance, hit.primitive, asu(hit.bary.x), asu(hit.bary.y)));
            sst(rec(w.hitIdx, id.base + pos), k);
        }
        nHit += total;
    };
    trace_stream<false, COUNT, true>(g, s, n, 0.0f, stack, cnt, fetch, commit);
    return nHit;
}

// ------------------------------------------------------------------------------------------
// shade
// ------------------------------------------------------------------------------------------

// The small scene tables every hit walks through - draw instances, instance transforms, materials and the
// light lists - staged into LDS per workgroup when they fit: the shade kernel streams ~200 B of path state
// per hit through the 16 KB vector L1, which keeps evicting them otherwise (an L2 round trip per table on the
// dependent chain hit -> instance -> material / transform -> light).
constexpr uint32_t kLdsTableBytes = 16u * 1024u;
__host__ __device__ inline uint32_t shade_table_bytes(const DeviceScene &s, bool withLights)
{
    const uint32_t scene = s.drawInstanceCount * (uint32_t)sizeof(prosper_DrawInstance) +
                           s.modelInstanceCount * (uint32_t)sizeof(prosper_ModelInstanceTransforms) +
                           s.materialCount * (uint32_t)(sizeof(prosper_MaterialData) + sizeof(MaterialPack)) +
                           (uint32_t)sizeof(prosper_DirectionalLightParameters) + 64u;
    const uint32_t lights = s.pointLightCount * (uint32_t)sizeof(prosper_PointLight) + s.spotLightCount * (uint32_t)sizeof(prosper_SpotLight);
    return scene + (withLights ? lights : 0u);
}
// copies `bytes` (a multiple of 4) from global memory to the next 16-byte aligned LDS offset
__device__ __forceinline__ const void *stage_table(uint32_t *lds, uint32_t &offsetWords, const void *src, uint32_t bytes)
{
    offsetWords = (offsetWords + 3u) & ~3u;
    uint32_t *dst = lds + offsetWords;
    const uint32_t words = bytes / 4u;
    const uint32_t *from = static_cast<const uint32_t *>(src);
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) dst[i] = from[i];
    offsetWords += words;
    return dst;
}

// LDS_TABLES: 0 = every table from global memory, 1 = all of them staged in LDS, 2 = all but the light lists (a
// compile-time choice: a pointer that may be either makes every access through it a flat one)
template <bool COUNT, int LDS_TABLES, bool BATCHED_TEXTURES>
__global__ __launch_bounds__(256, PPT_SHADE_WPE) void wf_shade(
    DeviceScene s, RenderParams p, WavefrontBuffers w, uint32_t bounce, uint32_t cur, uint32_t lastBounce,
    unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t ldsTables[LDS_TABLES != 0 ? kLdsTableBytes / 4u : 4u];
    // the direction towards the sun, once per workgroup instead of once per hit that draws light 0 (pt_device.hpp SunInLds)
    __shared__ float ldsSun[4];
    if (threadIdx.x == 0)
    {
        const f3 l = sun_direction(*s.directionalLight);
        ldsSun[0] = l.x;
        ldsSun[1] = l.y;
        ldsSun[2] = l.z;
    }
    const SunInLds sunL{(__attribute__((address_space(3))) const float *)ldsSun};
    if constexpr (LDS_TABLES == 0) __syncthreads();
    if constexpr (LDS_TABLES != 0)
    {
        uint32_t off = 0;
        s.drawInstances = static_cast<const prosper_DrawInstance *>(
            stage_table(ldsTables, off, s.drawInstances, s.drawInstanceCount * (uint32_t)sizeof(prosper_DrawInstance)));
        s.modelInstanceTransforms = static_cast<const prosper_ModelInstanceTransforms *>(stage_table(
            ldsTables, off, s.modelInstanceTransforms, s.modelInstanceCount * (uint32_t)sizeof(prosper_ModelInstanceTransforms)));
        s.materials = static_cast<const prosper_MaterialData *>(
            stage_table(ldsTables, off, s.materials, s.materialCount * (uint32_t)sizeof(prosper_MaterialData)));
        s.materialPacks = static_cast<const MaterialPack *>(
            stage_table(ldsTables, off, s.materialPacks, s.materialCount * (uint32_t)sizeof(MaterialPack)));
        s.directionalLight = static_cast<const prosper_DirectionalLightParameters *>(
            stage_table(ldsTables, off, s.directionalLight, (uint32_t)sizeof(prosper_DirectionalLightParameters)));
        // only the first `count` lights of each list are ever indexed (sample_light); a thousand lights (C4: 40 KB) do not
        // fit beside the rest and stay in global memory - the instance / transform / material chain still comes from LDS
        if constexpr (LDS_TABLES == 1)
        {
            s.pointLights = static_cast<const prosper_PointLightsBuffer *>(
                stage_table(ldsTables, off, s.pointLights, s.pointLightCount * (uint32_t)sizeof(prosper_PointLight)));
            s.spotLights = static_cast<const prosper_SpotLightsBuffer *>(
                stage_table(ldsTables, off, s.spotLights, s.spotLightCount * (uint32_t)sizeof(prosper_SpotLight)));
        }
        __syncthreads();
    }
    const SegmentId id = my_segment<true>(w);
    if (!id.valid) return;
    const uint32_t lane = lane_id();
    const uint32_t nxt = cur ^ 1u;
    const bool debugDraw =
        p.pc.drawType != PROSPER_DRAW_TYPE_DEFAULT && p.pc.drawType != PROSPER_DRAW_TYPE_MESHLET_ID;

    LaneCounters cnt = {};
    const uint32_t n = w.segHits[id.seg];
    uint32_t nShadow = 0, nNext = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += 64u)
    {
        const uint32_t j = j0 + lane;
        bool wantShadow = false, wantNext = false;
        // shadow-ray record
        f3 shP = {}, shL = {}, shC1 = {};
        float shDist = 0.0f;
        uint32_t shSeed = 0, nanMask = 0;
        // next-ray record
        f3 nO = {}, nD = {}, nT = {};
        Rng rng = {};
        uint32_t slot = 0;
        if (j < n)
        {
            const uint32_t i = sld(rec(w.hitIdx, id.base + j));
            const uint4 h = sld(rec(w.hit, id.base + j));
            const float4 b = sld(rec(w.rayB[cur], id.base + i));
            // bounce 0: no throughput record - it is (1, 1, 1) - and the slot comes from the camera paths' own array
            const float4 t = bounce == 0u ? make_float4(1.0f, 1.0f, 1.0f, asf(sld(rec(w.cameraSlot, id.base + i)))) : sld(rec(w.pathT[cur], id.base + i));
            const uint2 r = sld(rec(w.pathR[cur], id.base + i));
            slot = asu(t.w) & kSlotMask;
            rng = Rng{asu(b.w), r.x, r.y};
            const f3 throughput = xyz(t);
            Hit hit;
            hit.drawInstance = h.x;
            hit.primitive = h.y;
            hit.bary = f2{asf(h.z), asf(h.w)};
            hit.t = 0.0f;
            const Surface sf = evaluate_surface<COUNT, BATCHED_TEXTURES>(s, xyz(b), hit, cnt);
            if (debugDraw)
            {
                const f3 c = debug_color(s, p.pc.drawType, hit, sf);
                *rec(w.color, slot) = make_float4(c.x, c.y, c.z, 0.0f); // `color =`, not `+=` (main.rgen:262)
            }
            else
            {
                f3 l, irradiance;
                float d;
                const BrdfTerms bt = brdf_terms(sf); // for the light sample and the bounce sample alike
                if (prepare_direct_lighting<COUNT>(s, sf, throughput, rng, l, d, irradiance, cnt, sunL))
                {
                    if constexpr (COUNT) cnt.shadowRays++;
                    shSeed = pcg(rng.x ^ rng.y);
                    shP = sf.positionWS;
                    shL = l;
                    shDist = d;
                    const f3 brdf = eval_brdf_times_nol(l, sf, bt);
                    shC1 = direct_lighting_value(s, throughput, irradiance, brdf, 1.0f);
                    // what the reference adds when the light is occluded is (t * (irr*0*n)) * brdf:
                    // +-0 unless a factor is non-finite; remember which channels come out NaN
                    const f3 c0 = direct_lighting_value(s, throughput, irradiance, brdf, 0.0f);
                    nanMask = (c0.x != c0.x ? 1u : 0u) | (c0.y != c0.y ? 2u : 0u) | (c0.z != c0.z ? 4u : 0u);
                    // a ray that cannot change the radiance bits is not queued (zero-radiance light,
                    // outside the spot cone, beyond the light's range)
                    wantShadow = shadow_ray_matters(shC1, c0);
                }
                if (!lastBounce)
                {
                    f3 rd;
                    f3 tp = throughput;
                    importance_sample_bounce(sf, bt, rng, tp, rd);
                    bool alive = p.traceDeadPaths || !throughput_is_zero(tp);
                    if (alive && bounce > p.pc.rouletteStartBounce)
                        alive = !(rng.rnd01() < fmax_(0.05f, 1.0f - max3(tp)));
                    if (alive)
                    {
                        wantNext = true;
                        nO = offset_ray(sf.positionWS, sf.normalWS);
                        nD = rd;
                        nT = tp;
                    }
                }
            }
        }
        uint32_t total;
        uint32_t pos = nShadow + wave_rank(wantShadow, total);
        if (wantShadow)
        {
            sst(rec(w.shA, id.base + pos), make_float4(shP.x, shP.y, shP.z, asf(shSeed)));
            sst(rec(w.shB, id.base + pos), make_float4(shL.x, shL.y, shL.z, shDist));
            sst(rec(w.shC, id.base + pos), make_float4(shC1.x, shC1.y, shC1.z, asf(slot | (nanMask << 28))));
        }
        nShadow += total;
        pos = nNext + wave_rank(wantNext, total);
        if (wantNext)
        {
            sst(rec(w.rayA[nxt], id.base + pos), make_float4(nO.x, nO.y, nO.z, asf(pcg(rng.x ^ rng.z))));
            sst(rec(w.rayB[nxt], id.base + pos), make_float4(nD.x, nD.y, nD.z, asf(rng.x)));
            sst(rec(w.pathT[nxt], id.base + pos), make_float4(nT.x, nT.y, nT.z, asf(slot)));
            sst(rec(w.pathR[nxt], id.base + pos), make_uint2(rng.y, rng.z));
        }
        nNext += total;
    }
    if (lane == 0)
    {
        w.segShadow[id.seg] = nShadow;
        w.segRays[id.seg] = nNext;
    }
    flush_counters<COUNT>(cnt, counters);
}

// ------------------------------------------------------------------------------------------
// shadow
// ------------------------------------------------------------------------------------------

// One wave's shadow work: shadow() for the `n` shadow rays shade queued in its segment; adds the direct term of bounce
// `bounce` where the light is visible.
template <bool COUNT, class Geom>
__device__ __forceinline__ void shadow_segment(
    const Geom &g, const DeviceScene &s, const RenderParams &p, const WavefrontBuffers &w, const SegmentId &id, uint32_t n,
    uint32_t bounce, const TraversalStack &stack, LaneCounters &cnt)
{
    auto fetch = [&](uint32_t k) {
        const float4 a = sld(rec(w.shA, id.base + k));
        const float4 b = sld(rec(w.shB, id.base + k));
        StreamRay r;
        r.o = xyz(a);
        r.d = xyz(b);
        r.tMin = 0.1f; // main.rgen:217
        r.tMax = b.w;
        r.seed = asu(a.w);
        return r;
    };
    auto commit = [&](bool pred, uint32_t k, bool occluded, const Hit &, const f3 &) {
        if (pred)
        {
            const float4 c = sld(rec(w.shC, id.base + k));
            const uint32_t packed = asu(c.w);
            const uint32_t nanMask = packed >> 28;
            if (!occluded || nanMask)
            {
                f3 v = xyz(c);
                if (occluded)
                {
                    const float nan = __builtin_nanf("");
                    v = f3{(nanMask & 1u) ? nan : 0.0f, (nanMask & 2u) ? nan : 0.0f, (nanMask & 4u) ? nan : 0.0f};
                }
                add_to_slot(w.color, packed & kSlotMask, p.pc.flags, v, bounce);
            }
        }
    };
    trace_stream<true, COUNT, false>(g, s, n, 0.1f, stack, cnt, fetch, commit); // main.rgen:217
}

// Shadow rays of bounce `bounce` and (unless it was the last bounce) the closest-hit rays of bounce
// `bounce + 1` in ONE launch: both belong to the same wave-owned segment, neither depends on the
// other, and one launch has one tail instead of two.  The reference adds the direct term of bounce b
// before the sky term of bounce b + 1 (main.rgen:266 then :252); both may touch the same radiance
// slot from different lanes of this wave, hence shadow first, a fence, then extend.
template <bool COUNT, int STACK, bool LDS_SCENE>
__global__ __launch_bounds__(256, PPT_TRACE_WPE(STACK)) void wf_trace(
    DeviceScene s, RenderParams p, WavefrontBuffers w, uint32_t bounce, uint32_t nextCur, uint32_t doExtend,
    uint32_t nodeCount, uint32_t triCount, int32_t *__restrict__ stackOverflow,
    unsigned long long *__restrict__ counters)
{
    __shared__ int32_t ldsStack[STACK * 256];
    __shared__ float4 ldsScene[LDS_SCENE ? kLdsSceneFloat4s : 1];
    LdsGeom lg = {};
    if constexpr (LDS_SCENE) lg = stage_scene_in_lds(s, ldsScene, nodeCount, triCount);
    const GlobalGeom gg{s.nodes, s.triangles};
    const SegmentId vid = my_segment<false>(w);
    if (!vid.valid) return;
    const TraversalStack stack{(lds_int32 *)ldsStack + (threadIdx.x >> 6) * (STACK * 64u) + lane_id(),
                               stackOverflow + blockIdx.x * 256u + threadIdx.x, (uint32_t)STACK, gridDim.x * 256u, 64u, LDS_SCENE};
    LaneCounters cnt = {};
    // the stream lengths stay per-lane values (my_segment), the segment's number and base in the record addresses are
    // scalars: the thread index they come from is not kept - or spilled - through the two streams
    const uint32_t nShadow = w.segShadow[vid.seg];
    const uint32_t nRays = doExtend ? w.segRays[vid.seg] : 0u;
    const uint32_t segScalar = (uint32_t)__builtin_amdgcn_readfirstlane((int)vid.seg);
    const SegmentId id{segScalar, (uint32_t)__builtin_amdgcn_readfirstlane((int)vid.base), true};
    if constexpr (LDS_SCENE)
        shadow_segment<COUNT>(lg, s, p, w, id, nShadow, bounce, stack, cnt);
    else
        shadow_segment<COUNT>(gg, s, p, w, id, nShadow, bounce, stack, cnt);
    if (doExtend)
    {
        // same wave, same CU: a workgroup-scope fence (s_waitcnt vmcnt(0)) orders the shadow phase's
        // radiance stores before the extend phase's loads; the vector L1 is write-through
        __threadfence_block();
        uint32_t nHit;
        if constexpr (LDS_SCENE)
            nHit = extend_segment<COUNT>(lg, s, p, w, id, nRays, bounce + 1u, nextCur, stack, cnt);
        else
            nHit = extend_segment<COUNT>(gg, s, p, w, id, nRays, bounce + 1u, nextCur, stack, cnt);
        if (lanes_below(~0ull) == 0u) w.segHits[segScalar] = nHit; // (the wave's first lane)
    }
    flush_counters<COUNT>(cnt, counters);
}

// ------------------------------------------------------------------------------------------
// accumulate: main.rgen:285-298 over the frames of the batch, in order
// ------------------------------------------------------------------------------------------

template <bool COUNT>
__global__ __launch_bounds__(256) void wf_accumulate(
    RenderParams p, WavefrontBuffers w, float4 *__restrict__ hdr, unsigned long long *__restrict__ counters)
{
    const uint32_t rem = blockIdx.x * blockDim.x + threadIdx.x;
    LaneCounters cnt = {};
    if (rem < w.pixelsPadded)
    {
        const SlotPixel sp = decode_slot(w, p, rem);
        if (sp.valid)
        {
            float4 *texel = hdr + (size_t)sp.py * p.localWidth + sp.lx;
            float4 history = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (uint32_t f = 0; f < p.frameCount; ++f)
            {
#if PPT_STREAM_NT & 4
                const ppt_f4v cv = __builtin_nontemporal_load(reinterpret_cast<const ppt_f4v *>(rec(w.color, f * w.pixelsPadded + rem))); // (its last use)
                const float4 c = make_float4(cv.x, cv.y, cv.z, cv.w);
#else
                const float4 c = *rec(w.color, f * w.pixelsPadded + rem);
#endif
                const bool skip = (f == 0 && (p.pc.flags & PROSPER_PC_FLAG_SKIP_HISTORY)) ||
                                  !(p.pc.flags & PROSPER_PC_FLAG_ACCUMULATE);
                if (skip)
                    history = make_float4(c.x, c.y, c.z, 1.0f);
                else
                {
                    if (f == 0) history = *texel;
                    if constexpr (COUNT) cnt.historyReads++;
                    const float hc = history.w + 1.0f;
                const float invHc = 1.0f / hc;
                history = make_float4(
                    __builtin_fmaf(c.x - history.x, invHc, history.x), __builtin_fmaf(c.y - history.y, invHc, history.y),
                    __builtin_fmaf(c.z - history.z, invHc, history.z), hc);
                }
                if constexpr (COUNT) cnt.pixelsWritten++;
            }
            *texel = history;
        }
    }
    flush_counters<COUNT>(cnt, counters);
}

// ------------------------------------------------------------------------------------------
// host-side sequencing
// ------------------------------------------------------------------------------------------

template <bool COUNT, int STACK, bool LDS_SCENE>
static void enqueue_wavefront(
    const DeviceScene &s, const RenderParams &p, unsigned long long *counters, const WavefrontBuffers &w,
    const WavefrontPlan &plan, uint32_t nodeCount, uint32_t triCount, int32_t *stackOverflow, LaunchTimeline *timer,
    hipStream_t stream)
{
    unsigned long long *cGen = counters + kStageGenerate * kCounterCount, *cShade = counters + kStageShade * kCounterCount,
                       *cTrace = counters + kStageTrace * kCounterCount;
    auto mark = [&](uint32_t st) {
        if (timer) timer->mark(st, stream);
    };
    const dim3 grid(((w.groupCount + 7u) / 8u) * 8u), block(256);
    uint32_t bounces = p.pc.maxBounces < PROSPER_RT_MAX_BOUNCES ? p.pc.maxBounces : PROSPER_RT_MAX_BOUNCES;
    const bool debugDraw =
        p.pc.drawType != PROSPER_DRAW_TYPE_DEFAULT && p.pc.drawType != PROSPER_DRAW_TYPE_MESHLET_ID;
    if (debugDraw && bounces > 1) bounces = 1; // every hit ends its path in the first shade

    mark(kStageGenerate);
    hipLaunchKernelGGL(
        (wf_generate_extend<COUNT, STACK, LDS_SCENE>), grid, block, 0, stream, s, p, w, nodeCount, triCount,
        stackOverflow, cGen);
    for (uint32_t b = 0; b < bounces; ++b)
    {
        const uint32_t cur = b & 1u;
        const uint32_t last = (b + 1u == bounces) ? 1u : 0u;
        mark(kStageShade);
        const int ldsTables = !plan.tablesInLds ? 0 : (shade_table_bytes(s, true) <= kLdsTableBytes ? 1 : 2);
        auto shade = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, stream, s, p, w, b, cur, last, cShade); };
        if (s.batchedTextures)
            ldsTables == 1 ? shade(wf_shade<COUNT, 1, true>) : (ldsTables == 2 ? shade(wf_shade<COUNT, 2, true>) : shade(wf_shade<COUNT, 0, true>));
        else
            ldsTables == 1 ? shade(wf_shade<COUNT, 1, false>) : (ldsTables == 2 ? shade(wf_shade<COUNT, 2, false>) : shade(wf_shade<COUNT, 0, false>));
        if (!debugDraw)
        {
            mark(kStageTrace);
            hipLaunchKernelGGL(
                (wf_trace<COUNT, STACK, LDS_SCENE>), grid, block, 0, stream, s, p, w, b, cur ^ 1u, last ? 0u : 1u,
                nodeCount, triCount, stackOverflow, cTrace);
        }
    }
}

uint32_t wavefront_grid_blocks(const WavefrontBuffers &w)
{
    const uint32_t groups = (w.nSeg + 3u) / 4u;
    return ((groups + 7u) / 8u) * 8u + 8u * kMaxChains; // + the per-chain rounding of a split launch
}

uint32_t wavefront_lds_stack_entries(uint32_t stackBound, uint32_t forced)
{
    // test/tuning hook (debug option ldsStackEntries = 16 | 24 | 32): forces a variant (deeper entries then live in
    // the global overflow array, which is always safe, only slower)
    if (forced == 16u || forced == 24u || forced == 32u) return forced;
    // Deeper trees keep 24 entries in LDS and spill the rest to the global overflow array: the 4-wide
    // tree rarely has more than ~2 entries per level in flight, and a 32-entry LDS stack (32 KB per
    // workgroup) costs more in occupancy than the rare overflow access does (C3: 4.41 vs 3.89 ms/launch).
    return stackBound <= 16u ? 16u : 24u;
}

// Which kernel variants a render of this scene takes (also reported by prosper_pt_get_scene_stats, so that a
// test of a variant can assert it is the one that ran).
bool wavefront_shade_tables_in_lds(const DeviceScene &s, bool disabled)
{
    return shade_table_bytes(s, false) <= kLdsTableBytes && !disabled;
}
bool wavefront_scene_in_lds(uint32_t ldsStackEntries, uint32_t stackBound, uint32_t nodeCount, uint32_t triCount, bool disabled)
{
    // (stackBound <= 16: the LDS-scene kernels have no global stack path at all - TraversalStack::ldsOnly)
    return ldsStackEntries == 16u && stackBound <= 16u && nodeCount * kLdsNodeStride + triCount * kLdsTriStride <= kLdsSceneFloat4s && !disabled;
}

// The traversal kernels of a render and the global scratch they index: `overflowEntries` stack entries per lane.
WavefrontPlan wavefront_plan(
    uint32_t stackBound, uint32_t nodeCount, uint32_t triCount, const DeviceScene &s, const WavefrontOptions &opt)
{
    WavefrontPlan plan = {};
    plan.ldsStackEntries = wavefront_lds_stack_entries(stackBound, opt.ldsStackEntries);
    plan.overflowEntries = stackBound > plan.ldsStackEntries ? stackBound - plan.ldsStackEntries : 0u;
    plan.sceneInLds = wavefront_scene_in_lds(plan.ldsStackEntries, stackBound, nodeCount, triCount, opt.noLdsScene);
    plan.tablesInLds = wavefront_shade_tables_in_lds(s, opt.noLdsTables);
    plan.scratchDwordsPerBlock = plan.overflowEntries * 256u;
    return plan;
}

template <bool COUNT>
static void enqueue_for_stack(
    const DeviceScene &s, const RenderParams &p, unsigned long long *counters, const WavefrontBuffers &w,
    const WavefrontPlan &plan, int32_t *stackOverflow, uint32_t nodeCount, uint32_t triCount, LaunchTimeline *timer,
    hipStream_t stream)
{
    // a scene of a few KB is traversed out of LDS
    if (plan.sceneInLds)
        enqueue_wavefront<COUNT, 16, true>(s, p, counters, w, plan, nodeCount, triCount, stackOverflow, timer, stream);
    else if (plan.ldsStackEntries == 16u)
        enqueue_wavefront<COUNT, 16, false>(s, p, counters, w, plan, nodeCount, triCount, stackOverflow, timer, stream);
    else if (plan.ldsStackEntries == 24u)
        enqueue_wavefront<COUNT, 24, false>(s, p, counters, w, plan, nodeCount, triCount, stackOverflow, timer, stream);
    else
        enqueue_wavefront<COUNT, 32, false>(s, p, counters, w, plan, nodeCount, triCount, stackOverflow, timer, stream);
}

void launch_render_wavefront(
    const DeviceScene &s, const RenderParams &p, float4 *hdr, unsigned long long *counters, const WavefrontBuffers &w,
    const WavefrontPlan &plan, int32_t *stackOverflow, uint32_t nodeCount, uint32_t triCount, bool countWork,
    LaunchTimeline *timer, const WavefrontChains &chains, hipStream_t stream)
{
    if (w.nSeg == 0) return;
    static_assert(kTraversalStackDepth == 32, "largest LDS stack variant");
    const uint32_t groups = (w.nSeg + 3u) / 4u;
    // Two chains only pay when each still fills the machine a few times over (>= 1024 workgroups each).
    uint32_t parts = chains.count < kMaxChains ? chains.count : kMaxChains;
    while (parts > 1u && groups < 256u * parts) --parts;
    const bool ownStreams = parts > 1u || chains.detached;
    const uint32_t per = (groups + parts - 1u) / parts;
    // (detached chains - frames in flight - do not fork from the caller's stream: they wait for their slot's previous user)
    const bool forked = parts > 1u && !chains.detached;
    if (forked) (void)chains.fork->record(stream);
    uint32_t blocksBefore = 0;
    for (uint32_t i = 0; i < parts; ++i)
    {
        WavefrontBuffers part = w;
        part.groupBase = i * per;
        part.groupCount = (part.groupBase + per <= groups) ? per : groups - part.groupBase;
        hipStream_t cs = ownStreams ? chains.streams[i] : stream;
        LaunchTimeline *ct = ownStreams ? chains.timers[i] : timer;
        if (forked) (void)chains.fork->wait(cs);
        if (chains.detached && chains.after) (void)hipStreamWaitEvent(cs, chains.after, 0);
        if (ownStreams && chains.scene) (void)hipStreamWaitEvent(cs, chains.scene, 0);
        if (ownStreams && chains.lights) (void)hipStreamWaitEvent(cs, chains.lights, 0);
        if (ownStreams && chains.materials) (void)hipStreamWaitEvent(cs, chains.materials, 0);
        // every chain gets its own region of the stack-overflow array: its kernels index it by their own
        // blockIdx / gridDim (TraversalStack), and the chains run concurrently
        int32_t *ovf = stackOverflow ? stackOverflow + (size_t)blocksBefore * plan.scratchDwordsPerBlock : nullptr;
        if (countWork)
            enqueue_for_stack<true>(s, p, counters, part, plan, ovf, nodeCount, triCount, ct, cs);
        else
            enqueue_for_stack<false>(s, p, counters, part, plan, ovf, nodeCount, triCount, ct, cs);
        blocksBefore += ((part.groupCount + 7u) / 8u) * 8u;
        if (ownStreams)
        {
            if (ct) ct->close(cs);
            (void)chains.join[i]->record(cs);
            (void)chains.join[i]->wait(stream);
        }
    }
    if (timer) timer->mark(kStageAccumulate, stream);
    unsigned long long *cAcc = counters + kStageAccumulate * kCounterCount;
    const dim3 grid((w.pixelsPadded + 255u) / 256u), block(256);
    if (countWork)
        hipLaunchKernelGGL(wf_accumulate<true>, grid, block, 0, stream, p, w, hdr, cAcc);
    else
        hipLaunchKernelGGL(wf_accumulate<false>, grid, block, 0, stream, p, w, hdr, cAcc);
}

} // namespace ppt
