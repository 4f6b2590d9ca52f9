// prosper_pt.cpp — C-ABI of the MI355X path-tracing reference pass (include/prosper_pt/prosper_pt.h).
//
// The context - error string, scene-lifetime device memory, debug options, create / destroy - and the host side of what
// prosper does around `cb.traceRaysKHR` (src/render/RtReference.cpp:161-383): the render, its read-backs, counters and
// timing.  The scene itself is pt_scene_upload.cpp's, its updates pt_scene_updates.cpp's, its hierarchy pt_hierarchy.cpp's.
// There is no CPU fallback: without a usable HIP device every entry point fails with PROSPER_PT_ERR_NO_DEVICE.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pt_animation.hpp"
#include "pt_bvh_build.hpp"
#include "pt_context.hpp"
#include "pt_geometry.hpp"
#include "pt_kernels.hpp"
#include "pt_pass_support.hpp"
#include "pt_scene.hpp"
#include "pt_scene_updates.hpp"
#include "pt_tiling.hpp"

using namespace ppt;

namespace ppt
{
thread_local std::string g_lastErrorStorage;
// set by the worker thread of a mesh build: its scene allocations, so that a build that fails can give them back
thread_local std::vector<void *> *g_allocationLog = nullptr;
int fail(int code, const std::string &msg)
{
    g_lastErrorStorage = msg;
    return code;
}
} // namespace ppt

using RenderSlot = prosper_pt_ctx::RenderSlot;
constexpr uint32_t kStageChains = 4; // unnamed interval of the caller's stream: fork .. join of the chains

namespace ppt
{

int device_alloc(prosper_pt_ctx *ctx, size_t bytes, void **out)
{
    if (bytes == 0) bytes = 16;
    void *p = nullptr;
    PPT_HIP(hipMalloc(&p, bytes));
    if (g_allocationLog) g_allocationLog->push_back(p);
    const std::lock_guard<std::mutex> lock(ctx->allocMutex);
    ctx->sceneAllocations.push_back({p, bytes});
    ctx->sceneBytes += bytes;
    *out = p;
    return PROSPER_PT_OK;
}

// returns a scene allocation early (a texture only its material pack still mirrors, a node array that was outgrown)
void device_free(prosper_pt_ctx *ctx, const void *p)
{
    const std::lock_guard<std::mutex> lock(ctx->allocMutex);
    for (size_t i = 0; i < ctx->sceneAllocations.size(); ++i)
        if (ctx->sceneAllocations[i].ptr == p)
        {
            (void)hipFree(ctx->sceneAllocations[i].ptr);
            ctx->sceneBytes -= ctx->sceneAllocations[i].bytes;
            ctx->sceneAllocations.erase(ctx->sceneAllocations.begin() + (long)i);
            return;
        }
}

int upload(prosper_pt_ctx *ctx, const void *src, size_t bytes, void **out)
{
    const int rc = device_alloc(ctx, bytes, out);
    if (rc != PROSPER_PT_OK) return rc;
    if (bytes) PPT_HIP(hipMemcpy(*out, src, bytes, hipMemcpyHostToDevice));
    return PROSPER_PT_OK;
}

int grow_buffer(DeviceBuffer &buf, GrowWait wait, hipStream_t s, size_t bytes, size_t allocBytes, int fill)
{
    hipError_t e = hipSuccess;
    if (wait == GrowWait::Stream) e = hipStreamSynchronize(s);
    if (wait == GrowWait::Device) e = hipDeviceSynchronize();
    if (buf.ptr)
    {
        const hipError_t f = hipFree(buf.ptr);
        if (e == hipSuccess) e = f;
    }
    buf.ptr = nullptr;
    buf.bytes = 0;
    if (e == hipSuccess) e = hipMalloc(&buf.ptr, allocBytes);
    if (e == hipSuccess && fill >= 0) e = hipMemset(buf.ptr, fill, allocBytes);
    if (e != hipSuccess)
    {
        if (buf.ptr) (void)hipFree(buf.ptr);
        buf.ptr = nullptr;
        return fail(PROSPER_PT_ERR_HIP, std::string("growing a device buffer: ") + hipGetErrorString(e));
    }
    buf.bytes = bytes;
    return PROSPER_PT_OK;
}

} // namespace ppt

namespace
{

WavefrontOptions wavefront_options(const prosper_pt_ctx *ctx)
{
    const prosper_pt_debug_options &d = ctx->debug;
    WavefrontOptions o;
    o.ldsStackEntries = d.ldsStackEntries;
    o.noLdsScene = d.noLdsScene != 0;
    o.noLdsTables = d.noLdsTables != 0;
    return o;
}

} // namespace

namespace ppt
{

int ensure_stack_overflow(prosper_pt_ctx *ctx, RenderSlot &slot, uint32_t ldsEntries, uint32_t gridBlocks, int32_t **out)
{
    const uint32_t bound = ctx->stats.maxDepth;
    *out = nullptr;
    if (bound <= ldsEntries) return PROSPER_PT_OK;
    const size_t bytes = (size_t)(bound - ldsEntries) * 256u * gridBlocks * sizeof(int32_t);
    if (bytes > slot.stackOverflow.bytes)
    {
        // the other slots' renders may be in flight on their own streams
        const int rc = grow_buffer(slot.stackOverflow, GrowWait::Device, nullptr, bytes, bytes);
        if (rc != PROSPER_PT_OK) return rc;
    }
    *out = slot.stackOverflow.as<int32_t>();
    return PROSPER_PT_OK;
}

} // namespace ppt

namespace
{

// Sizes and carves the wavefront workspace for `frames` x (tilesX*tilesY*64) path slots.
int ensure_wavefront_workspace(
    prosper_pt_ctx *ctx, RenderSlot &slot, uint32_t tilesX, uint32_t tilesY, uint32_t frames, bool pipelined, bool banded,
    WavefrontBuffers *out)
{
    const uint64_t pixelsPadded = (uint64_t)tilesX * tilesY * 64u;
    const uint64_t slots = pixelsPadded * frames;
    // One segment per wave.  Segments take their 8x8 tiles strided over the whole batch (wf_generate_extend), so
    // all waves carry statistically equal work and there is nothing to balance dynamically: the best segment
    // count is about one round of resident waves for each of the two launch chains plus a little, ~11 500 segments (swept:
    // profiles/r01_seglen_sweep.txt).  The length is an ODD multiple of 64 slots: at even multiples the waves'
    // concurrent accesses to their segments' records, `segLen * 16` bytes apart, pile onto a few HBM channels.
    // (frames in flight, one chain each: the same total split over the kRenderSlots frames - 3 700)
    // (round 3, small batches re-swept - profiles/r03_seglen_sweep.txt: a 1-spp frame of C2 0.326 -> 0.317 ms at 2560 instead of
    // 3700 segments, FlightHelmet 0.524 -> 0.499, a 1/8 rank share 0.330 -> 0.317, C3 1.826 -> 1.867: 3000)
    uint64_t target = pipelined ? 3000u : 11500u;
    if (ctx->debug.segments >= 64u && ctx->debug.segments <= (1u << 20)) target = ctx->debug.segments; // tuning hook
    uint64_t batches = (slots / target + 32u) / 64u;
    if (batches < 2u) batches = 2u; // small renders: 128-slot segments
    if (batches > 2u && batches % 2u == 0u) batches += 1u;
    // At most 49 batches (3136 slots) per segment.  Re-swept in round 3 (profiles/r03_seglen_sweep.txt; the cap was 33 since
    // round 1): longer per-wave streams keep the later stages' waves fuller - what a sparse image (FlightHelmet: one camera
    // ray in seven hits anything) and expensive, uneven rays (C4's foliage) need - while a dense, texture-heavy scene (C3)
    // prefers short segments, whose waves work on neighbouring tiles.  8 spp, three frames in flight, 33 -> 49 -> 65 batches:
    // FlightHelmet 2.04 -> 1.91 -> 1.87 ms, C4 27.9 -> 27.05 -> 27.15, C2 1.95 -> 1.96 -> 1.94, C3 12.93 -> 13.07 -> 13.14.
    if (batches > 49u) batches = 49u;
    uint64_t segLen = batches * 64u;
    {
        const uint64_t v = ctx->debug.segmentLength; // tuning / test hook
        if (v >= 64u && v <= 8192u && v % 64u == 0u) segLen = v;
    }
    uint64_t nSeg = (slots + segLen - 1u) / segLen;
    // The stride between a segment's tiles is nSeg tiles.  A stride that is nearly a whole number of tile rows
    // would keep a segment in the same few tile columns (correlated work, the balance is gone): add segments
    // until the column step is at least an eighth of a row away from 0.
    if (tilesX >= 16u)
        for (uint32_t tries = 0; tries < tilesX; ++tries)
        {
            const uint64_t cols = (nSeg % ((uint64_t)tilesX * tilesY)) % tilesX;
            if (cols >= tilesX / 8u && tilesX - cols >= tilesX / 8u) break;
            ++nSeg;
        }
    // Banded batches: with a launch that covers all segment groups, XCD x runs the groups [x * perXcd, (x + 1) * perXcd)
    // (pt_wavefront.hip my_segment), i.e. the segments [x * bandSegments, ...).  Each band of segments takes the batches of
    // its own band of tiles - as many tiles as its segments have room for (batches per segment / batches per tile); when
    // rounding leaves a tile without a place, one more round of segments makes room.
    uint32_t bandSegments = 0, bandTile[9] = {};
    if (banded)
    {
        const uint64_t tiles = (uint64_t)tilesX * tilesY, perSegment = segLen / 64u; // batches a segment holds
        for (uint32_t tries = 0; tries < 64u; ++tries)
        {
            const uint64_t groups = (nSeg + 3u) / 4u, perXcd = (groups + 7u) / 8u;
            bandSegments = (uint32_t)(perXcd * 4u);
            uint64_t placed = 0;
            for (uint32_t x = 0; x < 8u; ++x)
            {
                const uint64_t first = (uint64_t)x * bandSegments;
                const uint64_t segs = first >= nSeg ? 0u : std::min<uint64_t>(bandSegments, nSeg - first);
                const uint64_t room = segs * perSegment / frames; // tiles: `frames` batches each
                // what is left, spread evenly over the bands that remain
                const uint64_t want = (tiles - placed + (8u - x) - 1u) / (8u - x);
                bandTile[x] = (uint32_t)placed;
                placed += std::min(room, want);
            }
            bandTile[8] = (uint32_t)placed;
            if (placed >= tiles) break;
            nSeg += 8u;
            bandSegments = 0;
        }
        if (bandSegments == 0) return fail(PROSPER_PT_ERR_UNSUPPORTED, "banded batches: no segment layout covers the image");
    }
    const uint64_t padded = nSeg * segLen;
    // (the kernels address a record as a 32-bit byte offset from its array: 16 B x 2^28 slots)
    if (padded >= (1ull << 28)) return fail(PROSPER_PT_ERR_UNSUPPORTED, "wavefront workspace beyond 2^28 path slots");
    // The arrays, each rounded up to 256 B: laid out from 0 to size the block, then over the block.
    // per slot: 2 x (3 x 16 + 8) B ping-pong state, camera slot 4, hit 16 + idx 4, shadow 48, colour 16; + 3 counters per segment
    WavefrontBuffers w = {};
    auto lay_out = [&](uintptr_t base) {
        uintptr_t cursor = base;
        auto carve = [&](size_t n) {
            void *r = reinterpret_cast<void *>(cursor);
            cursor += (n + 255u) & ~(size_t)255u;
            return r;
        };
        for (int k = 0; k < 2; ++k)
        {
            w.rayA[k] = static_cast<float4 *>(carve(padded * 16u));
            w.rayB[k] = static_cast<float4 *>(carve(padded * 16u));
            w.pathT[k] = static_cast<float4 *>(carve(padded * 16u));
            w.pathR[k] = static_cast<uint2 *>(carve(padded * 8u));
        }
        w.cameraSlot = static_cast<uint32_t *>(carve(padded * 4u));
        w.hit = static_cast<uint4 *>(carve(padded * 16u));
        w.hitIdx = static_cast<uint32_t *>(carve(padded * 4u));
        w.shA = static_cast<float4 *>(carve(padded * 16u));
        w.shB = static_cast<float4 *>(carve(padded * 16u));
        w.shC = static_cast<float4 *>(carve(padded * 16u));
        w.color = static_cast<float4 *>(carve(padded * 16u));
        w.segRays = static_cast<uint32_t *>(carve(nSeg * 4u));
        w.segHits = static_cast<uint32_t *>(carve(nSeg * 4u));
        w.segShadow = static_cast<uint32_t *>(carve(nSeg * 4u));
        return (size_t)(cursor - base);
    };
    const size_t bytes = lay_out(0);
    if (bytes > slot.wfBlock.bytes)
    {
        // the other slot's render may be in flight on its own streams
        const int rc = grow_buffer(slot.wfBlock, GrowWait::Device, nullptr, bytes, bytes);
        if (rc != PROSPER_PT_OK) return rc;
    }
    lay_out(reinterpret_cast<uintptr_t>(slot.wfBlock.ptr));
    w.segLen = (uint32_t)segLen;
    w.nSeg = (uint32_t)nSeg;
    w.pixelsPadded = (uint32_t)pixelsPadded;
    w.tilesX = tilesX;
    w.tilesY = tilesY;
    w.bandSegments = bandSegments;
    for (uint32_t x = 0; x < 9u; ++x) w.bandTile[x] = bandTile[x];
    w.divTilesX = make_magic_div(tilesX);
    w.divTiles = make_magic_div(tilesX * tilesY);
    for (uint32_t x = 0; x < 8u; ++x) w.divBandTiles[x] = make_magic_div(bandTile[x + 1u] - bandTile[x]);
    *out = w;
    return PROSPER_PT_OK;
}

uint32_t compute_local_width(uint32_t width, const prosper_pt_tile_desc *tile)
{
    if (!tile || tile->stripeCount <= 1 || tile->stripeWidth == 0) return width;
    uint32_t n = 0;
    for (uint32_t x = 0; x < width; x += tile->stripeWidth)
    {
        if ((x / tile->stripeWidth) % tile->stripeCount == tile->stripeIndex)
            n += (x + tile->stripeWidth <= width) ? tile->stripeWidth : (width - x);
    }
    return n;
}

// ---- debug options: validation, and the one opt-in reading of the environment (prosper_pt_create) ----

int check_debug_options(const prosper_pt_debug_options &o)
{
    // the reserved fields (prosper_pt.h): the removed experiments
    if (o.poolVariant || o.rawRecords || o.tileOrder || o.hipGraph || o.pipelinedChains || o.mergeLimit)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "debug options: poolVariant, rawRecords, tileOrder, hipGraph, pipelinedChains and mergeLimit are reserved and must be 0");
    if (o.ldsStackEntries != 0u && o.ldsStackEntries != 16u && o.ldsStackEntries != 24u && o.ldsStackEntries != 32u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "debug options: ldsStackEntries is 0, 16, 24 or 32");
    if (o.segmentLength != 0u && (o.segmentLength < 64u || o.segmentLength > 8192u || o.segmentLength % 64u != 0u))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "debug options: segmentLength is a multiple of 64 in [64, 8192]");
    if (o.chains > kMaxChains) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "debug options: at most three launch chains");
    if (o.leafSize > 8u || o.alphaCellShift > 15 || o.nodeOrder > 2)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "debug options: a value is out of range");
    if (!(o.sahTraversalCost >= 0.0f) || !(o.boxPad >= 0.0f) || !(o.rebuildCostRatio >= 0.0f))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "debug options: a coefficient is negative or NaN");
    return PROSPER_PT_OK;
}

// name -> field, for the "name=value,name=value" form of the environment gate
struct DebugField
{
    const char *name;
    size_t offset;
    char kind; // 'u' uint32, 'i' int32, 'f' float
};
#define PPT_FIELD(member, kind) {#member, offsetof(prosper_pt_debug_options, member), kind}
const DebugField kDebugFields[] = {
    PPT_FIELD(batchedTextures, 'i'), PPT_FIELD(widePacks, 'i'), PPT_FIELD(alphaCellShift, 'i'), PPT_FIELD(noTexturePacks, 'u'),
    PPT_FIELD(noAlphaBounds, 'u'), PPT_FIELD(noUploadRefit, 'u'), PPT_FIELD(flatBvh, 'u'), PPT_FIELD(sahTraversalCost, 'f'),
    PPT_FIELD(boxPad, 'f'), PPT_FIELD(leafSize, 'u'), PPT_FIELD(buildThreads, 'u'), PPT_FIELD(topEntries, 'u'),
    PPT_FIELD(nodeOrder, 'i'), PPT_FIELD(childOrder, 'i'), PPT_FIELD(buildTiming, 'u'), PPT_FIELD(segments, 'u'),
    PPT_FIELD(segmentLength, 'u'), PPT_FIELD(chains, 'u'), PPT_FIELD(ldsStackEntries, 'u'), PPT_FIELD(noLdsScene, 'u'),
    PPT_FIELD(noLdsTables, 'u'), PPT_FIELD(traceDeadPaths, 'u'), PPT_FIELD(bandedBatches, 'i'), PPT_FIELD(rebuildCostRatio, 'f'), PPT_FIELD(alwaysRebuild, 'u'),
    PPT_FIELD(failNextUpdate, 'u'), PPT_FIELD(poolVariant, 'u'), PPT_FIELD(rawRecords, 'u'), PPT_FIELD(tileOrder, 'u'),
    PPT_FIELD(hipGraph, 'u'), PPT_FIELD(pipelinedChains, 'u'), PPT_FIELD(mergeLimit, 'u'),
};
#undef PPT_FIELD

bool parse_debug_options(const char *text, prosper_pt_debug_options *out, std::string *err)
{
    std::string rest = text ? text : "";
    while (!rest.empty())
    {
        const size_t comma = rest.find(',');
        const std::string item = rest.substr(0, comma);
        rest = comma == std::string::npos ? std::string() : rest.substr(comma + 1);
        if (item.empty()) continue;
        const size_t eq = item.find('=');
        const std::string name = item.substr(0, eq), value = eq == std::string::npos ? std::string("1") : item.substr(eq + 1);
        const DebugField *field = nullptr;
        for (const DebugField &f : kDebugFields)
            if (name == f.name) field = &f;
        if (!field)
        {
            *err = "debug options: unknown option '" + name + "'";
            return false;
        }
        char *end = nullptr;
        uint8_t *at = reinterpret_cast<uint8_t *>(out) + field->offset;
        if (field->kind == 'f')
        {
            const float v = std::strtof(value.c_str(), &end);
            std::memcpy(at, &v, sizeof(v));
        }
        else if (field->kind == 'i')
        {
            const int32_t v = (int32_t)std::strtol(value.c_str(), &end, 10);
            std::memcpy(at, &v, sizeof(v));
        }
        else
        {
            const uint32_t v = (uint32_t)std::strtoul(value.c_str(), &end, 10);
            std::memcpy(at, &v, sizeof(v));
        }
        if (end == value.c_str() || *end != '\0')
        {
            *err = "debug options: '" + value + "' is not a value for '" + name + "'";
            return false;
        }
    }
    return true;
}

// false with the message in *err and the error code in *code (the reserved fields fail as through
// prosper_pt_set_debug_options, everything else as an invalid argument)
bool debug_options_from_environment(prosper_pt_debug_options *out, std::string *err, int *code)
{
    const char *gate = std::getenv("PROSPER_PT_DEBUG");
    if (!gate || std::strcmp(gate, "1") != 0) return true;
    const char *text = std::getenv("PROSPER_PT_DEBUG_OPTIONS");
    if (!text) return true;
    *code = PROSPER_PT_ERR_INVALID_ARGUMENT;
    if (!parse_debug_options(text, out, err)) return false;
    if ((*code = check_debug_options(*out)) != PROSPER_PT_OK)
    {
        *err = ppt::g_lastErrorStorage;
        return false;
    }
    return true;
}

} // namespace

extern "C" {

const char *prosper_pt_last_error(void) { return ppt::g_lastErrorStorage.c_str(); }
uint32_t prosper_pt_abi_version(void) { return PROSPER_PT_ABI_VERSION; }

uint32_t prosper_pt_has_experiments(void) { return 0u; }

void prosper_pt_debug_magic_divisor(uint32_t divisor, uint32_t *mul, uint32_t *shifts)
{
    const ppt::MagicDiv m = ppt::make_magic_div(divisor);
    if (mul) *mul = m.mul;
    if (shifts) *shifts = m.shifts;
}

void prosper_pt_debug_options_default(prosper_pt_debug_options *out)
{
    if (!out) return;
    *out = prosper_pt_debug_options{};
    out->struct_size = (uint32_t)sizeof(prosper_pt_debug_options);
    out->batchedTextures = -1;
    out->widePacks = -1;
    out->alphaCellShift = -1;
    out->nodeOrder = -1;
    out->childOrder = -1;
    out->bandedBatches = -1;
}

int prosper_pt_set_debug_options(prosper_pt_ctx *ctx, const prosper_pt_debug_options *options)
{
    if (!ctx || !options) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_debug_options: null argument");
    if (options->struct_size != sizeof(prosper_pt_debug_options))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_debug_options: struct_size mismatch");
    const int rc = check_debug_options(*options);
    if (rc != PROSPER_PT_OK) return rc;
    ctx->debug = *options;
    return PROSPER_PT_OK;
}

int prosper_pt_get_debug_options(prosper_pt_ctx *ctx, prosper_pt_debug_options *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_debug_options: null argument");
    *out = ctx->debug;
    return PROSPER_PT_OK;
}

} // extern "C"

namespace
{

// What a context owns from its creation on: the timed events of its renders, the work streams, the work counters, the
// passes' state.
int create_context_resources(prosper_pt_ctx *ctx)
{
    int rc;
    if ((rc = ctx->timeline.create())) return rc;
    for (Stream &ws : ctx->workStreams)
        if ((rc = ws.create())) return rc;
    for (RenderSlot &slot : ctx->slots)
        for (LaunchTimeline &chain : slot.chains)
            if ((rc = chain.create())) return rc;
    // Every work stream is used once here, so that the device's four hardware queues go to the caller's stream and these
    // three, in this order: a stream that comes into use later (the two of prosper_pt_update_meshes, made at first need)
    // then SHARES a queue.  Streams that claim queues before the work streams do leave two of those sharing one for the
    // life of the context: 4 % on FlightHelmet, 2 % on S-sponza-class, 60 % on a 256 x 256 frame (profiles/r04_mesh_streams.txt).
    for (Stream &ws : ctx->workStreams)
    {
        if ((rc = ctx->chainFork.record(ws.get()))) return rc;
        PPT_HIP(hipStreamSynchronize(ws.get()));
    }
    bool made = true;
    for (const PassModule *m : kPassModules) made = made && m->create(ctx);
    if (!made || !create_animation_state(ctx)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    const size_t counterBytes = kStageCount * kCounterCount * sizeof(unsigned long long);
    return grow_buffer(ctx->counters, GrowWait::None, nullptr, counterBytes, counterBytes, 0);
}

} // namespace

extern "C" {

int prosper_pt_create(const prosper_pt_device_desc *desc, prosper_pt_ctx **out_ctx)
{
    if (!desc || !out_ctx || desc->struct_size != sizeof(prosper_pt_device_desc))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_create: bad descriptor");
    *out_ctx = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PROSPER_PT_ERR_NO_DEVICE, "no HIP device is visible (this pass has no CPU fallback)");
    if (desc->device_ordinal < 0 || desc->device_ordinal >= count)
        return fail(PROSPER_PT_ERR_NO_DEVICE, "device ordinal out of range");
    PPT_HIP(hipSetDevice(desc->device_ordinal));
    hipDeviceProp_t prop;
    PPT_HIP(hipGetDeviceProperties(&prop, desc->device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PROSPER_PT_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only");
    if (desc->flags & PROSPER_PT_CREATE_PERSISTENT)
        return fail(PROSPER_PT_ERR_UNSUPPORTED, "PROSPER_PT_CREATE_PERSISTENT is reserved: the persistent pipeline was removed");
    prosper_pt_ctx *ctx = new (std::nothrow) prosper_pt_ctx();
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "out of host memory");
    ctx->device = desc->device_ordinal;
    ctx->flags = desc->flags;
    prosper_pt_debug_options_default(&ctx->debug);
    {
        // the ONE place the library looks at the environment, and only when asked to (prosper_pt.h, debug options)
        std::string err;
        int code = PROSPER_PT_OK;
        if (!debug_options_from_environment(&ctx->debug, &err, &code))
        {
            delete ctx;
            return fail(code, err);
        }
    }
    if (create_context_resources(ctx) != PROSPER_PT_OK)
    {
        prosper_pt_destroy(ctx);
        return fail(PROSPER_PT_ERR_HIP, "context allocation failed");
    }
    *out_ctx = ctx;
    return PROSPER_PT_OK;
}

void prosper_pt_destroy(prosper_pt_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    discard_mesh_build(ctx); // (a worker may still be launching)
    (void)hipDeviceSynchronize();
    destroy_tiling(ctx);
    free_scene(ctx);
    for (const PassModule *m : kPassModules) m->destroy(ctx);
    destroy_animation_state(ctx);
    delete ctx->lbvh;
    delete ctx->lbvhWorker;
    delete ctx; // (its events, streams and DeviceBuffers with it: the device is set and idle)
}

} // extern "C"

namespace ppt
{

// rt/ray.glsl:21-35 and scene/camera.glsl:46-51 read these parts of CameraUniforms
void set_camera_ray_params(RenderParams &p, const prosper_CameraUniforms *camera)
{
    p.eye[0] = camera->eye.x;
    p.eye[1] = camera->eye.y;
    p.eye[2] = camera->eye.z;
    const prosper_mat4 &w2c = camera->worldToCamera;
    p.right[0] = w2c.col[0].x; p.right[1] = w2c.col[1].x; p.right[2] = w2c.col[2].x;
    p.up[0] = w2c.col[0].y; p.up[1] = w2c.col[1].y; p.up[2] = w2c.col[2].y;
    p.fwd[0] = -w2c.col[0].z; p.fwd[1] = -w2c.col[1].z; p.fwd[2] = -w2c.col[2].z;
    {
        // volatile: keep the compiler from folding the two divisions into anything but IEEE fp32 divides
        volatile float c00 = camera->cameraToClip.col[0].x, c11 = camera->cameraToClip.col[1].y;
        p.aspect = c11 / c00;
        p.tanHalfFovY = 1.0f / c11;
    }
    std::memcpy(p.cameraToWorld, &camera->cameraToWorld, 64);
}

int prepare_hdr(prosper_pt_ctx *ctx, uint32_t width, uint32_t height, const prosper_pt_tile_desc *tile, hipStream_t s)
{
    const bool tiled = tile && tile->stripeCount > 1 && tile->stripeWidth > 0;
    const uint32_t localWidth = compute_local_width(width, tile);
    const size_t bytes = (size_t)localWidth * height * sizeof(float4);
    if (ctx->externalHdr)
    {
        if (ctx->externalHdrBytes < bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "caller-owned output buffer is too small");
        ctx->hdr = static_cast<float4 *>(ctx->externalHdr);
    }
    else
    {
        if (ctx->ownedHdr.bytes < bytes || !ctx->ownedHdr.ptr)
        {
            const int rc = grow_buffer(ctx->ownedHdr, GrowWait::Stream, s, bytes, bytes ? bytes : 16, 0);
            if (rc != PROSPER_PT_OK) return rc;
        }
        ctx->hdr = ctx->ownedHdr.as<float4>();
    }
    ctx->localWidth = localWidth;
    ctx->height = height;
    ctx->lastWidth = width;
    ctx->stripeWidth = tiled ? tile->stripeWidth : 0;
    ctx->stripeIndex = tiled ? tile->stripeIndex : 0;
    ctx->stripeCount = tiled ? tile->stripeCount : 1;
    // a gather of this tile may still be in flight on the communicator's stream (prosper_pt_gather_tiles): the
    // accumulate kernel, which writes the tile, is enqueued on `s` and must come after it; detached path stages
    // (PROSPER_PT_RENDER_PIPELINED) do not wait for `s` and overlap the gather
    wait_for_gather_before_writing_tile(ctx, s);
    return PROSPER_PT_OK;
}

} // namespace ppt

extern "C" {

int prosper_pt_get_scene_stats(prosper_pt_ctx *ctx, prosper_pt_scene_stats *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_scene_stats: null argument");
    if (!ctx->haveScene) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    *out = ctx->stats;
    // the variants depend on the context's debug options at launch time: report what a render started now would take
    const WavefrontPlan plan = wavefront_plan(
        ctx->stats.maxDepth, (uint32_t)ctx->stats.nodeCount, (uint32_t)ctx->stats.triangleCount, ctx->scene, wavefront_options(ctx));
    const uint32_t ldsEntries = plan.ldsStackEntries;
    out->variantFlags =
        (plan.sceneInLds ? PROSPER_PT_VARIANT_LDS_SCENE : 0u) | (plan.tablesInLds ? PROSPER_PT_VARIANT_LDS_TABLES : 0u) |
        (ctx->scene.batchedTextures ? PROSPER_PT_VARIANT_BATCHED_TEXTURES : 0u) |
        (ctx->packedMaterials ? PROSPER_PT_VARIANT_TEXTURE_PACKS : 0u) |
        (ldsEntries << PROSPER_PT_VARIANT_STACK_SHIFT);
    return PROSPER_PT_OK;
}

int prosper_pt_set_output_buffer(prosper_pt_ctx *ctx, void *device_rgba32f, size_t byte_size)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_output_buffer: null context");
    if (device_rgba32f && (reinterpret_cast<uintptr_t>(device_rgba32f) & 15u))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "output buffer must be 16-byte aligned");
    ctx->externalHdr = device_rgba32f;
    ctx->externalHdrBytes = device_rgba32f ? byte_size : 0;
    return PROSPER_PT_OK;
}

} // extern "C"

namespace
{

// The wavefront pipeline's render: all frames of the batch are in flight together, in chunks that keep the workspace
// under kMaxWavefrontSlots path slots, on render slot `slotIndex`.  `tp`: the caller's-stream timeline of a timed render.
int render_wavefront(
    prosper_pt_ctx *ctx, const RenderParams &p, bool countWork, bool pipelined, uint32_t slotIndex, LaunchTimeline *tp,
    hipStream_t s)
{
    const uint32_t tilesX = (p.localWidth + 7u) / 8u, tilesY = (p.height + 7u) / 8u;
    const uint64_t pixelsPadded = (uint64_t)tilesX * tilesY * 64u;
    constexpr uint64_t kMaxWavefrontSlots = 64ull << 20;
    if (pixelsPadded > kMaxWavefrontSlots) return fail(PROSPER_PT_ERR_UNSUPPORTED, "image too large for the wavefront workspace");
    uint32_t framesPerChunk = (uint32_t)(kMaxWavefrontSlots / pixelsPadded);
    if (framesPerChunk > p.frameCount) framesPerChunk = p.frameCount;
    RenderSlot &slot = ctx->slots[slotIndex];
    ctx->lastSlot = slotIndex;
    WavefrontChains chains;
    chains.count = (pipelined || (ctx->flags & PROSPER_PT_CREATE_SINGLE_CHAIN)) ? 1u : 2u;
    if (!pipelined && ctx->debug.chains >= 1u && ctx->debug.chains <= kMaxChains) chains.count = ctx->debug.chains; // tuning hook (in-order mode)
    chains.detached = pipelined;
    chains.fork = &ctx->chainFork;
    for (uint32_t i = 0; i < kMaxChains; ++i)
    {
        chains.streams[i] = ctx->workStreams[pipelined ? slotIndex : i].get();
        chains.join[i] = &slot.chainJoin[i];
        // (one running timeline per chain over all chunks of the render)
        slot.chains[i].begin();
        chains.timers[i] = tp ? &slot.chains[i] : nullptr;
    }
    for (uint32_t f0 = 0; f0 < p.frameCount; f0 += framesPerChunk)
    {
        const uint32_t frames = (p.frameCount - f0 < framesPerChunk) ? p.frameCount - f0 : framesPerChunk;
        WavefrontBuffers w = {};
        // Banded batches (debug option bandedBatches = 1; round 4, profiles/r04_banded_batches.txt): every XCD's segments take
        // the camera-ray batches of one band of the image, so that the paths an XCD traces START in one part of the scene.
        // Measured and NOT a default: on S-sponza-class wf_trace's FETCH_SIZE moves by 3 % (2.249 -> 2.184 GB per launch) -
        // three of its four launches trace bounce rays and sun shadows that cross the whole hall wherever they start -
        // while the bands' unequal costs bind the step to the slowest XCD: C3 13.0 -> 13.6 ms, C4 27.2 -> 30.7,
        // FlightHelmet (a band of sky is nearly free) 1.88 -> 2.48.
        const bool banded = ctx->debug.bandedBatches > 0;
        const int rc = ensure_wavefront_workspace(ctx, slot, tilesX, tilesY, frames, pipelined, banded, &w);
        if (rc != PROSPER_PT_OK) return rc;
        RenderParams pp = p;
        pp.frameCount = frames;
        pp.pc.frameIndex = (p.pc.frameIndex + f0) % PROSPER_RT_FRAME_PERIOD;
        if (f0 > 0) pp.pc.flags &= ~(uint32_t)PROSPER_PC_FLAG_SKIP_HISTORY;
        const WavefrontPlan plan = wavefront_plan(
            ctx->stats.maxDepth, (uint32_t)ctx->stats.nodeCount, (uint32_t)ctx->stats.triangleCount, ctx->scene, wavefront_options(ctx));
        int32_t *ovf = nullptr;
        const int orc = ensure_stack_overflow(ctx, slot, plan.ldsStackEntries, wavefront_grid_blocks(w), &ovf);
        if (orc != PROSPER_PT_OK) return orc;
        // the slot's previous user (a render of two calls ago, or the previous chunk of this one) must be done
        // with the workspace: detached chains wait for that on their own stream, the others on the caller's
        chains.after = slot.free.event();
        chains.scene = ctx->accel ? ctx->accel->sceneDone.event() : nullptr;
        chains.lights = ctx->lights ? ctx->lights->ready.event() : nullptr;
        chains.materials = ctx->materialState ? ctx->materialState->ready.event() : nullptr;
        if (!pipelined) wait_for_slot(slot, s);
        if (tp) tp->mark(kStageChains, s);
        launch_render_wavefront(
            ctx->scene, pp, ctx->hdr, ctx->counters.as<unsigned long long>(), w, plan, ovf, (uint32_t)ctx->stats.nodeCount,
            (uint32_t)ctx->stats.triangleCount, countWork, tp, chains, s);
        release_slot(slot, s);
    }
    if (tp) ctx->timedSlot = slotIndex;
    return PROSPER_PT_OK;
}

int read_stage_counters(prosper_pt_ctx *ctx, unsigned long long host[kStageCount * kCounterCount], void *stream)
{
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(host, ctx->counters.ptr, kStageCount * kCounterCount * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

} // namespace

extern "C" {

int prosper_pt_render_frames(
    prosper_pt_ctx *ctx, const prosper_ReferencePC *pc, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_tile_desc *tile, uint32_t frame_count, uint32_t render_flags, void *stream)
{
    if (!ctx || !pc || !camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_render: null argument");
    // (streamed-in meshes whose geometry a worker has finished meanwhile are the scene from this render on; a staged
    // update gets its chance below)
    if (const int crc = check_scene(ctx, "prosper_pt_render")) return crc;
    if (width == 0 || height == 0 || frame_count == 0)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_render: empty extent or frame count");
    if (pc->drawType >= PROSPER_DRAW_TYPE_COUNT) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "drawType out of range");
    const bool tiled = tile && tile->stripeCount > 1 && tile->stripeWidth > 0;
    if (tiled && tile->stripeIndex >= tile->stripeCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "tile stripeIndex >= stripeCount");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);

    const int hrc = prepare_hdr(ctx, width, height, tile, s);
    if (hrc != PROSPER_PT_OK) return hrc;
    const uint32_t localWidth = ctx->localWidth;

    RenderParams p = {};
    p.pc = *pc;
    set_camera_ray_params(p, camera);
    p.width = width;
    p.height = height;
    p.stripeWidth = tiled ? tile->stripeWidth : 0;
    p.stripeIndex = tiled ? tile->stripeIndex : 0;
    p.stripeCount = tiled ? tile->stripeCount : 1;
    p.localWidth = localWidth;
    p.frameCount = frame_count;
    p.traceDeadPaths = ctx->debug.traceDeadPaths ? 1u : 0u;

    if (localWidth == 0) return PROSPER_PT_OK;
    const bool countWork = (render_flags & PROSPER_PT_RENDER_COUNT_WORK) != 0;
    LaunchTimeline *tp = ctx->kernelTiming ? &ctx->timeline : nullptr;
    // Frames in flight.  Default: the chains fork from the caller's stream, i.e. after everything enqueued on
    // it so far, and use slot 0.  PROSPER_PT_RENDER_PIPELINED: the path stages (generate / shade / trace) of
    // this render run as ONE chain on the next slot's stream and wait only for that slot's previous render,
    // so they overlap the previous render's remaining work - a 2 M-path batch alone fills 55 % of the GPU,
    // two of them 80 % (profiles/r01_pipelined.txt).  The accumulate kernel stays on the caller's stream, in
    // order: history reads, output writes and everything the caller enqueues later see finished frames.
    const bool pipelined = !(ctx->flags & PROSPER_PT_CREATE_MEGAKERNEL) && (render_flags & PROSPER_PT_RENDER_PIPELINED) != 0 && !countWork;
    const uint32_t slotIndex = pipelined ? (ctx->lastSlot + 1u) % prosper_pt_ctx::kRenderSlots : 0u;
    // a staged prosper_pt_update_transforms runs now, on the stream this render's path stages use: a pipelined render's own
    // chain (beside the frames in flight, which keep reading their scene version), else the caller's stream
    if (const int frc = flush_scene_updates(ctx, pipelined ? ctx->workStreams[slotIndex].get() : s, s)) return frc;
    if (tp) tp->begin();
    if (ctx->flags & PROSPER_PT_CREATE_MEGAKERNEL)
    {
        int32_t *ovf = nullptr;
        const int orc = ensure_stack_overflow(ctx, ctx->slots[0], kTraversalStackDepth, megakernel_grid_blocks(p), &ovf);
        if (orc != PROSPER_PT_OK) return orc;
        wait_for_slot(ctx->slots[0], s);
        if (tp) tp->mark(kStageGenerate, s);
        launch_render_megakernel(ctx->scene, p, ctx->hdr, ctx->counters.as<unsigned long long>(), ovf, countWork, s);
        release_slot(ctx->slots[0], s);
    }
    else if (const int wrc = render_wavefront(ctx, p, countWork, pipelined, slotIndex, tp, s))
        return wrc;
    PPT_HIP(hipGetLastError());
    {
        const int mrc = mark_versions_read(ctx, s);
        if (mrc != PROSPER_PT_OK) return mrc;
    }
    if (tp)
    {
        tp->close(s);
        ctx->timingValid = true;
    }
    return PROSPER_PT_OK;
}

int prosper_pt_render(
    prosper_pt_ctx *ctx, const prosper_ReferencePC *pc, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_tile_desc *tile, uint32_t render_flags, void *stream)
{
    return prosper_pt_render_frames(ctx, pc, camera, width, height, tile, 1, render_flags, stream);
}

int prosper_pt_get_local_extent(prosper_pt_ctx *ctx, uint32_t *local_width, uint32_t *height)
{
    if (!ctx || !local_width || !height) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_local_extent: null argument");
    *local_width = ctx->localWidth;
    *height = ctx->height;
    return PROSPER_PT_OK;
}

int prosper_pt_get_hdr_device_ptr(prosper_pt_ctx *ctx, void **out_ptr, size_t *out_bytes)
{
    if (!ctx || !out_ptr) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_hdr_device_ptr: null argument");
    if (!ctx->hdr) return fail(PROSPER_PT_ERR_NO_SCENE, "nothing has been rendered yet");
    *out_ptr = ctx->hdr;
    if (out_bytes) *out_bytes = (size_t)ctx->localWidth * ctx->height * sizeof(float4);
    return PROSPER_PT_OK;
}

int prosper_pt_read_hdr(prosper_pt_ctx *ctx, float *rgba32f, size_t byte_size, void *stream)
{
    if (!ctx || !rgba32f) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_hdr: null argument");
    if (!ctx->hdr) return fail(PROSPER_PT_ERR_NO_SCENE, "nothing has been rendered yet");
    const size_t bytes = (size_t)ctx->localWidth * ctx->height * sizeof(float4);
    if (byte_size < bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_hdr: destination too small");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PPT_HIP(hipMemcpyAsync(rgba32f, ctx->hdr, bytes, hipMemcpyDeviceToHost, s));
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

int prosper_pt_blit_rgba16f(prosper_pt_ctx *ctx, uint16_t *host_rgba16f, size_t byte_size, void *stream)
{
    if (!ctx || !host_rgba16f) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_blit_rgba16f: null argument");
    if (!ctx->hdr) return fail(PROSPER_PT_ERR_NO_SCENE, "nothing has been rendered yet");
    const uint32_t count = ctx->localWidth * ctx->height;
    if (byte_size < (size_t)count * 8u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_blit_rgba16f: destination too small");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *tmp = nullptr;
    PPT_HIP(hipMalloc(&tmp, (size_t)count * 8u + 16));
    launch_blit_rgba16f(ctx->hdr, tmp, count, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_rgba16f, tmp, (size_t)count * 8u, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(PROSPER_PT_ERR_HIP, std::string("blit: ") + hipGetErrorString(e));
    return PROSPER_PT_OK;
}

int prosper_pt_set_tone_map_lut(prosper_pt_ctx *ctx, const uint32_t *lut, uint32_t dim)
{
    if (!ctx || !lut || dim < 2 || dim > 256) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_tone_map_lut: bad argument");
    PPT_HIP(hipSetDevice(ctx->device));
    ctx->toneLutDim = 0;
    const size_t bytes = (size_t)dim * dim * dim * sizeof(uint32_t);
    const int rc = grow_buffer(ctx->toneLut, GrowWait::Device, nullptr, bytes, bytes);
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemcpy(ctx->toneLut.ptr, lut, bytes, hipMemcpyHostToDevice));
    ctx->toneLutDim = dim;
    return PROSPER_PT_OK;
}

int prosper_pt_tone_map(
    prosper_pt_ctx *ctx, float exposure, float contrast, void *device_rgba8, uint8_t *host_rgba8, size_t byte_size,
    void *stream)
{
    if (!ctx || (!device_rgba8 && !host_rgba8)) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_tone_map: null argument");
    if (!ctx->hdr) return fail(PROSPER_PT_ERR_NO_SCENE, "nothing has been rendered yet");
    if (!ctx->toneLut.ptr) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_tone_map: no LUT (prosper_pt_set_tone_map_lut)");
    const uint32_t count = ctx->localWidth * ctx->height;
    const size_t bytes = (size_t)count * 4u;
    if (byte_size < bytes) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_tone_map: destination too small");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *out = device_rgba8;
    if (!out)
    {
        if (ctx->toneScratch.bytes < bytes)
        {
            const int rc = grow_buffer(ctx->toneScratch, GrowWait::Stream, s, bytes, bytes + 16);
            if (rc != PROSPER_PT_OK) return rc;
        }
        out = ctx->toneScratch.ptr;
    }
    // (the registry of the inspection passes lists the kept image)
    ctx->toneKeptWidth = device_rgba8 ? 0u : ctx->localWidth;
    ctx->toneKeptHeight = device_rgba8 ? 0u : ctx->height;
    launch_tone_map(ctx->hdr, ctx->toneLut.as<uint32_t>(), ctx->toneLutDim, exposure, contrast, out, count, s);
    PPT_HIP(hipGetLastError());
    if (host_rgba8)
    {
        PPT_HIP(hipMemcpyAsync(host_rgba8, out, bytes, hipMemcpyDeviceToHost, s));
        PPT_HIP(hipStreamSynchronize(s));
    }
    return PROSPER_PT_OK;
}

int prosper_pt_get_counters(prosper_pt_ctx *ctx, prosper_pt_counters *out, void *stream)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_counters: null argument");
    unsigned long long host[kStageCount * kCounterCount] = {};
    const int rc = read_stage_counters(ctx, host, stream);
    if (rc != PROSPER_PT_OK) return rc;
    static_assert(sizeof(prosper_pt_counters) == kCounterCount * sizeof(uint64_t), "counter layout");
    unsigned long long sum[kCounterCount] = {};
    for (uint32_t st = 0; st < kStageCount; ++st)
        for (uint32_t i = 0; i < kCounterCount; ++i) sum[i] += host[st * kCounterCount + i];
    std::memcpy(out, sum, sizeof(*out));
    return PROSPER_PT_OK;
}

int prosper_pt_get_stage_counters(prosper_pt_ctx *ctx, uint32_t stage, prosper_pt_counters *out, void *stream)
{
    if (!ctx || !out || stage >= kStageCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_stage_counters: bad argument");
    unsigned long long host[kStageCount * kCounterCount] = {};
    const int rc = read_stage_counters(ctx, host, stream);
    if (rc != PROSPER_PT_OK) return rc;
    std::memcpy(out, host + stage * kCounterCount, sizeof(*out));
    return PROSPER_PT_OK;
}

int prosper_pt_reset_counters(prosper_pt_ctx *ctx, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_reset_counters: null context");
    PPT_HIP(hipSetDevice(ctx->device));
    PPT_HIP(hipMemsetAsync(
        ctx->counters.ptr, 0, kStageCount * kCounterCount * sizeof(unsigned long long), static_cast<hipStream_t>(stream)));
    return PROSPER_PT_OK;
}

int prosper_pt_set_kernel_timing(prosper_pt_ctx *ctx, int enabled)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_kernel_timing: null context");
    // switching it off keeps the figures of the last timed render readable (later untimed renders record no events)
    if (enabled && !ctx->kernelTiming) ctx->timingValid = false;
    ctx->kernelTiming = enabled != 0;
    return PROSPER_PT_OK;
}

const char *prosper_pt_kernel_name(uint32_t index)
{
    static const char *names[PROSPER_PT_MAX_KERNELS] = {"wf_generate_extend", "wf_shade", "wf_trace", "wf_accumulate",
                                                        "",                   "",         "",         ""};
    return index < PROSPER_PT_MAX_KERNELS ? names[index] : "";
}

int prosper_pt_get_last_render_ms(prosper_pt_ctx *ctx, float *total_ms, float kernel_ms[PROSPER_PT_MAX_KERNELS])
{
    return prosper_pt_get_last_render_timing(ctx, total_ms, kernel_ms, nullptr);
}

int prosper_pt_get_last_render_timing(
    prosper_pt_ctx *ctx, float *total_ms, float kernel_ms[PROSPER_PT_MAX_KERNELS],
    uint32_t kernel_launches[PROSPER_PT_MAX_KERNELS])
{
    if (!ctx || !total_ms) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_last_render_timing: null argument");
    if (!ctx->timingValid)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "no render has run with kernel timing enabled (prosper_pt_set_kernel_timing)");
    PPT_HIP(hipSetDevice(ctx->device));
    if (const int rc = ctx->timeline.wait()) return rc;
    float perStage[PROSPER_PT_MAX_KERNELS] = {};
    uint32_t launches[PROSPER_PT_MAX_KERNELS] = {};
    float total = 0.0f;
    if (const int rc = ctx->timeline.add_to(perStage, launches, &total)) return rc;
    // The wavefront chains: their launches ran on the internal streams, between the caller's-stream
    // events counted above as the (unnamed) chains interval.  Their durations are as the device saw
    // them, i.e. a launch that shared the GPU with the other chain's is counted in full: per-stage sums
    // can exceed the wall time in `total_ms`, which stays the caller's-stream time.
    if (perStage[kStageChains] > 0.0f || launches[kStageChains] > 0)
    {
        uint32_t chainLaunches = 0;
        float chainMs = 0.0f; // (not part of the total)
        for (const LaunchTimeline &chain : ctx->slots[ctx->timedSlot].chains)
        {
            if (const int rc = chain.add_to(perStage, launches, &chainMs)) return rc;
            chainLaunches += chain.intervals();
        }
        if (chainLaunches)
        {
            perStage[kStageChains] = 0.0f;
            launches[kStageChains] = 0;
        }
    }
    *total_ms = total;
    for (int i = 0; i < PROSPER_PT_MAX_KERNELS; ++i)
    {
        if (kernel_ms) kernel_ms[i] = perStage[i];
        if (kernel_launches) kernel_launches[i] = launches[i];
    }
    return PROSPER_PT_OK;
}

int prosper_pt_debug_srgb_monotonicity(
    prosper_pt_ctx *ctx, uint32_t first_bits, uint32_t last_bits, float *max_defect, uint64_t *decreases)
{
    if (!ctx || !max_defect || !decreases || first_bits > last_bits || last_bits >= 0x7F800000u)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_srgb_monotonicity: bad argument");
    PPT_HIP(hipSetDevice(ctx->device));
    uint32_t *d = nullptr;
    PPT_HIP(hipMalloc((void **)&d, 8));
    hipError_t e = hipMemset(d, 0, 8);
    uint32_t host[2] = {0u, 0u};
    if (e == hipSuccess)
    {
        launch_srgb_monotonicity(first_bits, last_bits, d, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(host, d, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    PPT_HIP(e);
    std::memcpy(max_defect, &host[0], 4);
    *decreases = host[1];
    return PROSPER_PT_OK;
}

int prosper_pt_eval_device_fn(
    prosper_pt_ctx *ctx, uint32_t fn, const float *in, uint32_t in_stride, float *out, uint32_t out_stride, uint32_t n)
{
    if (!ctx || !in || !out || fn >= PROSPER_PT_FN_COUNT || in_stride == 0 || out_stride == 0 ||
        (fn == PROSPER_PT_FN_BC7_BLOCK && (in_stride < 4 || out_stride < 16)))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_eval_device_fn: bad argument");
    PPT_HIP(hipSetDevice(ctx->device));
    float *dIn = nullptr, *dOut = nullptr;
    const size_t inBytes = (size_t)n * in_stride * 4, outBytes = (size_t)n * out_stride * 4;
    PPT_HIP(hipMalloc((void **)&dIn, inBytes + 16));
    hipError_t e = hipMalloc((void **)&dOut, outBytes + 16);
    if (e == hipSuccess) e = hipMemcpy(dIn, in, inBytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dOut, 0, outBytes + 16);
    if (e == hipSuccess)
    {
        launch_eval_fn(fn, dIn, in_stride, dOut, out_stride, n, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);
    (void)hipFree(dIn);
    (void)hipFree(dOut);
    if (e != hipSuccess) return fail(PROSPER_PT_ERR_HIP, std::string("eval_device_fn: ") + hipGetErrorString(e));
    return PROSPER_PT_OK;
}

} // extern "C"
