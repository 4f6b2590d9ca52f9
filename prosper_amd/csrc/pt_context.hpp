// pt_context.hpp — the context behind the C-ABI handle (private to the library's translation units).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/prosper_pt/prosper_pt.h"
#include "bvh_build.hpp"
#include "pt_error.hpp"
#include "pt_kernels.hpp"
#include "pt_scene.hpp"
#include "pt_sync.hpp"

namespace ppt
{

struct DeviceAllocation
{
    void *ptr = nullptr;
    size_t bytes = 0;
};

// A device buffer of the context that only grows (grow_buffer) and is freed with its owner.  `bytes` is what the last
// grow asked for; the allocation may be padded beyond it.
struct DeviceBuffer
{
    void *ptr = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer()
    {
        if (ptr) (void)hipFree(ptr);
    }
    template <class T> T *as() const { return static_cast<T *>(ptr); }
};
// What a grow waits for before it frees the old allocation: nothing (a buffer allocated once), the stream of the call,
// or the whole device (work on other streams may still read the buffer)
enum class GrowWait
{
    None,
    Stream,
    Device,
};

#pragma GCC visibility push(hidden) // (not part of the library's exports)

// The one way a DeviceBuffer grows: wait (`wait`, on `s`), free the old allocation, allocate `allocBytes` (`bytes` and any
// padding), fill the new allocation with the byte `fill` unless it is negative, record `bytes`.  On failure the buffer is
// left empty (nullptr, 0).
int grow_buffer(DeviceBuffer &buf, GrowWait wait, hipStream_t s, size_t bytes, size_t allocBytes, int fill = -1);

// The state of a pass module (pt_*_passes.cpp, pt_materials.cpp's texture compression): its buffers and what the last
// call of each of its passes produced, defined in the module's own file.  Made by prosper_pt_create, freed by
// prosper_pt_destroy.
struct GBufferPassState;     // ReSTIR-DI, traced G-buffer, clustering, deferred shading, IBL; the context's last frame
struct ForwardPassState;     // ForwardRenderer's passes
struct DofPassState;         // the skybox fill and depth of field: the intermediates of the last call
struct BloomPassState;       // the working images of the last call, of both techniques
struct TaaPassState;         // the two history images
struct ParticlesPassState;   // the pool, its freelist and the render's per-pixel keys, which live across frames and scenes
struct DebugPassState;       // the debug lines' copy, their per-pixel keys and statistics
struct CullingPassState;     // the two depth pyramids, the draw lists with their argument triples and statistics
struct RasterPassState;      // the visibility image, the large pass's queue, the counts of the last draws
struct CompressPassState;    // prosper_pt_compress_texture (pt_materials.cpp)
struct MeshPreparePassState; // prosper_pt_prepare_mesh (pt_mesh_passes.cpp)
struct DenoisePassState;     // the denoiser's history (colour, moments, guide) and working images
// a new scene, or TemporalAntiAliasing::releasePreserved: the next resolve ignores the history
void forget_taa_history(prosper_pt_ctx *ctx);
struct AccelState;
// the scales of the table `transforms` into acc->dScalesV[v] (allocated at first need), enqueued on `stream`
int enqueue_instance_scales(prosper_pt_ctx *ctx, AccelState *acc, uint32_t v, const prosper_ModelInstanceTransforms *transforms, uint32_t count, hipStream_t stream);
// One 2-D image a pass module owns, as the registry of the inspection passes describes it (prosper_pt_get_debug_resource).
// Every module lists its images in a fixed order whether they are valid or not, so an index means the same image for
// the life of the context.  `valid`: the owning pass has run and the storage still holds what its last call left.
constexpr uint32_t kDebugImageMaxLevels = 16;
struct DebugImage
{
    const char *name = "";
    uint32_t format = 0; // PROSPER_PT_DEBUG_FORMAT_*
    uint32_t width = 0, height = 0, levelCount = 0; // extent of level 0
    bool valid = false;
    const void *level[kDebugImageMaxLevels] = {};
    uint32_t levelW[kDebugImageMaxLevels] = {}, levelH[kDebugImageMaxLevels] = {};
    void one_level(const void *p, uint32_t w, uint32_t h)
    {
        width = w, height = h, levelCount = 1;
        level[0] = p, levelW[0] = w, levelH[0] = h;
    }
};
// What the context asks of a pass module.  Each module defines one (pass_module, pt_pass_support.hpp).
struct PassModule
{
    bool (*create)(prosper_pt_ctx *);       // false: out of host memory
    void (*destroy)(prosper_pt_ctx *);
    void (*forget_scene)(prosper_pt_ctx *); // prosper_pt_upload_scene; nullptr: nothing of it describes a scene
    void (*list_debug_images)(const prosper_pt_ctx *, std::vector<DebugImage> &); // nullptr: it owns no listed image
};
extern const PassModule kGBufferPasses, kForwardPasses, kDofPasses, kBloomPasses, kTaaPasses, kParticlesPasses, kDebugPasses,
    kCullingPasses, kRasterPasses, kCompressPasses, kMeshPreparePasses, kDenoisePasses;
// Every module, in the order they are made.  The registry of debug images lists theirs in this order too, which is part
// of the interface: the G-buffer module's, dof's, bloom's, taa's.
inline const PassModule *const kPassModules[] = {&kGBufferPasses, &kForwardPasses,   &kDofPasses,         &kBloomPasses,
                                                 &kTaaPasses,     &kParticlesPasses, &kDebugPasses,       &kCullingPasses,
                                                 &kRasterPasses,  &kCompressPasses,  &kMeshPreparePasses, &kDenoisePasses};
// State of the keyframe animation (pt_animation.hip, pt_animation.hpp): the node and channel tables of the scene, the
// staged time and the read-back that feeds the host mirrors below.  Made and freed like the others.
struct AnimationState;
// Scratch arrays and timed events of the GPU hierarchy build (pt_bvh_build.hpp), made by the first such build.
struct LbvhState;

#pragma GCC visibility pop

// Host + device state of the acceleration structure that outlives prosper_pt_upload_scene, so that moved instances can
// be re-fitted without rebuilding the scene (prosper_pt_update_transforms): the world triangles in (drawInstance,
// primitive) order on both sides, the per-instance subtrees (bvh_build.hpp InstancedBvh), the instance table.
// The three light buffers of the scene (World.cpp:531-535 rewrites them every frame), versioned like the instance
// transforms: an update is staged by the call (an unchanged set is a no-op) and copied by the next render's own chain
// into the next of three device copies, so the frames in flight keep theirs and nothing synchronises the device.
// (VersionRing, StagingRing, Fence: pt_sync.hpp)
struct LightBlock
{
    alignas(16) prosper_DirectionalLightParameters directional;
    alignas(16) prosper_PointLightsBuffer points; // (16-byte aligned: the kernels read the lights as vec4s)
    alignas(16) prosper_SpotLightsBuffer spots;
};
struct LightState
{
    static constexpr uint32_t kVersions = 3;
    LightBlock *dBlocks[kVersions] = {}; // [0] is the upload's own allocation
    VersionRing<kVersions> versions;
    LightBlock *mirror = nullptr; // host copy of what the device holds (or will hold once `pending` is flushed)
    StagingRing<LightBlock> staging;
    bool pending = false;
    Fence ready; // behind the last flush: every later render's chains wait for it
    uint32_t updates = 0;
    ~LightState() { delete mirror; }
};

struct AccelState
{
    WorldTriangle *dFlat = nullptr; // (drawInstance, primitive) order: what flatten_triangles writes
    WorldTriangle *dTris = nullptr; // leaf order: what the traversal reads
    uint32_t *dOffsets = nullptr, *dFlags = nullptr, *dPerm = nullptr;
    BvhNode *dNodes = nullptr;
    size_t nodeCapacityBytes = 0;
    std::vector<uint32_t> triOffsets;
    std::vector<WorldTriangle> flat; // host copy of dFlat as of the last BUILD (flatStale: instances moved since)
    std::vector<InstancedBvh::Range> ranges;      // one per run of draw instances of a model instance
    std::vector<uint32_t> rangeModelInstance;
    std::vector<prosper_ModelInstanceTransforms> transforms;
    InstancedBvh bvh;
    bool instanced = false;
    // The tree on the device was built there (pt_bvh_build.hpp): `bvh` and `flat` describe an older one, so the next host
    // build of any kind splits every instance again.  What that build reported, for prosper_pt_get_hierarchy_build_info.
    bool foreignTree = false, gpuStagesValid = false;
    uint32_t gpuLeafSize = 0, gpuDepths = 0;
    uint32_t gpuMethod = 0, gpuRadius = 0, gpuRounds = 0, gpuFinishRounds = 0; // prosper_pt_get_gpu_hierarchy_method_info
    float gpuStageMs[8] = {};
    // a prosper_pt_update_transforms that failed half way leaves transforms, world triangles and nodes out of step: renders
    // are refused and the next update redoes every instance, whatever the transforms it is given
    bool stale = false;
    uint64_t total = 0;
    uint32_t drawInstanceCount = 0;

    // ---- refit of the tree after moved instances (pt_kernels.hip refit_bounds / encode_nodes) ----
    float4 *dNodeBounds = nullptr;     // [2 * nodes]: exact bounds below every node
    uint32_t *dRefitOrder = nullptr;   // node indices by height (leaves' parents first)
    uint32_t *dLeafPosition = nullptr; // [total]: (drawInstance, primitive)-order triangle -> its place in dTris
    size_t refitCapacityNodes = 0;
    std::vector<uint32_t> levelOffsets; // [levels + 1] into dRefitOrder
    uint32_t nodeCount = 0;
    // Surface-area measure of the refitted tree (encode_nodes_kernel), one slot per scene version: a refit writes the
    // slot of the version it produces, so a measure can be read as soon as ITS refit has finished - in a pipelined loop
    // that updates every frame the newest refit has only just been enqueued, but the one of two updates ago is done.
    float *dCost = nullptr;             // [kCostSlots] device
    Pinned<float> hCost;                // [kCostSlots]; slot i valid once costDone[i] has passed
    static constexpr uint32_t kCostSlots = 3;
    Fence costDone[kCostSlots];
    bool costPending[kCostSlots] = {}; // recorded, and the measure not taken yet
    uint64_t costSequence[kCostSlots] = {}; // which refit (a running number) the slot's measure belongs to
    uint64_t refitSequence = 0, costRead = 0; // refits enqueued so far / the newest one whose measure has been taken
    float builtCost = 0.0f;             // the same measure right after the last build
    float lastCostRatio = 1.0f;
    std::vector<uint8_t> movedSinceBuild; // per range: its subtree is out of date in `bvh` and `flat`
    bool flatStale = false;
    // the update's transforms go through pinned staging (a pageable source would make the async copy synchronous)
    StagingRing<prosper_ModelInstanceTransforms> staging;
    // recorded on the updating stream behind the refit: every later render's path stages wait for it
    Fence sceneDone;
    uint32_t refits = 0, rebuilds = 0;

    // ---- scene versions: what a refit rewrites - transform table, leaf-order triangles, nodes - exists up to three
    // times, like the per-frame TLAS / instance buffers of a Vulkan frame loop: an update writes the NEXT version while
    // the frames in flight go on reading theirs.  dNodes / dTris / ctx->dTransforms alias version `cur`.  The other
    // versions are allocated by the first update that needs them. ----
    static constexpr uint32_t kVersions = 3;
    WorldTriangle *dTrisV[kVersions] = {};
    BvhNode *dNodesV[kVersions] = {};
    prosper_ModelInstanceTransforms *dTransformsV[kVersions] = {};
    // one uniform scale per model instance beside every version's table (World.cpp:485-498; 0: non-uniform), made on the
    // GPU wherever that table is made: the upload, a flushed transform update or animation, a geometry build
    float *dScalesV[kVersions] = {};
    bool nodesCurrent[kVersions] = {}; // the version's node array holds the tree of the last build (child references)
    VersionRing<kVersions> versions;
    // an update waits here until the next consumer of the scene - normally the next render, which runs it at the head of
    // its own chain of launches, beside the frames in flight
    bool pending = false, pendingGeometry = false;
    uint32_t pendingCount = 0;
};

// The tables a streamed-in texture or material changes (prosper adopts loaded textures and materials a few per frame:
// src/scene/WorldData.cpp:588-647, 2182-2239; the material buffer is re-uploaded when materialsGeneration moves, :568-586):
// MaterialData[], MaterialPack[], AlphaMaterial[], DeviceTexture[] as ONE device block per version.  Version 0 is what
// prosper_pt_upload_scene made (four allocations of their own, never rewritten); prosper_pt_update_textures / _materials
// change the host mirrors, build the new texel arrays / packs / alpha bounds on `uploadStream`, and the next render copies
// the tables into the next of three rotating blocks at the head of its own chain of launches - the frames in flight keep
// reading theirs (pt_materials.cpp).  Replaced texel arrays / packs / bounds are retired, not freed: a frame in flight may
// still read them (a streamed scene replaces each placeholder once; 256 MB of retired memory buy one synchronisation).
struct MaterialState
{
    static constexpr uint32_t kVersions = 4; // 0: the upload's tables; 1..3: rotating blocks
    std::vector<prosper_MaterialData> materials;
    std::vector<MaterialPack> packs;
    std::vector<AlphaMaterial> alphaMaterials;
    std::vector<DeviceTexture> textures;
    std::vector<prosper_pt_sampler_desc> samplers;
    // levels >= 1 of every texture's chain, [textures.size()] on a context created with PROSPER_PT_CREATE_TEXTURE_MIPS
    // (empty otherwise); the device table is the block's fifth part and ctx->textureMips its current version
    std::vector<DeviceTextureMips> mips;
    uint64_t mipTexelBytes = 0;
    size_t mipsOffset = 0;
    uint64_t texelBytes = 0;       // level-0 texel footprint of the textures as the caller gave them (4 B per texel)
    uint64_t alphaBoundBytes = 0;
    uint32_t packedMaterials = 0;
    // device side
    uint8_t *dBlocks[kVersions] = {};
    size_t blockBytes = 0, packsOffset = 0, alphaOffset = 0, texturesOffset = 0;
    VersionRing<kVersions, 1> versions;
    StagingRing<uint8_t> staging; // images of the block, filled by the flush itself
    bool pending = false;          // the mirrors differ from version `cur`
    uint64_t changes = 0;          // bumped whenever an update changed a mirror (a background geometry build compares)
    bool pendingAlphaPatch = false; // ... in a MASK / BLEND material: the any-hit records' copies must follow
    Stream uploadStream;                // texel copies, re-tiling / BC7 decode, packs, alpha bounds of an update
    Fence uploaded;                     // behind the last of them
    Fence ready;                        // behind the last flush: every later render's chains wait for it
    void *linearStaging = nullptr;      // device: the texels of an update as the caller holds them, before re-tiling
    size_t linearStagingBytes = 0;
    Pinned<void> pinnedStaging;         // host: the same bytes on their way there (pt_materials.hpp create_device_texture)
    uint32_t updates = 0;
    // texel arrays, packs and alpha bounds an update replaced: a frame in flight may still read them, so they stay until
    // enough has piled up to be worth ONE device synchronisation (kRetireBytes), or the scene goes
    std::vector<const void *> retired;
    uint64_t retiredBytes = 0;
    static constexpr uint64_t kRetireBytes = 256ull << 20;
    ~MaterialState()
    {
        if (linearStaging) (void)hipFree(linearStaging);
    }
};

// What the geometry of the scene is made from, as the host gave it: prosper_pt_update_meshes changes these mirrors (and the
// device copies they describe) and lays the triangles out again.  The device pointer table has room for every geometry
// buffer prosper can create (sMaxGeometryBuffersCount, WorldData.cpp:31), the metadata table is written in place: a mesh
// that has not arrived has no triangle anywhere, so nothing in flight reads its slot.
struct GeometryState
{
    std::vector<prosper_GeometryMetadata> metadatas;
    std::vector<prosper_pt_mesh_info> infos;
    std::vector<prosper_DrawInstance> drawInstances;
    std::vector<void *> buffers;        // device copies of the geometry buffers (scene allocations)
    std::vector<uint64_t> bufferBytes;
    const void **dBufferTable = nullptr;           // device: [PROSPER_PT_MAX_GEOMETRY_BUFFERS]
    prosper_GeometryMetadata *dMetadatas = nullptr; // device: [meshCount]
    // prosper_pt_update_meshes keeps the arrived bytes in host memory (`arrived`); the worker thread of the next geometry build
    // (MeshBuild, pt_geometry.cpp) copies them to the device, on its own stream, before it lays the triangles out - the
    // calling thread touches no stream.  While a build runs `buffers` belongs to the worker (it allocates new geometry
    // buffers); the calling thread goes by bufferBytes (0: no such buffer yet).
    struct ArrivedMesh
    {
        uint32_t meshIndex = 0, bufferIndex = 0;
        uint64_t byteOffset = 0;
        std::vector<uint8_t> bytes;
        prosper_GeometryMetadata metadata = {};
    };
    std::vector<ArrivedMesh> arrived;
    bool dirty = false;      // meshes arrived that no build has taken up yet
    uint32_t meshUpdates = 0; // calls that handed meshes over
    uint32_t installs = 0;    // background builds whose result became the scene
};
struct MeshBuild;

// multi-GPU state of a context (pt_tiling.cpp): the communicator, its stream and the root's staging buffer
struct TilingState;

// scene-lifetime device memory of a context (prosper_pt.cpp): freed by the next upload / destroy
int device_alloc(prosper_pt_ctx *ctx, size_t bytes, void **out);
void device_free(prosper_pt_ctx *ctx, const void *p);
int upload(prosper_pt_ctx *ctx, const void *src, size_t bytes, void **out);

} // namespace ppt

struct prosper_pt_ctx
{
    int device = 0;
    uint32_t flags = 0;
    prosper_pt_debug_options debug = {}; // tuning / test options (prosper_pt_set_debug_options); never the environment
    std::vector<ppt::DeviceAllocation> sceneAllocations;
    std::atomic<uint64_t> sceneBytes{0}; // (the worker thread of a mesh build allocates too)
    bool haveScene = false;
    ppt::DeviceScene scene = {};
    const ppt::DeviceTextureMips *textureMips = nullptr; // beside scene.textures (nullptr: the context keeps no mip chains)
    prosper_pt_scene_stats stats = {};
    uint32_t packedMaterials = 0; // materials whose three textures are interleaved (MaterialPack)
    uint64_t alphaTriangleCount = 0, alphaBoundBytes = 0; // any-hit records and bytes of alpha bounds (AlphaMaterial)
    // light buffers are re-uploaded every frame in prosper; keep their device addresses mutable
    ppt::LightState *lights = nullptr; // the scene's light buffers (device copies in the scene's allocation list)
    ppt::MaterialState *materialState = nullptr; // mirrors + versions of the material / texture tables (pt_materials.cpp)
    ppt::GeometryState *geometry = nullptr;       // mirrors of the mesh tables and geometry buffers (prosper_pt_update_meshes)
    ppt::MeshBuild *meshBuild = nullptr;          // the geometry a worker thread is building from them, if any
    std::vector<ppt::AccelState *> retiredAccel;  // replaced generations: frames in flight may still use their events / staging
    std::mutex allocMutex;                        // sceneAllocations / sceneBytes (the worker thread allocates too)
    // the worker thread's stream: a plain one, made by the worker at first need - after prosper_pt_create has given the
    // hardware queues to the work streams (pt_geometry.cpp, "streamed-in meshes")
    ppt::Stream buildStream;
    // Pinned staging for the large host <-> device copies of a geometry build (pt_geometry.cpp staged_copy): a copy from
    // pageable memory has the runtime pin the caller's pages for its duration, and when those pages are freed soon after - the
    // builder's vectors are - the unmapping goes through the GPU driver and stops every queue of the process for 20-30 ms
    ppt::Pinned<void> pinnedStaging;

    float4 *hdr = nullptr; // current HDR buffer (internal or caller-owned)
    ppt::DeviceBuffer ownedHdr;
    void *externalHdr = nullptr;
    size_t externalHdrBytes = 0;
    uint32_t localWidth = 0, height = 0;

    ppt::DeviceBuffer counters; // kStageCount x kCounterCount u64: one block of work counters per kernel stage
    // wavefront workspace (one allocation, carved into the WavefrontBuffers arrays)
    // global overflow of the traversal stacks (only for trees whose stack bound exceeds the LDS stack)
    uint64_t wfSlots = 0;

    bool kernelTiming = false;
    ppt::LaunchTimeline timeline; // the caller's stream of the last timed render
    bool timingValid = false;

    ppt::GBufferPassState *gbufferPasses = nullptr; // ReSTIR-DI, traced G-buffer, clustering, deferred shading, IBL
    ppt::ForwardPassState *forwardPasses = nullptr; // the traced and the rasterised transparent pass, the forward opaque pass
    ppt::DofPassState *dofPasses = nullptr; // skybox fill, depth of field
    ppt::BloomPassState *bloomPasses = nullptr;
    ppt::TaaPassState *taaPasses = nullptr;
    ppt::DenoisePassState *denoisePasses = nullptr;
    ppt::ParticlesPassState *particlesPasses = nullptr;
    ppt::DebugPassState *debugPasses = nullptr;
    ppt::CullingPassState *cullingPasses = nullptr; // the depth pyramids, the draw lists, DrawStats
    ppt::RasterPassState *rasterPasses = nullptr;   // the visibility image drawn from the lists
    ppt::CompressPassState *compressPasses = nullptr;       // prosper_pt_compress_texture, prosper_pt_debug_bc7_encode_blocks
    ppt::MeshPreparePassState *meshPreparePasses = nullptr; // prosper_pt_prepare_mesh
    ppt::AnimationState *animation = nullptr;
    uint32_t hierarchyBuilder = PROSPER_PT_BUILDER_HOST; // prosper_pt_set_hierarchy_builder
    uint32_t gpuHierarchyMethod = PROSPER_PT_GPU_HIERARCHY_LINEAR, gpuHierarchyRadius = 0; // prosper_pt_set_gpu_hierarchy_method (0: the default radius)
    ppt::LbvhState *lbvh = nullptr;
    // prosper_pt_set_gpu_hierarchy_sites: the builds the GPU builder makes besides rebuilds (PROSPER_PT_GPU_BUILD_SITE_*), and
    // the scratch of those the worker thread runs (pt_geometry.hpp GeometryTarget::lbvh); grow-only like `lbvh`
    uint32_t gpuHierarchySites = 0;
    ppt::LbvhState *lbvhWorker = nullptr;
    ppt::DeviceBuffer toneLut; // dim^3 R9G9B9E5 texels
    uint32_t toneLutDim = 0;
    ppt::DeviceBuffer toneScratch; // RGBA8 output when the caller only wants a host copy
    uint32_t toneKeptWidth = 0, toneKeptHeight = 0; // of the image the last tone map left in toneScratch (0: it went to the caller's buffer)

    // Everything a render has in flight between its first launch and its accumulate kernel: the wavefront
    // workspace, the stack-overflow array and the launch chains (pt_kernels.hpp WavefrontChains) with their
    // timelines.  kRenderSlots slots = that many frames in flight (PROSPER_PT_RENDER_PIPELINED), the role `nextFrame` and
    // the per-frame descriptor sets play in RtReference::record; everything else uses slot 0.
    struct RenderSlot
    {
        ppt::DeviceBuffer stackOverflow;
        ppt::DeviceBuffer wfBlock;
        ppt::Fence chainJoin[ppt::kMaxChains];
        ppt::LaunchTimeline chains[ppt::kMaxChains];
        ppt::Fence free; // recorded after the accumulate kernel of the slot's last render
    };
    // prosper keeps two frames in flight; a third one fills the machine better at the batch sizes of a multi-GPU
    // rank share (1/4 share 0.71 -> 0.66 ms, C3 19.3 -> 18.9 ms; profiles/r01_pipelined.txt)
    static constexpr uint32_t kRenderSlots = 3;
    // The internal streams, three in all (+ the caller's = the four hardware queues of the device; more streams
    // share queues and serialise): a pipelined render's chain runs on workStreams[slot], the two chains of an
    // in-order render on workStreams[0] and [1].  All ordering between them goes through events.
    ppt::Stream workStreams[kRenderSlots];
    RenderSlot slots[kRenderSlots];
    uint32_t lastSlot = 0;  // of the last render
    uint32_t timedSlot = 0; // of the last render that ran with kernel timing on (timing readout)
    ppt::Fence chainFork;

    // stripe partition of the last render (prosper_pt_tile_desc) and the multi-GPU gather state
    uint32_t lastWidth = 0;
    uint32_t stripeWidth = 0, stripeIndex = 0, stripeCount = 1;
    ppt::TilingState *tiling = nullptr;
    ppt::AccelState *accel = nullptr;
    prosper_ModelInstanceTransforms *dTransforms = nullptr; // the scene's transform table (mutable alias)
};
