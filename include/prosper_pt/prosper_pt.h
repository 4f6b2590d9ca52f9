/*
 * prosper_pt/prosper_pt.h — C-ABI of the MI355X path-tracing reference pass.
 *
 * This library sits where prosper records `cb.traceRaysKHR(rgen, miss, hit, callable, W, H, 1)`
 * (reference: src/render/RtReference.cpp:328-330).  prosper has no FFI for this path — the pass is
 * a concrete C++ class (src/render/RtReference.hpp:32-60) — so the entry points below are the
 * smallest plain-C surface that class needs: they replace, one for one,
 *
 *   prosper_pt_create / _destroy      RtReference::init / ~RtReference            RtReference.cpp:92-120
 *                                     (pipeline + SBT creation -> load the gfx950 code object)
 *   prosper_pt_upload_scene           World::updateBuffers + buildNextBlas + buildCurrentTlas
 *                                                                                  src/scene/World.cpp:468-536,585-802
 *                                     and the descriptor sets the pass binds       RtReference.cpp:238-274
 *   prosper_pt_update_lights          lights ring write                            World.cpp:531-535
 *   prosper_pt_update_transforms      instance transforms + TLAS rebuild           World.cpp:359-466,749-802,878-928
 *   prosper_pt_update_textures /      adoption of streamed-in images / materials   src/scene/WorldData.cpp:568-647,2182-2239
 *   prosper_pt_update_materials
 *   prosper_pt_update_meshes          adoption of streamed-in meshes, BLAS once    WorldData.cpp:2003-2110, World.cpp:585-606,
 *                                     a model is complete, inactive until then     909-915
 *   prosper_pt_render                 pushConstants + traceRaysKHR                 RtReference.cpp:278-330
 *                                     + the previous/illumination ping-pong        RtReference.cpp:178-219,332-334
 *   prosper_pt_read_hdr               the RGBA32F "rtIllumination" image           RtReference.cpp:178-187
 *   prosper_pt_blit_rgba16f           blitImage RGBA32F -> RGBA16F                 RtReference.cpp:339-377
 *   prosper_pt_get_counters           (new) deterministic work counters for the roofline model
 *   prosper_pt_comm_* / _gather_tiles (new) multi-GPU: stripes per rank + one RCCL gather + de-interleave kernel
 *                                     (the reference asserts renderArea.offset == 0, RtReference.cpp:327)
 *
 * All entry points are `extern "C"`, take PODs / plain pointers and sizes, never throw and return
 * PROSPER_PT_OK (0) or a negative error code; prosper_pt_last_error() returns the message of the
 * calling thread's last failure.  A context is single-threaded for its callers (the reference makes all pass
 * calls on the main thread, src/Allocators.hpp:9); use one context per GPU.  While meshes stream in the context
 * runs ONE worker thread of its own (prosper_pt_update_meshes), which touches nothing a caller can see.
 *
 * Host pointers inside prosper_pt_scene_view are borrowed for the duration of the call only.
 */
#ifndef PROSPER_PT_H
#define PROSPER_PT_H

#include <stddef.h>
#include <stdint.h>

#include "shader_structs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PROSPER_PT_ABI_VERSION 4

enum
{
    PROSPER_PT_OK = 0,
    PROSPER_PT_ERR_INVALID_ARGUMENT = -1,
    PROSPER_PT_ERR_NO_DEVICE = -2,  /* no HIP device / HIP extension unusable: never falls back to CPU */
    PROSPER_PT_ERR_HIP = -3,        /* a HIP runtime call failed */
    PROSPER_PT_ERR_NO_SCENE = -4,   /* render before upload_scene */
    PROSPER_PT_ERR_SCENE = -5,      /* scene view failed validation (out-of-range index/offset) */
    PROSPER_PT_ERR_UNSUPPORTED = -6,
    PROSPER_PT_NOT_READY = -7,      /* prosper_pt_try_texture_readback: nothing queued, or not finished yet (sets no error message) */
};

typedef struct prosper_pt_ctx prosper_pt_ctx;

typedef struct prosper_pt_device_desc
{
    uint32_t struct_size;   /* sizeof(prosper_pt_device_desc) */
    int32_t device_ordinal; /* HIP device index; the pass runs on this GPU only */
    uint32_t flags;         /* PROSPER_PT_CREATE_* */
    uint32_t reserved;
} prosper_pt_device_desc;

enum
{
    /* Default pipeline: wavefront stage kernels (generate+extend / shade / shadow / extend /
     * accumulate) with per-wave ballot compaction.  MEGAKERNEL = one lane per pixel runs whole
     * paths: the same pixels, kept for A/B timing.
     * PERSISTENT is reserved (a removed experiment): prosper_pt_create refuses it with
     * PROSPER_PT_ERR_UNSUPPORTED. */
    PROSPER_PT_CREATE_MEGAKERNEL = 1u << 0,
    PROSPER_PT_CREATE_PERSISTENT = 1u << 1,
    /* run the wavefront pipeline as ONE chain of launches on the caller's stream instead of two
     * half-batches on two internal streams (A/B switch; the two-chain default hides launch tails) */
    PROSPER_PT_CREATE_SINGLE_CHAIN = 1u << 2,
    /* every material texture gets a mip chain at prosper_pt_upload_scene / prosper_pt_update_textures (generated on the
     * GPU, or taken from the caller: prosper_pt_texture_desc.mipLevelCount), kept beside its level 0 for
     * sample_texture_lod ("texture mip chains" below).  Without the flag nothing about textures changes and
     * mipLevelCount is not read. */
    PROSPER_PT_CREATE_TEXTURE_MIPS = 1u << 3,
};

/* Texel formats of material textures (reference: src/scene/Texture.cpp:217-296 stores UNORM,
 * sRGB decode happens in the shader, materials.glsl:56). */
enum
{
    PROSPER_PT_FORMAT_RGBA8_UNORM = 0,
    /* level 0 of prosper's texture cache as it is (src/scene/Texture.cpp:255-287 compresses every texture whose
     * mip chain divides by 4; src/utils/Dds.cpp:118-131 layout): (width/4)*(height/4) 16-byte blocks, row-major;
     * width and height are multiples of 4.  Decoded once at upload by a HIP kernel to the texels the GPU's
     * BC7 sampler returns in prosper. */
    PROSPER_PT_FORMAT_BC7_UNORM = 1,
};
enum
{
    PROSPER_PT_FILTER_NEAREST = 0,
    PROSPER_PT_FILTER_LINEAR = 1,
};
enum
{
    PROSPER_PT_WRAP_REPEAT = 0,
    PROSPER_PT_WRAP_MIRRORED_REPEAT = 1,
    PROSPER_PT_WRAP_CLAMP_TO_EDGE = 2,
};

/* One entry of the bindless materialTextures[] table (materials.glsl:23-24).  RT stages have no derivatives and sample
 * LOD 0: level 0 is all they read.  Index 0 is the "no texture" slot.
 * mipLevelCount (the former `reserved`) is read only by a context created with PROSPER_PT_CREATE_TEXTURE_MIPS:
 *   0 or 1   `texels` is level 0; the library generates the other levels of prosper's chain
 *            (max(floor(log2(max(w, h))) + 1 - 2, 1) levels of extent max(extent >> l, 1), src/scene/Texture.cpp:217-225)
 *   n > 1    `texels` holds n levels back to back as prosper's texture cache lays them out (src/utils/Dds.cpp:100-135;
 *            BC7 levels in whole 4x4 blocks); they are taken as they are.  n above prosper's count is refused. */
typedef struct prosper_pt_texture_desc
{
    const void *texels; /* RGBA8: width*height texels, row-major, tightly packed; BC7: the level's blocks */
    uint32_t width;
    uint32_t height;
    uint32_t format; /* PROSPER_PT_FORMAT_* */
    uint32_t mipLevelCount;
} prosper_pt_texture_desc;

/* One entry of materialSamplers[] (src/scene/WorldData.cpp:681-720); index 0 = repeat/linear. */
typedef struct prosper_pt_sampler_desc
{
    uint32_t magFilter; /* PROSPER_PT_FILTER_* (LOD 0 => magnification filter is the one used) */
    uint32_t minFilter;
    uint32_t wrapS; /* PROSPER_PT_WRAP_* */
    uint32_t wrapT;
} prosper_pt_sampler_desc;

/* scene::MeshInfo (src/scene/Mesh.hpp:17-23), needed for the triangle count of each mesh and for
 * the opaque flag (World.cpp:646-651 reads m_materials[info.materialIndex].alphaMode). */
typedef struct prosper_pt_mesh_info
{
    uint32_t vertexCount;
    uint32_t indexCount;
    uint32_t meshletCount;
    uint32_t materialIndex;
} prosper_pt_mesh_info;

/* Skybox cube: RGBA16F, mip 0, faces +X,-X,+Y,-Y,+Z,-Z, each faceSize x faceSize, row-major
 * (reference: src/scene/Texture.cpp:589-636, sampled by textureLod(skybox, d, 0) main.rgen:251). */
typedef struct prosper_pt_cube_desc
{
    const uint16_t *texels; /* 6 * faceSize * faceSize * 4 halfs; NULL = no skybox */
    uint32_t faceSize;
    uint32_t reserved;
} prosper_pt_cube_desc;

/* Everything the pass reads through its nine descriptor sets (RtReference.cpp:244-257). */
typedef struct prosper_pt_scene_view
{
    uint32_t struct_size; /* sizeof(prosper_pt_scene_view) */
    uint32_t reserved;

    /* GEOMETRY_SET: bindless geometry buffers + per-mesh metadata (geometry.glsl:7-55) */
    const void *const *geometryBuffers;
    const uint64_t *geometryBufferByteSizes;
    uint32_t geometryBufferCount;
    uint32_t meshCount;
    const prosper_GeometryMetadata *geometryMetadatas; /* [meshCount]; bufferIndex == PROSPER_PT_ABSENT: the mesh has not
                                                          been loaded yet (prosper_pt_update_meshes) */
    const prosper_pt_mesh_info *meshInfos;             /* [meshCount] */

    /* SCENE_INSTANCES_SET (instances.glsl:8-34) */
    const prosper_DrawInstance *drawInstances; /* [drawInstanceCount] */
    uint32_t drawInstanceCount;
    uint32_t modelInstanceCount;
    const prosper_ModelInstanceTransforms *modelInstanceTransforms; /* [modelInstanceCount] */

    /* MATERIAL_DATAS_SET + MATERIAL_TEXTURES_SET (materials.glsl:7-24) */
    const prosper_MaterialData *materials; /* [materialCount], index 0 = default material */
    uint32_t materialCount;
    uint32_t textureCount;
    const prosper_pt_texture_desc *textures; /* [textureCount], index 0 unused by shading */
    const prosper_pt_sampler_desc *samplers; /* [samplerCount], index 0 = default sampler */
    uint32_t samplerCount;
    uint32_t reserved2;

    /* LIGHTS_SET (lights.glsl:6-23) */
    const prosper_DirectionalLightParameters *directionalLight;
    const prosper_PointLightsBuffer *pointLights;
    const prosper_SpotLightsBuffer *spotLights;

    /* SKYBOX_SET binding 0 (skybox.glsl:4) */
    prosper_pt_cube_desc skybox;
} prosper_pt_scene_view;

/* The set of pixels one context renders.  The reference always renders the whole image
 * (asserts renderArea.offset == 0, RtReference.cpp:327); for multi-GPU tiling the image is cut
 * into vertical stripes `stripeWidth` pixels wide and this context renders stripes
 * s with s % stripeCount == stripeIndex.  RNG seeds use absolute pixel coordinates
 * (main.rgen:227-229), so any partition yields the same pixels as a whole-image render.
 * The context's HDR buffer holds only its own pixels, rows of localWidth texels, stripes in
 * ascending order.  NULL / {0,0,1} = whole image. */
typedef struct prosper_pt_tile_desc
{
    uint32_t stripeWidth;
    uint32_t stripeIndex;
    uint32_t stripeCount;
} prosper_pt_tile_desc;

/* Deterministic work counters (exact integers, independent of scheduling) used to price the
 * ALGORITHMIC bytes of a frame.  Collected only by prosper_pt_render calls made with
 * PROSPER_PT_RENDER_COUNT_WORK; accumulate until prosper_pt_reset_counters. */
typedef struct prosper_pt_counters
{
    uint64_t paths;            /* pixels rendered (one path per pixel per frame) */
    uint64_t closestRays;      /* traceClosest calls */
    uint64_t shadowRays;       /* shadow() calls */
    uint64_t nodeVisits;       /* BVH node fetches, all rays */
    uint64_t triangleTests;    /* ray/triangle tests, all rays */
    uint64_t closestHits;      /* evaluateSurface invocations */
    uint64_t anyHitCalls;      /* any-hit invocations (non-opaque candidates) */
    uint64_t lightSamples;     /* sampleLight calls: sun/point */
    uint64_t spotLightSamples; /* sampleLight calls that picked a spot light */
    uint64_t skyLookups;       /* IBL miss lookups */
    uint64_t pixelsWritten;    /* output texels written */
    uint64_t historyReads;     /* output texels whose history was read */
    uint64_t shortIndexHits;   /* of closestHits + anyHitCalls: those on u16-indexed meshes */
    uint64_t shortIndexTriangleTests; /* of triangleTests: those on u16-indexed meshes */
    uint64_t nodePhaseSteps;     /* wavefront pipeline: wave-level steps of the node phase (x64 lanes = issue slots) */
    uint64_t trianglePhaseSteps; /* same for the triangle phase; lane utilisation = visits / (64 * steps) */
    uint64_t anyHitTexelFetches; /* of anyHitCalls: those that fetched texels (not settled by the material's alpha bounds) */
} prosper_pt_counters;

/* Sizes the roofline model needs about the acceleration structure the library built. */
typedef struct prosper_pt_scene_stats
{
    uint64_t triangleCount; /* world-space triangles (instances expanded) */
    uint64_t nodeCount;
    uint32_t nodeBytes;     /* S_node: bytes fetched per node visit */
    uint32_t triangleBytes; /* bytes fetched per ray/triangle test */
    uint32_t maxDepth;
    uint32_t variantFlags;  /* PROSPER_PT_VARIANT_*: the kernel variants the next render of this scene takes */
    uint64_t deviceBytes;   /* HBM resident bytes for the scene */
    double buildSeconds;    /* acceleration structure: from the first flatten kernel to the uploaded nodes (since round 3
                             * the host BVH build runs on the host's threads WHILE the calling thread uploads textures,
                             * sky, lights and alpha tables: this span contains those too) */
    /* (ABI 2) where prosper_pt_upload_scene spent its time: the whole call, the host-side BVH construction alone
     * (the part a host-side rebuild would pay again), and the texture re-tiling / BC7 decode + copies - the last two
     * overlap, so they no longer add up to the first */
    double uploadSeconds;
    double bvhBuildSeconds;
    double textureSeconds;
    /* (ABI 3) non-opaque triangles (each has a 32-byte any-hit record) and the bytes of the materials' alpha bounds */
    uint64_t alphaTriangleCount;
    uint64_t alphaBoundBytes;
} prosper_pt_scene_stats;
enum
{
    PROSPER_PT_VARIANT_LDS_SCENE = 1u << 0,       /* BVH + triangles staged in LDS by the traversal kernels */
    PROSPER_PT_VARIANT_LDS_TABLES = 1u << 1,      /* wf_shade stages instances/transforms/materials/lights in LDS */
    PROSPER_PT_VARIANT_BATCHED_TEXTURES = 1u << 2, /* the twelve texel loads of a hit issued together */
    PROSPER_PT_VARIANT_TEXTURE_PACKS = 1u << 3,  /* some material's base / MR / normal texels are interleaved per texel */
    PROSPER_PT_VARIANT_RAW_RECORDS = 1u << 4,    /* reserved: never set */
    PROSPER_PT_VARIANT_STACK_SHIFT = 8,           /* bits 8..15: LDS traversal-stack entries (16/24/32) */
};

enum
{
    PROSPER_PT_RENDER_COUNT_WORK = 1u << 0, /* run the instrumented kernels (slower, same pixels) */
    /* Frames in flight, the role of `nextFrame` / the per-frame descriptor sets in RtReference::record
     * (src/render/RtReference.cpp:161-168; prosper keeps 2 frames in flight): the path stages of this render use the
     * context's NEXT workspace (it owns three) and may start before work enqueued earlier on `stream` - including the
     * two previous renders - has finished; they wait only for the render of three calls ago.  The accumulate kernel (history read,
     * output write) runs on `stream`, in order, so the image and everything enqueued after this call behave as
     * without the flag.  The caller promises that no input of this render (scene, lights) is produced by work still
     * pending on `stream`: uploads through this API are synchronous, so that holds unless the caller writes the
     * library's buffers itself.  Same pixels (tested); ignored with PROSPER_PT_RENDER_COUNT_WORK. */
    PROSPER_PT_RENDER_PIPELINED = 1u << 1,
};

/* Tuning and test options of a context.  NOTHING in the library reads the process environment while it uploads, updates or
 * renders: a host application's environment cannot change what this plugin does.  Tests and measurement scripts fill this
 * struct instead (prosper_pt_debug_options_default, change fields, prosper_pt_set_debug_options); options marked "upload"
 * take effect at the next prosper_pt_upload_scene, the others at the next render / update.  No option changes a pixel
 * (every one of them is exercised by a bit-exactness test).  The one concession to shell-driven sweeps: when the variable
 * PROSPER_PT_DEBUG is "1" at prosper_pt_create - and only then, and only there - PROSPER_PT_DEBUG_OPTIONS
 * ("name=value,name=value", the field names below) is parsed into the new context's options.
 * Zero (or -1 where zero is a value) always means "the library's default". */
typedef struct prosper_pt_debug_options
{
    uint32_t struct_size; /* sizeof(prosper_pt_debug_options) */
    /* ---- scene upload ---- */
    int32_t batchedTextures;   /* -1: by texel footprint; 0 / 1: a hit's texel loads one by one / issued together */
    int32_t widePacks;         /* -1: by texel footprint; 1 / 0: 16-byte / compact 8-byte material texture packs */
    int32_t alphaCellShift;    /* -1: default; s: alpha-bound cells of 2^s texels a side */
    uint32_t noTexturePacks;   /* every texture sampled by itself */
    uint32_t noAlphaBounds;    /* every any-hit candidate runs the exact code */
    uint32_t noUploadRefit;    /* keep the host emitter's node bytes (the test that compares them with the device encoder's) */
    uint32_t flatBvh;          /* one SAH tree over everything instead of per-instance subtrees */
    /* ---- hierarchy builder (upload and rebuild) ---- */
    float sahTraversalCost;    /* 0: 1.0 */
    float boxPad;              /* 0: 1.6e-5 (also the minimum) */
    uint32_t leafSize;         /* 0: 4 */
    uint32_t buildThreads;     /* 0: the host's threads */
    uint32_t topEntries;       /* 0: one per four triangles */
    int32_t nodeOrder;         /* -1: 2 (first 4096 nodes breadth-first, then depth-first subtrees); 0 depth-first; 1 breadth-first */
    int32_t childOrder;        /* -1 / 1: smallest box first; 0: build order */
    uint32_t buildTiming;      /* stage times of the hierarchy assembly and of a geometry build to stderr */
    /* ---- render ---- */
    uint32_t segments;         /* target segment count of the wavefront workspace */
    uint32_t segmentLength;    /* segment length in slots (a multiple of 64) */
    uint32_t chains;           /* launch chains of an in-order render (default 2) */
    uint32_t ldsStackEntries;  /* 16 / 24 / 32: LDS traversal-stack entries (deeper entries spill to global memory) */
    uint32_t noLdsScene;       /* keep a small scene in global memory */
    uint32_t noLdsTables;      /* keep the shading tables in global memory */
    uint32_t traceDeadPaths;   /* keep tracing zero-throughput paths, as the GLSL does (audit of the contract's rule) */
    int32_t bandedBatches;     /* 1: every XCD's segments take the camera-ray batches of ONE band of the image instead of batches
                                * strided over all of it (measured slower: profiles/r04_banded_batches.txt); -1 / 0: strided */
    /* ---- updates ---- */
    float rebuildCostRatio;    /* 0: 1.3 - growth of the tree's surface-area measure at which an update also rebuilds */
    uint32_t alwaysRebuild;    /* rebuild with every update, synchronously */
    uint32_t failNextUpdate;   /* the next host-side rebuild fails (the recovery test); cleared by that failure */
    /* ---- reserved: the switches of removed experiments.  They must be 0: a nonzero value fails with
     *      PROSPER_PT_ERR_UNSUPPORTED (prosper_pt_set_debug_options, and prosper_pt_create through
     *      PROSPER_PT_DEBUG_OPTIONS) ---- */
    uint32_t poolVariant;
    uint32_t rawRecords;
    uint32_t tileOrder;
    uint32_t hipGraph;
    uint32_t pipelinedChains;
    uint32_t mergeLimit;
} prosper_pt_debug_options;

const char *prosper_pt_last_error(void);
uint32_t prosper_pt_abi_version(void);
/* Always 0: the measured-slower kernel variants this reported on were removed from the library. */
uint32_t prosper_pt_has_experiments(void);
/* Test hook (needs no device): the terms the wavefront kernels divide by `divisor` with - a tile count fixed for a launch.
 * With t = the high 32 bits of *mul x n:  n / divisor = (t + ((n - t) >> (*shifts & 255))) >> (*shifts >> 8)  for every
 * 32-bit n.  A divisor of 0 gets the terms of 1. */
void prosper_pt_debug_magic_divisor(uint32_t divisor, uint32_t *mul, uint32_t *shifts);
void prosper_pt_debug_options_default(prosper_pt_debug_options *out);
int prosper_pt_set_debug_options(prosper_pt_ctx *ctx, const prosper_pt_debug_options *options);
int prosper_pt_get_debug_options(prosper_pt_ctx *ctx, prosper_pt_debug_options *out);

int prosper_pt_create(const prosper_pt_device_desc *desc, prosper_pt_ctx **out_ctx);
void prosper_pt_destroy(prosper_pt_ctx *ctx);

/* Copies the whole scene to HBM, flattens instances x triangles into world space from the
 * fp16 positions (the BVH must see the decoded halfs: World.cpp:635-644) and builds the BVH. */
int prosper_pt_upload_scene(prosper_pt_ctx *ctx, const prosper_pt_scene_view *scene);
/* The three light buffers only (prosper rewrites them every frame: World.cpp:531-535).  An unchanged set costs a memcmp.
 * A changed one is staged by the call and copied by the next render at the head of its own chain of launches into the
 * next of three device versions (ABI 3): the frames in flight keep theirs, nothing synchronises the device. */
int prosper_pt_update_lights(
    prosper_pt_ctx *ctx, const prosper_DirectionalLightParameters *directionalLight,
    const prosper_PointLightsBuffer *pointLights, const prosper_SpotLightsBuffer *spotLights);
/* New instance transforms for the uploaded scene (the whole ModelInstanceTransforms table, `count` = the scene's
 * modelInstanceCount; World::updateScene rewrites it every frame, World.cpp:359-466).  prosper then rebuilds its TLAS on
 * the GPU (World.cpp:749-802, 878-928).  Here (ABI 3) the update is a REFIT on the GPU: the transform table, the
 * world-space triangles and new boxes for the unchanged tree (one small kernel per tree level + one over all nodes) - no
 * host-side build, no device-wide synchronisation.  prosper_pt_update_transforms only STAGES the table (it returns in
 * microseconds; an unchanged table is a no-op); the refit runs at the head of the next render's own chain of launches,
 * into the next of three versions of the transform / triangle / node arrays - like the per-frame TLAS of a Vulkan frame
 * loop - so the frames in flight (PROSPER_PT_RENDER_PIPELINED) go on reading theirs and nothing waits for them.
 * prosper_pt_update_transforms_async with PROSPER_PT_UPDATE_NOW enqueues the refit on `stream` right away instead (any
 * stream, the null stream included); without the flag it stages like prosper_pt_update_transforms and ignores `stream`.  Same
 * pixels as a fresh prosper_pt_upload_scene of the moved scene (hits do not depend on the hierarchy).  A refit cannot keep
 * the tree good when instances travel far: each one leaves the tree's surface-area measure behind, and when that has
 * grown by 30 % (debug option rebuildCostRatio) over its value at the last build, the next update has the moved
 * instances split again - by the context's worker thread, into a new generation of the geometry that the first render
 * after it is done switches to, like streamed-in meshes (prosper_pt_update_meshes); the frame loop goes on refitting and
 * rendering meanwhile.  prosper_pt_finish_mesh_updates waits for it too; prosper_pt_rebuild_hierarchy does the same work
 * at once, synchronously. */
int prosper_pt_update_transforms(prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count);
enum
{
    PROSPER_PT_UPDATE_NOW = 1u << 0, /* enqueue the refit on `stream` inside the call instead of leaving it to the next render */
};
int prosper_pt_update_transforms_async(
    prosper_pt_ctx *ctx, const prosper_ModelInstanceTransforms *transforms, uint32_t count, uint32_t flags, void *stream);
/* ---- glTF keyframe animation, evaluated on the GPU ahead of the refit ----
 * World::updateAnimations + World::updateScene (src/scene/Animations.hpp, Accessors.cpp:25-75, World.cpp:349-466) as two
 * kernels at the head of the refit's chain of launches: one thread per animated (node, path) samples its keyframes into the
 * node's translation / rotation / scale, one thread per node multiplies the chain of its ancestors down and writes the
 * ModelInstanceTransforms entry, the light fields and the camera record of what the node carries.  A frame's update is one
 * float.
 *   prosper_pt_set_animations   the scene's node tree and its channels (flat tables, borrowed for the call); the scene must
 *                               be uploaded, and a new prosper_pt_upload_scene forgets them.  Nodes come in prosper's scene-node
 *                               order (WorldData.cpp:1364-1456): a parent has a lower index than its child.  The HAS_* flags say
 *                               which components the node keeps (a static one within 1e-3 of the identity is dropped,
 *                               WorldData.cpp:1197-1211; one a channel targets is kept whatever the flag says, :1237-1272).
 *                               Where several channels target one (node, path) the last one wins.
 *   prosper_pt_animate          stages `timeS` like prosper_pt_update_transforms stages a table: the kernels run at the head of
 *                               the next render's chain, into the next scene version (and the next light version when a light's
 *                               node is bound); PROSPER_PT_UPDATE_NOW enqueues them on `stream` inside the call.  A
 *                               prosper_pt_update_transforms that is still pending is the base table, otherwise the current
 *                               table is; only entries a node binds are overwritten.
 * Refused by prosper_pt_set_animations: no scene (PROSPER_PT_ERR_NO_SCENE); a wrong struct_size, an index out of range, a parent
 * that does not precede its child, a model instance or light bound by two nodes, more than one CAMERA node, keyCount = 0,
 * key times that decrease, offsets past the arrays, a path / interpolation that does not exist, a valueWidth other than 3
 * for translation and scale or 4 for rotation.  By prosper_pt_animate: no animations set, unknown flags, a time that is not
 * finite. */
#define PROSPER_PT_ANIMATION_NONE 0xFFFFFFFFu
enum
{
    PROSPER_PT_NODE_HAS_TRANSLATION = 1u << 0,
    PROSPER_PT_NODE_HAS_ROTATION = 1u << 1,
    PROSPER_PT_NODE_HAS_SCALE = 1u << 2,
    PROSPER_PT_NODE_DIRECTIONAL_LIGHT = 1u << 3, /* the node carries the scene's directional light */
    PROSPER_PT_NODE_CAMERA = 1u << 4,            /* the node carries the current camera */
};
enum
{
    PROSPER_PT_ANIMATION_PATH_TRANSLATION = 0,
    PROSPER_PT_ANIMATION_PATH_ROTATION = 1,
    PROSPER_PT_ANIMATION_PATH_SCALE = 2,
};
enum
{
    PROSPER_PT_ANIMATION_STEP = 0,
    PROSPER_PT_ANIMATION_LINEAR = 1,
    PROSPER_PT_ANIMATION_CUBICSPLINE = 2,
};
typedef struct prosper_pt_animation_node
{
    uint32_t parent;        /* PROSPER_PT_ANIMATION_NONE: a root */
    uint32_t modelInstance; /* index into the scene's ModelInstanceTransforms, or PROSPER_PT_ANIMATION_NONE */
    uint32_t pointLight;    /* index into PointLightsBuffer.lights, or PROSPER_PT_ANIMATION_NONE */
    uint32_t spotLight;     /* index into SpotLightsBuffer.lights, or PROSPER_PT_ANIMATION_NONE */
    uint32_t flags;         /* PROSPER_PT_NODE_* */
    float translation[3];   /* the static pose */
    float rotation[4];      /* x, y, z, w as glTF stores it */
    float scale[3];
} prosper_pt_animation_node;
typedef struct prosper_pt_animation_channel
{
    uint32_t node;
    uint32_t path;          /* PROSPER_PT_ANIMATION_PATH_* */
    uint32_t interpolation; /* PROSPER_PT_ANIMATION_STEP / _LINEAR / _CUBICSPLINE */
    uint32_t timeOffset;    /* first of keyCount key times in times[] */
    uint32_t keyCount;
    uint32_t valueOffset;   /* first float in values[]: valueWidth per key, three times that for CUBICSPLINE
                             * (in-tangent, value, out-tangent) */
    uint32_t valueWidth;    /* 3 for translation and scale, 4 for rotation */
    float startTimeS;       /* min and max of the input accessor */
    float endTimeS;
} prosper_pt_animation_channel;
typedef struct prosper_pt_animation_desc
{
    uint32_t struct_size;
    uint32_t nodeCount;
    const prosper_pt_animation_node *nodes;
    uint32_t channelCount;
    uint32_t timeCount;
    const prosper_pt_animation_channel *channels;
    const float *times;
    const float *values;
    uint32_t valueCount; /* floats */
    uint32_t reserved;
} prosper_pt_animation_desc;
int prosper_pt_set_animations(prosper_pt_ctx *ctx, const prosper_pt_animation_desc *desc);
/* `flags`: 0 or PROSPER_PT_UPDATE_NOW. */
int prosper_pt_animate(prosper_pt_ctx *ctx, float timeS, uint32_t flags, void *stream);
typedef struct prosper_pt_animation_state
{
    float endTimeS;             /* the largest channel end (Scene::endTimeS) */
    uint32_t nodeCount;
    uint32_t animatedNodeCount; /* nodes a channel targets, and their descendants (WorldData.cpp:1279-1320) */
    uint32_t updates;           /* prosper_pt_animate calls whose kernels have been enqueued */
    uint32_t cameraValid;       /* 1: a CAMERA node exists and an update has run */
    uint32_t lightUpdates;      /* light versions made since the upload, by prosper_pt_update_lights or by an update here */
    float eye[3], target[3], up[3]; /* CameraTransform of the last enqueued update (World.cpp:416-426) */
    float sampleMs, hierarchyMs;    /* the two kernels of the last enqueued update, between events on its stream */
} prosper_pt_animation_state;
/* Enqueues a staged update first and waits for the last one's camera record.  Before prosper_pt_set_animations: all zero. */
int prosper_pt_get_animation_state(prosper_pt_ctx *ctx, prosper_pt_animation_state *out);
/* The scene's ModelInstanceTransforms table as the device holds it (`which` = 0; a staged update is enqueued first), or as
 * it held it before the last animated update (`which` = 1; the current one while none has run): what
 * prosper_pt_trace_gbuffer_velocity takes as previousTransforms.  `count` = the scene's modelInstanceCount.  Synchronises. */
int prosper_pt_read_animated_transforms(prosper_pt_ctx *ctx, uint32_t which, prosper_ModelInstanceTransforms *out, uint32_t count);
/* The three light buffers as the device holds them (a staged update is enqueued first).  Synchronises. */
int prosper_pt_read_lights(
    prosper_pt_ctx *ctx, prosper_DirectionalLightParameters *directionalLight, prosper_PointLightsBuffer *pointLights,
    prosper_SpotLightsBuffer *spotLights);
/* Test hook: per node the translation, rotation (x, y, z, w) and scale of the last update (`trs`, 10 floats a node) and its
 * world matrix (`world`, 16 floats a node, column by column); either may be NULL.  `nodeCount` = the animations' own. */
int prosper_pt_debug_read_animation_nodes(prosper_pt_ctx *ctx, float *trs, float *world, uint32_t nodeCount);

/* ---- incremental adoption: streamed-in textures and materials ----
 * prosper loads a scene in the background and adopts what has arrived a few items per frame: new images get their slot in
 * materialTextures[] (src/scene/WorldData.cpp:2182-2206), a material switches from its placeholder - the default material
 * with the real alpha mode (WorldData.cpp:817-826) - to the real one once its three images are there (:2208-2239), and the
 * next frame's material buffer is rewritten when that happened (:568-586; App.cpp:526-529, 601).  No acceleration structure
 * is touched.  Upload the scene with placeholder textures (1 x 1 texels will do) and placeholder materials, then:
 *   prosper_pt_update_textures   replaces the texels of materialTextures[first .. first + count) (any extent / format);
 *                                the caller's memory is borrowed for the call only.  Materials that sample a replaced
 *                                texture get their texture pack and alpha bounds rebuilt.
 *   prosper_pt_update_materials  replaces MaterialData[first .. first + count); an unchanged entry costs a memcmp (prosper
 *                                rewrites the whole table).  A material's alpha mode must be the one it was uploaded with:
 *                                it decides the opaque flag of the geometry (World.cpp:646-651).
 * Both only stage: the copies, re-tiling / BC7 decode, packs and alpha bounds run on a stream the context owns, and the next
 * render switches to a new version of the material / texture tables at the head of its own chain of launches, like
 * prosper_pt_update_transforms - the frames in flight (PROSPER_PT_RENDER_PIPELINED) keep reading theirs.  (One exception: a
 * changed MASK / BLEND material rewrites the any-hit records in place, behind the frames in flight.)  Every frame shows the
 * scene a fresh prosper_pt_upload_scene of that state would show, bit for bit. */
int prosper_pt_update_textures(prosper_pt_ctx *ctx, const prosper_pt_texture_desc *textures, uint32_t first, uint32_t count);

/* ---- texture mip chains (PROSPER_PT_CREATE_TEXTURE_MIPS) ----
 * prosper's raster passes sample material textures through full mip chains (materials.glsl:40-45).  A context created
 * with the flag keeps levels >= 1 of every texture beside its level 0, in the same tiling, also where level 0 itself
 * lives only in a material pack.  A generated level is the 2 x 2 box of its parent - child (i, j) = mean of parent
 * (2i, min(2i + 1, pw - 1)) x (2j, min(2j + 1, ph - 1)) - as (a + b + c + d + 2) >> 2 per channel; a texture that some
 * material uses as base colour (at the time its texels arrive) has RGB averaged in linear light instead: the device's
 * srgb_to_linear of the four codes, ((l00 + l10) + (l01 + l11)) * 0.25 in float32, and back to the code whose
 * srgb_to_linear(c / 255) is nearest (ties to the lower code).
 * The ray-traced passes go on sampling LOD 0. */
typedef struct prosper_pt_texture_mips_info
{
    uint32_t width, height;  /* level 0 of `texture` */
    uint32_t levelCount;     /* levels of its chain, level 0 included (1: no further level) */
    uint32_t srgbAveraged;   /* its generated levels were averaged in linear light */
    uint64_t mipTexelBytes;  /* the whole scene: texel bytes of all levels >= 1 (4 B per texel, without tile padding) */
} prosper_pt_texture_mips_info;
/* prosper's level count for an extent: max(floor(log2(max(w, h))) + 1 - 2, 1); 0 for an empty extent. */
uint32_t prosper_pt_texture_mip_level_count(uint32_t width, uint32_t height);
/* What prosper_pt_upload_scene / prosper_pt_update_textures of a context created with `create_flags` say about one
 * descriptor (PROSPER_PT_OK, or the refusal with its message in prosper_pt_last_error).  Touches no device. */
int prosper_pt_check_texture_desc(const prosper_pt_texture_desc *desc, uint32_t create_flags);
/* PROSPER_PT_ERR_UNSUPPORTED on a context created without PROSPER_PT_CREATE_TEXTURE_MIPS. */
int prosper_pt_get_texture_mips_info(prosper_pt_ctx *ctx, uint32_t texture, prosper_pt_texture_mips_info *out);
/* Test hook: level `level` of `texture` un-tiled into `rgba8` (max(w >> level, 1) * max(h >> level, 1) * 4 = `bytes`
 * bytes, row-major).  Level 0 of a texture that lives only in a material pack is PROSPER_PT_ERR_UNSUPPORTED.
 * Enqueued on `stream` and waited for. */
int prosper_pt_read_texture_level(prosper_pt_ctx *ctx, uint32_t texture, uint32_t level, void *rgba8, uint64_t bytes, void *stream);
/* Test hook: sample_texture_lod over n records.  in6: (u, v, du/dx, dv/dx, du/dy, dv/dy) per record, the uv forward
 * differences towards the pixel's right and lower neighbour; out5: (R, G, B, A, lambda).
 *   rho_x = |(du/dx * w, dv/dx * h)|, rho_y likewise, lambda = log2(max(rho_x, rho_y)) + bias   (Vulkan 1.3 §16.5.7, no
 *   anisotropy, lambda kept in float); an inf / NaN derivative gives +inf (the last level), rho = 0 gives -inf.
 *   lambda <= 0: the LOD-0 sample as every other pass takes it (magFilter), bit for bit.
 *   lambda > 0: levels floor(lambda) and min(floor(lambda) + 1, last), each through minFilter and the wrap modes,
 *   blended by the fraction. */
int prosper_pt_debug_sample_texture_lod(
    prosper_pt_ctx *ctx, uint32_t texture, uint32_t sampler, const float *in6, uint32_t n, float bias, float *out5);

/* ---- texture compression: what prosper's compress() does before it writes a cache file ----
 * src/scene/Texture.cpp:213-296 builds a mip chain truncated at 4x4, compresses it to BC7 when every level divides by 4 in
 * both directions (otherwise the chain stays RGBA8), and writes the levels back to back (src/utils/Dds.cpp:100-135).  The
 * BC7 encoder is a HIP kernel, one lane per 4x4 block, with a rule of the library's own (prosper's third-party encoder is
 * not part of its tree): single-subset modes 6, 5 and 4, rotation 0, integer arithmetic throughout; prosper_amd/bc7.py
 * (encode_blocks) states it and the kernel reproduces it bit for bit.  Generated levels are the 2 x 2 box of "texture mip
 * chains" above, not stb's resize: the result is a valid payload of prosper's cache whose texels are this library's. */
enum
{
    PROSPER_PT_COMPRESS_SRGB = 1u << 0,          /* generated levels average RGB in linear light (a base-colour texture) */
    PROSPER_PT_COMPRESS_GENERATE_MIPS = 1u << 1, /* Texture2DOptions::generateMipMaps */
};
/* What compress() decides for an extent, host only: the level count (prosper_pt_texture_mip_level_count, or 1 without
 * generateMips), the format (PROSPER_PT_FORMAT_BC7_UNORM if every level divides by 4 in both directions, else
 * PROSPER_PT_FORMAT_RGBA8_UNORM) and the payload size of the levels back to back.  Refused: null pointers, an empty extent. */
int prosper_pt_compressed_texture_layout(
    uint32_t width, uint32_t height, uint32_t generateMips, uint32_t *format, uint32_t *levelCount, uint64_t *bytes);
/* Compresses `src` (RGBA8) into `dst`.  src->mipLevelCount <= 1: the layout is that of
 * prosper_pt_compressed_texture_layout(width, height, flags & GENERATE_MIPS) and the levels are generated on the GPU;
 * src->mipLevelCount = n > 1: the caller's n levels are taken as they are (the layout's rule over those n levels; SRGB and
 * GENERATE_MIPS are not read).  `dstBytes` must be the payload size.  With the RGBA8 format `dst` receives the raw chain.
 * Needs no scene and no PROSPER_PT_CREATE_TEXTURE_MIPS; uses staging of the context that only grows; tiling, mip
 * generation and encoding run on `stream`, the payload is copied to `dst` and the call waits for it.  One call at a time
 * per context.
 * Refused with nothing launched: null pointers, an empty extent, a BC7 `src`, unknown flags, a chain of more than 16
 * levels, a supplied chain longer than prosper's count for the extent, a `dstBytes` that is not the payload size. */
int prosper_pt_compress_texture(
    prosper_pt_ctx *ctx, const prosper_pt_texture_desc *src, uint32_t flags, void *dst, uint64_t dstBytes, void *stream);
/* Device time of the stages of the last completed prosper_pt_compress_texture, between events on its stream: the source's
 * way up with tiling and mip generation, the encode kernels of all levels (the un-tiling on the RGBA8 fallback), the
 * payload's way back.  Refused before any call has completed. */
int prosper_pt_get_compress_texture_timing(prosper_pt_ctx *ctx, float *prepareMs, float *encodeMs, float *readbackMs);
/* Test hook: the encoder's device function over n loose blocks.  texels: n x 16 RGBA8 words (R in the low byte), row-major
 * inside the block; blocks: n x 4 words; sse: n squared errors of the decoded block against the source over all four
 * channels.  modeMask: bits 4, 5 and 6 enable that mode, 0 enables all; other bits are refused.  n = 0 succeeds and
 * does nothing.  Enqueued on `stream` and waited for. */
int prosper_pt_debug_bc7_encode_blocks(
    prosper_pt_ctx *ctx, const uint32_t *texels, uint32_t n, uint32_t modeMask, uint32_t *blocks, uint32_t *sse, void *stream);

/* ---- mesh preparation: what prosper's loadNextMesh does before it writes a mesh cache file ----
 * src/scene/DeferredLoadingContext.cpp: generateTangents (a primitive with uvs and no tangents), generateMeshlets,
 * packMeshData, writeCache.  mikktspace and meshoptimizer are not part of prosper's tree, so the tangents and the
 * meshlet partition follow rules of the library's own in prosper's layout and conventions: prosper_amd/tangents.py
 * (w as mikktspace: bitangent = w * cross(n, t); vertex count and indices unchanged, no reweld) and
 * prosper_amd/meshlets.py (a greedy scan; bounds with ordered=True).  Tangents, packing and the meshlet bounds are HIP
 * kernels that reproduce those statements bit for bit; the partition runs on the host. */
enum
{
    PROSPER_PT_PREPARE_GENERATE_TANGENTS = 1u << 0, /* prosper's condition: acts when `tangents` is NULL and `texCoord0s` is not */
    PROSPER_PT_PREPARE_MESHLETS = 1u << 1,          /* the four meshlet sections */
};
typedef struct prosper_pt_mesh_source
{
    const float *positions;  /* 3 per vertex */
    const float *normals;    /* 3 per vertex, or NULL */
    const float *tangents;   /* 4 per vertex, or NULL */
    const float *texCoord0s; /* 2 per vertex, or NULL */
    const uint32_t *indices; /* indexCount of them (may be NULL when indexCount is 0) */
    uint32_t vertexCount;
    uint32_t indexCount;
} prosper_pt_mesh_source;
/* The thirteen fields of the cache header that follow the source write time (DeferredLoadingContext.hpp:59-78): offsets
 * count u32 words from the start of the blob (meshletVerticesOffset: index entries, meshletTrianglesByteOffset: bytes),
 * 0xFFFFFFFF = absent. */
typedef struct prosper_pt_prepared_mesh
{
    uint32_t indexCount, vertexCount, meshletCount;
    uint32_t positionsOffset, normalsOffset, tangentsOffset, texCoord0sOffset;
    uint32_t meshletsOffset, meshletBoundsOffset, meshletVerticesOffset, meshletTrianglesByteOffset;
    uint32_t usesShortIndices, blobByteCount;
} prosper_pt_prepared_mesh;
/* Prepares `src` into a cache blob the context keeps: header and blob are word for word what
 * prosper_amd/mesh_cache.py pack_cache(..., with_meshlets = flags & MESHLETS, ordered=True) gives for the source's
 * tangents, or for the generated ones.  Needs no scene; uses staging of the context that only grows; runs on `stream`
 * and waits; one call at a time per context.  indexCount = 0 is valid: no meshlets.
 * Refused with nothing launched, the last result left as it is: null pointers, zero vertices, an index count that is not
 * a multiple of 3, an index at or past the vertex count, GENERATE_TANGENTS acting without normals, unknown flags, a blob
 * of 4 GiB or more. */
int prosper_pt_prepare_mesh(
    prosper_pt_ctx *ctx, const prosper_pt_mesh_source *src, uint32_t flags, prosper_pt_prepared_mesh *out, void *stream);
/* The blob of the last prosper_pt_prepare_mesh.  Refused: null pointers, a `bytes` that is not its blobByteCount, no call yet. */
int prosper_pt_read_prepared_mesh(prosper_pt_ctx *ctx, void *dst, uint64_t bytes);
/* The float32 tangents (4 per vertex) of the last prosper_pt_prepare_mesh that generated any.  Refused: null pointers, a
 * `bytes` that is not their size, no such call yet. */
int prosper_pt_read_prepared_tangents(prosper_pt_ctx *ctx, float *dst, uint64_t bytes);
/* Times of the last completed prosper_pt_prepare_mesh.  Between events on its stream: the source's way up with the tangent
 * sums, the finish-and-pack kernel, the partition's way up with the bounds kernel, the blob's (and tangents') way back.
 * On the host's clock: the meshlet partition.  Stages that did not run read 0 or close to it.  Refused before any call
 * has completed. */
int prosper_pt_get_prepare_mesh_timing(
    prosper_pt_ctx *ctx, float *tangentsMs, float *packMs, float *meshletHostMs, float *boundsMs, float *readbackMs);

/* The traced G-buffer (prosper_pt_trace_gbuffer, prosper_pt_trace_gbuffer_velocity, and the records that trace one) samples
 * material textures through their mip chains: context state, the counterpart of the lodBias prosper writes with its
 * material buffer each frame (Renderer::lodBias(): -1 while TAA is on, otherwise 0).  The uv derivatives are the forward
 * differences a rasteriser's quad would see: the pinhole rays through (px + 1, py) and (px, py + 1), with the pixel's
 * own jitter offset, met with the hit triangle's plane (a ray parallel to it or meeting it behind the eye: inf, the last
 * level).  The hit, depth, velocity and every debug draw type that does not show the material are unchanged.  Default:
 * off.  Refused: a lodBias that is not finite; enabling on a context created without PROSPER_PT_CREATE_TEXTURE_MIPS
 * (PROSPER_PT_ERR_UNSUPPORTED).  prosper_pt_forward_transparent follows the same state: every peeled layer is sampled
 * with the same two neighbour rays, met with the layer's own triangle plane.  The path tracer samples LOD 0. */
int prosper_pt_set_texture_lod(prosper_pt_ctx *ctx, int enabled, float lodBias);
/* Test hook: with it (and texture LOD on) the next traced G-buffer also writes, per pixel, the float4
 * (du/dx, dv/dx, du/dy, dv/dy) it sampled with, zeros on a miss; prosper_pt_read_texture_lod_derivatives copies it out
 * (width * height * 16 bytes). */
int prosper_pt_set_texture_lod_debug(prosper_pt_ctx *ctx, int enabled);
int prosper_pt_read_texture_lod_derivatives(prosper_pt_ctx *ctx, float *out, size_t bytes, void *stream);
int prosper_pt_update_materials(prosper_pt_ctx *ctx, const prosper_MaterialData *materials, uint32_t first, uint32_t count);

/* ---- incremental adoption: streamed-in meshes ----
 * prosper's mesh worker fills the geometry buffers in the background; WorldData::pollMeshWorker adopts at most ten finished
 * meshes per frame - their GeometryMetadata and MeshInfo slots, their byte range of a geometry buffer, a new 64 MB buffer
 * now and then (src/scene/WorldData.cpp:2003-2110; at most sMaxGeometryBuffersCount = 100 of them, :31).  Until then a mesh's
 * metadata holds bufferIndex = 0xFFFFFFFF; World::buildNextBlas builds a model's BLAS only once ALL its sub-meshes are there
 * (World.cpp:598-606) and a TLAS instance without a BLAS is inactive (accelerationStructureReference 0, World.cpp:909-915):
 * rays pass through model instances that are still loading.
 * Here: upload the scene with every mesh slot, draw instance and transform it will have; a mesh that has not arrived has
 * geometryMetadatas[i].bufferIndex == PROSPER_PT_ABSENT (the rest of its metadata and its MeshInfo are ignored), and a model
 * instance - a run of draw instances with one modelInstanceIndex - contributes triangles only once every mesh it draws is
 * there.  prosper_pt_update_meshes hands over the meshes that arrived: metadata and MeshInfo as pollMeshWorker stores them,
 * and the bytes the worker wrote (`bytes`, borrowed for the call) with their place in geometryBuffers[metadata.bufferIndex].
 * A buffer index the scene has not seen yet creates that buffer, `bufferByteSize` bytes large (ignored otherwise).
 * The call keeps a copy of the bytes, notes the tables and returns (0.1 ms): a worker thread of the context writes the
 * bytes to the device, lays the triangles out again, builds the subtrees of the model instances that became complete (the
 * others are kept), re-assembles the hierarchy and writes the per-triangle records - all into arrays of its own, on a
 * stream of its own (the calling thread touches no stream) - while the frame loop goes on
 * rendering the geometry it has, frames in flight included.  The first render (or prosper_pt_update_meshes, or
 * prosper_pt_finish_mesh_updates) after the worker is done switches to the new geometry; instances that moved or materials
 * that changed meanwhile are brought up to date by that switch.  This is prosper's own timing: a BLAS is built on the
 * GPU while frames are drawn and its instances appear when it exists.  Meshes that arrive while a build is under way are
 * taken up by the next one, started at the switch.  Textures, material tables, lights and sky are not touched.  Once a state
 * is switched in, a render shows what a fresh prosper_pt_upload_scene of that state would show, bit for bit.
 * prosper_pt_finish_mesh_updates waits until everything handed over so far is in the scene (screenshots, tests, the end of
 * loading).  A mesh can be handed over once; its material's alpha mode is the one the table holds at the time of the call.
 * A build that fails (out of memory, a hierarchy too deep for the traversal) is reported by the call that would have
 * switched to it; the scene stays as it was and the meshes wait for the next build. */
#define PROSPER_PT_MAX_GEOMETRY_BUFFERS 100u
typedef struct prosper_pt_mesh_update
{
    uint32_t meshIndex;
    uint32_t reserved;
    prosper_GeometryMetadata metadata; /* bufferIndex < PROSPER_PT_MAX_GEOMETRY_BUFFERS */
    prosper_pt_mesh_info info;
    const void *bytes;       /* UploadedGeometryData: the mesh's part of the geometry buffer ... */
    uint64_t byteOffset;     /* ... its place in that buffer (a multiple of 4) ... */
    uint64_t byteCount;      /* ... and size; every stream `metadata` names must lie inside */
    uint64_t bufferByteSize; /* size of geometryBuffers[metadata.bufferIndex] if the scene does not have that buffer yet */
} prosper_pt_mesh_update;
int prosper_pt_update_meshes(prosper_pt_ctx *ctx, const prosper_pt_mesh_update *meshes, uint32_t count);
int prosper_pt_finish_mesh_updates(prosper_pt_ctx *ctx);

/* Re-splits the instances that moved since the last build and re-assembles the tree on the host (one subtree per model
 * instance under a re-braided top level); synchronises the device.  prosper_pt_scene_stats.bvhBuildSeconds reports it. */
int prosper_pt_rebuild_hierarchy(prosper_pt_ctx *ctx);
typedef struct prosper_pt_hierarchy_state
{
    uint32_t refits;    /* since the scene was uploaded */
    uint32_t rebuilds;
    float costRatio;    /* sum of the inner boxes' half-areas after the last refit / right after the last build */
    float builtCost;
    uint32_t nodeCount;
    uint32_t levels;    /* kernel launches of a refit = levels + 1 */
    uint32_t meshUpdates;        /* prosper_pt_update_meshes calls that handed meshes over */
    uint32_t geometryInstalls;   /* background geometry builds whose result has become the scene */
    uint32_t geometryBuildRunning; /* 1: a build is under way (or meshes wait for one) */
    uint32_t reserved;
} prosper_pt_hierarchy_state;
/* Waits for the last refit's measure if it is still on its way. */
int prosper_pt_get_hierarchy_state(prosper_pt_ctx *ctx, prosper_pt_hierarchy_state *out);
/* Test hook: the node array as the device holds it (prosper_pt_scene_stats.nodeCount x nodeBytes). */
int prosper_pt_debug_read_nodes(prosper_pt_ctx *ctx, void *out, size_t byte_size);

/* ---- the hierarchy built on the GPU (opt-in) ----
 * prosper builds its acceleration structures on the GPU and its TLAS again every frame (src/scene/World.cpp:585-802, 878-928).
 * prosper_pt_build_hierarchy_gpu makes the whole 4-wide tree on the device from the device's own world triangles: a linear
 * BVH (Morton order, a binary radix tree, a collapse to the same 80-byte nodes; the rule is prosper_amd/lbvh.py), then the
 * refit that writes every box.  Same contract as prosper_pt_rebuild_hierarchy: a pending background geometry is installed
 * first, a staged update flushed, the device synchronised; it counts in `rebuilds`, resets costRatio to 1 and fills nodeCount,
 * maxDepth and bvhBuildSeconds.  Hits do not depend on the hierarchy, so the image is the one the host's tree gives, bit for
 * bit; a linear BVH traces slower than the host's SAH tree and builds much faster, which is why it is a choice.  A tree whose
 * stack bound exceeds what the traversal can hold is refused with PROSPER_PT_ERR_UNSUPPORTED and the scene stays exactly as it
 * was.  Leaves hold at most prosper_pt_debug_options.leafSize triangles (1 .. 4; 0: the default).
 * prosper_pt_set_hierarchy_builder: PROSPER_PT_BUILDER_HOST (the default) changes nothing.  With PROSPER_PT_BUILDER_GPU,
 * prosper_pt_rebuild_hierarchy runs the GPU build, and so does an update whose refits have degraded the tree past
 * rebuildCostRatio - inside that call, in place of the worker thread.  prosper_pt_upload_scene and prosper_pt_update_meshes
 * build on the host in either mode, unless prosper_pt_set_gpu_hierarchy_sites (below) gives them to the GPU builder.  After a
 * GPU build the next host build splits every instance again. */
#define PROSPER_PT_BUILDER_HOST 0u
#define PROSPER_PT_BUILDER_GPU 1u
int prosper_pt_build_hierarchy_gpu(prosper_pt_ctx *ctx);
int prosper_pt_set_hierarchy_builder(prosper_pt_ctx *ctx, uint32_t builder);
#define PROSPER_PT_HIERARCHY_BUILD_STAGES 8u
typedef struct prosper_pt_hierarchy_build_info
{
    uint32_t builder;         /* PROSPER_PT_BUILDER_* of the build that made the tree in use */
    uint32_t selectedBuilder; /* prosper_pt_set_hierarchy_builder */
    uint32_t leafSize;        /* most triangles per leaf of that build */
    uint32_t nodeCount;
    uint32_t levels;          /* node heights: kernel launches of a refit = levels + 1 */
    uint32_t depths;          /* 4-wide depths the GPU build numbered (0 after a host build) */
    uint32_t stackBound;      /* prosper_pt_scene_stats.maxDepth */
    uint32_t reserved;
    /* device milliseconds of a GPU build (0 after a host build): centroid bounds, codes, sort, radix tree, collapse and
     * numbering, heights, refit tables, and the switch (copies, permuted triangles, the first refit) */
    float stageMs[PROSPER_PT_HIERARCHY_BUILD_STAGES];
    float totalMs;
    uint32_t reserved2;
} prosper_pt_hierarchy_build_info;
int prosper_pt_get_hierarchy_build_info(prosper_pt_ctx *ctx, prosper_pt_hierarchy_build_info *out);
/* ---- the GPU builder's method (opt-in) ----
 * How prosper_pt_build_hierarchy_gpu, and every path that PROSPER_PT_BUILDER_GPU routes to it, makes the binary tree over the
 * Morton order.  PROSPER_PT_GPU_HIERARCHY_LINEAR (the default) is the radix tree above.  PROSPER_PT_GPU_HIERARCHY_PLOC merges
 * clusters round by round with their nearest neighbour within `radius` positions of that order (parallel locally-ordered
 * clustering; the rule is prosper_amd/ploc.py) and collapses by box cost: a tree of lower cost, a longer build.  Everything
 * else - the 4-wide nodes, the stack bound and its refusal, the refit, the hit contract - is the same.  radius: 1 .. 32, 0 for
 * the default; anything else, or an unknown method, is refused with PROSPER_PT_ERR_INVALID_ARGUMENT and the selection stays as
 * it was.  The call needs no scene and builds nothing.  Without a leaf size in prosper_pt_debug_options the PLOC method uses its
 * own default.  In prosper_pt_hierarchy_build_info the stage slot of the radix tree holds the clustering and the ranges. */
#define PROSPER_PT_GPU_HIERARCHY_LINEAR 0u
#define PROSPER_PT_GPU_HIERARCHY_PLOC 1u
int prosper_pt_set_gpu_hierarchy_method(prosper_pt_ctx *ctx, uint32_t method, uint32_t radius);
typedef struct prosper_pt_gpu_hierarchy_method_info
{
    uint32_t selectedMethod; /* prosper_pt_set_gpu_hierarchy_method */
    uint32_t selectedRadius; /* (the default's value where 0 was given) */
    uint32_t method;         /* of the build that made the tree in use; LINEAR, and 0 below, after a host build */
    uint32_t radius;         /* 0 for the linear method */
    uint32_t rounds;         /* clustering rounds of that build */
    uint32_t finishRounds;   /* those of them that ran in the single-workgroup launch */
    uint32_t reserved[2];
} prosper_pt_gpu_hierarchy_method_info;
/* Needs no scene: without one only the selection is filled. */
int prosper_pt_get_gpu_hierarchy_method_info(prosper_pt_ctx *ctx, prosper_pt_gpu_hierarchy_method_info *out);
/* ---- the GPU builder's build sites (opt-in) ----
 * Which of the builds that are not a rebuild the GPU builder makes: a mask of the sites below, 0 (none) by default and
 * independent of prosper_pt_set_hierarchy_builder.  A mask with an unknown bit is refused with
 * PROSPER_PT_ERR_INVALID_ARGUMENT and the selection stays as it was.  The call needs no scene and builds nothing; method,
 * radius and leaf size are those of every other GPU build.
 *   UPLOAD        prosper_pt_upload_scene makes the scene's first tree on the device: the flat world triangles never cross
 *                 to the host and no host build runs.  Afterwards prosper_pt_hierarchy_build_info reports
 *                 PROSPER_PT_BUILDER_GPU with the build's stages (slot 0 is the launch that writes the world triangles, the
 *                 shading and any-hit records and the centroid bounds in one pass), `rebuilds` is 0, costRatio 1, and
 *                 bvhBuildSeconds is the wall time of the build section.  A tree that is refused (the stack bound,
 *                 PROSPER_PT_ERR_UNSUPPORTED) fails the upload like any failed upload; there is no fall-back to the host:
 *                 clear the bit and upload again.
 *   MESH_UPDATES  the generations the worker thread builds for prosper_pt_update_meshes get their tree from the GPU builder,
 *                 on the worker's own stream and in scratch arrays of the worker's own (grow-only, 152 bytes a triangle,
 *                 plus 112 with the PLOC method, beside those of the synchronous GPU build); no subtree is kept.
 *   DRIFT         an update whose refits have degraded the tree past rebuildCostRatio starts such a background generation
 *                 with the GPU builder, under either selected builder, in place of the synchronous GPU rebuild and of the
 *                 host's re-split; the call does not wait for the device.
 * A refused or failed background build follows prosper_pt_update_meshes' contract: the call that would have switched to it
 * reports it, the scene stays, the meshes wait.  A layout without triangles takes the host's path under every site.  The
 * host builder's debug options flatBvh and noUploadRefit have no effect on a generation the GPU builder makes. */
#define PROSPER_PT_GPU_BUILD_SITE_UPLOAD 1u       /* prosper_pt_upload_scene */
#define PROSPER_PT_GPU_BUILD_SITE_MESH_UPDATES 2u /* the generations the worker thread builds for prosper_pt_update_meshes */
#define PROSPER_PT_GPU_BUILD_SITE_DRIFT 4u        /* the re-split that drifting instances trigger: a background generation */
int prosper_pt_set_gpu_hierarchy_sites(prosper_pt_ctx *ctx, uint32_t sites);
int prosper_pt_get_gpu_hierarchy_sites(prosper_pt_ctx *ctx, uint32_t *sites);
/* Test hook: the flat world triangles ((drawInstance, primitive) order, 48 bytes each) and the leaf-order permutation
 * (uint32 per triangle) as the device holds them; a staged update is flushed first. */
int prosper_pt_debug_read_hierarchy_arrays(
    prosper_pt_ctx *ctx, void *triangles, size_t triangle_bytes, void *permutation, size_t permutation_bytes);
int prosper_pt_get_scene_stats(prosper_pt_ctx *ctx, prosper_pt_scene_stats *out);

/* Optional: render into caller-owned device memory (localWidth*height RGBA32F texels, 16-byte
 * aligned) instead of the context's own buffer — lets the host framework (e.g. a torch tensor
 * that RCCL gathers) own the HDR tile.  NULL restores the internal buffer.  History is read from
 * and written to the same buffer, like the reference's aliased previous/illumination image. */
int prosper_pt_set_output_buffer(prosper_pt_ctx *ctx, void *device_rgba32f, size_t byte_size);

/* One accumulated frame = one path per pixel (the reference's traceRaysKHR(W,H,1)).
 * `stream` is a hipStream_t (NULL = the null stream); the call only enqueues work.  Stream semantics are
 * those of a kernel launch on `stream`: the render starts after the work already queued there and work
 * queued afterwards sees its result.  (Internally large batches run as two chains of launches on two
 * streams the context owns, forked from and joined back into `stream` with events.) */
int prosper_pt_render(
    prosper_pt_ctx *ctx, const prosper_ReferencePC *pc, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_tile_desc *tile, uint32_t render_flags,
    void *stream);

/* `frame_count` consecutive accumulated frames in one launch: exactly the pixels that
 * frame_count calls of prosper_pt_render with frameIndex = (pc->frameIndex + f) % 4096 and
 * PROSPER_PC_FLAG_SKIP_HISTORY honoured on the first of them only would produce (the running mean
 * of main.rgen:289-297 is kept in registers between frames instead of going through HBM). */
int prosper_pt_render_frames(
    prosper_pt_ctx *ctx, const prosper_ReferencePC *pc, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_tile_desc *tile, uint32_t frame_count,
    uint32_t render_flags, void *stream);

/* Width in texels of this context's HDR rows for the last render (== width when untiled). */
int prosper_pt_get_local_extent(prosper_pt_ctx *ctx, uint32_t *local_width, uint32_t *height);
/* Device address of the current HDR buffer (for RCCL gathers); valid until the next render with a
 * different extent, set_output_buffer or destroy. */
int prosper_pt_get_hdr_device_ptr(prosper_pt_ctx *ctx, void **out_ptr, size_t *out_bytes);
/* Synchronises `stream` and copies the HDR tile (localWidth*height RGBA32F) to host memory. */
int prosper_pt_read_hdr(prosper_pt_ctx *ctx, float *rgba32f, size_t byte_size, void *stream);
/* RGBA32F -> RGBA16F (round-to-nearest-even), the image later passes consume. */
int prosper_pt_blit_rgba16f(prosper_pt_ctx *ctx, uint16_t *host_rgba16f, size_t byte_size, void *stream);

/* The step after the path: prosper tone-maps the RGBA16F illumination into an RGBA8 UNORM
 * image with res/shader/tone_map.comp (src/render/ToneMap.cpp:62-128): exposure, HSV contrast, the
 * Tony McMapface 3-D LUT (res/texture/tony_mc_mapface.dds, 48^3 R9G9B9E5, linear / clamp sampler), 1/2.2
 * gamma.  prosper_pt_set_tone_map_lut copies dim^3 R9G9B9E5 texels (x fastest) to the device;
 * prosper_pt_tone_map runs blit + tone map in one kernel over the current HDR tile and writes
 * localWidth*height RGBA8 texels to `device_rgba8` (device memory, may be NULL) and/or `host_rgba8`
 * (host memory, may be NULL; synchronises `stream`). */
int prosper_pt_set_tone_map_lut(prosper_pt_ctx *ctx, const uint32_t *lut_r9g9b9e5, uint32_t dim);
int prosper_pt_tone_map(
    prosper_pt_ctx *ctx, float exposure, float contrast, void *device_rgba8, uint8_t *host_rgba8, size_t byte_size,
    void *stream);

/* A second client of the traversal: prosper's ReSTIR-DI trace pass,
 * res/shader/rt/direct_illumination/main.rgen:44-165 dispatched by src/render/rtdi/Trace.cpp:297.  Per pixel:
 * the surface from the G-buffer (world position from the non-linear depth through camera->clipToWorld,
 * signed-octahedral normal), the light its reservoir holds, one shadow ray with the scene's any-hit rules, the
 * BRDF, and the running mean into the context's HDR image (whole image, no stripes).
 * TracePC = res/shader/shared/shader_structs/push_constants/restir_di/trace.h. */
typedef struct prosper_pt_restir_trace_pc
{
    uint32_t drawType;   /* PROSPER_DRAW_TYPE_*: Default traces; Position shows positions, others the albedo */
    uint32_t frameIndex;
    uint32_t flags;      /* bit 0 skipHistory, bit 1 accumulate */
} prosper_pt_restir_trace_pc;
typedef struct prosper_pt_restir_inputs
{
    const void *albedoRoughness;  /* width*height float4: albedo.rgb, roughness        (gbuffer.frag) */
    const void *normalMetallic;   /* width*height float4: octNormal.xy, metallic, octNormal.z */
    const float *nonLinearDepth;  /* width*height */
    const void *reservoirs;       /* width*height float2: bits of the int light index (< 0 = none), weight */
    uint32_t onDevice;            /* 1: the pointers are device memory; 0: host memory, copied by the call */
    uint32_t reserved;
} prosper_pt_restir_inputs;
int prosper_pt_restir_di_trace(
    prosper_pt_ctx *ctx, const prosper_pt_restir_trace_pc *pc, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_restir_inputs *inputs, void *stream);

/* The two passes that produce the reservoirs the trace reads (src/render/rtdi/RtDirectIllumination.cpp:70-115), same
 * surface reconstruction, seeded per pixel with (px, py, frameIndex):
 *   PROSPER_PT_RESTIR_INITIAL  res/shader/restir_di/initial_reservoirs.comp: RIS over 5 uniformly drawn lights,
 *                              target luminance(irradiance * BRDF * NoL), no visibility.  inputs->reservoirs is ignored.
 *   PROSPER_PT_RESTIR_SPATIAL  res/shader/restir_di/spatial_reuse.comp: resamples up to 5 neighbour reservoirs of
 *                              inputs->reservoirs (disc offsets, 10 % depth and 0.9 normal tests).
 * Writes width*height float2 reservoirs to `device_out_reservoirs` (device memory, 8-byte aligned; it must not be
 * inputs->reservoirs), or with NULL to a context-owned buffer (prosper_pt_get_restir_reservoirs_device_ptr). */
enum
{
    PROSPER_PT_RESTIR_INITIAL = 0,
    PROSPER_PT_RESTIR_SPATIAL = 1,
};
int prosper_pt_restir_di_resample(
    prosper_pt_ctx *ctx, uint32_t stage, uint32_t frameIndex, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, const prosper_pt_restir_inputs *inputs, void *device_out_reservoirs, void *stream);
/* RtDirectIllumination::record: initial reservoirs, the spatial pass when recordFlags has
 * PROSPER_PT_RESTIR_SPATIAL_REUSE, then prosper_pt_restir_di_trace's pass, all with pc->frameIndex, on `stream`.
 * inputs->reservoirs is ignored: the reservoirs live in two context-owned device buffers (8 bytes per pixel each).
 * Host G-buffer inputs are copied once per call.  All three kernels read the same scene and light version. */
enum
{
    PROSPER_PT_RESTIR_SPATIAL_REUSE = 1u << 0,
    /* trace the G-buffer first (prosper_pt_trace_gbuffer with pc->drawType, pc->frameIndex) into the context-owned
     * buffers and run the passes over it; `gbuffer` may then be NULL and is ignored.  All four kernels read one scene
     * and light version. */
    PROSPER_PT_RESTIR_TRACE_GBUFFER = 1u << 1,
    /* with PROSPER_PT_RESTIR_TRACE_GBUFFER only: the jittered G-buffer (PROSPER_PT_GBUFFER_JITTER) */
    PROSPER_PT_RESTIR_JITTER_GBUFFER = 1u << 2,
};
int prosper_pt_restir_di_record(
    prosper_pt_ctx *ctx, const prosper_pt_restir_trace_pc *pc, uint32_t recordFlags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_restir_inputs *gbuffer, void *stream);
/* The reservoirs the last prosper_pt_restir_di_record traced with (or the context-owned buffer the last
 * prosper_pt_restir_di_resample wrote): width*height float2 in device memory, valid until the next record / resample
 * with a larger extent or destroy.  *out_bytes may be NULL. */
int prosper_pt_get_restir_reservoirs_device_ptr(prosper_pt_ctx *ctx, void **out_ptr, size_t *out_bytes);
/* Synchronises `stream` and copies those reservoirs (byte_size = width*height*8 of the call that made them) to host memory. */
int prosper_pt_read_restir_reservoirs(prosper_pt_ctx *ctx, float *host_float2, size_t byte_size, void *stream);

/* The G-buffer the ReSTIR-DI passes read, ray traced over the context's scene: the ray-traced stand-in for prosper's
 * raster GBufferRenderer (src/render/GBufferRenderer.cpp; res/shader/gbuffer.frag).  One lane per pixel traces the
 * path tracer's primary ray without depth of field (rt/reference/main.rgen:225-231, the same any-hit rules) and writes
 *   albedoRoughness  float4 (albedo.rgb, roughness); other draw types (debug_color, 1), MeshletID counts as Default
 *   normalMetallic   float4 (signedOctEncode(shading normal).xy, metallic, .z); 0 for the other draw types
 *   nonLinearDepth   float: clip.z / clip.w of cameraToClip * worldToCamera * (position, 1)
 * and zeros where the ray misses (the targets' clear values).  With PROSPER_PT_GBUFFER_JITTER the ray goes through
 * the pixel's jittered sample (px, py) + rnd2d01() of the path tracer's rng (px, py, frameIndex): each texel is then
 * that frame's primary hit.  Without, through the pixel centre (px + 0.5, py + 0.5), as a rasteriser samples.
 * Unlike the raster G-buffer: no velocity target and no TAA jitter (currentJitter) in this entry -
 * prosper_pt_trace_gbuffer_velocity has both -, no meshlet IDs, float storage, BLEND
 * surfaces follow the path tracer's stochastic transparency unless PROSPER_PT_GBUFFER_OPAQUE_ONLY leaves them out, and PrimitiveID is the geometry's triangle index.
 * `targets`: three caller-owned device buffers (16-byte aligned), or NULL for context-owned ones (grown as needed,
 * separate from the ReSTIR scratch).  Pending transform, light and material updates take effect first. */
enum
{
    PROSPER_PT_GBUFFER_JITTER = 1u << 0,
    /* Both G-buffer entries: a candidate whose material is BLEND is always rejected by the any-hit, as prosper keeps
     * BLEND geometry out of its G-buffer (draw_list_generator.comp:43-54); MASK keeps its cutoff, opaque geometry and
     * everything else about the targets is unchanged.  prosper_pt_forward_transparent draws the BLEND surfaces afterwards.
     * (Bit 2: bit 1 stays an unknown flag of both entries.) */
    PROSPER_PT_GBUFFER_OPAQUE_ONLY = 1u << 2,
};
typedef struct prosper_pt_gbuffer_targets
{
    void *albedoRoughness; /* width*height float4 */
    void *normalMetallic;  /* width*height float4 */
    float *nonLinearDepth; /* width*height float */
} prosper_pt_gbuffer_targets;
int prosper_pt_trace_gbuffer(
    prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, uint32_t flags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_gbuffer_targets *targets, void *stream);
/* The traced G-buffer as prosper's rasteriser samples it under TAA, with a fourth target, the velocity (gbuffer.frag:74-84,
 * forward.mesh:81-88, skybox.vert / skybox.frag).  The primary ray goes through the point whose projection
 * by camera->cameraToClip * worldToCamera is the pixel centre: uv = (px + 0.5, py + 0.5) / extent - currentJitter * 0.5
 * (the jittered projection moves NDC by + currentJitter on both axes).  The rng draw and the any-hit seed are
 * prosper_pt_trace_gbuffer's; with currentJitter = (0, 0) the three targets are byte-identical to that entry's without
 * PROSPER_PT_GBUFFER_JITTER.  `flags` is 0 or PROSPER_PT_GBUFFER_OPAQUE_ONLY.
 *   velocity  float2: (posNDC - currentJitter) - (prevPosNDC - previousJitter), y negated, each component clamped as
 *             fminf(fmaxf(v, -1), 1).  posNDC = xy / w of cameraToClip * worldToCamera * (positionWS, 1), prevPosNDC the
 *             same through previousCameraToClip * previousWorldToCamera of prevPositionWS: the interpolated model-space
 *             vertex through previousTransforms[modelInstanceIndex].modelToWorld, or positionWS itself without
 *             previousTransforms (previousTransformValid = 0).  Where the ray misses: the same of the ray's direction d
 *             with worldToCamera and previousWorldToCamera as mat4(mat3(.)).  Both projections go through the same code
 *             (fma chains, the camera row first), w comes from the matrices: an unchanged camera, unchanged instances
 *             and equal jitters give exactly (0, 0).
 * Unlike prosper: float2 storage instead of R16G16_SNORM, and the sky's velocity is clamped too (the SNORM target clamps
 * it on store).  The previous transforms are copied on `stream` into a grow-only device buffer of the context.  Refused:
 * flags other than PROSPER_PT_GBUFFER_OPAQUE_ONLY, a partly given target set, misaligned targets, previousTransformCount that differs from the scene's
 * modelInstanceCount (or is given without previousTransforms). */
typedef struct prosper_pt_velocity_gbuffer_desc
{
    prosper_pt_gbuffer_targets targets; /* all three given, or all three NULL for context-owned ones */
    void *velocity;                     /* width*height float2 on the device (8-byte aligned); NULL: context-owned */
    const prosper_ModelInstanceTransforms *previousTransforms; /* host, the scene's modelInstanceCount entries; NULL: the
                                                                * instances did not move */
    uint32_t previousTransformCount;
} prosper_pt_velocity_gbuffer_desc;
int prosper_pt_trace_gbuffer_velocity(
    prosper_pt_ctx *ctx, uint32_t drawType, uint32_t frameIndex, uint32_t flags, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, const prosper_pt_velocity_gbuffer_desc *desc, void *stream);
/* The velocity target the last prosper_pt_trace_gbuffer_velocity wrote and its extent; NO_SCENE before the first.
 * width / height may be NULL. */
int prosper_pt_get_velocity_device_ptr(prosper_pt_ctx *ctx, void **out, uint32_t *width, uint32_t *height);
/* Synchronises `stream` and copies that velocity target to host memory: `pixels` = width*height of that trace. */
int prosper_pt_read_velocity(prosper_pt_ctx *ctx, float *host_float2, size_t pixels, void *stream);
/* The last traced G-buffer (either kind of target) as inputs of the ReSTIR-DI entries (onDevice = 1, reservoirs =
 * NULL) and its extent; NO_SCENE before the first trace.  width / height may be NULL. */
int prosper_pt_get_gbuffer_device_ptrs(
    prosper_pt_ctx *ctx, prosper_pt_restir_inputs *out, uint32_t *width, uint32_t *height);
/* Synchronises `stream` and copies the last traced G-buffer to host memory: `pixels` = width*height of that trace;
 * any of the three pointers may be NULL. */
int prosper_pt_read_gbuffer(
    prosper_pt_ctx *ctx, float *host_albedo_roughness, float *host_normal_metallic, float *host_depth, size_t pixels,
    void *stream);

/* ---- clustered lighting and deferred shading (src/render/LightClustering.cpp, src/render/DeferredShading.cpp) ----
 * prosper's default lighting of its G-buffer: LightClustering::record then DeferredShading::record, compute passes
 * over the lights, the camera and the G-buffer, unshadowed.
 *
 * prosper_pt_cluster_lights: light_clustering.comp into context-owned buffers (grown as needed).  The grid is
 * ceil(width/32) x ceil(height/32) x 17 clusters; the frustum's tile scale comes from camera->resolution, the slices
 * from camera->near_ / far_.  Per cluster, x fastest: uint32 pair (indexOffset, pointCount << 16 | spotCount); cluster
 * k's uint16 light indices sit at [k * 256, k * 256 + pointCount + spotCount), points first, each list in ascending
 * light order.  A point light is listed where its sphere touches the cluster's frustum, every spot light everywhere.
 * More than 128 of one type: the 128 lowest indices are kept and the rest counted as dropped.  Pending transform,
 * light and material updates take effect first. */
int prosper_pt_cluster_lights(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, void *stream);
/* The grid of the last clustering (x, y, z = 17); NO_SCENE before the first.  Any pointer may be NULL. */
int prosper_pt_get_light_cluster_dims(prosper_pt_ctx *ctx, uint32_t *x, uint32_t *y, uint32_t *z);
/* Synchronises `stream` and copies the last clustering to host memory; any pointer may be NULL.  `clusters` =
 * x * y * z of that clustering.  host_pointers: clusters uint32 pairs; host_indices: clusters * 256 uint16 (entries past
 * a cluster's counts are unspecified); host_count: entries kept (the GLSL's lightIndicesCount); host_dropped: entries
 * past the 128 of a type; host_overflowing: clusters that dropped any. */
int prosper_pt_read_light_clusters(
    prosper_pt_ctx *ctx, uint32_t *host_pointers, uint16_t *host_indices, uint32_t *host_count, uint32_t *host_dropped,
    uint32_t *host_overflowing, size_t clusters, void *stream);

/* DeferredShadingPC (res/shader/shared/shader_structs/push_constants/deferred_shading.h) */
typedef struct prosper_pt_deferred_shading_pc
{
    uint32_t drawType; /* prosper_DrawType: Position writes the position, other non-Default types the G-buffer albedo */
    uint32_t ibl;      /* 1 adds evalIBL over the maps of prosper_pt_generate_ibl; refused with PROSPER_PT_ERR_UNSUPPORTED
                        * until they exist for the current scene */
} prosper_pt_deferred_shading_pc;
enum
{
    /* trace the G-buffer first (prosper_pt_trace_gbuffer with pc->drawType and `frameIndex`) into the context-owned
     * buffers; `gbuffer` may then be NULL and is ignored */
    PROSPER_PT_DEFERRED_TRACE_GBUFFER = 1u << 0,
    /* with PROSPER_PT_DEFERRED_TRACE_GBUFFER only: the jittered G-buffer (PROSPER_PT_GBUFFER_JITTER) */
    PROSPER_PT_DEFERRED_JITTER_GBUFFER = 1u << 1,
};
/* LightClustering::record + DeferredShading::record: clusters the lights (prosper_pt_cluster_lights) and shades every
 * G-buffer texel into the context's HDR image (width x height RGBA32F, alpha 1; prosper_pt_read_hdr, _blit_rgba16f and
 * _tone_map read it).  It overwrites whatever a render or a ReSTIR trace accumulated there.  The colour is the sun,
 * then the cluster's point lights, then its spot lights, unshadowed, then with pc->ibl = 1 evalIBL over the maps of
 * prosper_pt_generate_ibl (refused with PROSPER_PT_ERR_UNSUPPORTED until they exist).  A texel past the far plane (slice > 16) gets no
 * point or spot lights; one nearer than the near plane uses slice 0.  `gbuffer`: host or device inputs
 * (reservoirs ignored).  Pending updates are flushed once: both kernels read one scene and light version.
 * `frameIndex` is read only by PROSPER_PT_DEFERRED_JITTER_GBUFFER. */
int prosper_pt_deferred_shading(
    prosper_pt_ctx *ctx, const prosper_pt_deferred_shading_pc *pc, uint32_t flags, uint32_t frameIndex,
    const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const prosper_pt_restir_inputs *gbuffer,
    void *stream);

/* ---- forward transparent pass (src/render/ForwardRenderer.cpp recordTransparent, res/shader/forward.frag) ----
 * What prosper draws between the skybox and bloom (Renderer.cpp:493-500): the BLEND surfaces, lit forward
 * over the light clusters and alpha-blended over the shaded, sky-filled image, in place over the context's HDR image.
 * Use it over a G-buffer traced with PROSPER_PT_GBUFFER_OPAQUE_ONLY.  Additive: the ABI version stays 4.
 *
 * One lane per pixel follows the G-buffer's own ray of that pixel: through the centre (flags 0), through the path
 * tracer's sample (px, py) + rnd2d01() of rng (px, py, frameIndex) (PROSPER_PT_TRANSPARENT_JITTER), or through the centre
 * minus currentJitter * 0.5 as prosper_pt_trace_gbuffer_velocity traces (PROSPER_PT_TRANSPARENT_CAMERA_JITTER).  A LAYER
 * of the pixel is an intersection of that ray with a triangle
 *   - whose material's alphaMode is BLEND (opaque and MASK triangles are ignored: the depth is the occluder),
 *   - met from the front of the world-space triangle, cross(p1 - p0, p2 - p0) . d < 0 (back faces are culled),
 *   - whose sampleMaterial alpha is not 0,
 *   - whose non-linear depth - positionWS through cameraToClip * worldToCamera, as the traced G-buffer computes it - is
 *     strictly greater than the stored one (reverse-Z eGreater, no depth write): 0, the sky, passes everything, a layer
 *     coplanar with the opaque surface fails.
 * A layer's colour is forward.frag's: the surface of the hit with invViewRayWS = normalize(eye - positionWS), the sun,
 * the point and spot lights of clusterIndex(pixel, zCam) (zCam = (worldToCamera * position).z; slice rules as deferred
 * shading), unshadowed, then with pc->ibl = 1 evalIBL; its alpha a is the material's.  Other draw types than Default
 * (and MeshletID, which counts as Default) give (debug colour, 1).  The layers are composited sorted per pixel, nearest
 * last, by prosper's blend state: rgb = src.rgb * a + dst.rgb * (1 - a), alpha = a * (1 - a) of the nearest layer; equal
 * distances order by (drawInstance, primitive), the lower one nearer.  It is evaluated front to back (C += T a src,
 * T *= 1 - a, at the end C + T dst), and ends at T == 0 exactly: layers behind are neither shaded nor counted.  A pixel
 * without a layer keeps its four floats bit for bit.  (prosper draws in the order an atomic counter hands out; per-pixel
 * sorted is the defined order here, the same wherever one layer covers a pixel.)
 *
 * `nonLinearDepth`, `onDevice`: as prosper_pt_skybox_fill (NULL: the last traced G-buffer's depth).  The HDR image must
 * have this extent.  The lights are clustered first on `stream`, unless the context's last clustering was made with the
 * same camera terms and extent and no light update took effect since.  Pending scene updates are flushed once: every
 * kernel of the call reads one scene and light version.  Refused: both jitter flags, unknown flags, drawType out of
 * range, ibl not 0 or 1, ibl = 1 before prosper_pt_generate_ibl (PROSPER_PT_ERR_UNSUPPORTED). */
typedef struct prosper_pt_forward_pc /* ForwardPC (shared/shader_structs/push_constants/forward.h) */
{
    uint32_t drawType;
    uint32_t ibl;
    uint32_t previousTransformValid; /* not read: the pass writes no velocity */
} prosper_pt_forward_pc;
enum
{
    PROSPER_PT_TRANSPARENT_JITTER = 1u << 0,
    PROSPER_PT_TRANSPARENT_CAMERA_JITTER = 1u << 1,
};
int prosper_pt_forward_transparent(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, uint32_t flags, uint32_t frameIndex,
    const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const float *nonLinearDepth, uint32_t onDevice,
    void *stream);
typedef struct prosper_pt_transparent_info
{
    uint32_t coveredPixels; /* pixels with at least one layer */
    uint32_t maxLayers;     /* the deepest pixel's layer count */
    uint64_t totalLayers;
    float ms;               /* device time of the last call, its clustering included */
    uint32_t reclustered;   /* 1: the last call clustered the lights itself */
} prosper_pt_transparent_info;
/* Of the last prosper_pt_forward_transparent (waits for it); NO_SCENE before the first. */
int prosper_pt_get_transparent_info(prosper_pt_ctx *ctx, prosper_pt_transparent_info *out);
/* Debug mode, for tests: with layersPerPixel > 0 every later prosper_pt_forward_transparent also writes each pixel's
 * layer count and its first layersPerPixel layers, front to back, into a context-owned grow-only buffer (the image is
 * the same bit for bit).  0 (the default) turns it off. */
typedef struct prosper_pt_transparent_layer
{
    uint32_t drawInstance, primitive;
    float positionWS[3];
    float nonLinearDepth;
    float albedo[3];
    float roughness;
    float normal[3]; /* the shading normal */
    float metallic;
    float alpha;
    uint32_t reserved;
} prosper_pt_transparent_layer;
int prosper_pt_set_transparent_debug_layers(prosper_pt_ctx *ctx, uint32_t layersPerPixel);
/* Synchronises `stream` and copies what the last call in debug mode wrote: host_counts `pixels` uint32, host_layers
 * pixels * layersPerPixel records (pixel-major; records past a pixel's count are unspecified); either may be NULL.
 * `pixels` and `layersPerPixel` must be that call's.  NO_SCENE if the last call did not run in debug mode. */
int prosper_pt_read_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels,
    uint32_t layersPerPixel, void *stream);

/* ---- particles (src/render/particles/, res/shader/particles/) ----
 * What prosper runs between bloom and TAA (Renderer.cpp:530-538): a pool of maxParticleCount
 * prosper_pt_particle records and a freelist of its dead slots (int32 count, int32 indices[max]), both owned by the
 * context and resident on the device across frames and scenes.  Additive: the ABI version stays 4.
 *
 * prosper_pt_particles runs, on `stream`, the stages `stages` names, in Particles::record's order:
 *   1. decay    decay.comp: a slot with the Decay bit and lifetime <= 0 - with pc->reset every slot that is not dead -
 *               becomes (-9999) x 4 and its index is pushed on the freelist;
 *   2. init     only with pc->reset: init.comp, one emitter per vertex of the mesh of draw instance
 *               pc->sourceDrawInstanceIndex (position and normal through the instance's transform, lifetime 0, spawn
 *               rate 0.1 s, mask Emit), each in a slot popped from the freelist.  A source mesh that is not loaded yet
 *               (bufferIndex == PROSPER_PT_ABSENT or indexCount == 0) skips the stage, as Init::record returns false:
 *               the call succeeds and prosper_pt_particles_info.initRecorded is 0;
 *   3. simulate simulate.comp per slot with rng (slot, slot % 256, pc->simulateFrameIndex): move, gravity, decay of
 *               the lifetime, and for an emitter the random push, the 0.05 speed clamp and, every spawn rate, a child
 *               (lifetime 4, Gravity | Decay) in a popped slot.  A child is never simulated in the step that spawned
 *               it.  With deltaTimeS == 0 an emitter's velocity can become 0 / 0, as in the reference;
 *   4. render   render.vert / render.frag as a compute rasteriser, in place over the context's HDR image AND the depth:
 *               one camera-facing quad of +-0.001 per live slot (lifetime >= 0), yellow (1, 1, 0, 1) for an emitter,
 *               otherwise magenta (1, 0, 1, 1) with the dithered fade saturate(lifetime * 4) against sBayerMatrix
 *               shifted by pc->renderFrameIndex (% 8 the column, / 8 the row), depth-tested strictly greater (reverse
 *               Z) against the stored depth and written to it.  Coverage: corners snapped to 1/256 pixel, the strip's
 *               triangles (0, 1, 2) and (2, 1, 3), pixel centres, top-left rule, back faces culled; the quad's depth is
 *               z / w of its centre.  Among equal depths the lowest slot wins.  Untouched pixels keep colour and depth
 *               bit for bit.
 * A pop that finds the freelist dry is refused lane by lane: a launch with k requesters and c free slots grants exactly
 * min(k, c), and the count is never negative when a call returns (DESIGN.md f13 says how this differs from the
 * reference's dry case).
 *
 * pc->maxParticleCount: the pool's size, 0 = prosper's 500 000; a call with another size than the pool's reallocates it
 * fresh (every slot dead, count = max, indices[i] = i), as does the first call.  `camera`, `width`, `height`,
 * `nonLinearDepth` are read by render only.  `nonLinearDepth` NULL: the last traced G-buffer's depth, whose extent must
 * be width x height; otherwise DEVICE memory, width * height floats - the pass writes it, so host memory is refused.
 * Refused before anything is launched: unknown stage bits; reset not 0 or 1; with init requested (the INIT bit and
 * pc->reset) no scene, or sourceDrawInstanceIndex out of range; with render requested no camera, an empty extent or one
 * that differs from the HDR image's. */
typedef struct prosper_pt_particles_pc
{
    uint32_t maxParticleCount;        /* 0: 500 000 */
    uint32_t sourceDrawInstanceIndex; /* InitPC.drawInstanceIndex */
    uint32_t reset;                   /* DecayPC.decayAll, and init runs */
    float deltaTimeS;                 /* SimulatePC.deltaTimeS */
    uint32_t simulateFrameIndex;      /* SimulatePC.frameIndex */
    uint32_t renderFrameIndex;        /* RenderPC.frameIndex */
} prosper_pt_particles_pc;
enum
{
    PROSPER_PT_PARTICLES_DECAY = 1u << 0,
    PROSPER_PT_PARTICLES_INIT = 1u << 1,
    PROSPER_PT_PARTICLES_SIMULATE = 1u << 2,
    PROSPER_PT_PARTICLES_RENDER = 1u << 3,
    PROSPER_PT_PARTICLES_ALL = 15u,
};
int prosper_pt_particles(
    prosper_pt_ctx *ctx, const prosper_pt_particles_pc *pc, uint32_t stages, const prosper_CameraUniforms *camera,
    uint32_t width, uint32_t height, float *nonLinearDepth, void *stream);
typedef struct prosper_pt_particles_info
{
    uint32_t valid;            /* 1 once prosper_pt_particles ran on the current pool; the rest is of its last call */
    uint32_t initRecorded;     /* 1: init ran (0: not requested, or the source mesh is not loaded yet) */
    uint32_t maxParticleCount; /* of the pool */
    uint32_t liveCount;        /* maxParticleCount - freelistCount */
    uint32_t freelistCount;    /* the freelist's count behind the call */
    uint32_t grantedSpawns;    /* children simulate placed */
    uint32_t refusedSpawns;    /* ... and spawns it refused because the freelist was dry */
    uint32_t fragmentsWritten; /* pixels render wrote */
    float decayMs, initMs, simulateMs, renderMs; /* device time per stage (0 for a stage that did not run) */
} prosper_pt_particles_info;
/* Of the last prosper_pt_particles (waits for it). */
int prosper_pt_get_particles_info(prosper_pt_ctx *ctx, prosper_pt_particles_info *out);
/* Synchronises `stream` and copies the pool to host memory: `particles` maxParticleCount records, `freelist`
 * 1 + maxParticleCount int32 (the count, then the indices); either may be NULL.  maxParticleCount must be the pool's (0:
 * 500 000).  NO_SCENE before there is a pool. */
int prosper_pt_read_particles(
    prosper_pt_ctx *ctx, prosper_pt_particle *particles, int32_t *freelist, uint32_t maxParticleCount, void *stream);
/* Uploads a caller's pool of maxParticleCount slots (reallocating one of another size) and returns when the arrays have
 * been read: for tests that place designed states.  The count must lie in [0, maxParticleCount] and every one of the
 * maxParticleCount indices in [0, maxParticleCount): the kernels index the pool with them. */
int prosper_pt_set_particles(
    prosper_pt_ctx *ctx, const prosper_pt_particle *particles, const int32_t *freelist, uint32_t maxParticleCount,
    void *stream);

/* ---- debug lines (src/render/DebugRenderer.cpp, src/scene/DebugGeometry.hpp, res/shader/debug_lines.vert) ----
 * What prosper runs between the transparents and bloom (Renderer.cpp:502): the line-list pipeline of
 * DebugRenderer as a compute rasteriser, in place over the context's HDR image AND the depth of the last traced G-buffer,
 * where prosper_pt_particles draws.  Additive: the ABI version stays 4.
 *
 * `lines`: count * 9 floats (p0, p1, colour: DebugLines::addLine), host or device memory; the call copies them, so the
 * array may go once it returns.  At most 100 000 lines (DebugLines::sMaxLineCount); 0 lines launch nothing.
 *   projection  clip = cameraToClip * (worldToCamera * (p, 1)) in float32, each row one chain of fused multiply-adds;
 *   clipping    in homogeneous space against -w <= x, y <= w, 0 <= z <= w by a Liang-Barsky parameter interval; a line
 *               with a non-finite clip coordinate or an empty interval draws nothing and counts in linesClippedAway;
 *   fragments   Vulkan leaves non-strict lines to the implementation, so the rule is this library's own (DESIGN.md f16
 *               states it, tests/debug_view_reference.py restates it): along the major axis of the clipped segment in
 *               framebuffer coordinates, one fragment per pixel centre in [start, end) - half-open, so a polyline that
 *               keeps its direction writes no pixel twice and leaves no gap at a joint; the minor coordinate and z / w
 *               are interpolated linearly in screen space; a segment of zero length on screen writes nothing;
 *   depth       strictly greater (reverse Z) against the stored depth - equal loses - and written; colour (rgb, 1).
 * Among the fragments of one pixel the nearest wins, among equal depths the higher line index: the image does not depend
 * on the order the lines are walked in.  Untouched pixels keep colour and depth bit for bit.
 * Refused before anything is launched: more than 100 000 lines, a null camera (or null lines with count > 0), an empty
 * extent or one above 32768; NO_SCENE without a traced G-buffer of that extent; an HDR image of another extent. */
int prosper_pt_debug_lines(
    prosper_pt_ctx *ctx, const float *lines, uint32_t count, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, void *stream);
typedef struct prosper_pt_debug_lines_info
{
    uint32_t valid;            /* 1 once prosper_pt_debug_lines ran; the rest is of its last call */
    uint32_t lineCount;        /* lines it was given */
    uint32_t fragmentsWritten; /* pixels it wrote */
    uint32_t linesClippedAway; /* lines with a non-finite endpoint or an empty clip interval */
    float ms;                  /* device time of the two kernels */
} prosper_pt_debug_lines_info;
/* Of the last prosper_pt_debug_lines (waits for it). */
int prosper_pt_get_debug_lines_info(prosper_pt_ctx *ctx, prosper_pt_debug_lines_info *out);

/* ---- the registry of the context's 2-D images, and the one-texel readback (src/render/TextureReadback.cpp,
 * res/shader/texture_readback.comp; Renderer.cpp:510-514, App.cpp:583-631) ----
 * Every pass module lists the images it owns, in a fixed order: an index names the same image for the life of the
 * context.  The entries: the HDR "illumination"; the traced G-buffer's "albedoRoughness", "normalMetalness", "depth";
 * "velocity"; the IBL "SpecularBrdfLut"; depth of field's eight stages ("HalfResIllumination" with its mips as levels);
 * bloom's three working images (the two blur images hold levels firstLevel .. firstLevel + 2, numbered from 0 here) and
 * the FFT technique's four; TAA's "previousResolvedIllumination"; "toneMapped", the tone map's RGBA8 while the context keeps
 * it (prosper_pt_tone_map asked for a host copy alone).  Cube maps are not 2-D and are not listed.  Names are prosper's debug names where the reference creates
 * the corresponding image.
 * `valid` is 0 until the owning pass has run, and 0 again when what the entry described is gone: a G-buffer or velocity
 * target traced into a caller's buffers (the context cannot vouch for them), the TAA history after
 * prosper_pt_taa_release_history or a new scene, the LUT after a new scene, the tone-mapped
 * image after a tone map into the caller's buffer.  A valid entry means "what the last call of
 * its pass left": prosper's pool preserves an image that is marked for debug, this library does not - a later call of
 * the pass overwrites it.  No two entries share storage. */
enum
{
    PROSPER_PT_DEBUG_FORMAT_RGBA32F = 0,
    PROSPER_PT_DEBUG_FORMAT_RG32F = 1,
    PROSPER_PT_DEBUG_FORMAT_R32F = 2,
    PROSPER_PT_DEBUG_FORMAT_RGBA16F = 3,
    PROSPER_PT_DEBUG_FORMAT_RG16F = 4,
    PROSPER_PT_DEBUG_FORMAT_R16F = 5,
    PROSPER_PT_DEBUG_FORMAT_RG16_UNORM = 6,
    PROSPER_PT_DEBUG_FORMAT_RGBA8_UNORM = 7,
};
typedef struct prosper_pt_debug_resource
{
    char name[64];
    uint32_t format;     /* PROSPER_PT_DEBUG_FORMAT_* */
    uint32_t width;      /* of level 0; 0 while the entry is not valid */
    uint32_t height;
    uint32_t levelCount; /* level l is max(width >> l, 1) x max(height >> l, 1) */
    uint32_t valid;
} prosper_pt_debug_resource;
uint32_t prosper_pt_debug_resource_count(prosper_pt_ctx *ctx); /* 0 for a null context */
int prosper_pt_get_debug_resource(prosper_pt_ctx *ctx, uint32_t index, prosper_pt_debug_resource *out);
/* texture_readback.comp over level 0 of registry entry `resource`, on `stream`: uv = (pxX, pxY) / extent in float32, one
 * nearest clamp-to-edge sample - texel clamp(floor(u * width), 0, width - 1) - as a float4 into pinned memory behind a
 * fence.  Missing components read as Vulkan defines them, (r, 0, 0, 1) and (r, g, 0, 1); fp16 decodes exactly, UNORM
 * codes are divided by 65535 or 255.  Refused: a bad index or an entry that is not valid (NO_SCENE), non-finite pixel
 * coordinates, and a second record while one is queued and unread (the reference asserts on it). */
int prosper_pt_texture_readback(prosper_pt_ctx *ctx, uint32_t resource, float pxX, float pxY, void *stream);
/* Never blocks.  PROSPER_PT_NOT_READY while nothing is queued or the queued readback has not finished; otherwise the
 * value, once: the slot is free again. */
int prosper_pt_try_texture_readback(prosper_pt_ctx *ctx, float out[4]);
/* Streams: the readback and the viewer below read the image on `stream` as the owning pass left it; a caller that ran
 * that pass on another stream orders the two itself (an event, or a synchronise), as for every pass that reads what
 * another wrote. */

/* ---- the texture viewer (src/render/TextureDebug.cpp, res/shader/texture_debug.comp; Renderer.cpp:621) ----
 * prosper_pt_texture_debug views level pc->lod of registry entry `resource` as outRes.x x outRes.y RGBA8, one lane per
 * output texel, restating the shader as it is compiled (the magnifier's warp is commented out in its main() and is not
 * here; the magnifier's peek and marker are), in this order: uv = (texel + 0.5) / outRes; aspect correction, only when
 * inRes() != outRes, either branch; zoom 4x (uv * 0.25 + 0.375); black unless 0 <= uv <= 1, both ends inclusive;
 * textureLod(uv, lod) with clamp-to-edge - useBilinearSampler 0: texel clamp(floor(u * W), 0, W - 1); 1: u * W - 0.5, its
 * floor and the unquantised float32 fraction, the four texels blended as prosper_pt's BRDF LUT lookup blends; channel
 * select (0-3 one component in all three, above 3 xyz); abs; (c - range.x) / (range.y - range.x); with the magnifier flag
 * the marker squares of 3 and 2 pixels around the cursor snapped to its input texel; alpha 1; float -> UNORM8 as
 * prosper_pt_tone_map converts (NaN stores 0).  inRes() = max(inRes / (1 << lod), 1).  Missing components read
 * (0, 0, 1), fp16 decodes exactly, UNORM codes are divided by 65535 or 255.
 * flags: bits 0-2 the channel, bit 3 abs before range, bit 4 zoom, bit 5 magnifier (the shader's bitfieldExtract calls).
 * With the magnifier flag the lane of output texel (0, 0) writes the peek - the nearest sample at the snapped cursor
 * texel, or +inf four times when the snapped uv lies outside [0, 1) - into a slot of the context, copied to pinned
 * memory behind a fence; prosper_pt_get_texture_debug_peek waits for that fence (NO_SCENE before any magnifier call).
 * The output goes to device_rgba8 and / or host_rgba8 (then `stream` is synchronised), byte_size >= 4 * outRes.x *
 * outRes.y, as prosper_pt_tone_map takes them.
 * Refused (prosper clears to black there): a bad index or an entry that is not valid (NO_SCENE); pc->inRes other than
 * the entry's extent; lod above levelCount - 1; an empty outRes or one above 32768; non-finite range or cursorUv is NOT
 * refused (the arithmetic is the shader's); flag bits above 5; useBilinearSampler above 1. */
typedef struct prosper_pt_texture_debug_pc
{
    int32_t inRes[2];
    int32_t outRes[2];
    float range[2];
    uint32_t lod;
    uint32_t flags;
    float cursorUv[2];
} prosper_pt_texture_debug_pc;
enum
{
    PROSPER_PT_TEXTURE_DEBUG_CHANNEL_R = 0,
    PROSPER_PT_TEXTURE_DEBUG_CHANNEL_G = 1,
    PROSPER_PT_TEXTURE_DEBUG_CHANNEL_B = 2,
    PROSPER_PT_TEXTURE_DEBUG_CHANNEL_A = 3,
    PROSPER_PT_TEXTURE_DEBUG_CHANNEL_RGB = 4,
    PROSPER_PT_TEXTURE_DEBUG_ABS_BEFORE_RANGE = 1u << 3,
    PROSPER_PT_TEXTURE_DEBUG_ZOOM = 1u << 4,
    PROSPER_PT_TEXTURE_DEBUG_MAGNIFIER = 1u << 5,
};
int prosper_pt_texture_debug(
    prosper_pt_ctx *ctx, uint32_t resource, const prosper_pt_texture_debug_pc *pc, uint32_t useBilinearSampler,
    void *device_rgba8, uint8_t *host_rgba8, size_t byte_size, void *stream);
int prosper_pt_get_texture_debug_peek(prosper_pt_ctx *ctx, float out[4]);

/* ---- hierarchical depth (src/render/HierarchicalDepthDownsampler.cpp, res/shader/hiz_downsampler.comp) ----
 * HierarchicalDepthDownsampler::record: the depth pyramid prosper's meshlet culling tests bounding spheres against
 * (DESIGN.md f17).  Additive: the ABI version stays 4.
 *
 * Input: `width` x `height` floats of reverse-Z depth (sky = 0), both sides above 1 (the reference asserts it) and at
 * most 4096 (its twelve levels).  `nonLinearDepth` NULL: the last traced G-buffer's depth, whose extent must be
 * width x height; otherwise the caller's array, on the device when `onDevice` is not 0, else host memory the call copies.
 * Output: the context-owned pyramid of `slot` (0 or 1: prosper keeps the previous frame's beside this frame's), R32F,
 *   level 0            bit_ceil(width) / 2 x bit_ceil(height) / 2
 *   level l            max(level 0 >> l, 1) per side
 *   levels             floor(log2(larger side of level 0)) + 1
 * Texel (x, y) of level l is the MINIMUM of depth[min(Y, height - 1)][min(X, width - 1)] over the square
 * x * 2^(l+1) <= X < (x + 1) * 2^(l+1), likewise Y: the farthest depth of the footprint, source coordinates clamped to the
 * edge.  The minimum is exact and order-free, so every level is defined bit for bit.  Finite depths are assumed: a NaN
 * loses against a number, and a footprint of NaNs alone gives a NaN.
 * It needs no scene with a caller's depth.  A call on another stream than the slot's previous one waits for that one on
 * the device; the caller keeps the slot's READERS on other streams ahead of the next call into it.  prosper_pt_upload_scene invalidates both slots.
 * Refused: slot > 1, a side of 0, 1 or above 4096, NULL depth with no traced G-buffer or one of another extent. */
int prosper_pt_hiz_downsample(
    prosper_pt_ctx *ctx, uint32_t slot, const float *nonLinearDepth, uint32_t onDevice, uint32_t width, uint32_t height,
    void *stream);
typedef struct prosper_pt_hiz_info
{
    uint32_t valid;       /* 1: the slot holds the pyramid of the last prosper_pt_hiz_downsample into it; else the rest is 0 */
    uint32_t width;       /* extent of level 0 */
    uint32_t height;
    uint32_t levelCount;
    uint32_t sourceWidth; /* extent of the depth it was made from */
    uint32_t sourceHeight;
    uint32_t launches;    /* kernel launches of that call: 1, or 2 with more than six levels */
    uint32_t reserved;
} prosper_pt_hiz_info;
int prosper_pt_get_hiz_info(prosper_pt_ctx *ctx, uint32_t slot, prosper_pt_hiz_info *out);
/* Level `level` of the slot's pyramid on the device (row-major floats, its extent in *width / *height, which may be
 * NULL); valid until the next call into that slot or the next scene.  A reader on the producing call's stream is ordered
 * behind it already; a reader on another stream calls prosper_pt_hiz_wait first. */
int prosper_pt_get_hiz_device_ptr(
    prosper_pt_ctx *ctx, uint32_t slot, uint32_t level, const float **out, uint32_t *width, uint32_t *height);
/* Makes `stream` wait, on the device, for the last prosper_pt_hiz_downsample into `slot` (nothing to wait for before the
 * first): what a binder's own kernels that read prosper_pt_get_hiz_device_ptr's levels on another stream enqueue first. */
int prosper_pt_hiz_wait(prosper_pt_ctx *ctx, uint32_t slot, void *stream);
/* Synchronises `stream` (behind the producing call, whatever its stream) and copies the level to host memory;
 * `bytes` is at least the level's width * height * 4. */
int prosper_pt_read_hiz_level(prosper_pt_ctx *ctx, uint32_t slot, uint32_t level, float *host, size_t bytes, void *stream);

/* ---- meshlet culling (src/render/MeshletCuller.cpp, res/shader/draw_list_generator.comp, draw_list_culler.comp) ----
 * Prosper's two-phase visibility over the scene's meshlets: which meshlets of which draw instances the
 * camera can see, given a depth pyramid.  The scene carries meshlets in prosper's layout (GeometryMetadata's four meshlet
 * offsets, prosper_pt_mesh_info.meshletCount); a mesh without any contributes nothing.
 *
 * A draw list is prosper's: uint count; { drawInstanceIndex, meshletIndex }[count].  Beside each culled list lies its
 * argument triple: (count, 1, 1) - groupsX mirrors the count - or (0, 0, 0) when the culler had nothing to cull (the
 * argument writer's empty case).  The library cannot dispatch indirectly: it launches the culler over the host's upper
 * bound, MeshletCuller::recordGenerateList's meshletCountUpperBound, and lanes past the list's count leave.  The order of
 * a list's entries is whatever the atomics gave; the SET is the contract.
 *
 * first phase   generates the list of `mode` (OPAQUE: every material that is not BLEND; TRANSPARENT: BLEND only), then
 *               culls it: an instance whose uniform scale is 0 (non-uniform) is always visible; otherwise the six frustum
 *               planes of `camera`, the normal cone, and - with a pyramid slot - the occlusion test against that pyramid,
 *               draw_list_culler.comp restated operation for operation in float32.  With `hizSlot` = PROSPER_PT_NO_HIZ
 *               there is no occlusion test and no second-phase input.  Otherwise the meshlets that failed ONLY the
 *               occlusion test form the second-phase input list.
 * second phase  culls that list against another slot; never a third list.
 * prosper_pt_cull_gbuffer  GBufferRenderer::record's sequence: first phase (OPAQUE) against the pyramid the previous call
 *               kept, if any and if its source extent is camera->resolution; the pyramid of the last traced G-buffer's
 *               depth into the other slot; the second phase against it (when the first had a pyramid); that pyramid is kept
 *               as the next call's previous.  A new scene forgets it.
 * Pending transform, animation and material updates take effect first.  The context holds ONE set of lists: a call
 * replaces what the call before left.  Calls on different streams are ordered on the device like prosper_pt_debug_lines.
 * Refused: no scene; an unknown mode or list; a slot that is not valid; camera->resolution differing from the pyramid's
 * source extent; the second phase without a first phase that produced its input; meshlet ranges of a loaded mesh that
 * leave its geometry buffer (PROSPER_PT_ERR_SCENE; checked once per geometry generation). */
enum
{
    PROSPER_PT_CULL_MODE_OPAQUE = 0,
    PROSPER_PT_CULL_MODE_TRANSPARENT = 1,
};
enum
{
    PROSPER_PT_DRAW_LIST_GENERATED = 0,
    PROSPER_PT_DRAW_LIST_FIRST_PHASE = 1,
    PROSPER_PT_DRAW_LIST_SECOND_PHASE_INPUT = 2,
    PROSPER_PT_DRAW_LIST_SECOND_PHASE = 3,
    PROSPER_PT_DRAW_LIST_COUNT = 4,
};
#define PROSPER_PT_NO_HIZ 0xFFFFFFFFu
int prosper_pt_cull_meshlets_first_phase(
    prosper_pt_ctx *ctx, uint32_t mode, const prosper_CameraUniforms *camera, uint32_t hizSlot, void *stream);
int prosper_pt_cull_meshlets_second_phase(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t hizSlot, void *stream);
int prosper_pt_cull_gbuffer(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, void *stream);
/* Synchronises `stream` and copies list `which` to host memory: *count, its first min(count, capacity) pairs (`pairs`
 * may be NULL with capacity 0) and, for the two culled lists, the argument triple (zeros for the other two; `args3` may be
 * NULL).  PROSPER_PT_ERR_NO_SCENE for a list the last calls did not produce. */
int prosper_pt_read_draw_list(
    prosper_pt_ctx *ctx, uint32_t which, uint32_t *count, uint32_t *pairs, uint32_t capacity, uint32_t args3[3], void *stream);
/* The list on the device (count first, then the pairs; room for *capacity pairs) and, for the culled lists, its argument
 * triple (NULL otherwise): what a binder hands to its own indirect dispatch.  Valid until the next culling call. */
int prosper_pt_get_draw_list_device_ptr(
    prosper_pt_ctx *ctx, uint32_t which, const uint32_t **list, const uint32_t **args3, uint32_t *capacity);
/* render::DrawStats.  The totals are counted on the host as recordGenerateList counts them, for the first phase's mode;
 * drawnMeshletCount is the sum of both phases' visible counts; rasterizedTriangleCount the sum of the drawn meshlets'
 * triangleCount, counted by the culler (prosper counts it in its mesh shader).  The two device counts travel through pinned
 * memory behind the phases: with `wait` = 0 the call never blocks and returns PROSPER_PT_NOT_READY until they have landed,
 * with the host's four totals in *out and the two device counts zero. */
typedef struct prosper_pt_draw_stats
{
    uint32_t drawnMeshletCount;
    uint32_t rasterizedTriangleCount;
    uint32_t totalTriangleCount;
    uint32_t totalMeshletCount;
    uint32_t totalMeshCount;
    uint32_t totalModelCount;
} prosper_pt_draw_stats;
int prosper_pt_get_draw_stats(prosper_pt_ctx *ctx, prosper_pt_draw_stats *out, uint32_t wait);
/* Device time (ms) of the kernels of the last phases, between events on their stream (waits for them): the generator,
 * the first-phase culler, the second-phase culler (0 where the last first phase was not followed by one). */
int prosper_pt_get_cull_stage_ms(prosper_pt_ctx *ctx, float ms[3]);
/* The per-model-instance uniform scales of the current scene version (World.cpp:485-498: the common length of the three
 * rows of modelToWorld, 0 where they differ by more than 1e-4 relative), which the library computes on the GPU wherever a
 * version's ModelInstanceTransforms table is made: the upload, prosper_pt_update_transforms, prosper_pt_animate.  Pending
 * updates take effect first; synchronises `stream`.  `count` = the scene's model instances. */
int prosper_pt_read_instance_scales(prosper_pt_ctx *ctx, float *host, uint32_t count, void *stream);

/* ---- the rasteriser over the draw lists (src/render/GBufferRenderer.cpp recordDraw) ----
 * A compute rasteriser that consumes the culled lists: it draws the meshlets of a list into the context's VISIBILITY
 * IMAGE, one 64-bit key per pixel: the reverse-Z depth's bits above ~(ordinal * 128 + meshlet triangle), 0 where nothing
 * is drawn.  ordinal = (prefix sum of the meshlet counts of the draw instances before this one) + meshletIndex.  The
 * greatest depth wins (eGreater against the clear value 0); among equal depths the lowest (drawInstanceIndex,
 * meshletIndex, triangle), whatever order the GPU ran in.  Vulkan's rasteriser cannot run here: the fragment rule
 * (vertices, snapping to 1/256 pixel, 64-bit edge functions with the top-left rule, back-face culling, the clipper and
 * its guard band, the depth) is this library's own, written out in DESIGN.md (f18) and restated in
 * tests/raster_reference.py.  Additive: the ABI version stays 4.
 *
 * prosper_pt_raster_meshlets    draws list `which` (GENERATED - the unculled list -, FIRST_PHASE or SECOND_PHASE) of the last
 *                               culling calls with `camera` (its worldToCamera, cameraToClip and resolution).  With
 *                               PROSPER_PT_RASTER_CLEAR every key is set to 0 first and the image takes camera->resolution;
 *                               without it the draw loads what is there (GBufferRenderer.cpp:475 loadOp).
 * prosper_pt_raster_visibility  GBufferRenderer::record's sequence over the rasteriser's OWN depth: first phase (OPAQUE)
 *                               against the pyramid the previous call kept, if any and if its source extent is
 *                               camera->resolution; clear and draw; when the first phase had a pyramid: the image's depth ->
 *                               pyramid in the other slot -> second phase -> draw without clear; the depth -> pyramid, kept
 *                               as the next call's previous.  The kept slot is the one prosper_pt_cull_gbuffer keeps; a new
 *                               scene forgets it.  The image then equals the one drawn from the GENERATED list.
 * Pending transform, animation and material updates take effect first.  Calls on different streams are ordered on the
 * device like prosper_pt_debug_lines.  MASK materials: gbuffer.frag:61-63 discards a fragment whose sampleMaterial alpha is 0
 * (the raw alpha * factor < cutoff, not the any-hit's sampleAlpha) before the depth write; the rasteriser makes that test
 * before its atomic with the resolve's own surface code - same pixel ray, same uv, same texture LOD state
 * (prosper_pt_set_texture_lod, camera->currentJitter) - so a draw and its resolve take the same camera and LOD state.
 * Refused before anything is launched: no scene or no meshlets in it (PROSPER_PT_ERR_NO_SCENE); a list the last culling
 * calls did not produce (PROSPER_PT_ERR_NO_SCENE); unknown flags or lists; camera->resolution empty, a side above 16384
 * (prosper_pt_raster_visibility: not above 1, or above 4096), or differing from the image's extent on a draw without
 * CLEAR; 2^25 meshlets or more (PROSPER_PT_ERR_SCENE).  A refused call leaves everything as it was.  A call that FAILS
 * later (a HIP or memory error) leaves the lists and the image as its steps so far made them, as a failed culling call
 * does; prosper_pt_raster_visibility then still keeps the pyramid it had kept before. */
#define PROSPER_PT_RASTER_CLEAR 1u
int prosper_pt_raster_meshlets(prosper_pt_ctx *ctx, uint32_t which, uint32_t flags, const prosper_CameraUniforms *camera, void *stream);
int prosper_pt_raster_visibility(prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, void *stream);
/* The resolve of the visibility image into the G-buffer targets, and GBufferRenderer::record:146-231 as one chain.
 *   prosper_pt_raster_resolve  albedoRoughness, normalMetalness, velocity and depth of camera->resolution from the image.
 *       Nothing is interpolated in screen space: for the pixel's winning triangle the pixel's own ray is formed as
 *       prosper_pt_trace_gbuffer_velocity forms it (centre minus currentJitter * 0.5), its barycentrics on the world-space
 *       triangle are taken unclamped, and from that hit the traced kernel's own code runs (material, texture LOD of
 *       prosper_pt_set_texture_lod, normal encoding, velocity with previous transforms, the debug draw types): where the
 *       traced G-buffer hits the same triangle the three attribute targets are bit-identical.  The depth is the
 *       rasteriser's.  MeshletID writes (uintToColor(meshletIndex), 1) and zeros (gbuffer.frag:88-93), PrimitiveID the
 *       meshlet-local triangle (forward.mesh:144).  Uncovered pixels get the clear values and the sky's velocity.
 *       `desc` and its refusals are prosper_pt_trace_gbuffer_velocity's: targets caller-owned or context-owned.  With
 *       context-owned targets the result IS the context's last G-buffer and velocity target for every call that takes
 *       "NULL: the last traced G-buffer".  Refused also: nothing drawn on this scene or on its geometry as it is now (meshes arrived since), an extent other than
 *       the image's.
 *   prosper_pt_raster_gbuffer  prosper_pt_raster_visibility, then the resolve.
 * A meshlet triangle is mapped to the mesh's index-buffer triangle with the same three vertices (any rotation, the
 * lowest on duplicates), on the host, by the first draw after a mesh arrived (per mesh: the others' maps are kept); a meshlet triangle without one, or
 * meshlet sections that leave the buffer, are PROSPER_PT_ERR_SCENE. */
int prosper_pt_raster_resolve(
    prosper_pt_ctx *ctx, uint32_t drawType, const prosper_CameraUniforms *camera, const prosper_pt_velocity_gbuffer_desc *desc, void *stream);
int prosper_pt_raster_gbuffer(
    prosper_pt_ctx *ctx, uint32_t drawType, const prosper_CameraUniforms *camera, const prosper_pt_velocity_gbuffer_desc *desc, void *stream);
/* GBufferRenderer::releasePreserved: forgets the pyramid the last sequence kept (prosper_pt_raster_visibility /
 * prosper_pt_raster_gbuffer / prosper_pt_cull_gbuffer): the next one runs a single phase, as the first after an upload. */
int prosper_pt_raster_release_preserved(prosper_pt_ctx *ctx);
/* ---- forward opaque pass (src/render/ForwardRenderer.cpp recordOpaque, forward.frag) ----
 * The third way to the opaque image (Renderer.cpp:404-483, m_renderDeferred == false): every pixel's winning triangle of
 * the visibility image is shaded directly over the light clusters, without a G-buffer in between.  Additive: the ABI
 * version stays 4.
 *   prosper_pt_raster_forward_shade  over the image as drawn.  A covered pixel's surface is the resolve's (the pixel's own
 *       ray, unclamped barycentrics on the world-space triangle, the traced kernel's material code, the texture LOD of
 *       prosper_pt_set_texture_lod) with forward.frag's view vector normalize(eye - positionWS); its colour is the sun, then
 *       the point and spot lights of clusterIndex(pixel, zCam) with zCam = (worldToCamera * position).z, unshadowed, then
 *       with pc->ibl = 1 evalIBL - what prosper_pt_forward_transparent sums for a layer; its alpha is the material's where
 *       that is above 0, else 1.  Other draw types than Default write (colour, 1) with the colour the resolve writes to
 *       albedoRoughness: MeshletID uintToColor(meshletIndex), PrimitiveID the meshlet-local triangle, the rest the debug
 *       colour.  Velocity (whatever the draw type) and depth are the resolve's, bit for bit.  An uncovered pixel gets
 *       (0, 0, 0, 0), depth 0 and the sky's velocity.  pc->previousTransformValid is not read: desc->previousTransforms
 *       decides.
 *   prosper_pt_raster_forward  prosper_pt_raster_visibility, then the shade: ForwardRenderer::recordOpaque:134-217.  The
 *       kept pyramid is the one prosper_pt_raster_gbuffer and prosper_pt_cull_gbuffer keep, and
 *       prosper_pt_raster_release_preserved is ForwardRenderer::releasePreserved as well.
 * The illumination is the context's HDR image at camera->resolution, overwritten and sized as prosper_pt_deferred_shading
 * does.  The lights are clustered first on `stream`, unless the context's last clustering serves (same camera terms and
 * extent, no light update since).  Pending scene updates are flushed once; calls on different streams are ordered on the
 * device as prosper_pt_raster_gbuffer orders them.
 * The depth and the velocity become the context's last depth and last velocity target for every call that takes "NULL:
 * the last traced G-buffer's" of either (prosper_pt_skybox_fill, prosper_pt_forward_transparent, prosper_pt_debug_lines,
 * prosper_pt_hiz_downsample, prosper_pt_taa_resolve, prosper_pt_depth_of_field, prosper_pt_particles,
 * prosper_pt_get_velocity_device_ptr).  A forward frame has no albedo or normal target: until the next G-buffer,
 * prosper_pt_get_gbuffer_device_ptrs and prosper_pt_read_gbuffer answer "no G-buffer has been traced yet", and the
 * registry lists albedoRoughness and normalMetalness as not yet run, depth as valid.
 * Refused before anything is launched, the HDR image, the depth and the velocity left as they were: what
 * prosper_pt_raster_resolve refuses (nothing drawn, geometry changed since, another extent, an unmatched triangle); drawType
 * out of range, ibl not 0 or 1, ibl = 1 before prosper_pt_generate_ibl (PROSPER_PT_ERR_UNSUPPORTED), a camera without
 * 0 < near_ < far_; a depth target that is not 4-byte or a velocity target that is not 8-byte aligned; a
 * previousTransformCount that is not the scene's modelInstanceCount, or one without previousTransforms. */
typedef struct prosper_pt_forward_opaque_desc
{
    float *nonLinearDepth; /* width*height float on the device; NULL: context-owned */
    void *velocity;        /* width*height float2 on the device (8-byte aligned); NULL: context-owned */
    const prosper_ModelInstanceTransforms *previousTransforms; /* as prosper_pt_velocity_gbuffer_desc */
    uint32_t previousTransformCount;
} prosper_pt_forward_opaque_desc;
int prosper_pt_raster_forward_shade(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc, void *stream);
int prosper_pt_raster_forward(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const prosper_pt_forward_opaque_desc *desc, void *stream);
/* Debug mode, for tests: every later forward shade also writes one prosper_pt_transparent_layer per pixel into a
 * context-owned buffer - drawInstance, the geometry primitive, positionWS, the key's nonLinearDepth, albedo, roughness, the
 * shading normal, metallic, alpha; drawInstance 0xFFFFFFFF (and zeros) where nothing is drawn.  The images are the same
 * bit for bit.  prosper_pt_read_forward_surfaces synchronises `stream` and copies the `pixels` records of the last call
 * out; NO_SCENE if that call did not run in debug mode. */
int prosper_pt_set_forward_debug_surfaces(prosper_pt_ctx *ctx, int enabled);
int prosper_pt_read_forward_surfaces(prosper_pt_ctx *ctx, prosper_pt_transparent_layer *out, size_t pixels, void *stream);
typedef struct prosper_pt_forward_opaque_info
{
    uint32_t shadedPixels; /* covered pixels */
    uint32_t reclustered;  /* 1: the last call clustered the lights itself */
    float ms;              /* device time of the last shade, its clustering included */
    float shadeMs;         /* of the shade kernel alone */
} prosper_pt_forward_opaque_info;
/* Of the last forward shade; never blocks: PROSPER_PT_NOT_READY (only `reclustered` filled in) while it is still running,
 * NO_SCENE before the first. */
int prosper_pt_get_forward_opaque_info(prosper_pt_ctx *ctx, prosper_pt_forward_opaque_info *out);
/* The depth target of the last forward frame, while it is the context's last depth (NO_SCENE before a forward frame and
 * after the next G-buffer): its device pointer and extent, and a copy to the host that synchronises `stream`; `pixels`
 * must be its width * height.  The velocity is prosper_pt_get_velocity_device_ptr's and prosper_pt_read_velocity's. */
int prosper_pt_get_forward_depth_device_ptr(prosper_pt_ctx *ctx, float **out, uint32_t *width, uint32_t *height);
int prosper_pt_read_forward_depth(prosper_pt_ctx *ctx, float *host_depth, size_t pixels, void *stream);
/* ---- rasterised transparent pass (src/render/ForwardRenderer.cpp recordTransparent:222-260) ----
 * The BLEND layers of the raster frame, from the meshlet draw lists instead of a ray per pixel: the rasteriser's own
 * coverage (the top-left rule the opaque image was drawn with), meshlet culling, draw statistics, and no hierarchy in the
 * loop.  In place over the context's HDR image, which must have camera->resolution.  Additive: the ABI version stays 4,
 * prosper_pt_forward_transparent stays.
 *
 * A LAYER CANDIDATE of a pixel is a fragment of the rasteriser's rule above (same vertices, snapping, edge functions,
 * culling, clipper and depth) of a triangle of the list's meshlets
 *   - whose depth is strictly greater than the stored depth of the pixel (reverse-Z eGreater, no depth write): a stored 0
 *     passes everything, a coplanar fragment fails;
 *   - whose sampleMaterial alpha is not 0 (forward.frag:57), decided by the MASK discard's own code: the pixel's ray, the
 *     uv and the texture LOD state of prosper_pt_set_texture_lod.
 * Every candidate contributes the visibility image's key, depth bits above ~(ordinal * 128 + triangle).  The keys of one
 * pixel are unique and totally ordered: the greatest is the nearest, on equal depths the lowest (drawInstanceIndex,
 * meshletIndex, triangle).  The lists are built in three steps - a raster pass that counts, an exclusive scan of the
 * per-pixel counts, the same raster pass again that fills - and resolved with one lane per pixel: front to back, each layer
 * with the surface prosper_pt_raster_forward_shade gives a winner, forward.frag's colour and alpha as there, composited
 * as prosper_pt_forward_transparent composites (C += T a src, T *= 1 - a, the end C + T dst at T == 0 or after the last
 * layer; alpha = a (1 - a) of the nearest layer).  A pixel without a layer keeps its four floats bit for bit.  Other draw
 * types than Default show the nearest layer with alpha 1: MeshletID uintToColor(meshletIndex), PrimitiveID the
 * meshlet-local triangle, the rest the debug colour.
 *
 *   prosper_pt_raster_transparent_draw     count, scan, fill and resolve over list `which` (GENERATED, FIRST_PHASE or
 *       SECOND_PHASE) of the last culling call.
 *   prosper_pt_raster_forward_transparent  recordTransparent: the first phase in TRANSPARENT mode with PROSPER_PT_NO_HIZ,
 *       then the draw of FIRST_PHASE.  The context holds ONE set of draw lists: after the call they are the transparent
 *       ones, and prosper_pt_get_draw_stats reports this cull.  The pyramid prosper_pt_raster_visibility kept is untouched.
 * THE CALL BLOCKS THE HOST ONCE, between scan and fill: it reads the 4-byte total of the scan from pinned memory behind an
 * event and grows the context-owned, grow-only fragment buffer to it.  A total of 0 launches nothing further.
 * `nonLinearDepth`, `onDevice`: as prosper_pt_skybox_fill (NULL: the context's last depth, a forward frame's included).
 * The lights are clustered first on `stream` unless the context's last clustering serves; pending scene updates are flushed
 * once; calls on different streams are ordered on the device as prosper_pt_raster_gbuffer orders them.
 * Refused before anything is launched, the image left as it was: what prosper_pt_raster_meshlets refuses (no scene, no
 * meshlets, a list the last culling calls did not produce, an unknown list, camera->resolution empty or above 16384);
 * drawType out of range, ibl not 0 or 1, ibl = 1 before prosper_pt_generate_ibl (PROSPER_PT_ERR_UNSUPPORTED), a camera
 * without 0 < near_ < far_, a depth that is not 4-byte aligned, NULL before any depth exists; an HDR image or a last depth
 * whose extent is not camera->resolution. */
int prosper_pt_raster_transparent_draw(
    prosper_pt_ctx *ctx, uint32_t which, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const float *nonLinearDepth,
    uint32_t onDevice, void *stream);
int prosper_pt_raster_forward_transparent(
    prosper_pt_ctx *ctx, const prosper_pt_forward_pc *pc, const prosper_CameraUniforms *camera, const float *nonLinearDepth, uint32_t onDevice,
    void *stream);
typedef struct prosper_pt_raster_transparent_info
{
    uint32_t fragments;     /* layer candidates in all lists (the scan's total) */
    uint32_t coveredPixels; /* pixels with at least one */
    uint32_t shadedLayers;  /* layers the resolve shaded: those behind a pixel's T == 0 are not */
    uint32_t maxLayers;     /* the longest list */
    uint32_t reclustered;   /* 1: the call clustered the lights itself */
    float countMs;          /* device time of the counting raster pass ... */
    float scanMs;           /* ... the scan ... */
    float fillMs;           /* ... the filling raster pass ... */
    float resolveMs;        /* ... and the resolve, its clustering included */
    uint32_t reserved;
} prosper_pt_raster_transparent_info;
/* Of the last pass; never blocks: PROSPER_PT_NOT_READY (`fragments` and `reclustered` filled in) until the counts have
 * landed, NO_SCENE before the first. */
int prosper_pt_get_raster_transparent_info(prosper_pt_ctx *ctx, prosper_pt_raster_transparent_info *out);
/* Synchronises `stream` and decodes the lists of the last pass on the host: `counts` pixels uint32, and the fragments
 * pixel after pixel - a pixel's run starts at the sum of the counts before it - each run sorted front to back.  *total: the
 * fragments in all lists (with counts and fragments NULL the call only reports it, without synchronising).  `pixels` must
 * be the pass's width * height, `capacity` at least *total. */
typedef struct prosper_pt_raster_fragment
{
    uint32_t drawInstance, meshlet, triangle;
    float depth;
} prosper_pt_raster_fragment;
int prosper_pt_read_raster_fragments(
    prosper_pt_ctx *ctx, uint32_t *counts, size_t pixels, prosper_pt_raster_fragment *fragments, size_t capacity, uint64_t *total, void *stream);
/* Debug mode, for tests, as prosper_pt_set_transparent_debug_layers: with layersPerPixel > 0 (at most 128) every later pass
 * also writes each pixel's count of SHADED layers and the first layersPerPixel of them, front to back (`primitive` is the
 * geometry triangle, nonLinearDepth the key's depth); the image is the same bit for bit. */
int prosper_pt_set_raster_transparent_debug_layers(prosper_pt_ctx *ctx, uint32_t layersPerPixel);
int prosper_pt_read_raster_transparent_layers(
    prosper_pt_ctx *ctx, uint32_t *host_counts, prosper_pt_transparent_layer *host_layers, size_t pixels, uint32_t layersPerPixel, void *stream);
/* Synchronises `stream` (behind the last draw, whatever its stream) and decodes the image on the host: per pixel
 * (drawInstanceIndex, meshletIndex, triangle) as three uint32 - 0xFFFFFFFF each where nothing is drawn - into `ids`, the
 * key's depth into `depth`; either may be NULL.  `pixels`: room in pixels, at least width * height of the image. */
int prosper_pt_read_raster_visibility(prosper_pt_ctx *ctx, uint32_t *ids, float *depth, size_t pixels, void *stream);
/* What the last draws counted.  draw[0]: the draw that cleared; draw[1]: the draw on top of it (valid = 0 without one).
 * Every count is a property of the list and the view: `fragments` passed coverage and the depth range, counted BEFORE the
 * depth test.  culledOutside: no pixel centre in the box, all three vertices beyond one clip plane, or clipped to nothing.
 * queued: triangles handed to the tile pass (large boxes, and every triangle the clipper sees).  queueOverflow stays 0
 * unless a mesh's meshlets hold more triangles than its index buffer.  The counts travel through pinned memory behind the
 * draws: the call never blocks and returns PROSPER_PT_NOT_READY (extent set, counts zero) until they have landed. */
typedef struct prosper_pt_raster_draw_info
{
    uint32_t valid;
    uint32_t triangles;
    uint32_t culledBackface;
    uint32_t culledZeroArea;
    uint32_t culledOutside;
    uint32_t clipped;
    uint32_t queued;
    uint32_t fragments;
    uint32_t queueOverflow;
    float meshletsMs; /* device time of the meshlet kernel ... */
    float largeMs;    /* ... and of the tile pass, between events on the draw's stream */
    uint32_t reserved;
} prosper_pt_raster_draw_info;
typedef struct prosper_pt_raster_info
{
    uint32_t width;
    uint32_t height;
    prosper_pt_raster_draw_info draw[2];
} prosper_pt_raster_info;
int prosper_pt_get_raster_info(prosper_pt_ctx *ctx, prosper_pt_raster_info *out);

/* ---- image-based lighting (src/render/ImageBasedLighting.cpp, res/shader/ibl/) ----
 * ImageBasedLighting::recordGeneration: the three products evalIBL reads, from the scene's sky.
 *
 * prosper_pt_generate_ibl runs the three passes on `stream` into context-owned maps (allocated by the first call, kept
 * for the context's lifetime): the 6 x 64^2 irradiance cube, the 6 x 512^2 prefiltered radiance cube with 10 mips
 * (roughness = mip / 10) and the 512^2 split-sum BRDF LUT.  Every environment lookup is the path tracer's seamless
 * bilinear sky lookup, clamped per channel to 10.  A scene without a sky gives all-zero cubes and the same LUT.  Calling
 * it again regenerates the maps, bit for bit the same.  NO_SCENE before the first prosper_pt_upload_scene, which clears
 * the maps' `generated` (they describe the old sky); light, transform, texture, material and mesh updates keep them. */
int prosper_pt_generate_ibl(prosper_pt_ctx *ctx, void *stream);
typedef struct prosper_pt_ibl_info
{
    uint32_t generated;      /* 1 once prosper_pt_generate_ibl ran for the current scene */
    uint32_t irradianceSize; /* 64 */
    uint32_t radianceSize;   /* 512 (mip 0) */
    uint32_t radianceMips;   /* 10 */
    uint32_t lutSize;        /* 512 */
    /* device time of each pass of the last generation (0 before the first); reading them waits for it */
    float irradianceMs, radianceMs, lutMs;
} prosper_pt_ibl_info;
int prosper_pt_get_ibl_info(prosper_pt_ctx *ctx, prosper_pt_ibl_info *out);
/* Synchronises `stream` and copies the maps without their borders to host memory; any pointer may be NULL, and each
 * given one must hold exactly its map.  Faces +X, -X, +Y, -Y, +Z, -Z, each row-major.
 *   irradiance: 6 x 64 x 64 RGBA16F (alpha 0), irradiance_bytes = 196 608
 *   radiance:   the mips one after another from mip 0, each 6 x n x n RGBA16F (alpha 0), radiance_bytes = 16 777 200
 *   lut:        512 x 512 R16G16 UNORM (scale, bias), row = roughness * 512, column = NoV * 512, lut_bytes = 1 048 576
 * NO_SCENE if nothing has been generated for the current scene. */
int prosper_pt_read_ibl(
    prosper_pt_ctx *ctx, uint16_t *irradiance_rgba16f, size_t irradiance_bytes, uint16_t *radiance_rgba16f,
    size_t radiance_bytes, uint16_t *lut_rg16, size_t lut_bytes, void *stream);

/* ---- skybox fill and depth of field (src/render/SkyboxRenderer.cpp, src/render/dof/, res/shader/dof/) ----
 * What prosper runs between the shaded G-buffer and the tone map: plain compute over the context's HDR
 * image and a non-linear depth.  Additive: the ABI version stays 4.
 *
 * prosper_pt_skybox_fill: every texel whose nonLinearDepth is 0 (reverse-Z far plane, the traced G-buffer's miss
 * value) gets (sky.rgb, 1) in the context's HDR image; every other texel is left bit for bit as it was.  The sky value
 * is the path tracer's seamless bilinear lookup of mip 0 of the scene's sky, unclamped, in the direction of the
 * G-buffer tracer's primary ray through the pixel centre (px + 0.5, py + 0.5); a cube lookup does not depend on the
 * direction's length, so this is the interpolated cube position of skybox.vert.  A scene without a sky fills
 * (0, 0, 0, 1).  No velocity output (prosper_pt_trace_gbuffer_velocity writes the sky's).  `nonLinearDepth`: width*height floats, on the device when `onDevice` is not 0;
 * NULL means the last traced G-buffer's depth (refused when its extent differs).  The HDR image must be what a render,
 * a ReSTIR trace or deferred shading produced at this extent.  Pending scene updates take effect first. */
int prosper_pt_skybox_fill(
    prosper_pt_ctx *ctx, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height, const float *nonLinearDepth,
    uint32_t onDevice, void *stream);

/* The push-constant values of the depth-of-field passes as prosper computes them (Setup.cpp:163-177,
 * Dilate.cpp:105-127); the host layer's DepthOfField derives them from the camera's aperture, focus distance and focal
 * length.  Given as numbers, so that small images can have large circles. */
typedef struct prosper_pt_dof_pc
{
    float focusDistance;    /* > 0 */
    float maxBackgroundCoC; /* >= 0, half-resolution pixels: the circle of a surface infinitely far away */
    float maxCoC;           /* >= 0: the foreground's circles are clamped to -maxCoC (2 x maxBackgroundCoC in prosper) */
    int32_t gatherRadius;   /* >= 1, tiles: how far the dilation looks */
} prosper_pt_dof_pc;
typedef struct prosper_pt_dof_inputs
{
    const void *illumination;    /* width*height RGBA32F; NULL: the context's HDR image, processed in place */
    const float *nonLinearDepth; /* width*height floats; NULL: the last traced G-buffer's depth (same extent) */
    uint32_t onDevice;           /* 0: the given pointers are host memory */
    uint32_t reserved;
} prosper_pt_dof_inputs;
/* render::dof::DepthOfField::record: seven compute passes over the illumination and the depth; the result is always
 * the context's HDR image (prosper_pt_read_hdr, _blit_rgba16f and _tone_map read it), with the input's alpha.  With
 * hw = ceil(width / 2), hh = ceil(height / 2) and tiles of 8 x 8 half-resolution texels, the context-owned
 * intermediates (grown as needed) are, in prosper's formats, stored with round-to-nearest-even:
 *   setup    half-resolution illumination RGBA16F (alpha 1) and circle of confusion R16F.  Each texel takes the four
 *            full-resolution texels min(2c + {(0,1), (1,1), (1,0), (0,0)}, extent - 1) (the textureGather of the GLSL
 *            is defined as exactly those); coc = max((1 - focusDistance / -viewZ) * maxBackgroundCoC, -maxCoC) with the
 *            G-buffer passes' linearizeDepth; the stored CoC is the minimum of the four, the colour their mean with
 *            weights saturate(1 - (cocOut - coc_i))
 *   reduce   the illumination's mips, 32 - clz(max(hw, hh)) levels in all, level k of max(hw >> k, 1) x
 *            max(hh >> k, 1) texels.  Levels 1-6: the float32 mean of four texels of the unrounded level below, over
 *            the source clamped to its edge (what FidelityFX SPD's 64 x 64 tile computes); levels 7 and up: the mean
 *            of four stored texels of the level below, clamped to that level's extent
 *   flatten  min and max CoC of every tile, RG16F
 *   dilate   over tiles (i, j) away, |i|, |j| <= gatherRadius: the min of the minima of the tiles with
 *            8 * sqrt(i*i + j*j) <= |min| + 4, likewise the max; tiles outside the image read the edge tile
 *   gather   foreground and background, RGBA16F: 121 octaweb taps (prosper_pt_dof_sample_offsets) at
 *            (coord + 0.5) + ringRadius * offset in half-resolution texel units; the CoC lookup is the texel
 *            clamp(floor(p), 0, size - 1), the colour lookup trilinear over the mips (level l bilinear at
 *            p * size_l / size_0 - 0.5, clamped to the edge, float weights).  Background (colour, 0), foreground
 *            (colour, weight); a tile the layer skips stores zeros, as does a foreground texel that takes no tap
 *   filter   a 3 x 3 median by luminance of each gather, neighbours clamped to the edge: the brightest of the nine goes
 *            to slot 8, then the three compare-swap rounds of the GLSL as written.  Its second round pairs (0, 2),
 *            (1, 3), (6, 8) and (7, 9); the last reaches past the nine elements (undefined in the GLSL) and is left out
 *   combine  the filtered layers over the full-resolution illumination.  The half-resolution coordinates
 *            floor((x + d) / 2) can lie one past the edge on an even extent: they are clamped to the edge (the GLSL
 *            leaves an out-of-bounds imageLoad to the driver)
 * All arithmetic is float32 without contraction.  Refused: non-finite pc values, focusDistance <= 0, a negative CoC,
 * gatherRadius < 1, an empty extent, illumination = NULL when the HDR image has another extent, nonLinearDepth = NULL
 * when the last traced G-buffer has another extent.  It needs no scene. */
int prosper_pt_depth_of_field(
    prosper_pt_ctx *ctx, const prosper_pt_dof_pc *pc, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height,
    const prosper_pt_dof_inputs *inputs, void *stream);
/* The 121 unit offsets (cos phi, sin phi) of the six octaweb rings (1 + 8 + 16 + 24 + 32 + 40 taps), ring by ring:
 * phi = (s + (ring even ? 0.5 : 0)) * 2 pi / count, float32 of double-precision cos / sin with pi itself.  Host only:
 * it needs neither a context nor a GPU. */
void prosper_pt_dof_sample_offsets(float out[242]);
enum
{
    PROSPER_PT_DOF_HALF_ILLUMINATION = 0, /* RGBA16F, `level` selects the mip: max(hw >> level, 1) x max(hh >> level, 1) */
    PROSPER_PT_DOF_HALF_COC = 1,          /* R16F, hw x hh */
    PROSPER_PT_DOF_TILE_MIN_MAX = 2,      /* RG16F, tiles */
    PROSPER_PT_DOF_DILATED_TILE_MIN_MAX = 3,
    PROSPER_PT_DOF_FG_GATHER = 4, /* RGBA16F, hw x hh */
    PROSPER_PT_DOF_BG_GATHER = 5,
    PROSPER_PT_DOF_FG_FILTERED = 6,
    PROSPER_PT_DOF_BG_FILTERED = 7,
    PROSPER_PT_DOF_STAGE_COUNT = 8,
};
/* Synchronises `stream` and copies one intermediate of the last prosper_pt_depth_of_field to host memory as raw fp16,
 * row-major; byte_size must be exactly its size.  `level` is read only for PROSPER_PT_DOF_HALF_ILLUMINATION.  NO_SCENE
 * before the first call. */
int prosper_pt_read_dof_stage(
    prosper_pt_ctx *ctx, uint32_t stage, uint32_t level, void *host, size_t byte_size, void *stream);
typedef struct prosper_pt_dof_info
{
    uint32_t valid; /* 1 once prosper_pt_depth_of_field ran */
    uint32_t width, height, halfWidth, halfHeight, tileWidth, tileHeight;
    uint32_t mips;  /* levels of the half-resolution illumination */
    /* device time of each stage of the last call (reading them waits for it) */
    float setupMs, reduceMs, flattenMs, dilateMs, gatherForegroundMs, gatherBackgroundMs, filterForegroundMs,
        filterBackgroundMs, combineMs;
} prosper_pt_dof_info;
int prosper_pt_get_dof_info(prosper_pt_ctx *ctx, prosper_pt_dof_info *out);

/* ---- bloom, the multi-resolution blur (src/render/bloom/{Separate,Reduce,Blur,Compose}.cpp, res/shader/bloom/) ----
 * What prosper runs first between the sky-filled illumination and the tone map (Renderer.cpp:516-573):
 * its default technique (Bloom.hpp:57-58: MultiResolutionBlur at half resolution), plain compute over the context's HDR
 * image.  The FFT technique: prosper_pt_bloom_fft below.  Additive: the ABI version stays 4. */
typedef struct prosper_pt_bloom_pc
{
    float threshold;          /* finite, >= 0; Separate.hpp: 1 */
    float blendFactors[3];    /* finite, >= 0; Compose.hpp: .9, .04, .04 */
    uint32_t resolutionScale; /* 0 Half, 1 Quarter */
    uint32_t biquadratic;     /* 0 / 1; Compose.hpp: 1 */
    uint32_t reserved[2];     /* 0 */
} prosper_pt_bloom_pc;
/* render::bloom::Bloom::record: separate, reduce, blur and compose; the result is always the context's HDR image
 * (prosper_pt_read_hdr, _blit_rgba16f, _tone_map and _depth_of_field read it), with alpha 1 as compose.comp writes it.
 * `illumination`: width*height RGBA32F (prosper's image is RGBA16F), on the device when `onDevice` is not 0; NULL: the
 * HDR image, in place (compose reads only the texel it writes).  With s = 2 (Half) or 4 (Quarter), the working extent
 * ww = width / s, wh = height / s (integer division, Separate.cpp:106-111) and level k of max(ww >> k, 1) x
 * max(wh >> k, 1) RGBA16F texels, the context owns three grow-only images of four levels, stored with
 * round-to-nearest-even: `highlights` (separate and reduce write it), `horizontal` and `blurred` (the horizontal and the
 * vertical blur's outputs; prosper ping-pongs two images and overwrites the blur's input).  Where the GLSL reads a
 * level of its working image that no blur pass wrote, that level is read from `highlights`.
 * A bilinear lookup of a level at uv has the texel coordinate c = uv * size - 0.5, i = floor(c), f = c - i, and blends
 * the texels i, i + 1 of both axes with float weights; texels outside are (0, 0, 0, 0) for separate and blur
 * (bilinearBorderTransparentBlackSampler, also in Blur.cpp:113-129) and clamped to the edge for compose.  Every uv here
 * is a ratio of integers, and c is formed from the integers, without the float round trip through uv.
 *   separate  over ww x wh.  Half: one lookup of the illumination at uv = 2 coord / resolution, i.e. the mean of the
 *             texels 2 coord - 1 and 2 coord of both axes; Quarter: the mean (sum / 4) of four such lookups at
 *             (4 coord + (-1 | 1, -1 | 1)) / resolution in the order (-1,-1), (-1,1), (1,-1), (1,1).  No + 0.5 is applied:
 *             at coord 0 the lookups take in the border.  Stores (max(rgb - threshold, 0), 0) into level 0
 *   reduce    levels 1-3 of `highlights` (SPD with three mips): level k is the float32 mean (((a + b) + c) + d) * 0.25
 *             of four unrounded level k - 1 texels over the source clamped to its edge, virtual texels past a level's
 *             extent included; only texels inside the level's extent are stored; alpha stays 0
 *   blur      horizontal (`highlights` -> `horizontal`), then vertical (`horizontal` -> `blurred`), of the levels
 *             first, first + 1, first + 2 with first = 0 (Half) or 1 (Quarter): four lookups of the level at
 *             (coord + 0.5 + dir * OFFSETS[i]) / resolution weighted by WEIGHTS[i] (blur.comp:20-25), summed in
 *             order, alpha 1.  The horizontal pass of level 1 adds the streak: with h = levelWidth / 2,
 *             sum over i in [-h, h) of w(i) * L0(uv + (i, 0) / resolution) divided by (2 levelWidth), L0 the lookup
 *             of `highlights` level 0 at the level-1 uv and w(i) of prosper_pt_bloom_streak_weights
 *   compose   over width x height, uv = (coord + 0.5) / resolution: illumination.rgb + sum_l blendFactors[l] * level_l
 *             for the levels 0, 1, 2, each read from `blurred` if a blur pass wrote it and from `highlights` otherwise
 *             (level 0 at Quarter).  biquadratic = 1 is sampleBiquadratic as written: the mean of the four lookups at
 *             uv -/+ c, c = (q (q - 1) + 0.5) / res, q = fract(uv res), in the order (-,-), (-,+), (+,+), (+,-), with
 *             res = vec2(width, height) / (s * 2^l), a float division and not the level's integer size
 * All arithmetic is float32 without contraction.  Refused, changing nothing: a NULL pc, non-finite or negative values,
 * an unknown scale, biquadratic above 1, non-zero reserved words, an empty extent or one above 32768, illumination = NULL
 * when the HDR image has another extent, and an extent on which a blurred level would be empty (ww or wh below 4 at
 * Half, below 8 at Quarter; prosper asserts there, Blur.cpp:196).  It needs no scene. */
int prosper_pt_bloom(
    prosper_pt_ctx *ctx, const prosper_pt_bloom_pc *pc, uint32_t width, uint32_t height, const void *illumination,
    uint32_t onDevice, void *stream);
/* The streak's weights for i = -halfWidth .. halfWidth - 1, 2 * halfWidth floats each (blur.comp:56-66):
 * b = 4 (|sin(.5 i)| + |cos(.95 i)| + |sin(.75 i)|) * (150 / max(.015 i^2 + |i|, 1)) and rg = c * that with c = .05 for
 * |i| < 10 and .01 otherwise (the GLSL's abs(i) / 10 is an integer division inside saturate), computed in double
 * precision from the integer i as ((c * 4) * wave) * fall and rounded once to float32.  This is the definition: GLSL's
 * float32 sin and cos have no stated precision.  Host only: it needs neither a context nor a GPU. */
void prosper_pt_bloom_streak_weights(uint32_t halfWidth, float *rg, float *b);
enum
{
    PROSPER_PT_BLOOM_HIGHLIGHTS = 0, /* levels 0-3 */
    PROSPER_PT_BLOOM_HORIZONTAL = 1, /* levels firstLevel .. firstLevel + 2 */
    PROSPER_PT_BLOOM_BLURRED = 2,    /* levels firstLevel .. firstLevel + 2 */
    PROSPER_PT_BLOOM_STAGE_COUNT = 3,
};
/* Synchronises `stream` and copies one level of one working image of the last prosper_pt_bloom to host memory as raw
 * RGBA16F, row-major; byte_size must be exactly its size.  A level the stage did not write is refused.  NO_SCENE before
 * the first call. */
int prosper_pt_read_bloom_stage(
    prosper_pt_ctx *ctx, uint32_t stage, uint32_t level, void *host, size_t byte_size, void *stream);
typedef struct prosper_pt_bloom_info
{
    uint32_t valid; /* 1 once prosper_pt_bloom ran */
    uint32_t width, height, workingWidth, workingHeight;
    uint32_t firstLevel;      /* the first blurred level */
    uint32_t streakHalfWidth; /* max(workingWidth >> 1, 1) / 2 */
    /* device time of each stage of the last call (reading them waits for it); the blurs by level firstLevel + n */
    float separateMs, reduceMs, blurHorizontalMs[3], blurVerticalMs[3], composeMs;
} prosper_pt_bloom_info;
int prosper_pt_get_bloom_info(prosper_pt_ctx *ctx, prosper_pt_bloom_info *out);

/* ---- bloom, the FFT technique (src/render/bloom/{Separate,GenerateKernel,Fft,Convolution,Compose}.cpp) ----
 * The other entry of render::bloom::Technique (Bloom.cpp:83-114): the highlights are convolved with a
 * generated kernel image through the DFT.  Plain compute over the context's HDR image, like prosper_pt_bloom, whose
 * images it does not touch.  Additive: the ABI version stays 4. */
typedef struct prosper_pt_bloom_fft_pc
{
    float threshold;           /* finite, >= 0; Separate.hpp: 1 */
    uint32_t resolutionScale;  /* 0 Half, 1 Quarter */
    uint32_t biquadratic;      /* 0 / 1; Compose.hpp: 1 */
    uint32_t regenerateKernel; /* 0 / 1: remake the kernel's DFT (prosper's "Re-generate kernel") */
    uint32_t reserved[4];      /* 0 */
} prosper_pt_bloom_fft_pc;
struct prosper_pt_bloom_fft_plan /* (no typedef: the function below has the name) */
{
    uint32_t dim;           /* max(bit_ceil(max(width, height)) / s, 256) with s = 2 (Half) or 4 (Quarter) */
    uint32_t kernelDim;     /* height / s */
    float convolutionScale; /* 2.f / float(kernelDim), times 2 at Quarter */
};
/* The extents prosper_pt_bloom_fft works on (Separate.cpp:98-101, GenerateKernel.cpp:81-85, Bloom.cpp:95-98).  Host
 * only: it needs neither a context nor a GPU.  -1 on an extent or a scale prosper_pt_bloom_fft refuses. */
int prosper_pt_bloom_fft_plan(uint32_t width, uint32_t height, uint32_t resolutionScale,
                              struct prosper_pt_bloom_fft_plan *out);
/* render::bloom::Bloom::record with Technique::Fft; `illumination`, `onDevice` and the result as prosper_pt_bloom.
 *   separate     separate.comp as in prosper_pt_bloom, over dim x dim into a one-level RGBA16F image: texels whose
 *                lookups fall outside the illumination store (0, 0, 0, 0)
 *   kernel       generate_kernel.comp: kernelDim x kernelDim RGBA32F, the mean of filterValue(p) over 8 x 8 sub-samples
 *                p = ((8 xy + (i, j) + .5) / (8 kernelDim)) 2 - 1, filterValue as written.  The definition is the value in
 *                double precision rounded once to float32 (GLSL's float32 exp, atan, sin and cos have no stated
 *                precision); it is evaluated on the device in double.  prepare_kernel.comp wraps it round the corners
 *                of a dim x dim RGBA32F image: pIn = pOut + kernelDim / 2 below dim / 2, pOut + (kernelDim - 2 dim) / 2
 *                from there on (formed in halves from integers, truncated), zero outside, .g = .a = 0.  Its forward
 *                DFT is kept by the context and remade when kernelDim or dim change or regenerateKernel is 1
 *   transform    a texel is the complex numbers r + i g and b + i a.  Forward: X[ky][kx] = (1 / dim) sum x[y][x]
 *                e^{-2 pi i (kx x + ky y) / dim} in natural order; inverse: the unnormalised inverse DFT.  Each
 *                dimension is one kernel that holds whole lines in LDS; twiddles from a table made in double
 *   convolution  DFT(highlights) * DFT(kernel) * convolutionScale as a complex product per channel pair, then the inverse.
 *                The pass runs rows forward; columns forward, the product and columns inverse in one launch; rows inverse
 *   compose      out = (illumination.rgb + highlight, 1): one edge-clamped bilinear lookup of the convolved RGBA32F image
 *                at the texel coordinate (2 coord + 1 - s) / (2 s); biquadratic = 1: sampleBiquadratic with res = dim
 * Refused, changing nothing: a NULL pc, a non-finite or negative threshold, an unknown scale, flags above 1, non-zero
 * reserved words, an empty extent, width / s or height / s of 0, max(width, height) above 8192 (dim is at most 4096),
 * and illumination = NULL when the HDR image has another extent.  It needs no scene. */
int prosper_pt_bloom_fft(
    prosper_pt_ctx *ctx, const prosper_pt_bloom_fft_pc *pc, uint32_t width, uint32_t height, const void *illumination,
    uint32_t onDevice, void *stream);
/* One 2-D transform of a dim x dim RGBA32F image (`in` and `out` on the device when `onDevice` is not 0; they may be the
 * same) with the kernels prosper_pt_bloom_fft uses: rows, then columns.  dim: a power of two in [256, 4096].  Waits for
 * `stream` when the images are on the host. */
int prosper_pt_bloom_fft_transform(
    prosper_pt_ctx *ctx, uint32_t dim, uint32_t inverse, const void *in, void *out, uint32_t onDevice, void *stream);
/* Drops the kernel's DFT the context keeps (GenerateKernel::releasePreserved): the next call remakes it. */
void prosper_pt_bloom_fft_release_kernel(prosper_pt_ctx *ctx);
enum
{
    PROSPER_PT_BLOOM_FFT_HIGHLIGHTS = 0, /* dim x dim RGBA16F */
    PROSPER_PT_BLOOM_FFT_KERNEL = 1,     /* kernelDim x kernelDim RGBA32F, centred */
    PROSPER_PT_BLOOM_FFT_KERNEL_DFT = 2, /* dim x dim RGBA32F */
    PROSPER_PT_BLOOM_FFT_CONVOLVED = 3,  /* dim x dim RGBA32F: what compose reads */
    PROSPER_PT_BLOOM_FFT_STAGE_COUNT = 4,
};
/* Synchronises `stream` and copies one image of the last prosper_pt_bloom_fft to host memory, row-major; byte_size must
 * be exactly its size.  NO_SCENE before the first call. */
int prosper_pt_read_bloom_fft_stage(prosper_pt_ctx *ctx, uint32_t stage, void *host, size_t byte_size, void *stream);
typedef struct prosper_pt_bloom_fft_info
{
    uint32_t valid; /* 1 once prosper_pt_bloom_fft ran */
    uint32_t width, height, dim, kernelDim;
    uint32_t kernelRemade; /* 1: the last call made the kernel's DFT; 0: it used the kept one */
    float convolutionScale;
    uint32_t fused; /* bit k: stage k of the times below shares a launch.  0x70: the forward columns, the convolution
                       and the inverse columns are one launch, timed as convolutionMs; forwardFftMs and inverseFftMs
                       are then the row launches alone */
    /* device time of each stage of the last call (reading them waits for it); generate, prepare and the kernel's FFT
     * are 0 when the kernel was not remade */
    float separateMs, generateMs, prepareMs, kernelFftMs, forwardFftMs, convolutionMs, inverseFftMs, composeMs;
} prosper_pt_bloom_fft_info;
int prosper_pt_get_bloom_fft_info(prosper_pt_ctx *ctx, prosper_pt_bloom_fft_info *out);

/* ---- temporal anti-aliasing: the resolve (src/render/TemporalAntiAliasing.cpp, res/shader/taa_resolve.comp) ----
 * What prosper runs between bloom and depth of field (Renderer.cpp:516-573), on by default there
 * (m_applyTaa).  Additive: the ABI version stays 4. */
typedef struct prosper_pt_taa_pc
{
    uint32_t catmullRom;         /* 0 / 1; TemporalAntiAliasing.hpp: 1 */
    uint32_t colorClipping;      /* 0 None, 1 MinMax, 2 Variance (the default) */
    uint32_t velocitySampling;   /* 0 Center, 1 Largest, 2 Closest (the default) */
    uint32_t luminanceWeighting; /* 0 / 1; the default is 1 */
    uint32_t resetHistory;       /* 1: IGNORE_HISTORY for this call */
} prosper_pt_taa_pc;
enum
{
    PROSPER_PT_TAA_CLIPPING_NONE = 0,
    PROSPER_PT_TAA_CLIPPING_MIN_MAX = 1,
    PROSPER_PT_TAA_CLIPPING_VARIANCE = 2,
    PROSPER_PT_TAA_VELOCITY_CENTER = 0,
    PROSPER_PT_TAA_VELOCITY_LARGEST = 1,
    PROSPER_PT_TAA_VELOCITY_CLOSEST = 2,
};
typedef struct prosper_pt_taa_inputs
{
    const void *illumination;    /* width*height RGBA32F; NULL: the context's HDR image, in place */
    const void *velocity;        /* width*height float2 (x, y), prosper's velocity target: (posNDC - currentJitter) -
                                  * (prevPosNDC - previousJitter) with y negated; NULL: the last traced velocity target
                                  * (prosper_pt_trace_gbuffer_velocity) */
    const float *nonLinearDepth; /* width*height reverse-Z depth, read by Closest alone; NULL: the last traced G-buffer's */
    uint32_t onDevice;           /* not 0: the given pointers are device pointers */
} prosper_pt_taa_inputs;
/* TemporalAntiAliasing::record: taa_resolve.comp over `width` x `height`, one of its 36 specialisations (catmullRom x
 * colorClipping x velocitySampling x luminanceWeighting) or IGNORE_HISTORY, each a kernel of its own picked by
 * prosper's specializationIndex.  The context owns two grow-only RGBA16F history images (prosper's resolved image is
 * RGBA16F): a call reads one and writes the other, stores round to nearest even with alpha 1, and the result in the
 * context's HDR image is the float32 expansion of the stored texel, so the HDR image and the history hold the same
 * values as prosper's one image does.  In place (illumination NULL or the HDR image itself) the pass is two kernels,
 * `resolve` into the new history and `expand` from it into the HDR image, because the 3 x 3 neighbourhood reaches
 * texels other blocks write; with another input image `resolve` writes both.  Both ways give the same bytes.
 * History is ignored (the output is the input's rgb) on the first call, when the extent differs from the last call's
 * (TemporalAntiAliasing.cpp:199-220), with resetHistory, after prosper_pt_taa_release_history and after
 * prosper_pt_upload_scene.
 * The arithmetic is float32 without contraction in the GLSL's order, with px the texel and res = (width, height):
 *   nearest lookups  at (px + offset + .5) / res: the texel px + offset clamped to the edge, formed from the integers;
 *                    every 3 x 3 loop runs x outer, y inner
 *   velocity         Center: the texel's; Largest: lenSqr = x x + y y, `retLenSqr < lenSqr` is strict (the first of equal
 *                    lengths wins, all zero gives (0, 0)); Closest: `depth > closestDepth` from 0 is strict (the first of
 *                    equal depths wins, all zero gives offset (0, 0)), then the velocity at that offset
 *   uv               ((px + .5) / res); reprojectedUv = uv - velocity * (.5, -.5); unless every component equals its
 *                    saturate (0 and 1 are inside, a NaN is not) the output is the illumination
 *   history lookup   c = reprojectedUv * res - 0.5, i = floor(c), f = c - i, texels clamped to the edge.  Bilinear: the
 *                    texels i, i + 1 of both axes with the weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy
 *                    summed in that order.  Catmull-Rom (optimizedCatmullRom, sharpness 70): w0 .. w3 from f per axis
 *                    as written, w12 = w1 + w2, t = w2 / w12; the five taps in texel space, without the round trip
 *                    through tc * res: (tc12.x, tc0.y) blends the texels ix, ix + 1 of row iy - 1 with (1 - tx, tx),
 *                    (tc0.x, tc12.y) the texels iy, iy + 1 of column ix - 1 with ty, the centre the four texels with
 *                    (tx, ty), (tc3.x, tc12.y) column ix + 2, (tc12.x, tc3.y) row iy + 2; weighted by w12.x w0.y,
 *                    w0.x w12.y, w12.x w12.y, w3.x w12.y, w12.x w3.y, summed in that order and divided by the weights' sum
 *   clipping         MinMax: clamp to the neighbourhood's min and max (from 9999 and -9999); Variance: mu = m1 / 9,
 *                    sigma = sqrt(max(m2 / 9 - mu mu, 0)) - the max is a deviation: the GLSL's argument can go negative
 *                    on a flat neighbourhood and give NaN - clamp to mu -/+ sigma.  clamp(x, lo, hi) = min(max(x, lo), hi)
 *   blend            currentWeight .1, historyWeight 1 - .1, each times 1 / (1 + luminance) with luminance weighting
 *                    (luminance = (.299 r + .587 g) + .114 b); (illumination cw + previous hw) / max(cw + hw, .00001)
 * Host inputs go through a grow-only staging buffer.  It needs no scene.  Refused, changing nothing: a NULL pc or
 * inputs, a flag above 1 or an unknown clipping or sampling type, an empty extent or one above 32768, illumination =
 * NULL when the HDR image has another extent, a NULL velocity when no velocity target of this extent has been traced,
 * and with Closest a NULL depth when no G-buffer of this extent has been traced. */
int prosper_pt_taa_resolve(
    prosper_pt_ctx *ctx, const prosper_pt_taa_pc *pc, uint32_t width, uint32_t height, const prosper_pt_taa_inputs *inputs,
    void *stream);
/* TemporalAntiAliasing::releasePreserved: the next call ignores the history.  (The images stay allocated.) */
void prosper_pt_taa_release_history(prosper_pt_ctx *ctx);
/* Synchronises `stream` and copies the history the NEXT call will read to host memory as raw RGBA16F, row-major;
 * `bytes` must be exactly width*height*8 of the last call.  NO_SCENE when there is no history. */
int prosper_pt_read_taa_history(prosper_pt_ctx *ctx, uint16_t *rgba16f, size_t bytes, void *stream);
typedef struct prosper_pt_taa_info
{
    uint32_t valid;          /* 1 once prosper_pt_taa_resolve ran */
    uint32_t width, height;  /* of the last call */
    uint32_t historyValid;   /* 1: the next call of this extent reads a history */
    uint32_t ignoredHistory; /* 1: the last call ran IGNORE_HISTORY */
    /* device time of the two kernels of the last call (reading them waits for it); expandMs covers nothing when
     * `resolve` wrote the HDR image itself */
    float resolveMs, expandMs;
} prosper_pt_taa_info;
int prosper_pt_get_taa_info(prosper_pt_ctx *ctx, prosper_pt_taa_info *out);
/* Camera::perspective's jitter (Camera.cpp:119-128): (halton23[jitterIndex % 8] * 2 - 1) / (width, height) in float32,
 * in that order of operations, for callers that build their own prosper_CameraUniforms.  Host only. */
void prosper_pt_taa_jitter(uint32_t jitterIndex, uint32_t width, uint32_t height, float out[2]);

/* ---- spatiotemporal denoiser of the path-traced image ----
 * prosper has no denoiser: the rule below is this library's own, stated operation for operation in
 * prosper_amd/denoise.py (NumPy, float32) and met by the kernels bit for bit.  An SVGF-style pass over the HDR image:
 * temporal accumulation of colour and luminance moments reprojected through the velocity target, a variance estimate,
 * and an edge-avoiding a-trous wavelet filter guided by depth, normal and variance.  Opt-in: nothing else calls it.
 * Additive: the ABI version stays 4. */
typedef struct prosper_pt_denoise_pc
{
    uint32_t iterations;        /* a-trous passes, 0 .. 5; the step of pass i is 1 << i; default 5 */
    uint32_t demodulate;        /* 0 / 1: filter illumination / max(albedo, 1/64), multiply back at the end; default 1 */
    uint32_t maxHistoryLength;  /* 1 .. 255; default 32 */
    uint32_t feedbackIteration; /* which a-trous output becomes the next frame's colour history; >= iterations: the
                                 * temporal result; default 1 */
    uint32_t normalPowerLog2;   /* 0 .. 8: the normal weight is max(0, n.n') squared this many times; default 7 */
    uint32_t resetHistory;      /* 0 / 1; default 0 */
    float minAlpha;             /* lower bound of the temporal blend weight, (0, 1]; default 0.05 */
    float depthTolerance;       /* reprojection: |zPrev - z| <= depthTolerance * max(z, zPrev); default 0.1 */
    float normalThreshold;      /* reprojection: dot(nPrev, n) >= normalThreshold; default 0.9 */
    float sigmaDepth;           /* default 1 */
    float sigmaLuminance;       /* default 4 */
} prosper_pt_denoise_pc;
/* The defaults named above.  Host only. */
void prosper_pt_denoise_pc_default(prosper_pt_denoise_pc *out);
typedef struct prosper_pt_denoise_inputs
{
    const void *illumination;    /* width*height RGBA32F; NULL: the context's HDR image, in place */
    const void *albedoRoughness; /* width*height float4 each and the reverse-Z depth, given together; all three NULL: */
    const void *normalMetallic;  /* the last traced or rastered G-buffer */
    const float *nonLinearDepth;
    const void *velocity;        /* width*height float2 as for prosper_pt_taa_resolve; NULL: the last traced velocity target */
    uint32_t onDevice;           /* not 0: the given pointers are device pointers */
} prosper_pt_denoise_inputs;
/* One denoise of `width` x `height` into the context's HDR image, so that tone map, bloom, TAA and depth of field consume
 * the result unchanged.  `camera` supplies linearize_depth's two terms (cameraToClip[2][2] and [3][2]), as for depth of
 * field.  It needs no scene.  History is ignored on the first call, when the extent differs from the last call's, with
 * resetHistory, after prosper_pt_denoise_release_history and after prosper_pt_upload_scene.
 *
 * Everything is stored as float32: the rule has no quantisation.  Arithmetic is float32 without contraction, only
 * + - * / sqrt min max floor abs and comparisons, in this order (min/max: a NaN operand loses); px the texel, res =
 * (width, height):
 *   per pixel    geometry: nonLinearDepth != 0.  z = cameraToClip32 / (depth + cameraToClip22), -viewZ.  n = signedOctDecode of
 *                normalMetallic's (x, y, w) with dot(a, b) = (ax bx + ay by) + az bz and n = o * (1 / sqrt(dot(o, o))).
 *                x = illumination.rgb, with demodulate each channel / max(albedo, 1/64).  l = (.299 r + .587 g) + .114 b.
 *                A sky texel leaves the pass byte for byte as it came in, has length 0 and is nobody's tap.  A texel
 *                whose x has a non-finite component is an invalid sample: it keeps its reprojected history, the length
 *                not incremented; without a history its colour, moments and length are 0.
 *   guide        z, n, the flag and a depth gradient per axis: the forward (z[+1] - z) and backward (z - z[-1])
 *                differences to geometry neighbours inside the image, the one of smaller magnitude (ties: forward); 0
 *                without one
 *   reprojection uv = (px + .5) / res; reprojectedUv = uv - velocity * (.5, -.5); c = reprojectedUv * res - .5; unless
 *                -1 <= c <= res on both axes there is no history; i = floor(c), f = c - i.  The taps (0,0) (1,0) (0,1)
 *                (1,1) with the weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  A tap counts if it lies inside the
 *                image (no clamping), the previous guide there is geometry, |zPrev - z| <= depthTolerance max(z, zPrev)
 *                and dot(nPrev, n) >= normalThreshold.  The counted weights are summed in that order (so are w * colour
 *                and w * moments); a sum that is not > 0 means no history; else prev = sum / weight sum
 *   length       with history min(maxHistoryLength, max(lengths of the counted taps) + 1), without 1
 *   blend        alpha = max(1 / N', minAlpha), keep = 1 - alpha; x' = keep * prev + alpha * x for the colour, for
 *                m1 (x = l) and m2 (x = l * l); without history x' = x.  Temporal variance max(m2' - m1' m1', 0)
 *   variance     where N' < 4: over the 7 x 7 window, dy outer, dx inner, the taps inside the image that are geometry,
 *                the centre with weight 1, the others with w_n F(x_z) below at step 1; m = sum(w m) / sum(w) for both
 *                moments, variance = max(m2 - m1 m1, 0) * (4 / max(N', 1)).  Elsewhere the temporal variance stands
 *   a-trous i    s = 1 << i; h = (1/16, 1/4, 3/8, 1/4, 1/16); taps p + s (dx, dy), dy outer, dx inner, inside the image
 *                and geometry; the centre counts with w = h(0) h(0).  vbar: the 3 x 3 Gaussian (centre 1/4, edge 1/8,
 *                corner 1/16) of the variance at p + (dx, dy) over the geometry taps inside, sum(k v) / sum(k).
 *                x_l = |l_q - l_p| / (sigmaLuminance sqrt(vbar) + 1e-4), l of the pass's input colours
 *                t_x = g_x * float(s dx), t_y = g_y * float(s dy)
 *                x_z = |z_q - ((z_p + t_x) + t_y)| / (sigmaDepth (|t_x| + |t_y|) + 1e-3 z_p)
 *                w_n = max(0, dot(n_p, n_q)) squared normalPowerLog2 times
 *                F(x) = t^8, t = max(0, 1 - x * .125), by three squarings; w = (h(dx) h(dy)) * (w_n * F(x_z + x_l))
 *                colour = sum(w c_q) / sum(w), variance = sum((w w) v_q) / (sum(w) sum(w))
 *   output       passes ping-pong between two images.  The output of pass feedbackIteration (rgb and variance) is the
 *                next call's colour history; moments, length and guide come from the temporal stage.  After the last
 *                pass: times max(albedo, 1/64) with demodulate, the input's alpha, stored to the HDR image
 * Host inputs go through a grow-only staging buffer; the working and history images (176 bytes per pixel) are
 * grow-only too.  Refused, before the device is touched and changing nothing: a NULL pc, camera or inputs; iterations
 * above 5, demodulate or resetHistory above 1, maxHistoryLength outside 1 .. 255, normalPowerLog2 above 8; a float
 * parameter that is not finite or not positive, minAlpha above 1; an empty extent or one above 32768; a partly given
 * G-buffer; with onDevice an illumination, albedo or normal pointer that is not 16-byte, a velocity that is not 8-byte
 * or a depth that is not 4-byte aligned; illumination = NULL when the HDR image has another extent; a NULL velocity or
 * G-buffer when none of this extent has been traced. */
int prosper_pt_denoise(
    prosper_pt_ctx *ctx, const prosper_pt_denoise_pc *pc, const prosper_CameraUniforms *camera, uint32_t width, uint32_t height,
    const prosper_pt_denoise_inputs *inputs, void *stream);
/* The next call ignores the history.  (The images stay allocated.) */
void prosper_pt_denoise_release_history(prosper_pt_ctx *ctx);
/* The images of the last call, each width*height records of 16 bytes.  The guide and the moments are what the temporal
 * stage made AND what the next call reads as its previous frame; HISTORY_COLOUR is the colour history the next call
 * reads.  An a-trous image is held while no later pass has written over it: the last two passes' are. */
enum
{
    PROSPER_PT_DENOISE_GUIDE_A = 0,        /* float z, dz/dx, dz/dy; uint32 geometry flag */
    PROSPER_PT_DENOISE_GUIDE_B = 1,        /* float n.x, n.y, n.z, 0 */
    PROSPER_PT_DENOISE_MOMENTS = 2,        /* float m1, m2; uint32 history length; 0 */
    PROSPER_PT_DENOISE_TEMPORAL = 3,       /* float r, g, b of the temporal stage, the variance after the estimate */
    PROSPER_PT_DENOISE_ATROUS_0 = 4,       /* .. ATROUS_0 + 4: float r, g, b, variance after that pass */
    PROSPER_PT_DENOISE_HISTORY_COLOUR = 9, /* float r, g, b, variance of the fed-back image */
    PROSPER_PT_DENOISE_STAGE_COUNT = 10,
};
/* Synchronises `stream` and copies one of them to host memory; `bytes` must be exactly width*height*16 of the last
 * call.  NO_SCENE before the first call, and for the history images when there is no history. */
int prosper_pt_read_denoise_stage(prosper_pt_ctx *ctx, uint32_t stage, void *host, size_t bytes, void *stream);
typedef struct prosper_pt_denoise_info
{
    uint32_t valid;           /* 1 once prosper_pt_denoise ran */
    uint32_t width, height;   /* of the last call */
    uint32_t historyValid;    /* 1: the next call of this extent reads a history */
    uint32_t ignoredHistory;  /* 1: the last call ignored the history */
    uint32_t iterations;      /* of the last call */
    uint32_t historyPixels;   /* geometry pixels of the last call with a usable history ... */
    uint32_t noHistoryPixels; /* ... and without; counted by the temporal kernel, one atomic per wave and counter */
    /* device time of each stage of the last call (reading them waits for it); an a-trous pass that did not run takes
     * none; finishMs covers the store to the HDR image when no a-trous pass ran (otherwise the last pass stores) */
    float temporalMs, varianceMs, atrousMs[5], finishMs, totalMs;
} prosper_pt_denoise_info;
int prosper_pt_get_denoise_info(prosper_pt_ctx *ctx, prosper_pt_denoise_info *out);

/* ---- multi-GPU: image stripes per rank + ONE gather of the per-rank HDR tiles over RCCL + de-interleave ----
 * (north star: "the image is tiled across the 8 GPUs of one node with an RCCL gather over xGMI of
 * per-tile HDR buffers".)  The reference renders the whole image on one GPU and asserts renderArea.offset == 0
 * (src/render/RtReference.cpp:327): these entry points have no counterpart there.  One process (or thread) per GPU,
 * one context each; rank r renders with prosper_pt_tile_desc{stripeWidth, r, ranks}; pixels are independent
 * (seed = absolute pixel + frame index, main.rgen:229), so nothing is exchanged while rendering.
 *
 * RCCL is loaded on first use (dlopen librccl.so.1); without it these calls fail with PROSPER_PT_ERR_UNSUPPORTED.
 *   prosper_pt_comm_get_unique_id  ncclGetUniqueId: call on ONE rank, hand the 128 bytes to the others by any means
 *   prosper_pt_comm_init           ncclCommInitRank on the context's device (collective over the ranks)
 *   prosper_pt_comm_adopt          use the caller's ncclComm_t instead (borrowed, not destroyed)
 *   prosper_pt_gather_tiles        after a render with a tile: ncclGather of every rank's localWidth*height RGBA32F
 *                                  tile to `root` (grouped ncclSend/ncclRecv with per-rank counts when the stripes do
 *                                  not divide evenly), then on the root a HIP kernel writes the width*height image into
 *                                  `device_full_rgba32f` (ignored on the other ranks; NULL on the root: a buffer the context owns;
 *                                  with one rank: a copy).
 *                                  Enqueue-only.  Default: gather and de-interleave run on a stream the context owns,
 *                                  after the work queued on `stream` so far, and overlap what the caller enqueues next -
 *                                  the next render's accumulate kernel (the one writer of the tile) waits for them by
 *                                  itself; readers of `device_full_rgba32f` call prosper_pt_gather_wait first.
 *                                  PROSPER_PT_GATHER_IN_STREAM runs everything on `stream` instead.
 *   prosper_pt_gather_wait         makes `stream` wait for the last gather (+ de-interleave)
 *   prosper_pt_comm_query          the communicator's own rank count / rank / device and the last gather's device time
 *   prosper_pt_deinterleave_tiles  the root's kernel alone: `device_tiles` = the ranks' tiles back to back in rank order
 */
#define PROSPER_PT_COMM_ID_BYTES 128
enum
{
    PROSPER_PT_GATHER_IN_STREAM = 1u << 0,
};
int prosper_pt_comm_get_unique_id(uint8_t id[PROSPER_PT_COMM_ID_BYTES]);
int prosper_pt_comm_init(prosper_pt_ctx *ctx, const uint8_t id[PROSPER_PT_COMM_ID_BYTES], uint32_t rank, uint32_t ranks);
int prosper_pt_comm_adopt(prosper_pt_ctx *ctx, void *nccl_comm, uint32_t rank, uint32_t ranks);
int prosper_pt_comm_destroy(prosper_pt_ctx *ctx);
int prosper_pt_gather_tiles(
    prosper_pt_ctx *ctx, uint32_t root, void *device_full_rgba32f, size_t byte_size, uint32_t flags, void *stream);
int prosper_pt_gather_wait(prosper_pt_ctx *ctx, void *stream);
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice - not what the caller passed
 * to prosper_pt_comm_init), the gathers enqueued so far, and the device time of the last one: its collective + on the
 * root the de-interleave kernel, between two events on the stream it ran on (waits for it; 0 before the first).
 * Without a communicator: ranks 1, rank 0, the context's device. */
typedef struct prosper_pt_comm_info
{
    uint32_t ranks;
    uint32_t rank;
    int32_t device;
    uint32_t gathers;
    float lastGatherMs;
    uint32_t reserved;
} prosper_pt_comm_info;
int prosper_pt_comm_query(prosper_pt_ctx *ctx, prosper_pt_comm_info *out);
/* The root's gathered image: where the last prosper_pt_gather_tiles put it (the caller's buffer, or the context's own
 * when `device_full_rgba32f` was NULL), and a synchronising copy of it to host memory (width*height RGBA32F). */
int prosper_pt_get_gathered_device_ptr(prosper_pt_ctx *ctx, void **out_ptr, uint32_t *width, uint32_t *height);
int prosper_pt_read_gathered(prosper_pt_ctx *ctx, float *rgba32f, size_t byte_size, void *stream);
int prosper_pt_deinterleave_tiles(
    prosper_pt_ctx *ctx, const void *device_tiles, uint32_t ranks, uint32_t stripe_width, uint32_t width, uint32_t height,
    void *device_full_rgba32f, size_t byte_size, void *stream);

int prosper_pt_get_counters(prosper_pt_ctx *ctx, prosper_pt_counters *out, void *stream);
/* The same counters for one kernel stage (index as in prosper_pt_kernel_name): lets the roofline
 * of a single kernel be priced from the work that kernel did. */
int prosper_pt_get_stage_counters(prosper_pt_ctx *ctx, uint32_t stage, prosper_pt_counters *out, void *stream);
int prosper_pt_reset_counters(prosper_pt_ctx *ctx, void *stream);

/* Device time (ms) of the kernels launched by the last `prosper_pt_render(_frames)`, measured with
 * hipEvents around every launch on the stream it was launched on; blocks until they finish.
 * total_ms is the time on the caller's stream (wall time of the render on the device).  kernel_ms[i] is
 * the SUM over the kernel_launches[i] launches of stage i, named by prosper_pt_kernel_name(i); with the
 * two-chain default a launch that shared the GPU with the other chain's launch counts in full, so the
 * kernel_ms can add up to more than total_ms. */
#define PROSPER_PT_MAX_KERNELS 8
int prosper_pt_get_last_render_ms(prosper_pt_ctx *ctx, float *total_ms, float kernel_ms[PROSPER_PT_MAX_KERNELS]);
int prosper_pt_get_last_render_timing(
    prosper_pt_ctx *ctx, float *total_ms, float kernel_ms[PROSPER_PT_MAX_KERNELS],
    uint32_t kernel_launches[PROSPER_PT_MAX_KERNELS]);
const char *prosper_pt_kernel_name(uint32_t index);
/* Enables per-kernel hipEvent timing for subsequent renders (off by default: events add launches).  The readout
 * functions above report the last render that ran with timing on, also after timing has been switched off again
 * and further (untimed) renders have followed - up to two of them with PROSPER_PT_RENDER_PIPELINED. */
int prosper_pt_set_kernel_timing(prosper_pt_ctx *ctx, int enabled);

enum
{
    PROSPER_PT_FN_SINCOS = 0,         /* in: x                                out: sin, cos */
    PROSPER_PT_FN_POW = 1,            /* in: x, y                             out: pow */
    PROSPER_PT_FN_SRGB_TO_LINEAR = 2, /* in: x                                out: y */
    PROSPER_PT_FN_NORMALIZE = 3,      /* in: v3                               out: v3 */
    PROSPER_PT_FN_UNPACK_SNORM = 4,   /* in: bits (u32 in a float)            out: n3, sign */
    PROSPER_PT_FN_ONB = 5,            /* in: n3                               out: rows b1, b2, n */
    PROSPER_PT_FN_COSINE_SAMPLE = 6,  /* in: n3, u2                           out: v3 */
    PROSPER_PT_FN_VNDF_SAMPLE = 7,    /* in: Ve3, alpha, u2                   out: v3 */
    PROSPER_PT_FN_VNDF_PDF = 8,       /* in: Ve3, Le3, alpha                  out: pdf */
    PROSPER_PT_FN_EVAL_BRDF = 9,      /* in: l3, n3, v3, albedo3, rough, metal out: v3 */
    PROSPER_PT_FN_OFFSET_RAY = 10,    /* in: p3, n3                           out: v3 */
    PROSPER_PT_FN_POINT_LIGHT = 11,   /* in: pos3, radiance3, radius, surf3   out: l3, d, irr3 */
    PROSPER_PT_FN_SPOT_LIGHT = 12,    /* in: pos3, off, rad3, scale, dir3, surf3 out: l3, d, irr3 */
    PROSPER_PT_FN_TRIANGLE = 13,      /* in: o3, d3, v0, v1, v2, tmin, tmax   out: hit, t, bu, bv */
    PROSPER_PT_FN_HALF = 14,          /* in: f                                out: unpack(pack(f)), bits */
    PROSPER_PT_FN_RNG = 15,           /* in: px, py, frame (u32 bits)         out: rnd01, rnd2d01, seed */
    PROSPER_PT_FN_BC7_BLOCK = 16,     /* in: 4 words of a block (u32 bits)    out: 16 RGBA8 texels (u32 bits) */
    PROSPER_PT_FN_COUNT = 17,
};

/* Test hook for the alpha bounds (DESIGN.md "alpha bounds"): evaluates the device's sRGBtoLinear on EVERY float whose bit
 * pattern lies in [first_bits, last_bits] (non-negative floats, increasing) and reports how far it is from monotone:
 * *max_defect = max over x of (max of L over the inputs shortly before x) - L(x), 0 if monotone; *decreases = adjacent
 * input pairs whose outputs decrease.  The bounds are valid while max_defect < 4e-6 (kAlphaCurveSlack). */
int prosper_pt_debug_srgb_monotonicity(
    prosper_pt_ctx *ctx, uint32_t first_bits, uint32_t last_bits, float *max_defect, uint64_t *decreases);

/* Device self-test: evaluates device function `fn` (PROSPER_PT_FN_*) element-wise over `n`
 * records of `in_stride` floats and writes `out_stride` floats per record.  Test-only entry that
 * lets tests/ compare every device function with the oracle's restatement bit for bit. */
int prosper_pt_eval_device_fn(
    prosper_pt_ctx *ctx, uint32_t fn, const float *in, uint32_t in_stride, float *out,
    uint32_t out_stride, uint32_t n);

#ifdef __cplusplus
}
#endif

#endif /* PROSPER_PT_H */
