"""ctypes mirrors of include/prosper_pt/{shader_structs,prosper_pt}.h.

Layouts follow prosper's shared host/device structs (reference:
res/shader/shared/shader_structs/scene/*.h, push_constants/rt_reference.h); sizes are checked
against the C headers' static asserts in tests/test_structs.py.
"""
import ctypes as C

import numpy as np


class Vec4(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("w", C.c_float)]


class Mat4(C.Structure):
    _fields_ = [("col", Vec4 * 4)]


class Mat3x4(C.Structure):
    _fields_ = [("col", Vec4 * 3)]


class ReferencePC(C.Structure):
    """push_constants/rt_reference.h:6-16"""

    _fields_ = [
        ("drawType", C.c_uint32),
        ("flags", C.c_uint32),
        ("frameIndex", C.c_uint32),
        ("apertureDiameter", C.c_float),
        ("focusDistance", C.c_float),
        ("focalLength", C.c_float),
        ("rouletteStartBounce", C.c_uint32),
        ("maxBounces", C.c_uint32),
    ]


PC_FLAG_SKIP_HISTORY = 1 << 0
PC_FLAG_ACCUMULATE = 1 << 1
PC_FLAG_IBL = 1 << 2
PC_FLAG_DEPTH_OF_FIELD = 1 << 3
PC_FLAG_CLAMP_INDIRECT = 1 << 4

# src/scene/DrawType.hpp:8-10
DRAW_TYPES = [
    "Default", "PrimitiveID", "MeshletID", "MeshID", "MaterialID", "Position", "ShadingNormal",
    "TexCoord0", "Albedo", "Roughness", "Metallic",
]
DrawType = {name: i for i, name in enumerate(DRAW_TYPES)}

RT_MAX_BOUNCES = 6      # RtReference::sMaxBounces, src/render/RtReference.hpp:22
RT_FRAME_PERIOD = 4096  # sFramePeriod, src/render/RtReference.cpp:31


class CameraUniforms(C.Structure):
    """scene/camera.h:11-34"""

    _fields_ = [
        ("worldToCamera", Mat4),
        ("cameraToWorld", Mat4),
        ("cameraToClip", Mat4),
        ("clipToWorld", Mat4),
        ("previousWorldToCamera", Mat4),
        ("previousCameraToClip", Mat4),
        ("eye", Vec4),
        ("nearPlane", Vec4),
        ("farPlane", Vec4),
        ("leftPlane", Vec4),
        ("rightPlane", Vec4),
        ("topPlane", Vec4),
        ("bottomPlane", Vec4),
        ("resolution", C.c_uint32 * 2),
        ("currentJitter", C.c_float * 2),
        ("previousJitter", C.c_float * 2),
        ("near_", C.c_float),
        ("far_", C.c_float),
        ("maxViewScale", C.c_float),
    ]


class DrawInstance(C.Structure):
    _fields_ = [("modelInstanceIndex", C.c_uint32), ("meshIndex", C.c_uint32), ("materialIndex", C.c_uint32)]


class GeometryMetadata(C.Structure):
    _fields_ = [
        ("bufferIndex", C.c_uint32),
        ("indicesOffset", C.c_uint32),
        ("positionsOffset", C.c_uint32),
        ("normalsOffset", C.c_uint32),
        ("tangentsOffset", C.c_uint32),
        ("texCoord0sOffset", C.c_uint32),
        ("meshletsOffset", C.c_uint32),
        ("meshletBoundsOffset", C.c_uint32),
        ("meshletVerticesOffset", C.c_uint32),
        ("meshletTrianglesByteOffset", C.c_uint32),
        ("usesShortIndices", C.c_uint32),
    ]


ABSENT = 0xFFFFFFFF
ALPHA_MODE_OPAQUE, ALPHA_MODE_MASK, ALPHA_MODE_BLEND = 0, 1, 2


class MaterialData(C.Structure):
    _fields_ = [
        ("baseColorFactor", Vec4),
        ("metallicFactor", C.c_float),
        ("roughnessFactor", C.c_float),
        ("alphaCutoff", C.c_float),
        ("alphaMode", C.c_uint32),
        ("baseColorTextureSampler", C.c_uint32),
        ("metallicRoughnessTextureSampler", C.c_uint32),
        ("normalTextureSampler", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class ModelInstanceTransforms(C.Structure):
    _fields_ = [("modelToWorld", Mat3x4), ("normalToWorld", Mat3x4)]


class DirectionalLightParameters(C.Structure):
    _fields_ = [("irradiance", Vec4), ("direction", Vec4)]


class PointLight(C.Structure):
    _fields_ = [("radianceAndRadius", Vec4), ("position", Vec4)]


class SpotLight(C.Structure):
    _fields_ = [("radianceAndAngleScale", Vec4), ("positionAndAngleOffset", Vec4), ("direction", Vec4)]


MAX_POINT_LIGHT_COUNT = 1024
MAX_SPOT_LIGHT_COUNT = 1024


class PointLightsBuffer(C.Structure):
    _fields_ = [("lights", PointLight * MAX_POINT_LIGHT_COUNT), ("count", C.c_uint32)]


class SpotLightsBuffer(C.Structure):
    _fields_ = [("lights", SpotLight * MAX_SPOT_LIGHT_COUNT), ("count", C.c_uint32)]


# ---- prosper_pt.h ----

FORMAT_RGBA8_UNORM = 0
FORMAT_BC7_UNORM = 1
COMPRESS_SRGB = 1 << 0           # prosper_pt_compress_texture: generated levels average RGB in linear light
COMPRESS_GENERATE_MIPS = 1 << 1  # ... Texture2DOptions::generateMipMaps
PREPARE_GENERATE_TANGENTS = 1 << 0  # prosper_pt_prepare_mesh: tangents for a primitive with uvs and none of its own
PREPARE_MESHLETS = 1 << 1           # ... the four meshlet sections
FILTER_NEAREST, FILTER_LINEAR = 0, 1
WRAP_REPEAT, WRAP_MIRRORED_REPEAT, WRAP_CLAMP_TO_EDGE = 0, 1, 2

CREATE_MEGAKERNEL = 1 << 0
CREATE_PERSISTENT = 1 << 1  # reserved: prosper_pt_create refuses it
CREATE_SINGLE_CHAIN = 1 << 2
CREATE_TEXTURE_MIPS = 1 << 3  # every material texture keeps a mip chain (generated, or supplied: TextureDesc.mipLevelCount)
RENDER_COUNT_WORK = 1 << 0
RENDER_PIPELINED = 1 << 1
MAX_KERNELS = 8


class DeviceDesc(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device_ordinal", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class TextureDesc(C.Structure):
    _fields_ = [
        ("texels", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("format", C.c_uint32),
        ("mipLevelCount", C.c_uint32),  # read by a CREATE_TEXTURE_MIPS context only: levels held by `texels` (0 / 1: level 0)
    ]


class MeshSource(C.Structure):
    """prosper_pt_mesh_source"""
    _fields_ = [
        ("positions", C.c_void_p),
        ("normals", C.c_void_p),
        ("tangents", C.c_void_p),
        ("texCoord0s", C.c_void_p),
        ("indices", C.c_void_p),
        ("vertexCount", C.c_uint32),
        ("indexCount", C.c_uint32),
    ]


class PreparedMesh(C.Structure):
    """prosper_pt_prepared_mesh: the cache header's thirteen fields, as mesh_cache._FIELDS"""
    _fields_ = [(name, C.c_uint32) for name in (
        "indexCount", "vertexCount", "meshletCount", "positionsOffset", "normalsOffset", "tangentsOffset", "texCoord0sOffset",
        "meshletsOffset", "meshletBoundsOffset", "meshletVerticesOffset", "meshletTrianglesByteOffset", "usesShortIndices",
        "blobByteCount")]


class TextureMipsInfo(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("levelCount", C.c_uint32),
        ("srgbAveraged", C.c_uint32),
        ("mipTexelBytes", C.c_uint64),
    ]


class SamplerDesc(C.Structure):
    _fields_ = [("magFilter", C.c_uint32), ("minFilter", C.c_uint32), ("wrapS", C.c_uint32), ("wrapT", C.c_uint32)]


class MeshInfo(C.Structure):
    _fields_ = [
        ("vertexCount", C.c_uint32),
        ("indexCount", C.c_uint32),
        ("meshletCount", C.c_uint32),
        ("materialIndex", C.c_uint32),
    ]


class CubeDesc(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("faceSize", C.c_uint32), ("reserved", C.c_uint32)]


class SceneView(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("reserved", C.c_uint32),
        ("geometryBuffers", C.POINTER(C.c_void_p)),
        ("geometryBufferByteSizes", C.POINTER(C.c_uint64)),
        ("geometryBufferCount", C.c_uint32),
        ("meshCount", C.c_uint32),
        ("geometryMetadatas", C.POINTER(GeometryMetadata)),
        ("meshInfos", C.POINTER(MeshInfo)),
        ("drawInstances", C.POINTER(DrawInstance)),
        ("drawInstanceCount", C.c_uint32),
        ("modelInstanceCount", C.c_uint32),
        ("modelInstanceTransforms", C.POINTER(ModelInstanceTransforms)),
        ("materials", C.POINTER(MaterialData)),
        ("materialCount", C.c_uint32),
        ("textureCount", C.c_uint32),
        ("textures", C.POINTER(TextureDesc)),
        ("samplers", C.POINTER(SamplerDesc)),
        ("samplerCount", C.c_uint32),
        ("reserved2", C.c_uint32),
        ("directionalLight", C.POINTER(DirectionalLightParameters)),
        ("pointLights", C.POINTER(PointLightsBuffer)),
        ("spotLights", C.POINTER(SpotLightsBuffer)),
        ("skybox", CubeDesc),
    ]


class TileDesc(C.Structure):
    _fields_ = [("stripeWidth", C.c_uint32), ("stripeIndex", C.c_uint32), ("stripeCount", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [
        ("paths", C.c_uint64),
        ("closestRays", C.c_uint64),
        ("shadowRays", C.c_uint64),
        ("nodeVisits", C.c_uint64),
        ("triangleTests", C.c_uint64),
        ("closestHits", C.c_uint64),
        ("anyHitCalls", C.c_uint64),
        ("lightSamples", C.c_uint64),
        ("spotLightSamples", C.c_uint64),
        ("skyLookups", C.c_uint64),
        ("pixelsWritten", C.c_uint64),
        ("historyReads", C.c_uint64),
        ("shortIndexHits", C.c_uint64),
        ("shortIndexTriangleTests", C.c_uint64),
        ("nodePhaseSteps", C.c_uint64),
        ("trianglePhaseSteps", C.c_uint64),
        ("anyHitTexelFetches", C.c_uint64),
    ]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "reserved"}


class SceneStats(C.Structure):
    _fields_ = [
        ("triangleCount", C.c_uint64),
        ("nodeCount", C.c_uint64),
        ("nodeBytes", C.c_uint32),
        ("triangleBytes", C.c_uint32),
        ("maxDepth", C.c_uint32),
        ("variantFlags", C.c_uint32),
        ("deviceBytes", C.c_uint64),
        ("buildSeconds", C.c_double),
        ("uploadSeconds", C.c_double),
        ("bvhBuildSeconds", C.c_double),
        ("textureSeconds", C.c_double),
        ("alphaTriangleCount", C.c_uint64),
        ("alphaBoundBytes", C.c_uint64),
    ]


class HierarchyState(C.Structure):
    _fields_ = [("refits", C.c_uint32), ("rebuilds", C.c_uint32), ("costRatio", C.c_float), ("builtCost", C.c_float),
                ("nodeCount", C.c_uint32), ("levels", C.c_uint32), ("meshUpdates", C.c_uint32), ("geometryInstalls", C.c_uint32),
                ("geometryBuildRunning", C.c_uint32), ("reserved", C.c_uint32)]


# ---- the hierarchy built on the GPU (prosper_pt_build_hierarchy_gpu / prosper_pt_set_hierarchy_builder) ----
BUILDER_HOST, BUILDER_GPU = 0, 1
HIERARCHY_BUILD_STAGES = 8
HIERARCHY_BUILD_STAGE_NAMES = ("bounds", "codes", "sort", "radixTree", "collapse", "heights", "tables", "install")


class HierarchyBuildInfo(C.Structure):
    _fields_ = [("builder", C.c_uint32), ("selectedBuilder", C.c_uint32), ("leafSize", C.c_uint32), ("nodeCount", C.c_uint32),
                ("levels", C.c_uint32), ("depths", C.c_uint32), ("stackBound", C.c_uint32), ("reserved", C.c_uint32),
                ("stageMs", C.c_float * HIERARCHY_BUILD_STAGES), ("totalMs", C.c_float), ("reserved2", C.c_uint32)]


# the GPU builder's method (prosper_pt_set_gpu_hierarchy_method; prosper_amd/ploc.py states the PLOC rule)
GPU_HIERARCHY_LINEAR, GPU_HIERARCHY_PLOC = 0, 1


class GpuHierarchyMethodInfo(C.Structure):
    _fields_ = [("selectedMethod", C.c_uint32), ("selectedRadius", C.c_uint32), ("method", C.c_uint32), ("radius", C.c_uint32),
                ("rounds", C.c_uint32), ("finishRounds", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# the builds the GPU builder makes besides rebuilds (prosper_pt_set_gpu_hierarchy_sites): a mask, 0 by default
GPU_BUILD_SITE_UPLOAD, GPU_BUILD_SITE_MESH_UPDATES, GPU_BUILD_SITE_DRIFT = 1, 2, 4


# ---- keyframe animation (prosper_pt_set_animations / prosper_pt_animate) ----
ANIMATION_NONE = 0xFFFFFFFF
NODE_HAS_TRANSLATION, NODE_HAS_ROTATION, NODE_HAS_SCALE, NODE_DIRECTIONAL_LIGHT, NODE_CAMERA = 1, 2, 4, 8, 16
ANIMATION_PATH_TRANSLATION, ANIMATION_PATH_ROTATION, ANIMATION_PATH_SCALE = 0, 1, 2
ANIMATION_STEP, ANIMATION_LINEAR, ANIMATION_CUBICSPLINE = 0, 1, 2


class AnimationNode(C.Structure):
    _fields_ = [("parent", C.c_uint32), ("modelInstance", C.c_uint32), ("pointLight", C.c_uint32), ("spotLight", C.c_uint32),
                ("flags", C.c_uint32), ("translation", C.c_float * 3), ("rotation", C.c_float * 4), ("scale", C.c_float * 3)]


class AnimationChannel(C.Structure):
    _fields_ = [("node", C.c_uint32), ("path", C.c_uint32), ("interpolation", C.c_uint32), ("timeOffset", C.c_uint32),
                ("keyCount", C.c_uint32), ("valueOffset", C.c_uint32), ("valueWidth", C.c_uint32),
                ("startTimeS", C.c_float), ("endTimeS", C.c_float)]


class AnimationDesc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nodeCount", C.c_uint32), ("nodes", C.c_void_p),
                ("channelCount", C.c_uint32), ("timeCount", C.c_uint32), ("channels", C.c_void_p),
                ("times", C.c_void_p), ("values", C.c_void_p), ("valueCount", C.c_uint32), ("reserved", C.c_uint32)]


class AnimationStateInfo(C.Structure):
    """prosper_pt_animation_state"""

    _fields_ = [("endTimeS", C.c_float), ("nodeCount", C.c_uint32), ("animatedNodeCount", C.c_uint32), ("updates", C.c_uint32),
                ("cameraValid", C.c_uint32), ("lightUpdates", C.c_uint32), ("eye", C.c_float * 3), ("target", C.c_float * 3), ("up", C.c_float * 3),
                ("sampleMs", C.c_float), ("hierarchyMs", C.c_float)]


class DebugOptions(C.Structure):
    """prosper_pt_debug_options (include/prosper_pt/prosper_pt.h): tuning / test options of a context."""

    _fields_ = [("struct_size", C.c_uint32),
                ("batchedTextures", C.c_int32), ("widePacks", C.c_int32), ("alphaCellShift", C.c_int32),
                ("noTexturePacks", C.c_uint32), ("noAlphaBounds", C.c_uint32), ("noUploadRefit", C.c_uint32), ("flatBvh", C.c_uint32),
                ("sahTraversalCost", C.c_float), ("boxPad", C.c_float), ("leafSize", C.c_uint32), ("buildThreads", C.c_uint32),
                ("topEntries", C.c_uint32), ("nodeOrder", C.c_int32), ("childOrder", C.c_int32), ("buildTiming", C.c_uint32),
                ("segments", C.c_uint32), ("segmentLength", C.c_uint32), ("chains", C.c_uint32), ("ldsStackEntries", C.c_uint32),
                ("noLdsScene", C.c_uint32), ("noLdsTables", C.c_uint32), ("traceDeadPaths", C.c_uint32), ("bandedBatches", C.c_int32),
                ("rebuildCostRatio", C.c_float), ("alwaysRebuild", C.c_uint32), ("failNextUpdate", C.c_uint32),
                # reserved (removed experiments): must be 0
                ("poolVariant", C.c_uint32), ("rawRecords", C.c_uint32), ("tileOrder", C.c_uint32), ("hipGraph", C.c_uint32),
                ("pipelinedChains", C.c_uint32), ("mergeLimit", C.c_uint32)]


class CommInfo(C.Structure):
    _fields_ = [("ranks", C.c_uint32), ("rank", C.c_uint32), ("device", C.c_int32), ("gathers", C.c_uint32),
                ("lastGatherMs", C.c_float), ("reserved", C.c_uint32)]


class MeshUpdate(C.Structure):
    """prosper_pt_mesh_update: one streamed-in mesh (WorldData::pollMeshWorker)."""
    _fields_ = [("meshIndex", C.c_uint32), ("reserved", C.c_uint32), ("metadata", GeometryMetadata), ("info", MeshInfo),
                ("bytes", C.c_void_p), ("byteOffset", C.c_uint64), ("byteCount", C.c_uint64), ("bufferByteSize", C.c_uint64)]


MAX_GEOMETRY_BUFFERS = 100
GATHER_IN_STREAM = 1
UPDATE_NOW = 1
VARIANT_LDS_SCENE = 1
VARIANT_LDS_TABLES = 2
VARIANT_BATCHED_TEXTURES = 4
VARIANT_TEXTURE_PACKS = 8
VARIANT_RAW_RECORDS = 16  # reserved: never set
VARIANT_STACK_SHIFT = 8


def as_numpy(struct_array, dtype=np.uint8):
    """View a ctypes structure/array as a numpy byte array (no copy)."""
    return np.frombuffer(struct_array, dtype=dtype)


class RestirTracePC(C.Structure):
    """TracePC, res/shader/shared/shader_structs/push_constants/restir_di/trace.h"""
    _fields_ = [("drawType", C.c_uint32), ("frameIndex", C.c_uint32), ("flags", C.c_uint32)]


class RestirInputs(C.Structure):
    _fields_ = [("albedoRoughness", C.c_void_p), ("normalMetallic", C.c_void_p), ("nonLinearDepth", C.c_void_p),
                ("reservoirs", C.c_void_p), ("onDevice", C.c_uint32), ("reserved", C.c_uint32)]


# prosper_pt_restir_di_resample stages and prosper_pt_restir_di_record flags
RESTIR_INITIAL = 0
RESTIR_SPATIAL = 1
RESTIR_SPATIAL_REUSE = 1

# prosper_pt_restir_di_record: trace the G-buffer first (optionally jittered)
RESTIR_TRACE_GBUFFER = 1 << 1
RESTIR_JITTER_GBUFFER = 1 << 2
# prosper_pt_trace_gbuffer flags
GBUFFER_JITTER = 1 << 0
GBUFFER_OPAQUE_ONLY = 1 << 2  # BLEND candidates always rejected (both G-buffer entries); bit 1 stays an unknown flag


class GBufferTargets(C.Structure):
    _fields_ = [("albedoRoughness", C.c_void_p), ("normalMetallic", C.c_void_p), ("nonLinearDepth", C.c_void_p)]


class VelocityGBufferDesc(C.Structure):
    """prosper_pt_velocity_gbuffer_desc: the three targets (all or none), the velocity target (None: context-owned), the
    previous frame's instance transforms on the host (None: the instances did not move)"""
    _fields_ = [("targets", GBufferTargets), ("velocity", C.c_void_p), ("previousTransforms", C.c_void_p),
                ("previousTransformCount", C.c_uint32)]


class DeferredShadingPC(C.Structure):
    """DeferredShadingPC, res/shader/shared/shader_structs/push_constants/deferred_shading.h"""
    _fields_ = [("drawType", C.c_uint32), ("ibl", C.c_uint32)]


# prosper_pt_deferred_shading flags: trace the G-buffer first (optionally jittered)
DEFERRED_TRACE_GBUFFER = 1 << 0
DEFERRED_JITTER_GBUFFER = 1 << 1
# LightClustering: 32x32-pixel tiles, 16 depth slices (+ 1), 128 point + 128 spot entries per cluster
CLUSTER_DIM = 32
CLUSTER_Z_SLICES = 16
CLUSTER_MAX_POINTS = 128
CLUSTER_MAX_SPOTS = 128


class ForwardPC(C.Structure):
    """ForwardPC, res/shader/shared/shader_structs/push_constants/forward.h (previousTransformValid is not read)"""
    _fields_ = [("drawType", C.c_uint32), ("ibl", C.c_uint32), ("previousTransformValid", C.c_uint32)]


class ForwardOpaqueDesc(C.Structure):
    """prosper_pt_forward_opaque_desc: the depth and velocity targets on the device (None: context-owned), the previous
    frame's instance transforms on the host (None: the instances did not move)"""
    _fields_ = [("nonLinearDepth", C.c_void_p), ("velocity", C.c_void_p), ("previousTransforms", C.c_void_p),
                ("previousTransformCount", C.c_uint32)]


class ForwardOpaqueInfo(C.Structure):
    """prosper_pt_forward_opaque_info of the last forward shade"""
    _fields_ = [("shadedPixels", C.c_uint32), ("reclustered", C.c_uint32), ("ms", C.c_float), ("shadeMs", C.c_float)]


class RasterTransparentInfo(C.Structure):
    """prosper_pt_raster_transparent_info of the last rasterised transparent pass"""
    _fields_ = [("fragments", C.c_uint32), ("coveredPixels", C.c_uint32), ("shadedLayers", C.c_uint32), ("maxLayers", C.c_uint32),
                ("reclustered", C.c_uint32), ("countMs", C.c_float), ("scanMs", C.c_float), ("fillMs", C.c_float),
                ("resolveMs", C.c_float), ("reserved", C.c_uint32)]


class RasterFragment(C.Structure):
    """prosper_pt_raster_fragment: one entry of a pixel's list as prosper_pt_read_raster_fragments decodes it (16 bytes)"""
    _fields_ = [("drawInstance", C.c_uint32), ("meshlet", C.c_uint32), ("triangle", C.c_uint32), ("depth", C.c_float)]


# prosper_pt_forward_transparent flags: which of the G-buffer's rays the pass follows (neither: the pixel centre)
TRANSPARENT_JITTER = 1 << 0
TRANSPARENT_CAMERA_JITTER = 1 << 1


class TransparentInfo(C.Structure):
    """prosper_pt_transparent_info of the last prosper_pt_forward_transparent"""
    _fields_ = [("coveredPixels", C.c_uint32), ("maxLayers", C.c_uint32), ("totalLayers", C.c_uint64),
                ("ms", C.c_float), ("reclustered", C.c_uint32)]


class TransparentLayer(C.Structure):
    """prosper_pt_transparent_layer: one layer of a pixel as the pass's debug mode records it (64 bytes)"""
    _fields_ = [("drawInstance", C.c_uint32), ("primitive", C.c_uint32), ("positionWS", C.c_float * 3),
                ("nonLinearDepth", C.c_float), ("albedo", C.c_float * 3), ("roughness", C.c_float),
                ("normal", C.c_float * 3), ("metallic", C.c_float), ("alpha", C.c_float), ("reserved", C.c_uint32)]


class Particle(C.Structure):
    """prosper_pt_particle == Particle, res/shader/shared/shader_structs/particles/particle.h (64 bytes)"""
    _fields_ = [("position_lifetime", Vec4), ("normal_spawnRateS", Vec4), ("velocity_spawnTimerS", Vec4),
                ("mask", C.c_uint32), ("_pad0", C.c_uint32), ("_pad1", C.c_uint32), ("_pad2", C.c_uint32)]


# the same record as a NumPy structured dtype (what Context.read_particles returns)
PARTICLE_DTYPE = np.dtype([("position_lifetime", np.float32, 4), ("normal_spawnRateS", np.float32, 4),
                           ("velocity_spawnTimerS", np.float32, 4), ("mask", np.uint32), ("_pad", np.uint32, 3)])
PARTICLE_MASK_GRAVITY = 1 << 0
PARTICLE_MASK_DECAY = 1 << 1
PARTICLE_MASK_EMIT = 1 << 2
PARTICLE_DEAD = -9999.0            # a dead slot's position_lifetime, all four
MAX_PARTICLE_COUNT = 500000        # Particles.hpp sMaxParticleCount: what maxParticleCount 0 means
PARTICLES_DECAY = 1 << 0           # prosper_pt_particles stages
PARTICLES_INIT = 1 << 1
PARTICLES_SIMULATE = 1 << 2
PARTICLES_RENDER = 1 << 3
PARTICLES_ALL = 15


class ParticlesPC(C.Structure):
    """prosper_pt_particles_pc: DecayPC, InitPC, SimulatePC and RenderPC of push_constants/particles/ in one"""
    _fields_ = [("maxParticleCount", C.c_uint32), ("sourceDrawInstanceIndex", C.c_uint32), ("reset", C.c_uint32),
                ("deltaTimeS", C.c_float), ("simulateFrameIndex", C.c_uint32), ("renderFrameIndex", C.c_uint32)]


class ParticlesInfo(C.Structure):
    """prosper_pt_particles_info of the last prosper_pt_particles"""
    _fields_ = [("valid", C.c_uint32), ("initRecorded", C.c_uint32), ("maxParticleCount", C.c_uint32),
                ("liveCount", C.c_uint32), ("freelistCount", C.c_uint32), ("grantedSpawns", C.c_uint32),
                ("refusedSpawns", C.c_uint32), ("fragmentsWritten", C.c_uint32), ("decayMs", C.c_float),
                ("initMs", C.c_float), ("simulateMs", C.c_float), ("renderMs", C.c_float)]


MAX_DEBUG_LINE_COUNT = 100000  # DebugGeometry.hpp DebugLines::sMaxLineCount


class DebugLinesInfo(C.Structure):
    """prosper_pt_debug_lines_info of the last prosper_pt_debug_lines"""
    _fields_ = [("valid", C.c_uint32), ("lineCount", C.c_uint32), ("fragmentsWritten", C.c_uint32),
                ("linesClippedAway", C.c_uint32), ("ms", C.c_float)]


class HizInfo(C.Structure):
    """prosper_pt_hiz_info: one slot's depth pyramid (level 0's extent, the depth's extent it was made from)"""
    _fields_ = [("valid", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("levelCount", C.c_uint32),
                ("sourceWidth", C.c_uint32), ("sourceHeight", C.c_uint32), ("launches", C.c_uint32), ("reserved", C.c_uint32)]


CULL_MODE_OPAQUE, CULL_MODE_TRANSPARENT = 0, 1
DRAW_LIST_GENERATED, DRAW_LIST_FIRST_PHASE, DRAW_LIST_SECOND_PHASE_INPUT, DRAW_LIST_SECOND_PHASE = range(4)
NO_HIZ = 0xFFFFFFFF  # PROSPER_PT_NO_HIZ


class DrawStats(C.Structure):
    """prosper_pt_draw_stats: render::DrawStats"""
    _fields_ = [("drawnMeshletCount", C.c_uint32), ("rasterizedTriangleCount", C.c_uint32), ("totalTriangleCount", C.c_uint32),
                ("totalMeshletCount", C.c_uint32), ("totalMeshCount", C.c_uint32), ("totalModelCount", C.c_uint32)]


RASTER_CLEAR = 1  # PROSPER_PT_RASTER_CLEAR


class GBufferRendererOutput(C.Structure):
    """prosper_host_gbuffer_renderer_output: device pointers in place of the reference's image handles"""
    _fields_ = [("albedoRoughness", C.c_void_p), ("normalMetalness", C.c_void_p), ("velocity", C.c_void_p), ("depth", C.c_void_p)]


class ForwardRendererOutput(C.Structure):
    """prosper_host_forward_renderer_output: device pointers in place of the reference's image handles"""
    _fields_ = [("illumination", C.c_void_p), ("velocity", C.c_void_p), ("depth", C.c_void_p)]


class RasterDrawInfo(C.Structure):
    """prosper_pt_raster_draw_info: what one draw of the rasteriser counted, and the device time of its two kernels"""
    _fields_ = [("valid", C.c_uint32), ("triangles", C.c_uint32), ("culledBackface", C.c_uint32), ("culledZeroArea", C.c_uint32),
                ("culledOutside", C.c_uint32), ("clipped", C.c_uint32), ("queued", C.c_uint32), ("fragments", C.c_uint32),
                ("queueOverflow", C.c_uint32), ("meshletsMs", C.c_float), ("largeMs", C.c_float), ("reserved", C.c_uint32)]


class RasterInfo(C.Structure):
    """prosper_pt_raster_info: the visibility image's extent; draw[0] cleared it, draw[1] drew on top"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("draw", RasterDrawInfo * 2)]


class MeshletCullerOutput(C.Structure):
    """prosper_host_meshlet_culler_output: device pointers in place of the reference's buffer handles"""
    _fields_ = [("dataBuffer", C.c_void_p), ("argumentBuffer", C.c_void_p), ("secondPhaseInput", C.c_void_p),
                ("capacity", C.c_uint32), ("reserved", C.c_uint32)]


NOT_READY = -7  # PROSPER_PT_NOT_READY
(DEBUG_FORMAT_RGBA32F, DEBUG_FORMAT_RG32F, DEBUG_FORMAT_R32F, DEBUG_FORMAT_RGBA16F, DEBUG_FORMAT_RG16F, DEBUG_FORMAT_R16F,
 DEBUG_FORMAT_RG16_UNORM, DEBUG_FORMAT_RGBA8_UNORM) = range(8)


TEXTURE_DEBUG_CHANNEL_RGB = 4  # channels 0-3: one component in all three
TEXTURE_DEBUG_ABS_BEFORE_RANGE, TEXTURE_DEBUG_ZOOM, TEXTURE_DEBUG_MAGNIFIER = 1 << 3, 1 << 4, 1 << 5


class TextureDebugPC(C.Structure):
    """prosper_pt_texture_debug_pc: TextureDebugPC of push_constants/texture_debug.h"""
    _fields_ = [("inRes", C.c_int32 * 2), ("outRes", C.c_int32 * 2), ("range", C.c_float * 2), ("lod", C.c_uint32),
                ("flags", C.c_uint32), ("cursorUv", C.c_float * 2)]


class DebugResource(C.Structure):
    """prosper_pt_debug_resource: one 2-D image of the context's registry"""
    _fields_ = [("name", C.c_char * 64), ("format", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("levelCount", C.c_uint32), ("valid", C.c_uint32)]


class IblInfo(C.Structure):
    """prosper_pt_ibl_info: whether the maps exist for the current scene, their sizes, the last generation's pass times"""
    _fields_ = [("generated", C.c_uint32), ("irradianceSize", C.c_uint32), ("radianceSize", C.c_uint32),
                ("radianceMips", C.c_uint32), ("lutSize", C.c_uint32), ("irradianceMs", C.c_float),
                ("radianceMs", C.c_float), ("lutMs", C.c_float)]


class DofPC(C.Structure):
    """prosper_pt_dof_pc: the push-constant values of the depth-of-field passes (Setup.cpp:163-177, Dilate.cpp:105-127)"""
    _fields_ = [("focusDistance", C.c_float), ("maxBackgroundCoC", C.c_float), ("maxCoC", C.c_float),
                ("gatherRadius", C.c_int32)]


class DofInputs(C.Structure):
    """prosper_pt_dof_inputs: illumination (None: the HDR image in place), depth (None: the last traced G-buffer's)"""
    _fields_ = [("illumination", C.c_void_p), ("nonLinearDepth", C.c_void_p), ("onDevice", C.c_uint32),
                ("reserved", C.c_uint32)]


class DofInfo(C.Structure):
    """prosper_pt_dof_info: the last depth-of-field call's extents, mip count and per-stage device times"""
    _fields_ = [(n, C.c_uint32) for n in ("valid", "width", "height", "halfWidth", "halfHeight", "tileWidth",
                                          "tileHeight", "mips")] + [
        (n, C.c_float) for n in ("setupMs", "reduceMs", "flattenMs", "dilateMs", "gatherForegroundMs",
                                 "gatherBackgroundMs", "filterForegroundMs", "filterBackgroundMs", "combineMs")]


# prosper_pt_read_dof_stage: one value per intermediate of depth of field
DOF_STAGES = ("half_illumination", "half_coc", "tile_min_max", "dilated_tile_min_max", "fg_gather", "bg_gather",
              "fg_filtered", "bg_filtered")
(DOF_HALF_ILLUMINATION, DOF_HALF_COC, DOF_TILE_MIN_MAX, DOF_DILATED_TILE_MIN_MAX, DOF_FG_GATHER, DOF_BG_GATHER,
 DOF_FG_FILTERED, DOF_BG_FILTERED) = range(8)
DOF_TAPS = 121  # six octaweb rings: 1 + 8 + 16 + 24 + 32 + 40


class BloomPC(C.Structure):
    """prosper_pt_bloom_pc: threshold (Separate.hpp), blend factors and sampling (Compose.hpp), resolution scale
    (0 Half, 1 Quarter; Bloom.hpp).  BloomPC.default() holds prosper's defaults."""
    _fields_ = [("threshold", C.c_float), ("blendFactors", C.c_float * 3), ("resolutionScale", C.c_uint32),
                ("biquadratic", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def default(cls, threshold=1.0, blend_factors=(0.9, 0.04, 0.04), resolution_scale=0, biquadratic=1):
        return cls(threshold, (C.c_float * 3)(*blend_factors), resolution_scale, biquadratic, (C.c_uint32 * 2)(0, 0))


class BloomInfo(C.Structure):
    """prosper_pt_bloom_info: the last bloom call's extents, first blurred level, streak half-width and per-stage device
    times"""
    _fields_ = [(n, C.c_uint32) for n in ("valid", "width", "height", "workingWidth", "workingHeight", "firstLevel",
                                          "streakHalfWidth")] + [
        ("separateMs", C.c_float), ("reduceMs", C.c_float), ("blurHorizontalMs", C.c_float * 3),
        ("blurVerticalMs", C.c_float * 3), ("composeMs", C.c_float)]


# prosper_pt_read_bloom_stage: the three working images of bloom, four levels each
BLOOM_STAGES = ("highlights", "horizontal", "blurred")
BLOOM_HIGHLIGHTS, BLOOM_HORIZONTAL, BLOOM_BLURRED = range(3)
BLOOM_LEVELS = 4
BLOOM_HALF, BLOOM_QUARTER = 0, 1


class BloomFftPC(C.Structure):
    """prosper_pt_bloom_fft_pc: threshold (Separate.hpp), resolution scale (0 Half, 1 Quarter), sampling (Compose.hpp) and
    prosper's "Re-generate kernel".  BloomFftPC.default() holds prosper's defaults."""
    _fields_ = [("threshold", C.c_float), ("resolutionScale", C.c_uint32), ("biquadratic", C.c_uint32),
                ("regenerateKernel", C.c_uint32), ("reserved", C.c_uint32 * 4)]

    @classmethod
    def default(cls, threshold=1.0, resolution_scale=0, biquadratic=1, regenerate_kernel=0):
        return cls(threshold, resolution_scale, biquadratic, regenerate_kernel, (C.c_uint32 * 4)(0, 0, 0, 0))


class BloomFftPlan(C.Structure):
    """prosper_pt_bloom_fft_plan: the transform's and the kernel image's extents and the convolution's scale"""
    _fields_ = [("dim", C.c_uint32), ("kernelDim", C.c_uint32), ("convolutionScale", C.c_float)]


class BloomFftInfo(C.Structure):
    """prosper_pt_bloom_fft_info: the last FFT bloom's extents, whether it remade the kernel's DFT, which stages ran
    fused and the per-stage device times"""
    _fields_ = [(n, C.c_uint32) for n in ("valid", "width", "height", "dim", "kernelDim", "kernelRemade")] + [
        ("convolutionScale", C.c_float), ("fused", C.c_uint32)] + [
        (n, C.c_float) for n in ("separateMs", "generateMs", "prepareMs", "kernelFftMs", "forwardFftMs", "convolutionMs",
                                 "inverseFftMs", "composeMs")]


# prosper_pt_read_bloom_fft_stage: the images of the FFT technique
BLOOM_FFT_STAGES = ("highlights", "kernel", "kernel_dft", "convolved")
BLOOM_FFT_HIGHLIGHTS, BLOOM_FFT_KERNEL, BLOOM_FFT_KERNEL_DFT, BLOOM_FFT_CONVOLVED = range(4)
BLOOM_MULTI_RESOLUTION_BLUR, BLOOM_FFT = 0, 1  # render::bloom::Technique


TAA_CLIPPING_NONE, TAA_CLIPPING_MIN_MAX, TAA_CLIPPING_VARIANCE = range(3)
TAA_VELOCITY_CENTER, TAA_VELOCITY_LARGEST, TAA_VELOCITY_CLOSEST = range(3)


class TaaPC(C.Structure):
    """prosper_pt_taa_pc: the specialisation constants of taa_resolve.comp and resetHistory.  TaaPC.default() holds
    prosper's defaults (TemporalAntiAliasing.hpp): Catmull-Rom, Variance, Closest, luminance weighting."""
    _fields_ = [(n, C.c_uint32) for n in ("catmullRom", "colorClipping", "velocitySampling", "luminanceWeighting",
                                          "resetHistory")]

    @classmethod
    def default(cls, catmull_rom=1, color_clipping=TAA_CLIPPING_VARIANCE, velocity_sampling=TAA_VELOCITY_CLOSEST,
                luminance_weighting=1, reset_history=0):
        return cls(catmull_rom, color_clipping, velocity_sampling, luminance_weighting, reset_history)


class TaaInputs(C.Structure):
    """prosper_pt_taa_inputs: illumination (None: the HDR image in place), velocity, depth (None: the last traced
    G-buffer's; read by Closest alone)"""
    _fields_ = [("illumination", C.c_void_p), ("velocity", C.c_void_p), ("nonLinearDepth", C.c_void_p),
                ("onDevice", C.c_uint32)]


class TaaInfo(C.Structure):
    """prosper_pt_taa_info: the last resolve's extent, whether a history exists, whether the call ignored it, and the
    device times of its two kernels"""
    _fields_ = [(n, C.c_uint32) for n in ("valid", "width", "height", "historyValid", "ignoredHistory")] + [
        ("resolveMs", C.c_float), ("expandMs", C.c_float)]


class DenoisePC(C.Structure):
    """prosper_pt_denoise_pc: the parameters of the spatiotemporal denoiser.  DenoisePC.default() holds
    prosper_pt_denoise_pc_default's values."""
    _fields_ = [(n, C.c_uint32) for n in ("iterations", "demodulate", "maxHistoryLength", "feedbackIteration",
                                          "normalPowerLog2", "resetHistory")] + [
        (n, C.c_float) for n in ("minAlpha", "depthTolerance", "normalThreshold", "sigmaDepth", "sigmaLuminance")]

    @classmethod
    def default(cls, iterations=5, demodulate=1, max_history_length=32, feedback_iteration=1, normal_power_log2=7,
                reset_history=0, min_alpha=0.05, depth_tolerance=0.1, normal_threshold=0.9, sigma_depth=1.0,
                sigma_luminance=4.0):
        return cls(iterations, demodulate, max_history_length, feedback_iteration, normal_power_log2, reset_history,
                   min_alpha, depth_tolerance, normal_threshold, sigma_depth, sigma_luminance)


class DenoiseInputs(C.Structure):
    """prosper_pt_denoise_inputs: illumination (None: the HDR image in place), the G-buffer (all None: the last traced
    one), velocity (None: the last traced velocity target)"""
    _fields_ = [("illumination", C.c_void_p), ("albedoRoughness", C.c_void_p), ("normalMetallic", C.c_void_p),
                ("nonLinearDepth", C.c_void_p), ("velocity", C.c_void_p), ("onDevice", C.c_uint32)]


class DenoiseInfo(C.Structure):
    """prosper_pt_denoise_info: the last call's extent, history flags, the pixels with and without a usable history and
    the device time per stage"""
    _fields_ = [(n, C.c_uint32) for n in ("valid", "width", "height", "historyValid", "ignoredHistory", "iterations",
                                          "historyPixels", "noHistoryPixels")] + [
        ("temporalMs", C.c_float), ("varianceMs", C.c_float), ("atrousMs", C.c_float * 5), ("finishMs", C.c_float),
        ("totalMs", C.c_float)]


# prosper_pt_read_denoise_stage: the images of the last denoise, 16 bytes per pixel each
DENOISE_GUIDE_A, DENOISE_GUIDE_B, DENOISE_MOMENTS, DENOISE_TEMPORAL, DENOISE_ATROUS_0 = range(5)
DENOISE_HISTORY_COLOUR = 9
DENOISE_STAGE_COUNT = 10


# ImageBasedLighting: the irradiance cube, the prefiltered radiance cube (mips 512 ... 1) and the BRDF LUT
IBL_IRRADIANCE_SIZE = 64
IBL_RADIANCE_SIZE = 512
IBL_RADIANCE_MIPS = 10
IBL_LUT_SIZE = 512
