// pt_particles_passes.cpp — C-ABI of prosper's particle system (include/prosper_pt/prosper_pt.h): prosper_pt_particles
// over the context's particle pool, freelist and HDR image, and what reads and places them.  Kernels: pt_particles.hip.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include "pt_context.hpp"
#include "pt_math.hpp"
#include "pt_particles.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

struct ParticlesPassState
{
    DeviceBuffer particles, freelist, staging, stats, keys;
    uint32_t maxParticleCount = 0; // of the pool the buffers hold; 0: none yet
    size_t keyPixels = 0;          // the keys are zero for this many pixels
    bool valid = false;            // a call has run
    bool initRecorded = false;     // ... and recorded init
    StageEvents<kParticleStages> timing;
};

extern const PassModule kParticlesPasses = pass_module<ParticlesPassState, &prosper_pt_ctx::particlesPasses>();

} // namespace ppt

namespace
{

constexpr uint32_t kAllStages =
    PROSPER_PT_PARTICLES_DECAY | PROSPER_PT_PARTICLES_INIT | PROSPER_PT_PARTICLES_SIMULATE | PROSPER_PT_PARTICLES_RENDER;
constexpr uint32_t kMaxPool = 1u << 26; // 4 GiB of records

uint32_t pool_size(uint32_t maxParticleCount) { return maxParticleCount ? maxParticleCount : kDefaultMaxParticleCount; }

ParticleBuffers buffers_of(const ParticlesPassState &st)
{
    ParticleBuffers b = {};
    b.particles = st.particles.as<prosper_pt_particle>();
    b.freelist = st.freelist.as<int32_t>();
    b.staging = st.staging.as<prosper_pt_particle>();
    b.stats = st.stats.as<ParticleCallStats>();
    b.maxParticleCount = st.maxParticleCount;
    return b;
}

// The pool holds `max` slots: as it is, or reallocated (`fresh`: filled as Particles::init uploads it)
int ensure_pool(ParticlesPassState &st, uint32_t max, bool fresh, hipStream_t s)
{
    if (st.maxParticleCount == max) return PROSPER_PT_OK;
    st.maxParticleCount = 0;
    st.valid = false;
    int rc = grow_to(st.particles, (size_t)max * sizeof(prosper_pt_particle), s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.staging, (size_t)max * sizeof(prosper_pt_particle), s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.freelist, ((size_t)max + 1u) * sizeof(int32_t), s);
    if (rc == PROSPER_PT_OK) rc = grow_to(st.stats, sizeof(ParticleCallStats), s);
    if (rc != PROSPER_PT_OK) return rc;
    st.maxParticleCount = max;
    if (fresh)
    {
        launch_particles_fresh_pool(buffers_of(st), s);
        PPT_HIP(hipGetLastError());
    }
    return PROSPER_PT_OK;
}

} // namespace

extern "C" {

int prosper_pt_particles(
    prosper_pt_ctx *ctx, const prosper_pt_particles_pc *pc, uint32_t stages, const prosper_CameraUniforms *camera, uint32_t width,
    uint32_t height, float *nonLinearDepth, void *stream)
{
    // the arguments are checked before the context, so that every refusal happens without a GPU
    if (!pc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: null argument");
    if (stages & ~kAllStages) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: unknown stage bits");
    if (pc->reset > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: reset is 0 or 1");
    if (pc->maxParticleCount > kMaxPool) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: maxParticleCount above 2^26");
    const bool render = (stages & PROSPER_PT_PARTICLES_RENDER) != 0u;
    const bool init = (stages & PROSPER_PT_PARTICLES_INIT) != 0u && pc->reset != 0u;
    if (render)
    {
        if (!camera) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: render needs a camera");
        if (width == 0 || height == 0) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: empty extent");
        if (width > kMaxExtent || height > kMaxExtent)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: an extent above 32768 is not supported");
    }
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: null argument");
    uint32_t vertexCount = 0;
    bool initRecorded = false;
    if (init)
    {
        const int crc = check_scene(ctx, "prosper_pt_particles");
        if (crc != PROSPER_PT_OK) return crc;
        const GeometryState &geo = *ctx->geometry;
        if (pc->sourceDrawInstanceIndex >= geo.drawInstances.size())
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: sourceDrawInstanceIndex out of range");
        const uint32_t mesh = geo.drawInstances[pc->sourceDrawInstanceIndex].meshIndex;
        if (mesh >= geo.metadatas.size() || mesh >= geo.infos.size())
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: the source draw instance names no mesh");
        // Init.cpp:86-91: a mesh that has not been loaded yet records nothing
        initRecorded = geo.metadatas[mesh].bufferIndex != PROSPER_PT_ABSENT && geo.infos[mesh].indexCount != 0u;
        vertexCount = geo.infos[mesh].vertexCount;
    }
    const float *depth = nullptr; // (written through: the caller's device memory, or the last traced G-buffer's own)
    if (render)
    {
        if (!hdr_has_extent(ctx, width, height))
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: the HDR image has another extent");
        if (const int rc = resolve_depth(ctx, "prosper_pt_particles", nonLinearDepth, true, width, height, &depth)) return rc;
    }
    PPT_HIP(hipSetDevice(ctx->device));
    // the pass writes the depth: only device memory will do
    if (render && nonLinearDepth && !is_device_pointer(nonLinearDepth))
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_particles: nonLinearDepth must be device memory (the pass writes it)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    ParticlesPassState &st = *ctx->particlesPasses;
    st.valid = false;
    int rc = ensure_pool(st, pool_size(pc->maxParticleCount), true, s);
    if (rc != PROSPER_PT_OK) return rc;
    const size_t pixels = (size_t)width * height;
    if (render && (st.keyPixels < pixels || !st.keys.ptr))
    {
        st.keyPixels = 0;
        rc = grow_buffer(st.keys, GrowWait::Stream, s, pixels * 8u, pixels * 8u, 0);
        if (rc != PROSPER_PT_OK) return rc;
        st.keyPixels = pixels;
    }
    if ((rc = st.timing.create())) return rc;
    if (init && initRecorded && (rc = flush_scene_updates(ctx, s, s)) != PROSPER_PT_OK) return rc;

    const ParticleBuffers b = buffers_of(st);
    PPT_HIP(hipMemsetAsync(b.stats, 0, sizeof(ParticleCallStats), s));
    hipEvent_t *ev = st.timing.events;
    PPT_HIP(hipEventRecord(ev[0], s));
    if (stages & PROSPER_PT_PARTICLES_DECAY) launch_particles_decay(b, pc->reset, s);
    PPT_HIP(hipEventRecord(ev[1], s));
    if (init && initRecorded) launch_particles_init(ctx->scene, b, pc->sourceDrawInstanceIndex, vertexCount, s);
    PPT_HIP(hipEventRecord(ev[2], s));
    if (stages & PROSPER_PT_PARTICLES_SIMULATE) launch_particles_simulate(b, pc->deltaTimeS, pc->simulateFrameIndex, s);
    PPT_HIP(hipEventRecord(ev[3], s));
    if (render)
    {
        ParticleRenderParams r = {};
        // worldToClip = cameraToClip * worldToCamera (column-major), in double, rounded once: the traced G-buffer's
        for (int c = 0; c < 4; ++c)
            for (int row = 0; row < 4; ++row)
            {
                double v = 0.0;
                for (int k = 0; k < 4; ++k)
                    v += (double)(&camera->cameraToClip.col[k].x)[row] * (double)(&camera->worldToCamera.col[c].x)[k];
                r.worldToClip[c * 4 + row] = (float)v;
            }
        // scene/camera.glsl:32-44
        const prosper_mat4 &w2c = camera->worldToCamera;
        const f3 up = normalize(f3{w2c.col[0].y, w2c.col[1].y, w2c.col[2].y});
        const f3 right = normalize(f3{-w2c.col[0].x, -w2c.col[1].x, -w2c.col[2].x});
        r.up[0] = up.x, r.up[1] = up.y, r.up[2] = up.z;
        r.right[0] = right.x, r.right[1] = right.y, r.right[2] = right.z;
        r.width = width;
        r.height = height;
        r.frameIndex = pc->renderFrameIndex;
        r.hdr = ctx->hdr;
        r.nonLinearDepth = const_cast<float *>(depth);
        r.keys = st.keys.as<unsigned long long>();
        launch_particles_render(b, r, s);
    }
    PPT_HIP(hipMemcpyAsync(&b.stats->finalCount, b.freelist, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    PPT_HIP(hipEventRecord(ev[4], s));
    PPT_HIP(hipGetLastError());
    if (init && initRecorded && (rc = mark_versions_read(ctx, s)) != PROSPER_PT_OK) return rc;
    st.initRecorded = init && initRecorded;
    st.valid = true;
    return PROSPER_PT_OK;
}

int prosper_pt_get_particles_info(prosper_pt_ctx *ctx, prosper_pt_particles_info *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_particles_info: null argument");
    const ParticlesPassState &st = *ctx->particlesPasses;
    prosper_pt_particles_info info = {};
    info.maxParticleCount = st.maxParticleCount;
    if (st.valid)
    {
        PPT_HIP(hipSetDevice(ctx->device));
        float ms[kParticleStages] = {};
        if (const int rc = st.timing.elapsed(ms)) return rc;
        ParticleCallStats stats = {};
        PPT_HIP(hipMemcpy(&stats, st.stats.ptr, sizeof(stats), hipMemcpyDeviceToHost));
        info.valid = 1u;
        info.initRecorded = st.initRecorded ? 1u : 0u;
        info.freelistCount = stats.finalCount < 0 ? 0u : (uint32_t)stats.finalCount;
        info.liveCount = st.maxParticleCount - (info.freelistCount < st.maxParticleCount ? info.freelistCount : st.maxParticleCount);
        info.grantedSpawns = stats.grantedSpawns;
        info.refusedSpawns = stats.refusedSpawns;
        info.fragmentsWritten = stats.fragmentsWritten;
        info.decayMs = ms[0];
        info.initMs = ms[1];
        info.simulateMs = ms[2];
        info.renderMs = ms[3];
    }
    *out = info;
    return PROSPER_PT_OK;
}

int prosper_pt_read_particles(
    prosper_pt_ctx *ctx, prosper_pt_particle *particles, int32_t *freelist, uint32_t maxParticleCount, void *stream)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_particles: null argument");
    const ParticlesPassState &st = *ctx->particlesPasses;
    if (st.maxParticleCount == 0u) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_read_particles: there is no particle pool yet");
    if (pool_size(maxParticleCount) != st.maxParticleCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_particles: maxParticleCount differs from the pool's");
    const size_t n = st.maxParticleCount;
    return read_back(
        ctx, static_cast<hipStream_t>(stream),
        {{particles, st.particles.ptr, n * sizeof(prosper_pt_particle)}, {freelist, st.freelist.ptr, (n + 1u) * sizeof(int32_t)}});
}

int prosper_pt_set_particles(
    prosper_pt_ctx *ctx, const prosper_pt_particle *particles, const int32_t *freelist, uint32_t maxParticleCount, void *stream)
{
    if (!particles || !freelist) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_particles: null argument");
    if (maxParticleCount > kMaxPool) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_particles: maxParticleCount above 2^26");
    const uint32_t n = pool_size(maxParticleCount);
    // the kernels index the pool with what the freelist holds
    if (freelist[0] < 0 || (uint32_t)freelist[0] > n)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_particles: the freelist's count is outside [0, maxParticleCount]");
    for (uint32_t i = 0; i < n; ++i)
        if (freelist[1u + i] < 0 || (uint32_t)freelist[1u + i] >= n)
            return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_particles: a freelist index is outside the pool");
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_particles: null argument");
    PPT_HIP(hipSetDevice(ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    ParticlesPassState &st = *ctx->particlesPasses;
    const int rc = ensure_pool(st, n, false, s);
    if (rc != PROSPER_PT_OK) return rc;
    PPT_HIP(hipMemcpyAsync(st.particles.ptr, particles, (size_t)n * sizeof(prosper_pt_particle), hipMemcpyHostToDevice, s));
    PPT_HIP(hipMemcpyAsync(st.freelist.ptr, freelist, ((size_t)n + 1u) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // (the caller's arrays may go once this returns)
    PPT_HIP(hipStreamSynchronize(s));
    return PROSPER_PT_OK;
}

} // extern "C"
