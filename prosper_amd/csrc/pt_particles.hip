// pt_particles.hip — gfx950 kernels of prosper's particle system (src/render/particles/*, res/shader/particles/*;
// DESIGN.md f13): a pool of Particle records that lives on the device across frames, and a freelist of its dead slots.
//
//   particles_fresh_pool_kernel     what Particles::init uploads: every slot dead, every index free
//   particles_decay_kernel          decay.comp: frees the Decay slots whose lifetime ran out (or, decayAll, every live one)
//   particles_init_kernel           init.comp: one emitter per vertex of the source draw instance's mesh
//   particles_clamp_kernel          one thread: the count a dry launch left negative back to 0
//   particles_simulate_kernel       simulate.comp; a child is written to the staging array at its ticket ...
//   particles_place_children_kernel ... and moved into its slot here, so no child is simulated in its birth step
//   particles_splat_kernel          render.vert + rasterisation + render.frag: a 64-bit atomic maximum per covered pixel
//   particles_resolve_kernel        colour and depth where a key was left; zeroes the key
//
// The freelist's counter moves once per wave: ballot, population count, the lane's rank (mbcnt).  Block size 256 =
// the reference's groupSize (simulate.comp seeds its rng with gl_LocalInvocationID.x).
#include "pt_particles.hpp"

#include "pt_device.hpp"

namespace ppt
{

constexpr uint32_t kMaskGravity = 1u << 0, kMaskDecay = 1u << 1, kMaskEmit = 1u << 2; // particle.h ParticleMaskBits_*
constexpr float kDead = -9999.0f;

// subgroupBallotExclusiveBitCount of the lane within `mask`
PPT_D int32_t lane_rank(unsigned long long mask)
{
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// One atomic for the wave's `want` lanes (call it where the wave's control flow is uniform): what the counter held
// before it moved by `sign` * their number, in every lane; *rank: the lane's place among them.  No lane wants: the
// counter is not touched.
PPT_D int32_t freelist_move(int32_t *count, bool want, int32_t sign, int32_t &rank, bool &leads)
{
    const unsigned long long mask = __ballot(want);
    rank = lane_rank(mask);
    leads = false;
    if (mask == 0ull) return 0;
    const int32_t n = (int32_t)__popcll(mask);
    const int32_t leader = (int32_t)__ffsll((long long)mask) - 1;
    leads = (int32_t)(threadIdx.x & 63u) == leader;
    int32_t old = 0;
    if (leads) old = atomicAdd(count, sign * n);
    return __shfl(old, leader);
}

// freelist.glsl freelistPushIndex; -1 for a lane that does not push
PPT_D int32_t freelist_push_index(int32_t *freelist, bool want)
{
    int32_t rank;
    bool leads;
    const int32_t old = freelist_move(freelist, want, 1, rank, leads);
    return want ? old + rank : -1;
}

// freelistPopIndex as DESIGN.md (f13) defines it: the lane of rank r gets ticket old - 1 - r, granted iff >= 0.  The
// launch that follows clamps the counter.  *old, *leads: for the caller's statistics.
PPT_D int32_t freelist_pop_index(int32_t *freelist, bool want, int32_t &old, bool &leads)
{
    int32_t rank;
    old = freelist_move(freelist, want, -1, rank, leads);
    return want ? old - 1 - rank : -1;
}

__global__ __launch_bounds__(256) void particles_fresh_pool_kernel(ParticleBuffers b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= b.maxParticleCount) return;
    float4 *rec = reinterpret_cast<float4 *>(b.particles + i);
    rec[0] = make_float4(kDead, kDead, kDead, kDead);
    rec[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rec[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    rec[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    b.freelist[1u + i] = (int32_t)i;
    if (i == 0u) b.freelist[0] = (int32_t)b.maxParticleCount;
}

__global__ __launch_bounds__(256) void particles_decay_kernel(ParticleBuffers b, uint32_t decayAll)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool shouldDecay = false;
    if (i < b.maxParticleCount)
    {
        const float lifetime = b.particles[i].position_lifetime.w;
        const uint32_t mask = b.particles[i].mask;
        shouldDecay = lifetime != kDead && (decayAll == 1u || ((mask & kMaskDecay) != 0u && lifetime <= 0.0f));
    }
    if (shouldDecay) b.particles[i].position_lifetime = prosper_vec4{kDead, kDead, kDead, kDead};
    const int32_t pushIndex = freelist_push_index(b.freelist, shouldDecay);
    // (past the end only after a double free, which a caller's own state can hold: never written)
    if (shouldDecay && pushIndex >= 0 && (uint32_t)pushIndex < b.maxParticleCount) b.freelist[1 + pushIndex] = (int32_t)i;
}

__global__ __launch_bounds__(256) void particles_init_kernel(DeviceScene s, ParticleBuffers b, uint32_t drawInstanceIndex, uint32_t vertexCount)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    const bool live = v < vertexCount;
    f3 position = {0.0f, 0.0f, 0.0f}, normal = {0.0f, 0.0f, 0.0f};
    if (live)
    {
        const prosper_DrawInstance instance = s.drawInstances[drawInstanceIndex];
        const prosper_GeometryMetadata m = s.geometryMetadatas[instance.meshIndex];
        // geometry.glsl:220-235 (the tangent and the uv are not read)
        const f3 pm = load_r16g16b16a16(s, m.bufferIndex, m.positionsOffset, v);
        const f3 nm = m.normalsOffset == PROSPER_PT_ABSENT ? f3{0.0f, 0.0f, 0.0f}
                                                           : unpack_snorm_r10g10b10(geo_u32(s, m.bufferIndex)[m.normalsOffset + v]);
        // instances.glsl:36-42
        const prosper_ModelInstanceTransforms &t = s.modelInstanceTransforms[instance.modelInstanceIndex];
        position = mul_point_mat3x4(pm, t.modelToWorld);
        normal = normalize(mul_vec_mat3(nm, t.normalToWorld));
    }
    int32_t old;
    bool leads;
    const int32_t popIndex = freelist_pop_index(b.freelist, live, old, leads);
    if (popIndex >= 0 && (uint32_t)popIndex < b.maxParticleCount)
    {
        const uint32_t slot = (uint32_t)b.freelist[1 + popIndex];
        if (slot < b.maxParticleCount)
        {
            // init.comp:51-57: four stores, the padding stays
            prosper_pt_particle &p = b.particles[slot];
            p.position_lifetime = prosper_vec4{position.x, position.y, position.z, 0.0f};
            p.normal_spawnRateS = prosper_vec4{normal.x, normal.y, normal.z, 0.1f};
            p.velocity_spawnTimerS = prosper_vec4{0.0f, 0.0f, 0.0f, 0.0f};
            p.mask = kMaskEmit;
        }
    }
}

__global__ void particles_clamp_kernel(ParticleBuffers b)
{
    if (blockIdx.x == 0u && threadIdx.x == 0u && b.freelist[0] < 0) b.freelist[0] = 0;
}

__global__ __launch_bounds__(256) void particles_simulate_kernel(ParticleBuffers b, float dt, uint32_t frameIndex)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool spawn = false;
    f3 childPosition = {0.0f, 0.0f, 0.0f}, childNormal = {0.0f, 0.0f, 0.0f}, childVelocity = {0.0f, 0.0f, 0.0f};
    if (i < b.maxParticleCount)
    {
        prosper_pt_particle &p = b.particles[i];
        Rng rng{i, threadIdx.x, frameIndex};
        const prosper_vec4 pl = p.position_lifetime;
        f3 position = {pl.x, pl.y, pl.z};
        float lifetime = pl.w;
        if (!(lifetime < 0.0f))
        {
            const prosper_vec4 vs = p.velocity_spawnTimerS;
            f3 velocity = {vs.x, vs.y, vs.z};
            float spawnTimerS = vs.w;
            position = position + velocity * dt;
            const uint32_t mask = p.mask;
            if (mask & kMaskGravity) velocity.y = velocity.y - (9.81f * 0.01f) * dt;
            if (mask & kMaskDecay) lifetime = lifetime - dt;
            if (mask & kMaskEmit)
            {
                const prosper_vec4 ns = p.normal_spawnRateS;
                f3 normal = {ns.x, ns.y, ns.z};
                const float spawnRateS = ns.w;
                rng.step();
                const f3 r = {Rng::to01(rng.x), Rng::to01(rng.y), Rng::to01(rng.z)};
                // (normal + rnd3d01() * 2. - 1.) * .5 * dt
                const f3 push = {(((normal.x + r.x * 2.0f) - 1.0f) * 0.5f) * dt, (((normal.y + r.y * 2.0f) - 1.0f) * 0.5f) * dt,
                                 (((normal.z + r.z * 2.0f) - 1.0f) * 0.5f) * dt};
                velocity = velocity + push;
                float scalarVelocity = length(velocity);
                velocity = velocity / scalarVelocity;
                scalarVelocity = fmin_(scalarVelocity, 0.05f);
                velocity = velocity * scalarVelocity;
                normal = normalize(velocity);
                p.normal_spawnRateS = prosper_vec4{normal.x, normal.y, normal.z, spawnRateS};
                spawnTimerS = spawnTimerS + dt;
                if (spawnTimerS >= spawnRateS)
                {
                    spawnTimerS = 0.0f;
                    spawn = true;
                    childPosition = position;
                    childNormal = normal;
                    childVelocity = (normal * scalarVelocity) * 2.0f;
                }
            }
            p.position_lifetime = prosper_vec4{position.x, position.y, position.z, lifetime};
            p.velocity_spawnTimerS = prosper_vec4{velocity.x, velocity.y, velocity.z, spawnTimerS};
        }
    }
    int32_t old;
    bool leads;
    const int32_t popIndex = freelist_pop_index(b.freelist, spawn, old, leads);
    if (leads)
    {
        // the first pop of the launch saw the count the launch began with; every later one saw less
        atomicMax(&b.stats->countBeforeSimulate, old);
        b.stats->simulatePopped = 1u;
    }
    if (popIndex >= 0 && (uint32_t)popIndex < b.maxParticleCount)
    {
        prosper_pt_particle &c = b.staging[popIndex];
        c.position_lifetime = prosper_vec4{childPosition.x, childPosition.y, childPosition.z, 4.0f};
        c.normal_spawnRateS = prosper_vec4{childNormal.x, childNormal.y, childNormal.z, 0.0f};
        c.velocity_spawnTimerS = prosper_vec4{childVelocity.x, childVelocity.y, childVelocity.z, 0.0f};
        c.mask = kMaskGravity | kMaskDecay;
    }
}

// staging[t] -> particles[indices[t]] for the tickets t in [max(count, 0), count before simulate); thread 0 clamps the
// count (an atomic, so that the other lanes read either value: both give the same range) and writes the statistics.
__global__ __launch_bounds__(256) void particles_place_children_kernel(ParticleBuffers b)
{
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    int32_t raw;
    if (gid == 0u)
        raw = atomicMax(b.freelist, 0);
    else
        raw = __atomic_load_n(b.freelist, __ATOMIC_RELAXED);
    if (b.stats->simulatePopped == 0u) return;
    const int32_t before = b.stats->countBeforeSimulate;
    const int32_t after = raw < 0 ? 0 : raw;
    if (gid == 0u)
    {
        b.stats->grantedSpawns = (uint32_t)(before - after);
        b.stats->refusedSpawns = raw < 0 ? (uint32_t)(-raw) : 0u;
    }
    const int64_t t = (int64_t)after + (int64_t)gid;
    if (t >= (int64_t)before || t >= (int64_t)b.maxParticleCount) return;
    const uint32_t slot = (uint32_t)b.freelist[1 + t];
    if (slot >= b.maxParticleCount) return;
    // simulate.comp's four stores, the padding stays
    const prosper_pt_particle &c = b.staging[t];
    prosper_pt_particle &p = b.particles[slot];
    p.position_lifetime = c.position_lifetime;
    p.normal_spawnRateS = c.normal_spawnRateS;
    p.velocity_spawnTimerS = c.velocity_spawnTimerS;
    p.mask = c.mask;
}

// ---- render ----

// common/dither.glsl sBayerMatrix, times 64
__device__ const uint8_t kBayer64[8][8] = {
    {0, 32, 8, 40, 2, 34, 10, 42},  {48, 16, 56, 24, 50, 18, 58, 26}, {12, 44, 4, 36, 14, 46, 6, 38},
    {60, 28, 52, 20, 62, 30, 54, 22}, {3, 35, 11, 43, 1, 33, 9, 41},    {51, 19, 59, 27, 49, 17, 57, 25},
    {15, 47, 7, 39, 13, 45, 5, 37},  {63, 31, 55, 23, 61, 29, 53, 21},
};

// row `row` of worldToClip * (p, 1), as gbuffer_trace_kernel computes the depth's z and w
PPT_D float clip_row(const float *m, uint32_t row, f3 p)
{
    return __builtin_fmaf(m[8 + row], p.z, __builtin_fmaf(m[4 + row], p.y, __builtin_fmaf(m[row], p.x, m[12 + row])));
}

__global__ __launch_bounds__(256) void particles_splat_kernel(ParticleBuffers b, ParticleRenderParams r)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= b.maxParticleCount) return;
    const prosper_vec4 pl = b.particles[i].position_lifetime;
    const float lifetime = pl.w;
    if (!(lifetime >= 0.0f)) return; // render.vert pushes a dead slot to infinity
    const f3 centre = {pl.x, pl.y, pl.z};
    const float w = clip_row(r.worldToClip, 3u, centre);
    if (!(w > 0.0f)) return;
    const float depth = clip_row(r.worldToClip, 2u, centre) / w;
    if (!(depth >= 0.0f && depth <= 1.0f)) return;

    const f3 up = {r.up[0], r.up[1], r.up[2]}, right = {r.right[0], r.right[1], r.right[2]};
    int32_t X[4], Y[4];
    for (uint32_t k = 0; k < 4u; ++k)
    {
        // render.vert: xOffset = (2 (k % 2) - 1) .001, yOffset = -(2 (k / 2) - 1) .001
        const float xOffset = (k & 1u) ? 0.001f : -0.001f;
        const float yOffset = (k & 2u) ? -0.001f : 0.001f;
        f3 p = centre + up * yOffset;
        p = p + right * xOffset;
        const float cw = clip_row(r.worldToClip, 3u, p);
        const float fx = ((clip_row(r.worldToClip, 0u, p) / cw) * 0.5f + 0.5f) * (float)r.width;
        const float fy = ((clip_row(r.worldToClip, 1u, p) / cw) * 0.5f + 0.5f) * (float)r.height;
        const float sx = __builtin_rintf(fx * 256.0f), sy = __builtin_rintf(fy * 256.0f);
        if (!(fabs_(sx) <= 8388608.0f && fabs_(sy) <= 8388608.0f)) return;
        X[k] = (int32_t)sx;
        Y[k] = (int32_t)sy;
    }
    int32_t minX = X[0], maxX = X[0], minY = Y[0], maxY = Y[0];
    for (uint32_t k = 1; k < 4u; ++k)
    {
        minX = X[k] < minX ? X[k] : minX;
        maxX = X[k] > maxX ? X[k] : maxX;
        minY = Y[k] < minY ? Y[k] : minY;
        maxY = Y[k] > maxY ? Y[k] : maxY;
    }
    // the pixels whose centres (256 p + 128) lie in the box
    int32_t px0 = (minX + 127) >> 8, px1 = (maxX - 128) >> 8, py0 = (minY + 127) >> 8, py1 = (maxY - 128) >> 8;
    px0 = px0 < 0 ? 0 : px0;
    py0 = py0 < 0 ? 0 : py0;
    px1 = px1 > (int32_t)r.width - 1 ? (int32_t)r.width - 1 : px1;
    py1 = py1 > (int32_t)r.height - 1 ? (int32_t)r.height - 1 : py1;
    if (px0 > px1 || py0 > py1) return;

    const bool emitter = (b.particles[i].mask & kMaskEmit) != 0u;
    const float alpha = emitter ? 1.0f : saturate(lifetime * 4.0f);
    const unsigned long long key = ((unsigned long long)f2u(depth) << 32) | (unsigned long long)(~i);
    const uint32_t shiftX = r.frameIndex % 8u, shiftY = r.frameIndex / 8u;

    for (uint32_t t = 0; t < 2u; ++t)
    {
        // the strip's triangles (0, 1, 2) and (2, 1, 3)
        const uint32_t ia = t ? 2u : 0u, ib = 1u, ic = t ? 3u : 2u;
        const int64_t ax = X[ia], ay = Y[ia], bx = X[ib], by = Y[ib], cx = X[ic], cy = Y[ic];
        // twice the area in framebuffer coordinates, y down; Vulkan's a = -1/2 of it, positive a is the front ((f12))
        const int64_t area2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
        if (area2 >= 0) continue;
        const int64_t ex[3] = {bx - ax, cx - bx, ax - cx}, ey[3] = {by - ay, cy - by, ay - cy};
        const int64_t ox[3] = {ax, bx, cx}, oy[3] = {ay, by, cy};
        for (int32_t py = py0; py <= py1; ++py)
            for (int32_t px = px0; px <= px1; ++px)
            {
                const int64_t sx = (int64_t)px * 256 + 128, sy = (int64_t)py * 256 + 128;
                bool inside = true;
                for (uint32_t e = 0; e < 3u; ++e)
                {
                    // positive inside a front-facing triangle; on the edge, the top-left rule
                    const int64_t f = ey[e] * (sx - ox[e]) - ex[e] * (sy - oy[e]);
                    const bool topLeft = ey[e] > 0 || (ey[e] == 0 && ex[e] < 0);
                    inside = inside && (f > 0 || (f == 0 && topLeft));
                }
                if (!inside) continue;
                // render.frag: ditherAlpha with the matrix cycled by the frame index
                const float threshold = (float)kBayer64[((uint32_t)py + shiftY) % 8u][((uint32_t)px + shiftX) % 8u] * (1.0f / 64.0f);
                if (alpha < threshold) continue;
                const size_t pixel = (size_t)py * r.width + (size_t)px;
                if (!(depth > r.nonLinearDepth[pixel])) continue; // reverse-Z eGreater against the stored depth
                atomicMax(r.keys + pixel, key);
            }
    }
}

__global__ __launch_bounds__(256) void particles_resolve_kernel(ParticleBuffers b, ParticleRenderParams r)
{
    const size_t pixel = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool wrote = false;
    if (pixel < (size_t)r.width * r.height)
    {
        const unsigned long long key = r.keys[pixel];
        if (key != 0ull)
        {
            const uint32_t slot = ~(uint32_t)key;
            const bool emitter = slot < b.maxParticleCount && (b.particles[slot].mask & kMaskEmit) != 0u;
            r.hdr[pixel] = emitter ? make_float4(1.0f, 1.0f, 0.0f, 1.0f) : make_float4(1.0f, 0.0f, 1.0f, 1.0f);
            r.nonLinearDepth[pixel] = u2f((uint32_t)(key >> 32));
            r.keys[pixel] = 0ull;
            wrote = true;
        }
    }
    const unsigned long long mask = __ballot(wrote);
    if (mask != 0ull && (int32_t)(threadIdx.x & 63u) == (int32_t)__ffsll((long long)mask) - 1)
        atomicAdd(&b.stats->fragmentsWritten, (uint32_t)__popcll(mask));
}

// ---- launchers ----

static dim3 slot_grid(uint32_t n) { return dim3((n + kParticleGroupSize - 1u) / kParticleGroupSize); }

void launch_particles_fresh_pool(const ParticleBuffers &b, hipStream_t stream)
{
    hipLaunchKernelGGL(particles_fresh_pool_kernel, slot_grid(b.maxParticleCount), dim3(256), 0, stream, b);
}

void launch_particles_decay(const ParticleBuffers &b, uint32_t decayAll, hipStream_t stream)
{
    hipLaunchKernelGGL(particles_decay_kernel, slot_grid(b.maxParticleCount), dim3(256), 0, stream, b, decayAll);
}

void launch_particles_init(
    const DeviceScene &s, const ParticleBuffers &b, uint32_t drawInstanceIndex, uint32_t vertexCount, hipStream_t stream)
{
    if (vertexCount == 0u) return;
    hipLaunchKernelGGL(particles_init_kernel, slot_grid(vertexCount), dim3(256), 0, stream, s, b, drawInstanceIndex, vertexCount);
    hipLaunchKernelGGL(particles_clamp_kernel, dim3(1), dim3(64), 0, stream, b);
}

void launch_particles_simulate(const ParticleBuffers &b, float deltaTimeS, uint32_t frameIndex, hipStream_t stream)
{
    hipLaunchKernelGGL(particles_simulate_kernel, slot_grid(b.maxParticleCount), dim3(256), 0, stream, b, deltaTimeS, frameIndex);
    hipLaunchKernelGGL(particles_place_children_kernel, slot_grid(b.maxParticleCount), dim3(256), 0, stream, b);
}

void launch_particles_render(const ParticleBuffers &b, const ParticleRenderParams &r, hipStream_t stream)
{
    if (r.width == 0u || r.height == 0u) return;
    hipLaunchKernelGGL(particles_splat_kernel, slot_grid(b.maxParticleCount), dim3(256), 0, stream, b, r);
    const size_t pixels = (size_t)r.width * r.height;
    hipLaunchKernelGGL(particles_resolve_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, stream, b, r);
}

} // namespace ppt
