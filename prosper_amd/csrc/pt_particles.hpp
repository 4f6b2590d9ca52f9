// pt_particles.hpp — host-callable launchers of the gfx950 kernels of prosper's particle system (pt_particles.hip;
// src/render/particles/, res/shader/particles/).  Their C entry points: pt_particles_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/prosper_pt/prosper_pt.h"
#include "pt_scene.hpp"

namespace ppt
{

constexpr uint32_t kParticleStages = 4;      // decay, init, simulate, render
constexpr uint32_t kParticleGroupSize = 256; // the reference's groupSize: simulate.comp seeds its rng with the local id
constexpr uint32_t kDefaultMaxParticleCount = 500000; // Particles.hpp sMaxParticleCount

// What a call counts on the device (zeroed at its start, read by prosper_pt_get_particles_info)
struct ParticleCallStats
{
    int32_t countBeforeSimulate; // the freelist count simulate's first pop saw (the atomic maximum of what the pops returned)
    uint32_t simulatePopped;     // 1: some wave of simulate popped
    uint32_t grantedSpawns;
    uint32_t refusedSpawns;
    uint32_t fragmentsWritten; // pixels the render's resolve wrote
    int32_t finalCount;        // the freelist count behind the call's last launch
    uint32_t reserved[2];
};

struct ParticleBuffers
{
    prosper_pt_particle *particles; // [max]
    int32_t *freelist;              // count, then indices[max]
    prosper_pt_particle *staging;   // [max]: a child of simulate waits at its ticket for place_children
    ParticleCallStats *stats;
    uint32_t maxParticleCount;
};

// what render reads of the camera, and the targets
struct ParticleRenderParams
{
    float worldToClip[16]; // cameraToClip * worldToCamera, column-major, as the traced G-buffer's depth uses it
    float up[3], right[3]; // normalize(cameraWorldUp()), normalize(cameraWorldRight())
    uint32_t width, height;
    uint32_t frameIndex;
    float4 *hdr;
    float *nonLinearDepth;
    unsigned long long *keys; // [width * height], zero between calls
};

// Particles::init's upload: every position_lifetime (-9999) x 4, the rest zero, count = max, indices[i] = i
void launch_particles_fresh_pool(const ParticleBuffers &b, hipStream_t stream);
void launch_particles_decay(const ParticleBuffers &b, uint32_t decayAll, hipStream_t stream);
// init.comp over the `vertexCount` vertices of draw instance `drawInstanceIndex`, then the one-thread clamp
void launch_particles_init(
    const DeviceScene &s, const ParticleBuffers &b, uint32_t drawInstanceIndex, uint32_t vertexCount, hipStream_t stream);
// simulate.comp, then the launch that moves the children from their tickets into their slots and clamps the count
void launch_particles_simulate(const ParticleBuffers &b, float deltaTimeS, uint32_t frameIndex, hipStream_t stream);
// splat and resolve
void launch_particles_render(const ParticleBuffers &b, const ParticleRenderParams &r, hipStream_t stream);

} // namespace ppt
