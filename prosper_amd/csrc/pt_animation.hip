// pt_animation.hip — glTF keyframe animation on the GPU (include/prosper_pt/prosper_pt.h "glTF keyframe animation";
// DESIGN.md (f15)): World::updateAnimations + World::updateScene of the reference (src/scene/Animations.hpp:71-125,
// Accessors.cpp:25-75, World.cpp:349-466) as two kernels that the scene update (pt_scene_updates.cpp flush_pending_update) runs
// ahead of the refit, the tables prosper_pt_set_animations makes for them, and the read-back that keeps the host mirrors of
// the transform table and the light buffers in step.  The arithmetic is glm's, one operation per rounding
// (-ffp-contract=off); DESIGN.md (f15) carries the formulas.
#include "../../include/prosper_pt/prosper_pt.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "pt_animation.hpp"
#include "pt_context.hpp"
#include "pt_pass_support.hpp"

using namespace ppt;

namespace ppt
{

namespace
{

constexpr uint32_t kNone = PROSPER_PT_ANIMATION_NONE;
constexpr uint32_t kTrsFloats = 10; // translation, rotation (x, y, z, w), scale
constexpr uint32_t kCameraFloats = 9; // eye, target, up
constexpr uint32_t kBlock = 64;

// one per (node, path) that some channel targets: the channel that wins it
struct AnimTarget
{
    uint32_t node, path, interpolation, timeOffset, keyCount, valueOffset;
    float startTimeS, endTimeS;
};
struct AnimNode
{
    uint32_t modelInstance, pointLight, spotLight, flags;
    uint32_t chainOffset, chainCount; // its ancestors from the root down, then the node itself
};

} // namespace

struct AnimationState
{
    bool have = false;
    uint32_t nodeCount = 0, targetCount = 0, animatedNodeCount = 0;
    float endTimeS = 0.0f;
    bool movesLights = false, hasCamera = false;
    std::vector<uint32_t> boundInstances;    // model instances a node binds
    std::vector<uint32_t> animatedInstances; // ... at or under a node some channel targets
    bool firstUpdate = true; // the first update rewrites every bound instance from the static pose
    DeviceBuffer nodes, targets, times, values, chain, trs, world, camera, previousTable;
    bool previousValid = false;
    bool pending = false;
    float pendingTimeS = 0.0f;
    uint32_t updates = 0;
    // the last update's table, light buffers and camera record on their way back (pinned; behind `readBack`)
    Pinned<prosper_ModelInstanceTransforms> hTable;
    Pinned<LightBlock> hLights;
    Pinned<float> hCamera;
    Fence readBack;
    uint32_t enqueuedCount = 0;   // what the flush under way has enqueued ...
    bool enqueuedLights = false;
    uint32_t readBackCount = 0;   // ... and what a committed flush left for the mirrors to take up
    bool readBackQueued = false, readBackLights = false;
    float cameraRecord[kCameraFloats] = {};
    bool cameraValid = false;
    StageEvents<2> timing; // around the two kernels of the last update
};

namespace
{

// ---------------------------------------------------------------------------------------------------------------------
// kernel A: one thread per target.  TimeAccessor::interpolation + Animation<T>::update
// ---------------------------------------------------------------------------------------------------------------------

struct KeyFrame
{
    float t, stepDuration;
    uint32_t firstFrame;
};

// Accessors.cpp:25-75.  The reference scans the key times from the front; the binary search returns the same frame: the
// last key at or before timeS (repeats included), at most keyCount - 2.
__device__ KeyFrame key_frame(const float *times, uint32_t keyCount, float startTimeS, float endTimeS, float timeS)
{
    KeyFrame k = {0.0f, 0.0f, 0u};
    if (timeS <= startTimeS || timeS < times[0]) return k;
    const uint32_t lastFrame = keyCount - 1u;
    k.firstFrame = lastFrame;
    if (timeS >= endTimeS || lastFrame == 0u) return k;
    uint32_t lo = 0u, hi = lastFrame; // the first frame in [0, lastFrame) whose time exceeds timeS, or lastFrame
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi) >> 1;
        if (times[mid] > timeS)
            hi = mid;
        else
            lo = mid + 1u;
    }
    k.firstFrame = lo - 1u; // (times[0] <= timeS: lo >= 1)
    const float firstTime = times[k.firstFrame];
    const float secondTime = times[k.firstFrame + 1u];
    const float duration = secondTime - firstTime;
    k.stepDuration = timeS - firstTime; // the time since the key, not the key interval: the reference's own
    k.t = k.stepDuration / duration;
    return k;
}

struct Value4
{
    float v[4];
};

__device__ Value4 read_value(const float *values, uint32_t width, uint32_t index)
{
    const float *p = values + (size_t)index * width;
    return Value4{{p[0], p[1], p[2], width == 4u ? p[3] : 0.0f}};
}

// glm::dot of two quaternions (x, y, z, w in v[0..3]): (w w + x x) + (y y + z z)
__device__ float quat_dot(const Value4 &a, const Value4 &b)
{
    return (a.v[3] * b.v[3] + a.v[0] * b.v[0]) + (a.v[1] * b.v[1] + a.v[2] * b.v[2]);
}

// glm::slerp
__device__ Value4 quat_slerp(const Value4 &x, const Value4 &y, float a)
{
    Value4 z = y;
    float cosTheta = quat_dot(x, y);
    if (cosTheta < 0.0f)
    {
        for (float &c : z.v) c = -c;
        cosTheta = -cosTheta;
    }
    Value4 r;
    if (cosTheta > 1.0f - FLT_EPSILON)
    {
        for (uint32_t c = 0; c < 4; ++c) r.v[c] = x.v[c] * (1.0f - a) + z.v[c] * a; // glm::mix
    }
    else
    {
        const float angle = acosf(cosTheta);
        const float s0 = sinf((1.0f - a) * angle), s1 = sinf(a * angle), s = sinf(angle);
        for (uint32_t c = 0; c < 4; ++c) r.v[c] = (s0 * x.v[c] + s1 * z.v[c]) / s;
    }
    return r;
}

__global__ __launch_bounds__(kBlock) void animation_sample_kernel(
    const AnimTarget *targets, uint32_t targetCount, const float *times, const float *values, float timeS, float *trs)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= targetCount) return;
    const AnimTarget g = targets[i];
    const bool quat = g.path == PROSPER_PT_ANIMATION_PATH_ROTATION;
    const uint32_t width = quat ? 4u : 3u;
    const float *v = values + g.valueOffset;
    const KeyFrame k = key_frame(times + g.timeOffset, g.keyCount, g.startTimeS, g.endTimeS, timeS);
    const bool cubic = g.interpolation == PROSPER_PT_ANIMATION_CUBICSPLINE;
    Value4 value;
    if (k.t == 0.0f || g.interpolation == PROSPER_PT_ANIMATION_STEP)
    {
        // (three values per key of a cubic spline, the property in the middle - which the reference reads only at t = 0)
        value = read_value(v, width, (k.t == 0.0f && cubic) ? k.firstFrame * 3u + 1u : k.firstFrame);
    }
    else if (g.interpolation == PROSPER_PT_ANIMATION_LINEAR)
    {
        const Value4 a = read_value(v, width, k.firstFrame), b = read_value(v, width, k.firstFrame + 1u);
        if (quat)
            value = quat_slerp(a, b, k.t);
        else
            for (uint32_t c = 0; c < 4; ++c) value.v[c] = (1.0f - k.t) * a.v[c] + k.t * b.v[c];
    }
    else
    {
        const uint32_t firstIndex = k.firstFrame * 3u;
        const Value4 vk = read_value(v, width, firstIndex + 1u), bk = read_value(v, width, firstIndex + 2u);
        const Value4 vk1 = read_value(v, width, firstIndex + 4u), ak1 = read_value(v, width, firstIndex + 3u);
        const float t = k.t, td = k.stepDuration;
        const float t3 = t * t * t, t2 = t * t, t2Times2 = 2.0f * t * t, t3Times2 = 2.0f * t * t * t, t2Times3 = 3.0f * t * t;
        const float c0 = t3Times2 - t2Times3 + 1.0f, c1 = td * (t3 - t2Times2 + t), c2 = -t3Times2 + t2Times3, c3 = td * (t3 - t2);
        for (uint32_t c = 0; c < 4; ++c) value.v[c] = c0 * vk.v[c] + c1 * bk.v[c] + c2 * vk1.v[c] + c3 * ak1.v[c];
        if (quat)
        {
            // glm::normalize
            const float len = __builtin_sqrtf(quat_dot(value, value)) /* (correctly rounded, like pt_math.hpp sqrt_) */;
            if (len <= 0.0f)
            {
                value = Value4{{0.0f, 0.0f, 0.0f, 1.0f}};
            }
            else
            {
                const float oneOverLen = 1.0f / len;
                for (float &c : value.v) c = c * oneOverLen;
            }
        }
    }
    float *out = trs + (size_t)g.node * kTrsFloats + (g.path == PROSPER_PT_ANIMATION_PATH_TRANSLATION ? 0u : (quat ? 3u : 7u));
    out[0] = value.v[0];
    out[1] = value.v[1];
    out[2] = value.v[2];
    if (quat) out[3] = value.v[3];
}

// ---------------------------------------------------------------------------------------------------------------------
// kernel B: one thread per node.  The node's world matrix from its chain of ancestors, and what the node carries
// ---------------------------------------------------------------------------------------------------------------------

struct Mat4
{
    float c[4][4]; // [column][row]
};

// glm::translate(m, v): m[3] = m[0] v.x + m[1] v.y + m[2] v.z + m[3]
__device__ void mat_translate(Mat4 &m, const float *v)
{
    for (uint32_t r = 0; r < 4; ++r) m.c[3][r] = m.c[0][r] * v[0] + m.c[1][r] * v[1] + m.c[2][r] * v[2] + m.c[3][r];
}

// m *= glm::mat4_cast(q), q = (x, y, z, w)
__device__ void mat_rotate(Mat4 &m, const float *q)
{
    const float qx = q[0], qy = q[1], qz = q[2], qw = q[3];
    const float qxx = qx * qx, qyy = qy * qy, qzz = qz * qz, qxz = qx * qz, qxy = qx * qy, qyz = qy * qz, qwx = qw * qx, qwy = qw * qy,
                qwz = qw * qz;
    Mat4 b;
    b.c[0][0] = 1.0f - 2.0f * (qyy + qzz);
    b.c[0][1] = 2.0f * (qxy + qwz);
    b.c[0][2] = 2.0f * (qxz - qwy);
    b.c[0][3] = 0.0f;
    b.c[1][0] = 2.0f * (qxy - qwz);
    b.c[1][1] = 1.0f - 2.0f * (qxx + qzz);
    b.c[1][2] = 2.0f * (qyz + qwx);
    b.c[1][3] = 0.0f;
    b.c[2][0] = 2.0f * (qxz + qwy);
    b.c[2][1] = 2.0f * (qyz - qwx);
    b.c[2][2] = 1.0f - 2.0f * (qxx + qyy);
    b.c[2][3] = 0.0f;
    b.c[3][0] = 0.0f;
    b.c[3][1] = 0.0f;
    b.c[3][2] = 0.0f;
    b.c[3][3] = 1.0f;
    // glm's mat4 * mat4: column j = a[0] b[j][0] + a[1] b[j][1] + a[2] b[j][2] + a[3] b[j][3]
    Mat4 a = m;
    for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t r = 0; r < 4; ++r)
            m.c[j][r] = a.c[0][r] * b.c[j][0] + a.c[1][r] * b.c[j][1] + a.c[2][r] * b.c[j][2] + a.c[3][r] * b.c[j][3];
}

// glm::scale(m, v)
__device__ void mat_scale(Mat4 &m, const float *v)
{
    for (uint32_t j = 0; j < 3; ++j)
        for (uint32_t r = 0; r < 4; ++r) m.c[j][r] = m.c[j][r] * v[j];
}

// glm::inverse of a mat4 (cofactors, one division)
__device__ Mat4 mat_inverse(const Mat4 &m)
{
    const float coef00 = m.c[2][2] * m.c[3][3] - m.c[3][2] * m.c[2][3];
    const float coef02 = m.c[1][2] * m.c[3][3] - m.c[3][2] * m.c[1][3];
    const float coef03 = m.c[1][2] * m.c[2][3] - m.c[2][2] * m.c[1][3];
    const float coef04 = m.c[2][1] * m.c[3][3] - m.c[3][1] * m.c[2][3];
    const float coef06 = m.c[1][1] * m.c[3][3] - m.c[3][1] * m.c[1][3];
    const float coef07 = m.c[1][1] * m.c[2][3] - m.c[2][1] * m.c[1][3];
    const float coef08 = m.c[2][1] * m.c[3][2] - m.c[3][1] * m.c[2][2];
    const float coef10 = m.c[1][1] * m.c[3][2] - m.c[3][1] * m.c[1][2];
    const float coef11 = m.c[1][1] * m.c[2][2] - m.c[2][1] * m.c[1][2];
    const float coef12 = m.c[2][0] * m.c[3][3] - m.c[3][0] * m.c[2][3];
    const float coef14 = m.c[1][0] * m.c[3][3] - m.c[3][0] * m.c[1][3];
    const float coef15 = m.c[1][0] * m.c[2][3] - m.c[2][0] * m.c[1][3];
    const float coef16 = m.c[2][0] * m.c[3][2] - m.c[3][0] * m.c[2][2];
    const float coef18 = m.c[1][0] * m.c[3][2] - m.c[3][0] * m.c[1][2];
    const float coef19 = m.c[1][0] * m.c[2][2] - m.c[2][0] * m.c[1][2];
    const float coef20 = m.c[2][0] * m.c[3][1] - m.c[3][0] * m.c[2][1];
    const float coef22 = m.c[1][0] * m.c[3][1] - m.c[3][0] * m.c[1][1];
    const float coef23 = m.c[1][0] * m.c[2][1] - m.c[2][0] * m.c[1][1];
    const float fac0[4] = {coef00, coef00, coef02, coef03}, fac1[4] = {coef04, coef04, coef06, coef07};
    const float fac2[4] = {coef08, coef08, coef10, coef11}, fac3[4] = {coef12, coef12, coef14, coef15};
    const float fac4[4] = {coef16, coef16, coef18, coef19}, fac5[4] = {coef20, coef20, coef22, coef23};
    const float vec0[4] = {m.c[1][0], m.c[0][0], m.c[0][0], m.c[0][0]}, vec1[4] = {m.c[1][1], m.c[0][1], m.c[0][1], m.c[0][1]};
    const float vec2[4] = {m.c[1][2], m.c[0][2], m.c[0][2], m.c[0][2]}, vec3[4] = {m.c[1][3], m.c[0][3], m.c[0][3], m.c[0][3]};
    const float signA[4] = {1.0f, -1.0f, 1.0f, -1.0f}, signB[4] = {-1.0f, 1.0f, -1.0f, 1.0f};
    Mat4 inv;
    for (uint32_t r = 0; r < 4; ++r)
    {
        inv.c[0][r] = (vec1[r] * fac0[r] - vec2[r] * fac1[r] + vec3[r] * fac2[r]) * signA[r];
        inv.c[1][r] = (vec0[r] * fac0[r] - vec2[r] * fac3[r] + vec3[r] * fac4[r]) * signB[r];
        inv.c[2][r] = (vec0[r] * fac1[r] - vec1[r] * fac3[r] + vec3[r] * fac5[r]) * signA[r];
        inv.c[3][r] = (vec0[r] * fac2[r] - vec1[r] * fac4[r] + vec2[r] * fac5[r]) * signB[r];
    }
    const float dot0[4] = {m.c[0][0] * inv.c[0][0], m.c[0][1] * inv.c[1][0], m.c[0][2] * inv.c[2][0], m.c[0][3] * inv.c[3][0]};
    const float dot1 = (dot0[0] + dot0[1]) + (dot0[2] + dot0[3]);
    const float oneOverDeterminant = 1.0f / dot1;
    for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t r = 0; r < 4; ++r) inv.c[j][r] = inv.c[j][r] * oneOverDeterminant;
    return inv;
}

// glm's mat4 * vec4: (m[0] v.x + m[1] v.y) + (m[2] v.z + m[3] v.w)
__device__ void mat_mul_vec4(const Mat4 &m, float x, float y, float z, float w, float *out)
{
    for (uint32_t r = 0; r < 4; ++r) out[r] = (m.c[0][r] * x + m.c[1][r] * y) + (m.c[2][r] * z + m.c[3][r] * w);
}

// glm's mat3(m) * vec3: m[0] v.x + m[1] v.y + m[2] v.z
__device__ void mat3_mul_vec3(const Mat4 &m, float x, float y, float z, float *out)
{
    for (uint32_t r = 0; r < 3; ++r) out[r] = m.c[0][r] * x + m.c[1][r] * y + m.c[2][r] * z;
}

__global__ __launch_bounds__(kBlock) void animation_hierarchy_kernel(
    const AnimNode *nodes, uint32_t nodeCount, const uint32_t *chain, const float *trs, float *world,
    prosper_ModelInstanceTransforms *table, uint32_t instanceCount, LightBlock *lights, float *camera)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= nodeCount) return;
    const AnimNode node = nodes[i];
    Mat4 m;
    for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t r = 0; r < 4; ++r) m.c[j][r] = j == r ? 1.0f : 0.0f;
    for (uint32_t k = 0; k < node.chainCount; ++k)
    {
        const uint32_t n = chain[node.chainOffset + k];
        const uint32_t flags = nodes[n].flags;
        const float *p = trs + (size_t)n * kTrsFloats;
        if (flags & PROSPER_PT_NODE_HAS_TRANSLATION) mat_translate(m, p);
        if (flags & PROSPER_PT_NODE_HAS_ROTATION) mat_rotate(m, p + 3);
        if (flags & PROSPER_PT_NODE_HAS_SCALE) mat_scale(m, p + 7);
    }
    for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t r = 0; r < 4; ++r) world[(size_t)i * 16u + j * 4u + r] = m.c[j][r];
    if (node.modelInstance < instanceCount)
    {
        // mat3x4(transpose(M)) and mat3x4(inverse(M)): the first three columns of either (World.cpp:405-407)
        const Mat4 inv = mat_inverse(m);
        prosper_ModelInstanceTransforms t;
        for (uint32_t j = 0; j < 3; ++j)
        {
            t.modelToWorld.col[j] = prosper_vec4{m.c[0][j], m.c[1][j], m.c[2][j], m.c[3][j]};
            t.normalToWorld.col[j] = prosper_vec4{inv.c[j][0], inv.c[j][1], inv.c[j][2], inv.c[j][3]};
        }
        table[node.modelInstance] = t;
    }
    const bool light = (node.flags & PROSPER_PT_NODE_DIRECTIONAL_LIGHT) || node.pointLight != kNone || node.spotLight != kNone;
    if (!light && !(node.flags & PROSPER_PT_NODE_CAMERA)) return;
    float position[4], direction[3];
    mat_mul_vec4(m, 0.0f, 0.0f, 0.0f, 1.0f, position);
    mat3_mul_vec3(m, 0.0f, 0.0f, -1.0f, direction);
    if (lights)
    {
        if (node.flags & PROSPER_PT_NODE_DIRECTIONAL_LIGHT)
            lights->directional.direction = prosper_vec4{direction[0], direction[1], direction[2], 0.0f};
        if (node.pointLight < PROSPER_MAX_POINT_LIGHT_COUNT)
            lights->points.lights[node.pointLight].position = prosper_vec4{position[0], position[1], position[2], position[3]};
        if (node.spotLight < PROSPER_MAX_SPOT_LIGHT_COUNT)
        {
            prosper_SpotLight &s = lights->spots.lights[node.spotLight];
            s.positionAndAngleOffset.x = position[0];
            s.positionAndAngleOffset.y = position[1];
            s.positionAndAngleOffset.z = position[2];
            s.direction = prosper_vec4{direction[0], direction[1], direction[2], 0.0f};
        }
    }
    if (node.flags & PROSPER_PT_NODE_CAMERA)
    {
        float target[4], up[3];
        mat_mul_vec4(m, 0.0f, 0.0f, -1.0f, 1.0f, target);
        mat3_mul_vec3(m, 0.0f, 1.0f, 0.0f, up);
        for (uint32_t r = 0; r < 3; ++r)
        {
            camera[r] = position[r];
            camera[3u + r] = target[r];
            camera[6u + r] = up[r];
        }
    }
}

int refuse(const std::string &why) { return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_animations: " + why); }

// (the device is idle: prosper_pt_set_animations has synchronised it)
int fill_buffer(DeviceBuffer &b, const void *src, size_t bytes)
{
    if (const int rc = grow_buffer(b, GrowWait::None, nullptr, bytes, bytes ? bytes : 16u)) return rc;
    if (bytes) PPT_HIP(hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
    return PROSPER_PT_OK;
}

void forget(AnimationState *an)
{
    an->have = false;
    an->pending = false;
    an->previousValid = false;
    an->readBackQueued = false;
    an->readBackLights = false;
    an->cameraValid = false;
    an->firstUpdate = true;
    an->updates = 0;
    an->nodeCount = an->targetCount = an->animatedNodeCount = 0;
    an->endTimeS = 0.0f;
    an->movesLights = an->hasCamera = false;
    an->boundInstances.clear();
    an->animatedInstances.clear();
}

} // namespace

bool create_animation_state(prosper_pt_ctx *ctx)
{
    ctx->animation = new (std::nothrow) AnimationState();
    return ctx->animation != nullptr;
}

void destroy_animation_state(prosper_pt_ctx *ctx)
{
    delete ctx->animation;
    ctx->animation = nullptr;
}

void forget_animations(prosper_pt_ctx *ctx)
{
    if (ctx->animation) forget(ctx->animation);
}

bool animation_pending(const prosper_pt_ctx *ctx) { return ctx->animation && ctx->animation->have && ctx->animation->pending; }

bool animation_moves_lights(const prosper_pt_ctx *ctx) { return ctx->animation && ctx->animation->movesLights; }

int enqueue_animation(prosper_pt_ctx *ctx, prosper_ModelInstanceTransforms *table, uint32_t count, LightBlock *lights, hipStream_t stream)
{
    AnimationState *an = ctx->animation;
    const size_t tableBytes = sizeof(prosper_ModelInstanceTransforms) * (size_t)count;
    int rc;
    if ((rc = grow_to(an->previousTable, tableBytes, stream))) return rc;
    // (a larger pinned buffer replaces one the previous read-back may still be writing)
    if (an->hTable.bytes < tableBytes)
    {
        if ((rc = an->readBack.host_wait())) return rc;
        if ((rc = an->hTable.allocate(tableBytes))) return rc;
    }
    if (!an->hLights.ptr && (rc = an->hLights.allocate(sizeof(LightBlock)))) return rc;
    if (!an->hCamera.ptr && (rc = an->hCamera.allocate(sizeof(float) * kCameraFloats))) return rc;
    if ((rc = an->timing.create())) return rc;
    if (count) PPT_HIP(hipMemcpyAsync(an->previousTable.ptr, ctx->dTransforms, tableBytes, hipMemcpyDeviceToDevice, stream));
    PPT_HIP(hipEventRecord(an->timing.events[0], stream));
    if (an->targetCount)
    {
        animation_sample_kernel<<<(an->targetCount + kBlock - 1u) / kBlock, kBlock, 0, stream>>>(
            an->targets.as<AnimTarget>(), an->targetCount, an->times.as<float>(), an->values.as<float>(), an->pendingTimeS,
            an->trs.as<float>());
        PPT_HIP(hipGetLastError());
    }
    PPT_HIP(hipEventRecord(an->timing.events[1], stream));
    animation_hierarchy_kernel<<<(an->nodeCount + kBlock - 1u) / kBlock, kBlock, 0, stream>>>(
        an->nodes.as<AnimNode>(), an->nodeCount, an->chain.as<uint32_t>(), an->trs.as<float>(), an->world.as<float>(), table, count,
        lights, an->camera.as<float>());
    PPT_HIP(hipGetLastError());
    PPT_HIP(hipEventRecord(an->timing.events[2], stream));
    if (count) PPT_HIP(hipMemcpyAsync(an->hTable.ptr, table, tableBytes, hipMemcpyDeviceToHost, stream));
    if (lights) PPT_HIP(hipMemcpyAsync(an->hLights.ptr, lights, sizeof(LightBlock), hipMemcpyDeviceToHost, stream));
    if (an->hasCamera)
        PPT_HIP(hipMemcpyAsync(an->hCamera.ptr, an->camera.ptr, sizeof(float) * kCameraFloats, hipMemcpyDeviceToHost, stream));
    if ((rc = an->readBack.record(stream))) return rc;
    an->enqueuedCount = count;
    an->enqueuedLights = lights != nullptr;
    return PROSPER_PT_OK;
}

// Every range whose model instance sits at or under an animated node counts as moved since the last build (the first
// update rewrites every bound instance from the static pose).  At the call and again at the flush: a geometry generation
// may have been switched in between.
static void mark_moved(prosper_pt_ctx *ctx)
{
    const AnimationState *an = ctx->animation;
    AccelState *acc = ctx->accel;
    std::vector<uint8_t> moved(acc->transforms.size(), 0);
    for (uint32_t mi : an->firstUpdate ? an->boundInstances : an->animatedInstances)
        if (mi < moved.size()) moved[mi] = 1;
    for (size_t r = 0; r < acc->ranges.size() && r < acc->movedSinceBuild.size(); ++r)
        if (acc->rangeModelInstance[r] < moved.size() && moved[acc->rangeModelInstance[r]]) acc->movedSinceBuild[r] = 1;
}

void animation_committed(prosper_pt_ctx *ctx)
{
    AnimationState *an = ctx->animation;
    mark_moved(ctx);
    an->pending = false;
    an->previousValid = true;
    an->firstUpdate = false;
    an->updates++;
    an->readBackQueued = true;
    an->readBackCount = an->enqueuedCount;
    an->readBackLights = an->readBackLights || an->enqueuedLights;
}

int sync_animation_mirrors(prosper_pt_ctx *ctx)
{
    AnimationState *an = ctx->animation;
    if (!an || !an->readBackQueued) return PROSPER_PT_OK;
    PPT_HIP(hipSetDevice(ctx->device));
    if (const int rc = an->readBack.host_wait()) return rc;
    an->readBackQueued = false;
    if (ctx->accel && ctx->accel->transforms.size() == an->readBackCount && an->readBackCount)
        std::memcpy(ctx->accel->transforms.data(), an->hTable.ptr, sizeof(prosper_ModelInstanceTransforms) * (size_t)an->readBackCount);
    if (an->readBackLights && ctx->lights && ctx->lights->mirror) *ctx->lights->mirror = *an->hLights.ptr;
    an->readBackLights = false;
    if (an->hasCamera)
    {
        std::memcpy(an->cameraRecord, an->hCamera.ptr, sizeof(an->cameraRecord));
        an->cameraValid = true;
    }
    return PROSPER_PT_OK;
}

// prosper_pt_animate up to the flush (pt_scene_updates.cpp): the time is staged and the instances it moves count as moved
int stage_animation(prosper_pt_ctx *ctx, float timeS)
{
    AnimationState *an = ctx->animation;
    if (!an || !an->have) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_animate called before prosper_pt_set_animations");
    mark_moved(ctx);
    an->pending = true;
    an->pendingTimeS = timeS;
    return PROSPER_PT_OK;
}

} // namespace ppt

extern "C" {

int prosper_pt_set_animations(prosper_pt_ctx *ctx, const prosper_pt_animation_desc *desc)
{
    if (!ctx || !desc) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_set_animations: null argument");
    if (desc->struct_size != sizeof(prosper_pt_animation_desc)) return refuse("struct_size mismatch");
    if (!ctx->haveScene || !ctx->accel || !ctx->animation) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_set_animations: no scene uploaded");
    if ((desc->nodeCount && !desc->nodes) || (desc->channelCount && !desc->channels) || (desc->timeCount && !desc->times) ||
        (desc->valueCount && !desc->values))
        return refuse("a table is null");
    if (desc->nodeCount == 0) return refuse("no nodes");
    if (desc->nodeCount >= kNone) return refuse("too many nodes");
    const uint32_t instanceCount = (uint32_t)ctx->accel->transforms.size();
    const uint32_t pointCount = ctx->scene.pointLightCount, spotCount = ctx->scene.spotLightCount;
    const uint32_t knownFlags = PROSPER_PT_NODE_HAS_TRANSLATION | PROSPER_PT_NODE_HAS_ROTATION | PROSPER_PT_NODE_HAS_SCALE |
                                PROSPER_PT_NODE_DIRECTIONAL_LIGHT | PROSPER_PT_NODE_CAMERA;

    // ---- nodes ----
    std::vector<prosper_pt_animation_node> nodes(desc->nodes, desc->nodes + desc->nodeCount);
    std::vector<uint8_t> instanceBound(instanceCount, 0), pointBound(pointCount, 0), spotBound(spotCount, 0);
    uint32_t cameras = 0, suns = 0;
    for (uint32_t i = 0; i < desc->nodeCount; ++i)
    {
        const prosper_pt_animation_node &n = nodes[i];
        const std::string name = "node " + std::to_string(i);
        if (n.parent != kNone && n.parent >= i) return refuse(name + ": its parent does not precede it");
        if (n.flags & ~knownFlags) return refuse(name + ": unknown flags");
        if (n.modelInstance != kNone)
        {
            if (n.modelInstance >= instanceCount) return refuse(name + ": modelInstance exceeds the scene's modelInstanceCount");
            if (instanceBound[n.modelInstance]++) return refuse(name + ": its model instance is bound by another node");
        }
        if (n.pointLight != kNone)
        {
            if (n.pointLight >= pointCount) return refuse(name + ": pointLight exceeds the scene's point light count");
            if (pointBound[n.pointLight]++) return refuse(name + ": its point light is bound by another node");
        }
        if (n.spotLight != kNone)
        {
            if (n.spotLight >= spotCount) return refuse(name + ": spotLight exceeds the scene's spot light count");
            if (spotBound[n.spotLight]++) return refuse(name + ": its spot light is bound by another node");
        }
        if ((n.flags & PROSPER_PT_NODE_CAMERA) && ++cameras > 1u) return refuse("more than one CAMERA node");
        if ((n.flags & PROSPER_PT_NODE_DIRECTIONAL_LIGHT) && ++suns > 1u) return refuse("the directional light is bound by two nodes");
    }

    // ---- channels: one writer per (node, path), the last channel that targets it ----
    std::vector<uint32_t> winner((size_t)desc->nodeCount * 3u, kNone);
    float endTimeS = 0.0f;
    for (uint32_t c = 0; c < desc->channelCount; ++c)
    {
        const prosper_pt_animation_channel &ch = desc->channels[c];
        const std::string name = "channel " + std::to_string(c);
        if (ch.node >= desc->nodeCount) return refuse(name + ": node out of range");
        if (ch.path > PROSPER_PT_ANIMATION_PATH_SCALE) return refuse(name + ": unknown path");
        if (ch.interpolation > PROSPER_PT_ANIMATION_CUBICSPLINE) return refuse(name + ": unknown interpolation");
        const uint32_t width = ch.path == PROSPER_PT_ANIMATION_PATH_ROTATION ? 4u : 3u;
        if (ch.valueWidth != width)
            return refuse(name + (width == 4u ? ": a rotation path takes values 4 floats wide" : ": a translation or scale path takes values 3 floats wide"));
        if (ch.keyCount == 0) return refuse(name + ": keyCount is 0");
        if (ch.timeOffset > desc->timeCount || ch.keyCount > desc->timeCount - ch.timeOffset) return refuse(name + ": its key times lie past times[]");
        const uint64_t floats = (uint64_t)ch.keyCount * width * (ch.interpolation == PROSPER_PT_ANIMATION_CUBICSPLINE ? 3u : 1u);
        if (ch.valueOffset > desc->valueCount || floats > (uint64_t)(desc->valueCount - ch.valueOffset))
            return refuse(name + ": its values lie past values[]");
        const float *t = desc->times + ch.timeOffset;
        for (uint32_t k = 0; k < ch.keyCount; ++k)
            if (!std::isfinite(t[k]) || (k && t[k] < t[k - 1u])) return refuse(name + ": its key times decrease (or are not finite)");
        if (!std::isfinite(ch.startTimeS) || !std::isfinite(ch.endTimeS)) return refuse(name + ": its interval is not finite");
        winner[(size_t)ch.node * 3u + ch.path] = c;
        endTimeS = std::max(endTimeS, ch.endTimeS);
    }
    std::vector<AnimTarget> targets;
    std::vector<uint8_t> dynamic(desc->nodeCount, 0);
    for (uint32_t i = 0; i < desc->nodeCount; ++i)
        for (uint32_t path = 0; path < 3u; ++path)
        {
            const uint32_t c = winner[(size_t)i * 3u + path];
            if (c == kNone) continue;
            const prosper_pt_animation_channel &ch = desc->channels[c];
            targets.push_back(AnimTarget{i, path, ch.interpolation, ch.timeOffset, ch.keyCount, ch.valueOffset, ch.startTimeS, ch.endTimeS});
            dynamic[i] = 1;
            // a targeted component exists; one that had been dropped starts at the identity (WorldData.cpp:1237-1272)
            prosper_pt_animation_node &n = nodes[i];
            const uint32_t flag = path == PROSPER_PT_ANIMATION_PATH_TRANSLATION ? PROSPER_PT_NODE_HAS_TRANSLATION
                                  : path == PROSPER_PT_ANIMATION_PATH_ROTATION  ? PROSPER_PT_NODE_HAS_ROTATION
                                                                                 : PROSPER_PT_NODE_HAS_SCALE;
            if (!(n.flags & flag))
            {
                n.flags |= flag;
                if (path == PROSPER_PT_ANIMATION_PATH_TRANSLATION) n.translation[0] = n.translation[1] = n.translation[2] = 0.0f;
                if (path == PROSPER_PT_ANIMATION_PATH_SCALE) n.scale[0] = n.scale[1] = n.scale[2] = 1.0f;
                if (path == PROSPER_PT_ANIMATION_PATH_ROTATION)
                {
                    n.rotation[0] = n.rotation[1] = n.rotation[2] = 0.0f;
                    n.rotation[3] = 1.0f;
                }
            }
        }

    // ---- what the kernels read: ancestor chains, the pose ----
    std::vector<AnimNode> devNodes(desc->nodeCount);
    std::vector<uint32_t> chain, depth(desc->nodeCount, 0);
    std::vector<float> trs((size_t)desc->nodeCount * kTrsFloats);
    AnimationState *an = ctx->animation;
    std::vector<uint32_t> bound, animated;
    uint32_t animatedNodes = 0;
    bool movesLights = false, hasCamera = false;
    for (uint32_t i = 0; i < desc->nodeCount; ++i)
    {
        const prosper_pt_animation_node &n = nodes[i];
        if (n.parent != kNone)
        {
            dynamic[i] = dynamic[i] | dynamic[n.parent]; // (WorldData.cpp:1279-1320)
            depth[i] = depth[n.parent] + 1u;
        }
        animatedNodes += dynamic[i];
        AnimNode &d = devNodes[i];
        d = AnimNode{n.modelInstance, n.pointLight, n.spotLight, n.flags, (uint32_t)chain.size(), depth[i] + 1u};
        chain.resize(chain.size() + d.chainCount);
        for (uint32_t k = d.chainCount, a = i; k-- > 0u; a = nodes[a].parent) chain[d.chainOffset + k] = a;
        float *p = trs.data() + (size_t)i * kTrsFloats;
        std::memcpy(p, n.translation, sizeof(float) * 3u);
        std::memcpy(p + 3, n.rotation, sizeof(float) * 4u);
        std::memcpy(p + 7, n.scale, sizeof(float) * 3u);
        if (n.modelInstance != kNone)
        {
            bound.push_back(n.modelInstance);
            if (dynamic[i]) animated.push_back(n.modelInstance);
        }
        movesLights = movesLights || (n.flags & PROSPER_PT_NODE_DIRECTIONAL_LIGHT) || n.pointLight != kNone || n.spotLight != kNone;
        hasCamera = hasCamera || (n.flags & PROSPER_PT_NODE_CAMERA);
    }
    if (chain.size() >= (size_t)kNone) return refuse("the node tree is too deep");

    // ---- upload (a flush of the previous tables may be in flight: the device is made idle) ----
    PPT_HIP(hipSetDevice(ctx->device));
    if (const int rc = sync_animation_mirrors(ctx)) return rc;
    PPT_HIP(hipDeviceSynchronize());
    forget(an);
    int rc;
    if ((rc = fill_buffer(an->nodes, devNodes.data(), devNodes.size() * sizeof(AnimNode)))) return rc;
    if ((rc = fill_buffer(an->targets, targets.data(), targets.size() * sizeof(AnimTarget)))) return rc;
    if ((rc = fill_buffer(an->times, desc->times, (size_t)desc->timeCount * sizeof(float)))) return rc;
    if ((rc = fill_buffer(an->values, desc->values, (size_t)desc->valueCount * sizeof(float)))) return rc;
    if ((rc = fill_buffer(an->chain, chain.data(), chain.size() * sizeof(uint32_t)))) return rc;
    if ((rc = fill_buffer(an->trs, trs.data(), trs.size() * sizeof(float)))) return rc;
    if ((rc = grow_buffer(an->world, GrowWait::None, nullptr, (size_t)desc->nodeCount * 16u * sizeof(float), (size_t)desc->nodeCount * 16u * sizeof(float), 0))) return rc;
    if ((rc = grow_buffer(an->camera, GrowWait::None, nullptr, sizeof(float) * kCameraFloats, 64, 0))) return rc;
    an->nodeCount = desc->nodeCount;
    an->targetCount = (uint32_t)targets.size();
    an->animatedNodeCount = animatedNodes;
    an->endTimeS = endTimeS;
    an->movesLights = movesLights;
    an->hasCamera = hasCamera;
    an->boundInstances.swap(bound);
    an->animatedInstances.swap(animated);
    an->have = true;
    return PROSPER_PT_OK;
}

int prosper_pt_get_animation_state(prosper_pt_ctx *ctx, prosper_pt_animation_state *out)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_get_animation_state: null argument");
    *out = prosper_pt_animation_state{};
    const AnimationState *an = ctx->animation;
    if (!an || !an->have) return PROSPER_PT_OK;
    int rc;
    if ((rc = check_scene(ctx, "prosper_pt_get_animation_state"))) return rc;
    if ((rc = flush_scene_updates(ctx, nullptr, nullptr))) return rc;
    if ((rc = sync_animation_mirrors(ctx))) return rc;
    out->endTimeS = an->endTimeS;
    out->nodeCount = an->nodeCount;
    out->animatedNodeCount = an->animatedNodeCount;
    out->updates = an->updates;
    out->cameraValid = an->cameraValid ? 1u : 0u;
    out->lightUpdates = ctx->lights ? ctx->lights->updates : 0u;
    if (an->updates && an->timing.created())
    {
        float ms[2] = {};
        if ((rc = an->timing.elapsed(ms))) return rc;
        out->sampleMs = ms[0];
        out->hierarchyMs = ms[1];
    }
    std::memcpy(out->eye, an->cameraRecord, sizeof(float) * 3u);
    std::memcpy(out->target, an->cameraRecord + 3, sizeof(float) * 3u);
    std::memcpy(out->up, an->cameraRecord + 6, sizeof(float) * 3u);
    return PROSPER_PT_OK;
}

int prosper_pt_read_animated_transforms(prosper_pt_ctx *ctx, uint32_t which, prosper_ModelInstanceTransforms *out, uint32_t count)
{
    if (!ctx || !out) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_animated_transforms: null argument");
    if (which > 1u) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_animated_transforms: which is 0 (current) or 1 (previous)");
    if (!ctx->haveScene || !ctx->accel) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    if (count != ctx->accel->transforms.size())
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_animated_transforms: count differs from the scene's modelInstanceCount");
    if (const int rc = check_scene(ctx, "prosper_pt_read_animated_transforms")) return rc;
    if (const int rc = flush_scene_updates(ctx, nullptr, nullptr)) return rc;
    PPT_HIP(hipDeviceSynchronize());
    const AnimationState *an = ctx->animation;
    const void *src = (which == 1u && an && an->previousValid) ? an->previousTable.ptr : ctx->dTransforms;
    if (count) PPT_HIP(hipMemcpy(out, src, sizeof(prosper_ModelInstanceTransforms) * (size_t)count, hipMemcpyDeviceToHost));
    return PROSPER_PT_OK;
}

int prosper_pt_read_lights(
    prosper_pt_ctx *ctx, prosper_DirectionalLightParameters *directionalLight, prosper_PointLightsBuffer *pointLights,
    prosper_SpotLightsBuffer *spotLights)
{
    if (!ctx || !directionalLight || !pointLights || !spotLights)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_read_lights: null argument");
    if (!ctx->haveScene || !ctx->lights) return fail(PROSPER_PT_ERR_NO_SCENE, "no scene uploaded");
    if (const int rc = check_scene(ctx, "prosper_pt_read_lights")) return rc;
    if (const int rc = flush_scene_updates(ctx, nullptr, nullptr)) return rc;
    PPT_HIP(hipDeviceSynchronize());
    const LightBlock *block = ctx->lights->dBlocks[ctx->lights->versions.cur];
    PPT_HIP(hipMemcpy(directionalLight, &block->directional, sizeof(*directionalLight), hipMemcpyDeviceToHost));
    PPT_HIP(hipMemcpy(pointLights, &block->points, sizeof(*pointLights), hipMemcpyDeviceToHost));
    PPT_HIP(hipMemcpy(spotLights, &block->spots, sizeof(*spotLights), hipMemcpyDeviceToHost));
    return PROSPER_PT_OK;
}

int prosper_pt_debug_read_animation_nodes(prosper_pt_ctx *ctx, float *trs, float *world, uint32_t nodeCount)
{
    if (!ctx) return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_animation_nodes: null argument");
    const AnimationState *an = ctx->animation;
    if (!ctx->haveScene || !an || !an->have) return fail(PROSPER_PT_ERR_NO_SCENE, "prosper_pt_debug_read_animation_nodes: no animations set");
    if (nodeCount != an->nodeCount)
        return fail(PROSPER_PT_ERR_INVALID_ARGUMENT, "prosper_pt_debug_read_animation_nodes: nodeCount differs from the animations' own");
    if (const int rc = check_scene(ctx, "prosper_pt_debug_read_animation_nodes")) return rc;
    if (const int rc = flush_scene_updates(ctx, nullptr, nullptr)) return rc;
    PPT_HIP(hipDeviceSynchronize());
    if (trs) PPT_HIP(hipMemcpy(trs, an->trs.ptr, sizeof(float) * kTrsFloats * (size_t)nodeCount, hipMemcpyDeviceToHost));
    if (world) PPT_HIP(hipMemcpy(world, an->world.ptr, sizeof(float) * 16u * (size_t)nodeCount, hipMemcpyDeviceToHost));
    return PROSPER_PT_OK;
}

} // extern "C"
