// host/camera.cpp — see camera.hpp.  Matrices are column-major float[16] like glm::mat4.
#include "camera.hpp"

#include <cmath>

#include "../../../include/prosper_pt/prosper_pt.h"
#include <cstring>

namespace scene
{

namespace
{

struct V3
{
    float x, y, z;
};
V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 norm3(V3 a)
{
    const float inv = 1.f / std::sqrt(dot3(a, a));
    return {a.x * inv, a.y * inv, a.z * inv};
}

V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 mul(float f, V3 a) { return {f * a.x, f * a.y, f * a.z}; }

// src/scene/Camera.cpp:39-45 getPlane: the plane through three points, (normal, -dot(normal, p0))
prosper_vec4 plane_through(V3 p0, V3 p1, V3 p2)
{
    const V3 normal = norm3(cross3(sub(p1, p0), sub(p2, p0)));
    return prosper_vec4{normal.x, normal.y, normal.z, -dot3(normal, p0)};
}

// Gauss-Jordan inverse of a column-major 4x4 (well conditioned for rigid/projective camera matrices)
void invert4(const float in[16], float out[16])
{
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
        {
            a[r][c] = in[c * 4 + r];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; ++col)
    {
        int pivot = col;
        for (int r = col + 1; r < 4; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[pivot][col])) pivot = r;
        if (pivot != col)
            for (int c = 0; c < 8; ++c)
            {
                const double t = a[col][c];
                a[col][c] = a[pivot][c];
                a[pivot][c] = t;
            }
        const double inv = 1.0 / a[col][col];
        for (int c = 0; c < 8; ++c) a[col][c] *= inv;
        for (int r = 0; r < 4; ++r)
        {
            if (r == col) continue;
            const double f = a[r][col];
            for (int c = 0; c < 8; ++c) a[r][c] -= f * a[col][c];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[c * 4 + r] = (float)a[r][4 + c];
}

void mul4(const float a[16], const float b[16], float out[16])
{
    float r[16];
    for (int c = 0; c < 4; ++c)
        for (int row = 0; row < 4; ++row)
        {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s += a[k * 4 + row] * b[c * 4 + k];
            r[c * 4 + row] = s;
        }
    std::memcpy(out, r, sizeof(r));
}

} // namespace

void Camera::lookAt(const CameraTransform &transform)
{
    m_transform = transform;
    updateWorldToCamera();
}

// src/scene/Camera.cpp:71-80
void Camera::endFrame()
{
    m_changedThisFrame = false;
    std::memcpy(m_previousCameraToClip, m_cameraToClip, 64);
    std::memcpy(m_previousWorldToCamera, m_worldToCamera, 64);
    m_havePrevious = true;
    m_previousJitter[0] = m_currentJitter[0];
    m_previousJitter[1] = m_currentJitter[1];
    m_jitterIndex = (m_jitterIndex + 1u) % 8u;
}

void Camera::setParameters(const CameraParameters &parameters)
{
    m_parameters = parameters;
    m_changedThisFrame = true;
}

void Camera::updateResolution(uint32_t width, uint32_t height)
{
    if (m_resolution[0] != width || m_resolution[1] != height) m_changedThisFrame = true;
    m_resolution[0] = width;
    m_resolution[1] = height;
}

// src/scene/Camera.cpp:366-395
void Camera::updateWorldToCamera()
{
    const V3 eye{m_transform.eye[0], m_transform.eye[1], m_transform.eye[2]};
    const V3 target{m_transform.target[0], m_transform.target[1], m_transform.target[2]};
    const V3 up{m_transform.up[0], m_transform.up[1], m_transform.up[2]};
    const V3 fwd = norm3(sub(target, eye));
    const V3 z{-fwd.x, -fwd.y, -fwd.z};
    const V3 right = norm3(cross3(up, z));
    const V3 newUp = norm3(cross3(z, right));
    const float w2c[16] = {right.x, newUp.x, z.x, 0.f, right.y, newUp.y, z.y, 0.f,
                           right.z, newUp.z, z.z, 0.f, -dot3(right, eye), -dot3(newUp, eye), -dot3(z, eye), 1.f};
    std::memcpy(m_worldToCamera, w2c, sizeof(w2c));
    invert4(m_worldToCamera, m_cameraToWorld);
    m_maxViewScale = 1.f; // rows of a rigid look-at matrix have unit length
    m_changedThisFrame = true;
}

// src/scene/Camera.cpp:105-153
void Camera::perspective()
{
    const float ar = (float)m_resolution[0] / (float)m_resolution[1];
    // reverse-z: near and far swapped
    const float zN = m_parameters.zF;
    const float zF = m_parameters.zN;
    const float tf = 1.f / std::tan(m_parameters.fov * 0.5f);
    m_currentJitter[0] = m_currentJitter[1] = 0.f;
    if (m_applyJitter) prosper_pt_taa_jitter(m_jitterIndex, m_resolution[0], m_resolution[1], m_currentJitter);
    // the jitter goes into column 2 ahead of the y-flip, with x negated: a shader unjitters with the value as it is
    const float jx = m_applyJitter ? -m_currentJitter[0] : 0.f, jy = m_applyJitter ? m_currentJitter[1] : 0.f;
    const float flip[16] = {1.f, 0.f, 0.f, 0.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 0.5f, 0.f, 0.f, 0.f, 0.5f, 1.f};
    const float proj[16] = {tf / ar, 0.f, 0.f, 0.f, 0.f, tf, 0.f, 0.f,
                            jx, jy, (zF + zN) / (zN - zF), -1.f, 0.f, 0.f, 2 * zF * zN / (zN - zF), 0.f};
    mul4(flip, proj, m_cameraToClip);
    float c2cw[16];
    mul4(m_cameraToClip, m_worldToCamera, c2cw);
    invert4(c2cw, m_clipToWorld);
    const float sensorHeight = sensorWidth() / ar;
    m_parameters.focalLength = sensorHeight * tf * 0.5f;
}

// src/scene/Camera.cpp:274-315 getFrustumCorners, then :397-415 updateFrustumPlanes: the six planes through the
// frustum's world-space corners, normals pointing into the frustum
void Camera::updateFrustumPlanes(prosper_CameraUniforms &u) const
{
    const float *m = m_worldToCamera; // rows 0, 1, 2 of the matrix: right, up, -forward
    const V3 right{m[0], m[4], m[8]}, up{m[1], m[5], m[9]}, fwd{-m[2], -m[6], -m[10]};
    const V3 eye{m_transform.eye[0], m_transform.eye[1], m_transform.eye[2]};
    const float ar = (float)m_resolution[0] / (float)m_resolution[1];
    const float halfYFar = m_parameters.zF * std::tan(m_parameters.fov * 0.5f);
    const float halfXFar = halfYFar * ar;
    const float halfYNear = m_parameters.zN * std::tan(m_parameters.fov * 0.5f);
    const float halfXNear = halfYNear * ar;
    // eye + z * fwd -+ halfX * right -+ halfY * up, summed in that order
    const auto corner = [&](float z, float sx, float halfX, float sy, float halfY)
    { return add(add(add(eye, mul(z, fwd)), mul(sx * halfX, right)), mul(sy * halfY, up)); };
    const float zN = m_parameters.zN, zF = m_parameters.zF;
    const V3 bottomLeftNear = corner(zN, -1.f, halfXNear, -1.f, halfYNear), bottomRightNear = corner(zN, 1.f, halfXNear, -1.f, halfYNear);
    const V3 topLeftNear = corner(zN, -1.f, halfXNear, 1.f, halfYNear), topRightNear = corner(zN, 1.f, halfXNear, 1.f, halfYNear);
    const V3 bottomLeftFar = corner(zF, -1.f, halfXFar, -1.f, halfYFar), bottomRightFar = corner(zF, 1.f, halfXFar, -1.f, halfYFar);
    const V3 topLeftFar = corner(zF, -1.f, halfXFar, 1.f, halfYFar), topRightFar = corner(zF, 1.f, halfXFar, 1.f, halfYFar);
    u.nearPlane = plane_through(bottomRightNear, bottomLeftNear, topRightNear);
    u.farPlane = plane_through(bottomRightFar, topRightFar, bottomLeftFar);
    u.leftPlane = plane_through(bottomLeftNear, bottomLeftFar, topLeftNear);
    u.rightPlane = plane_through(bottomRightNear, topRightNear, bottomRightFar);
    u.topPlane = plane_through(topLeftNear, topLeftFar, topRightNear);
    u.bottomPlane = plane_through(bottomLeftNear, bottomRightNear, bottomLeftFar);
}

// src/scene/Camera.cpp:162-204
const prosper_CameraUniforms &Camera::updateBuffer()
{
    perspective();
    prosper_CameraUniforms u = {};
    updateFrustumPlanes(u);
    std::memcpy(&u.worldToCamera, m_worldToCamera, 64);
    std::memcpy(&u.cameraToWorld, m_cameraToWorld, 64);
    std::memcpy(&u.cameraToClip, m_cameraToClip, 64);
    std::memcpy(&u.clipToWorld, m_clipToWorld, 64);
    std::memcpy(&u.previousWorldToCamera, m_havePrevious ? m_previousWorldToCamera : m_worldToCamera, 64);
    std::memcpy(&u.previousCameraToClip, m_havePrevious ? m_previousCameraToClip : m_cameraToClip, 64);
    u.eye = prosper_vec4{m_transform.eye[0], m_transform.eye[1], m_transform.eye[2], 1.f};
    u.resolution[0] = m_resolution[0];
    u.resolution[1] = m_resolution[1];
    u.currentJitter[0] = m_currentJitter[0];
    u.currentJitter[1] = m_currentJitter[1];
    u.previousJitter[0] = m_previousJitter[0];
    u.previousJitter[1] = m_previousJitter[1];
    u.near_ = m_parameters.zN;
    u.far_ = m_parameters.zF;
    u.maxViewScale = m_maxViewScale;
    m_uniforms = u;
    return m_uniforms;
}

} // namespace scene
