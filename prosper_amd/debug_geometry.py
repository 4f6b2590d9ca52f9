"""Debug geometry of the host side: the line list prosper_pt_debug_lines draws, and what prosper's App fills it with.

DebugLines is scene::DebugLines (src/scene/DebugGeometry.hpp); light_axes and frustum_lines restate
App::updateDebugLines (src/App.cpp:1086-1156); focus_distance_from_depth restates the click-to-focus of
App.cpp:607-626 over one read-back depth texel."""
import numpy as np

F = np.float32

DEBUG_LINE_LENGTH = 0.2
DEBUG_RED = (1.0, 0.05, 0.05)
DEBUG_GREEN = (0.05, 1.0, 0.05)
DEBUG_BLUE = (0.05, 0.05, 1.0)

FRUSTUM_CORNER_NAMES = ("bottomLeftNear", "bottomRightNear", "topLeftNear", "topRightNear",
                        "bottomLeftFar", "bottomRightFar", "topLeftFar", "topRightFar")


class DebugLines:
    """scene::DebugLines: at most sMaxLineCount lines of two positions and a colour."""

    sMaxLineCount = 100000
    sLineFloats = 9

    def __init__(self):
        self._lines = []

    @property
    def count(self):
        return len(self._lines)

    def reset(self):
        self._lines = []

    def addLine(self, p0, p1, color):
        """The reference writes past its mapped buffer when it is full; here that is an error."""
        if len(self._lines) >= self.sMaxLineCount:
            raise OverflowError("DebugLines holds sMaxLineCount = %d lines" % self.sMaxLineCount)
        line = np.concatenate([np.asarray(p0, F).reshape(3), np.asarray(p1, F).reshape(3), np.asarray(color, F).reshape(3)])
        self._lines.append(line)

    add_line = addLine

    def extend(self, lines):
        for line in np.asarray(lines, F).reshape(-1, 9):
            self.addLine(line[0:3], line[3:6], line[6:9])

    def array(self):
        """[count, 9] float32, what Context.debug_lines takes"""
        if not self._lines:
            return np.zeros((0, 9), F)
        return np.stack(self._lines).astype(F)


def _normalize(v):
    return (v / np.sqrt(np.dot(v, v).astype(F))).astype(F)


def _xyz(v):
    if hasattr(v, "x"):
        return np.array([v.x, v.y, v.z], F)
    return np.asarray(v, F).reshape(-1)[:3].copy()


def light_axes(point_lights, spot_lights):
    """App::updateDebugLines' light axes -> [3 * (points + spots), 9] float32.

    `point_lights`: the positions (xyz[w]) or S.PointLight records; `spot_lights`: (position, direction) pairs or
    S.SpotLight records.  A point light gets the world axes, a spot light its right / up / forward, each 0.2 long in
    red / green / blue.  right = normalize(cross(fwd, (0, 0, -1))) when |1 - direction.y| < 0.1, otherwise
    normalize(cross(fwd, (0, 1, 0))); up = normalize(cross(right, fwd))."""
    length = F(DEBUG_LINE_LENGTH)
    red, green, blue = (np.array(c, F) for c in (DEBUG_RED, DEBUG_GREEN, DEBUG_BLUE))
    out = []
    for pl in point_lights:
        pos = _xyz(pl.position if hasattr(pl, "position") else pl)
        for axis, colour in ((0, red), (1, green), (2, blue)):
            offset = np.zeros(3, F)
            offset[axis] = length
            out.append(np.concatenate([pos, pos + offset, colour]))
    for sl in spot_lights:
        if hasattr(sl, "positionAndAngleOffset"):
            pos, fwd = _xyz(sl.positionAndAngleOffset), _xyz(sl.direction)
        else:
            pos, fwd = _xyz(sl[0]), _xyz(sl[1])
        ref = np.array([0.0, 0.0, -1.0], F) if abs(1.0 - float(fwd[1])) < 0.1 else np.array([0.0, 1.0, 0.0], F)
        right = _normalize(np.cross(fwd, ref).astype(F))
        up = _normalize(np.cross(right, fwd).astype(F))
        for direction, colour in ((right, red), (up, green), (fwd, blue)):
            out.append(np.concatenate([pos, pos + direction * length, colour]))
    if not out:
        return np.zeros((0, 9), F)
    return np.stack(out).astype(F)


def light_axes_from_buffers(points, spots):
    """light_axes over a S.PointLightsBuffer and a S.SpotLightsBuffer (what Context.read_lights returns)"""
    return light_axes([points.lights[i] for i in range(points.count)], [spots.lights[i] for i in range(spots.count)])


def frustum_lines(corners, colour):
    """App::updateDebugLines' frozen frustum -> [12, 9] float32: the near plane's four edges, the far plane's, then the
    four pyramid edges, in the reference's order.  `corners`: a mapping from scene::FrustumCorners' member names
    (FRUSTUM_CORNER_NAMES) to positions."""
    c = {name: _xyz(corners[name]) for name in FRUSTUM_CORNER_NAMES}
    pairs = [
        ("bottomLeftNear", "topLeftNear"), ("bottomLeftNear", "bottomRightNear"),
        ("topRightNear", "topLeftNear"), ("topRightNear", "bottomRightNear"),
        ("bottomLeftFar", "topLeftFar"), ("bottomLeftFar", "bottomRightFar"),
        ("topRightFar", "topLeftFar"), ("topRightFar", "bottomRightFar"),
        ("bottomLeftNear", "bottomLeftFar"), ("bottomRightNear", "bottomRightFar"),
        ("topLeftNear", "topLeftFar"), ("topRightNear", "topRightFar"),
    ]
    col = np.asarray(colour, F).reshape(3)
    return np.stack([np.concatenate([c[a], c[b], col]) for a, b in pairs]).astype(F)


def frustum_corners(camera):
    """The eight world-space corners of a S.CameraUniforms' frustum through clipToWorld (reverse Z: the near plane is
    depth 1, the far plane depth 0), as frustum_lines takes them."""
    m = mat4(camera.clipToWorld).astype(np.float64)
    out = {}
    for name in FRUSTUM_CORNER_NAMES:
        x = -1.0 if "Left" in name else 1.0
        y = 1.0 if name.startswith("bottom") else -1.0  # Vulkan clip space: y down
        z = 1.0 if name.endswith("Near") else 0.0
        p = m @ np.array([x, y, z, 1.0])
        out[name] = (p[:3] / p[3]).astype(F)
    return out


def mat4(m):
    """A S.Mat4 (column-major) -> [4, 4] float32 with m[row, col]"""
    return np.array([[getattr(m.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], F)


def focus_distance_from_depth(camera, px, extent, nonLinearDepth, dtype=np.float32):
    """App.cpp:607-626: the focus distance of the surface under pixel `px` (x, y; may be fractional) of an image of
    `extent` (width, height) whose depth texel read `nonLinearDepth`.

    `camera`: a S.CameraUniforms, or the [4, 4] cameraToClip matrix itself.  clipToCamera is the inverse of cameraToClip,
    taken in float64 and rounded to `dtype`; everything after it runs in `dtype` (float32 restates the reference's
    arithmetic, float64 is the yardstick of the tests)."""
    T = np.dtype(dtype).type
    c2c = mat4(camera.cameraToClip) if hasattr(camera, "cameraToClip") else np.asarray(camera)
    clip_to_camera = np.linalg.inv(np.asarray(c2c, np.float64)).astype(T)
    uv = (np.array([px[0], px[1]], T) + T(0.5)) / np.array([extent[0], extent[1]], T)
    clip_xy = uv * T(2.0) - T(1.0)
    v = np.array([clip_xy[0], clip_xy[1], T(nonLinearDepth), T(1.0)], T)
    projected = (clip_to_camera * v[None, :]).sum(axis=1, dtype=T)
    direction = projected[:3] / projected[3]
    depth = np.sqrt((direction * direction).sum(dtype=T))
    direction = direction / depth
    cos_theta = -direction[2]  # dot((0, 0, -1), dir)
    return T(depth * cos_theta)
