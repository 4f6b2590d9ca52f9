"""NumPy restatement of prosper's clustered lighting (not a test module), for tests/test_deferred_shading.py:

  clusters(world, cam, w, h)   res/shader/light_clustering.comp + scene/light_clusters.glsl: which point lights each
                               cluster lists, and how far each sphere test was from going the other way
  slices(cam, lin_depth)       clusterIndex's slice, with the library's rules past the far and before the near plane
  shade(world, cam, ...)       res/shader/deferred_shading.comp over given lists (or every light: the brute force)

Everything is float64.  The surface, sampleLight's point / spot evaluation and evalBRDFTimesNoL come from
tests/restir_resampling_reference.py.
"""
import numpy as np

import restir_resampling_reference as R

DIM, SLICES, MAX_POINTS, MAX_SPOTS = 32, 16, 128, 128
SLOT = MAX_POINTS + MAX_SPOTS


def mat(m):
    """A CameraUniforms mat4 as a float64 row-major matrix."""
    return np.frombuffer(bytes(m), np.float32).reshape(4, 4).T.astype(np.float64)


def dims(w, h):
    return (w + DIM - 1) // DIM, (h + DIM - 1) // DIM, SLICES + 1


def slice_start(cam, s):
    """sliceStart: near * (far / near)^(s / 16)."""
    near, far = float(cam.near_), float(cam.far_)
    return near * (far / near) ** (np.asarray(s, np.float64) / SLICES)


def frustum(cam, cx, cy, cz):
    """clusterFrustum: six planes (xyz, w) of cluster (cx, cy, cz), the side planes normalised."""
    c2c = mat(cam.cameraToClip)
    sx, sy = float(cam.resolution[0]) / (2 * DIM), float(cam.resolution[1]) / (2 * DIM)
    bx, by = sx - cx, sy - cy
    c1 = np.array([c2c[0, 0] * sx, 0.0, -bx, 0.0])
    c2 = np.array([0.0, c2c[1, 1] * sy, -by, 0.0])
    c4 = np.array([0.0, 0.0, -1.0, 0.0])
    planes = np.array([c4 - c1, c4 + c1, c4 - c2, c4 + c2,
                       [0.0, 0.0, -1.0, 0.0 if cz == 0 else slice_start(cam, cz)],
                       [0.0, 0.0, 1.0, -slice_start(cam, cz + 1)]])
    planes[:4] /= np.linalg.norm(planes[:4, :3], axis=1, keepdims=True)
    return planes


def signed_distances(planes, p):
    """signedDistance of points p [n, 3] to every plane: [n, 6]."""
    return p @ planes[:, :3].T - planes[:, 3]


def point_spheres(world, cam):
    """View-space centres [n, 3] and radii [n] of the point lights (worldToCamera * position)."""
    n = world.point_lights.count
    pos = np.array([[L.position.x, L.position.y, L.position.z, L.position.w]
                    for L in world.point_lights.lights[:n]], np.float64).reshape(n, 4)
    r = np.array([L.radianceAndRadius.w for L in world.point_lights.lights[:n]], np.float64)
    return (pos @ mat(cam.worldToCamera).T)[:, :3], r


def clusters(world, cam, w, h):
    """(visible bool [z, y, x, points], margin float64 [z, y, x, points]): a point light is listed where its sphere is
    on the inner side of all six planes (>= -r); margin = min over the planes of distance + r (>= 0 listed)."""
    nx, ny, nz = dims(w, h)
    centre, r = point_spheres(world, cam)
    margin = np.empty((nz, ny, nx, len(r)))
    for cz in range(nz):
        for cy in range(ny):
            for cx in range(nx):
                d = signed_distances(frustum(cam, cx, cy, cz), centre)
                margin[cz, cy, cx] = (d + r[:, None]).min(axis=1)
    return margin >= 0.0, margin


def slices(cam, lin_depth):
    """clusterIndex's slice of view-space z (float64): uint(16 * log(-z / near) / log(far / near)).  Returns (slice int
    [n], beyond bool [n], margin [n]): nearer than the near plane (or NaN) is slice 0, slice > 16 is `beyond` (no lights);
    margin is the distance of the real-valued slice to the nearest integer (how close the pick was to another)."""
    near, far = float(cam.near_), float(cam.far_)
    z = np.asarray(lin_depth, np.float64)
    with np.errstate(all="ignore"):
        f = SLICES * np.log(-z / near) / np.log(far / near)
    f = np.where(f >= 0.0, f, 0.0)  # also NaN
    beyond = f >= SLICES + 1
    margin = np.where(f > 0.0, np.abs(f - np.round(f)), np.inf)
    return np.where(beyond, 0, np.floor(f)).astype(np.int64), beyond, margin


def membership(got, n_point, n_spot):
    """A read-back clustering (Context.read_light_clusters) as (point bool [z, y, x, n_point], spot bool [.., n_spot])."""
    ptrs, idx = got["pointers"], got["indices"]
    pc, sc = ptrs[..., 1] >> 16, ptrs[..., 1] & 0xFFFF
    k = np.arange(SLOT)
    points = np.zeros(ptrs.shape[:3] + (n_point,), bool)
    spots = np.zeros(ptrs.shape[:3] + (n_spot,), bool)
    for c in np.ndindex(ptrs.shape[:3]):
        points[c][idx[c][k < pc[c]].astype(np.int64)] = True
        spots[c][idx[c][(k >= pc[c]) & (k < pc[c] + sc[c])].astype(np.int64)] = True
    return points, spots


def shade(world, cam, ar, nm, depth, draw_type=0, lists=None):
    """deferred_shading.comp in float64.  `lists` (point bool [z, y, x, points], spot bool [.., spots]) or None for the
    brute force (every light, every cluster).  Returns (rgb [h, w, 3], sum of the absolute terms [h, w], slice margin
    [h, w])."""
    h, w = depth.shape
    sf = R.Surfaces(cam, ar, nm, depth)
    if draw_type != 0:
        out = sf.pos if draw_type == 5 else sf.albedo
        return out.reshape(h, w, 3), np.abs(out).sum(-1).reshape(h, w), np.full((h, w), np.inf)
    L = R.Lights(world)
    n_point, n_spot = world.point_lights.count, world.spot_lights.count
    npx = h * w
    # evalDirectionalLight
    b, _ = R.brdf_times_nol(sf, np.broadcast_to(L.sun_l, (npx, 3)))
    color = L.rad[0] * b
    total = np.abs(color).sum(-1)
    s, beyond, margin = slices(cam, sf.lin_depth.astype(np.float64))
    tx, ty = sf.px.astype(np.int64) // DIM, sf.py.astype(np.int64) // DIM
    for kind, count, offset in ((1, n_point, 1), (2, n_spot, 1 + n_point)):
        part = np.zeros((npx, 3))
        for i in range(count):
            if lists is None:
                member = ~beyond & (kind == 1 or i < MAX_SPOTS)
            else:
                member = ~beyond & lists[kind - 1][s, ty, tx, i]
            if not member.any():
                continue
            c, _ = R.light_contribution(sf, L, np.full(npx, offset + i))
            c = np.where(member[:, None], c, 0.0)
            part += c
            total += np.abs(c).sum(-1)
        color = color + part
    return color.reshape(h, w, 3), total.reshape(h, w), margin.reshape(h, w)
