"""NumPy restatement of prosper's visibility system as this library builds it (a helper, like the other
*_reference.py files).

The depth pyramid of HierarchicalDepthDownsampler::record: its extents, its definition (every texel the minimum of its
clamped source footprint) and, to check that definition, the literal level-by-level 2 x 2 reduction that
hiz_downsampler.comp runs over ext/ffx_spd.h.  min rounds nothing, so both are exact.

The per-instance uniform scales (World.cpp:485-498), the draw-list generator as a set, the culler of
draw_list_culler.comp - one float32 operation per rounding, in the order pt_culling.hip fixes - its two
lists, and DrawStats."""
import numpy as np

from particles_reference import dot3, fma, normalize3

F = np.float32
HIZ_MAX_LEVELS = 12  # HierarchicalDepthDownsampler.cpp sMaxMips


def bit_ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def hiz_extents(width, height):
    """[(w, h)] of every level: level 0 is bit_ceil(extent) / 2, level l max(level 0 >> l, 1),
    floor(log2(larger side of level 0)) + 1 levels"""
    assert width > 1 and height > 1
    w0, h0 = bit_ceil(width) // 2, bit_ceil(height) // 2
    count = max(w0, h0).bit_length()
    assert count <= HIZ_MAX_LEVELS
    return [(max(w0 >> l, 1), max(h0 >> l, 1)) for l in range(count)]


def hiz_pyramid(depth):
    """The definition.  Level l, texel (x, y) = min of depth[min(Y, h - 1)][min(X, w - 1)] over
    x * 2^(l+1) <= X < (x + 1) * 2^(l+1) and likewise Y.  -> [float32 [hl, wl]]"""
    depth = np.ascontiguousarray(depth, F)
    h, w = depth.shape
    levels = []
    for l, (wl, hl) in enumerate(hiz_extents(w, h)):
        side = 2 << l
        ys = np.minimum(np.arange(hl * side), h - 1)
        xs = np.minimum(np.arange(wl * side), w - 1)
        levels.append(depth[np.ix_(ys, xs)].reshape(hl, side, wl, side).min(axis=(1, 3)))
    return levels


def hiz_pyramid_literal(depth):
    """What the shader does: level 0 from 2 x 2 source texels fetched with their coordinates clamped to
    inputResolution - 1 (SpdLoadSourceImage), every further level from 2 x 2 texels of the one before.  Inside a tile SPD
    keeps the texels that SpdStore skipped (those past a level whose side has reached 1) in registers and LDS; they are
    minima over clamped coordinates, i.e. over edge texels the stored neighbour covers as well, so reading the stored
    neighbour instead - the clamp below, which is also SpdLoad's clamp at level 5 - gives the same minimum."""
    depth = np.ascontiguousarray(depth, F)
    h, w = depth.shape
    levels = []
    src = depth
    for wl, hl in hiz_extents(w, h):
        sh, sw = src.shape
        out = np.empty((hl, wl), F)
        for y in range(hl):
            for x in range(wl):
                y0, y1 = min(2 * y, sh - 1), min(2 * y + 1, sh - 1)
                x0, x1 = min(2 * x, sw - 1), min(2 * x + 1, sw - 1)
                out[y, x] = min(min(src[y0, x0], src[y0, x1]), min(src[y1, x0], src[y1, x1]))
        levels.append(out)
        src = out
    return levels


def designed_depth(width, height, seed):
    """A depth for the pyramid's tests: random in [0.25, 1), and below all of it a minimum of its own, every one a
    different value in (0, 0.25), planted at the four corners of every 64 x 64 tile (clipped to the image), along the
    last column and the last row - the texels the clamp repeats - and at a few random places."""
    rng = np.random.default_rng(seed)
    d = (F(0.25) + F(0.75) * rng.random((height, width), dtype=F)).astype(F)
    places = set()
    for ty in range(0, height, 64):
        for tx in range(0, width, 64):
            for y in (ty, min(ty + 63, height - 1)):
                for x in (tx, min(tx + 63, width - 1)):
                    places.add((y, x))
    for y in range(0, height, 7):
        places.add((y, width - 1))
    for x in range(0, width, 5):
        places.add((height - 1, x))
    for _ in range(16):
        places.add((int(rng.integers(height)), int(rng.integers(width))))
    places = sorted(places)
    values = (F(0.25) * (np.arange(1, len(places) + 1, dtype=F) / F(len(places) + 1))).astype(F)
    rng.shuffle(values)
    for (y, x), v in zip(places, values):
        d[y, x] = v
    assert len(np.unique(values)) == len(values) and values.min() > 0 and values.max() < F(0.25)
    return d


# ---- the uniform scales, the generator, the culler, DrawStats ----

ALPHA_MODE_BLEND = 2
MODE_OPAQUE, MODE_TRANSPARENT = 0, 1


def instance_scales(model_to_world):
    """World.cpp:485-498.  `model_to_world` float32 [n, 3, 4]: the three vec4 columns of every mat3x4 -> float32 [n]"""
    m = np.ascontiguousarray(model_to_world, F).reshape(-1, 3, 4)
    with np.errstate(all="ignore"):
        # lengths of rows instead of columns because of the transposed 3x4: row r = (col0[r], col1[r], col2[r])
        sx, sy, sz = (np.sqrt(dot3(m[:, :, r], m[:, :, r])) for r in range(3))

        def relative_eq(a, b):
            return np.abs(a - b) < F(0.0001) * np.fmax(np.abs(a), np.abs(b))
        return np.where(relative_eq(sx, sy) & relative_eq(sx, sz), sx, F(0.0)).astype(F)


def transforms_of(world):
    """float32 [n, 3, 4] of a World's frozen ModelInstanceTransforms.modelToWorld"""
    t = world.freeze()["transforms"]
    n = len(world.model_instances)
    return np.array([[[getattr(t[i].modelToWorld.col[c], k) for k in "xyzw"] for c in range(3)] for i in range(n)], F).reshape(n, 3, 4)


def draw_instances_of(world):
    f = world.freeze()
    return [(d.modelInstanceIndex, d.meshIndex, d.materialIndex) for d in f["draw_instances"][:f["draw_instance_count"]]]


def _drawn(world, material_index, mode):
    blend = world.materials[material_index].alphaMode == ALPHA_MODE_BLEND
    return blend == (mode == MODE_TRANSPARENT)


def generate(world, mode):
    """draw_list_generator.comp as a set -> uint32 [n, 2] of (drawInstanceIndex, meshletIndex), sorted"""
    out = []
    for di, (mi, mesh, mat) in enumerate(draw_instances_of(world)):
        count = world.mesh_infos[mesh].meshletCount
        if count and _drawn(world, mat, mode):
            out += [(di, m) for m in range(count)]
    return np.array(sorted(out), np.uint32).reshape(-1, 2)


def totals(world, mode):
    """recordGenerateList's host loop -> dict of DrawStats' four totals and the list's upper bound"""
    t = dict(totalMeshCount=0, totalTriangleCount=0, totalMeshletCount=0, totalModelCount=0)
    models = set()
    for mi, mesh, mat in draw_instances_of(world):
        info = world.mesh_infos[mesh]
        if info.indexCount > 0 and _drawn(world, mat, mode):
            t["totalMeshCount"] += 1
            t["totalTriangleCount"] += info.indexCount // 3
            t["totalMeshletCount"] += info.meshletCount
            models.add(mi)
    t["totalModelCount"] = len(models)
    return t


def mat4_of(m):
    """S.Mat4 (column-major) -> float32 [4, 4] indexed [row, col]"""
    return np.array([[getattr(m.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], F)


def mat4_mul(a, b):
    """pt_culling.hip mat4_mul: [r, j] = fma(a[r,3], b[3,j], fma(a[r,2], b[2,j], fma(a[r,1], b[1,j], a[r,0] * b[0,j])))"""
    out = np.empty((4, 4), F)
    for r in range(4):
        for j in range(4):
            out[r, j] = fma(a[r, 3], b[3, j], fma(a[r, 2], b[2, j], fma(a[r, 1], b[1, j], a[r, 0] * b[0, j])))
    return out


def _row_point(m, r, p):
    return fma(m[r, 2], p[:, 2], fma(m[r, 1], p[:, 1], fma(m[r, 0], p[:, 0], m[r, 3])))


def _row_vec4(m, r, v):
    return fma(m[r, 3], v[3], fma(m[r, 2], v[2], fma(m[r, 1], v[1], m[r, 0] * v[0])))


def _f2i(x):
    """pt_math.hpp f2i: saturating, NaN -> 0"""
    x64 = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x64), 0, np.clip(x64, -2147483648.0, 2147483647.0)).astype(np.int64)


def _texel(level, x, y):
    """nearestBorderBlackFloatSampler: 0 outside the level"""
    h, w = level.shape
    ok = (x >= 0) & (y >= 0) & (x < w) & (y < h)
    return np.where(ok, level[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], F(0.0)).astype(F)


class View:
    """what the culler reads of a S.CameraUniforms"""

    def __init__(self, camera):
        v4 = lambda p: np.array([p.x, p.y, p.z, p.w], F)
        self.planes = [v4(getattr(camera, n)) for n in ("nearPlane", "farPlane", "leftPlane", "rightPlane", "bottomPlane", "topPlane")]
        self.eye = v4(camera.eye)[:3]
        self.world_to_camera, self.camera_to_clip = mat4_of(camera.worldToCamera), mat4_of(camera.cameraToClip)
        self.clip_from_world = mat4_mul(self.camera_to_clip, self.world_to_camera)
        self.near, self.max_view_scale = F(camera.near_), F(camera.maxViewScale)
        self.resolution = (int(camera.resolution[0]), int(camera.resolution[1]))


def meshlet_words(world, pairs):
    """-> (bounds words uint32 [n, 5], triangleCount uint32 [n], modelInstanceIndex [n]) of list entries"""
    f = world.freeze()
    di = draw_instances_of(world)
    bounds, tris, inst = np.empty((len(pairs), 5), np.uint32), np.empty(len(pairs), np.uint32), np.empty(len(pairs), np.int64)
    for k, (d, m) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        mi, mesh, _ = di[d]
        md = world.metadatas[mesh]
        words = f["geometry_buffers"][md.bufferIndex]
        bounds[k] = words[md.meshletBoundsOffset + 5 * m:md.meshletBoundsOffset + 5 * m + 5]
        tris[k] = words[md.meshletsOffset + 4 * m + 3]
        inst[k] = mi
    return bounds, tris, inst


def cull(bounds, model_to_world, scales, view, hiz=None):
    """draw_list_culler.comp over entries whose bounds words, mat3x4 [n, 3, 4] and scale are given.  `hiz`: the levels of
    the pyramid (finest first; its source extent is view.resolution) or None -> dict of bool [n]: visible, occluded, and
    outside / cone_hidden for the tests' own questions."""
    n = len(bounds)
    bounds = np.ascontiguousarray(bounds, np.uint32).reshape(n, 5)
    m = np.ascontiguousarray(model_to_world, F).reshape(n, 3, 4)
    scales = np.ascontiguousarray(scales, F).reshape(n)
    with np.errstate(all="ignore"):
        c = bounds[:, :3].copy().view(F)
        cone = bounds[:, 4].copy().view(np.int32)
        axis = np.stack([((cone << s) >> 24).astype(F) / F(127.0) for s in (24, 16, 8)], axis=1)
        cutoff = (cone >> 24).astype(F) / F(127.0)
        center = np.stack([fma(c[:, 2], m[:, i, 2], fma(c[:, 1], m[:, i, 1], fma(c[:, 0], m[:, i, 0], m[:, i, 3]))) for i in range(3)], axis=1)
        radius = np.abs(bounds[:, 3].copy().view(F) * scales)
        axis_w = np.stack([fma(axis[:, 2], m[:, i, 2], fma(axis[:, 1], m[:, i, 1], axis[:, 0] * m[:, i, 0])) for i in range(3)], axis=1)
        cone_axis = normalize3(axis_w)

        outside = np.zeros(n, bool)
        for plane in view.planes:
            sd = fma(plane[2], center[:, 2], fma(plane[1], center[:, 1], fma(plane[0], center[:, 0], plane[3])))
            outside |= sd < -radius
        d = (center - view.eye[None, :]).astype(F)
        cone_hidden = dot3(d, cone_axis) >= cutoff * np.sqrt(dot3(d, d)) + radius

        occluded = np.zeros(n, bool)
        if hiz is not None:
            occluded = _occluded(center, radius, view, hiz)
        tested = scales != F(0.0)
        visible = ~tested | (~outside & ~cone_hidden & ~occluded)
        occluded_only = tested & ~outside & ~cone_hidden & occluded
    return dict(visible=visible, occluded=occluded_only, outside=tested & outside, cone_hidden=tested & ~outside & cone_hidden,
                center=center, radius=radius)


def _occluded(center, radius, view, hiz):
    n = len(center)
    w2c, c2c, cfw = view.world_to_camera, view.camera_to_clip, view.clip_from_world
    cv = [_row_point(w2c, r, center) for r in range(4)]
    cx, cy, cz = cv[0], cv[1], -cv[2]
    r = radius * view.max_view_scale
    projects = ~(cz < r + view.near)
    crx, cry, crz = cx * r, cy * r, cz * r
    czr2 = cz * cz - r * r
    vx = np.sqrt(cx * cx + czr2)
    minx = (vx * cx - crz) / (vx * cz + crx)
    maxx = (vx * cx + crz) / (vx * cz - crx)
    vy = np.sqrt(cy * cy + czr2)
    miny = (vy * cy - crz) / (vy * cz + cry)
    maxy = (vy * cy + crz) / (vy * cz - cry)
    p00, p11 = c2c[0, 0], c2c[1, 1]
    ax, ay = minx * p00 * F(0.5) + F(0.5), maxy * p11 * F(-0.5) + F(0.5)
    az, aw = maxx * p00 * F(0.5) + F(0.5), miny * p11 * F(-0.5) + F(0.5)
    dx, dy = (az - ax) * F(view.resolution[0]), (aw - ay) * F(view.resolution[1])
    px = np.sqrt(fma(dy, dy, dx * dx)).astype(F)
    exponent = (px.view(np.uint32) >> 23) & 0xFF
    mip = np.where(exponent > 127, exponent - 127, 0).astype(np.int64)

    view_dir = normalize3((view.eye[None, :] - center).astype(F))
    closest = (center + view_dir * radius[:, None]).astype(F)
    closest_depth = _row_point(cfw, 2, closest) / _row_point(cfw, 3, closest)

    count = len(hiz)
    hw, hh = hiz[0].shape[1], hiz[0].shape[0]
    uv_scale = (F(view.resolution[0]) / (F(2.0) * F(hw)), F(view.resolution[1]) / (F(2.0) * F(hh)))
    inv = F(1.0) / _row_vec4(c2c, 3, cv)
    u0 = _row_vec4(c2c, 0, cv) * inv * F(0.5) + F(0.5)
    v0 = _row_vec4(c2c, 1, cv) * inv * F(0.5) + F(0.5)
    out = np.zeros(n, bool)
    for k in range(n):
        if not projects[k]:
            continue
        if mip[k] >= count - 1:
            out[k] = closest_depth[k] < hiz[-1][0, 0]
            continue
        level = hiz[mip[k]]
        mw, mh = max(hw >> mip[k], 1), max(hh >> mip[k], 1)
        assert level.shape == (mh, mw)
        u = u0[k] * uv_scale[0] * F(mw) - F(0.5)
        v = v0[k] * uv_scale[1] * F(mh) - F(0.5)
        x0, y0 = int(_f2i(np.floor(u))), int(_f2i(np.floor(v)))
        x1 = x0 if x0 == 2147483647 else x0 + 1
        y1 = y0 if y0 == 2147483647 else y0 + 1
        t = [_texel(level, np.int64(x), np.int64(y)) for x, y in ((x0, y0), (x1, y0), (x0, y1), (x1, y1))]
        out[k] = closest_depth[k] < np.fmin(np.fmin(t[0], t[1]), np.fmin(t[2], t[3]))
    return out


def cull_list(world, pairs, view, model_to_world=None, hiz=None):
    """The culler over a list of a World -> (visible pairs, occluded pairs, triangles of the visible), the pairs sorted"""
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    m2w = transforms_of(world) if model_to_world is None else np.asarray(model_to_world, F)
    scales = instance_scales(m2w)
    if len(pairs) == 0:
        return pairs, pairs, 0
    bounds, tris, inst = meshlet_words(world, pairs)
    r = cull(bounds, m2w[inst], scales[inst], view, hiz)
    order = lambda a: a[np.lexsort((a[:, 1], a[:, 0]))] if len(a) else a
    return order(pairs[r["visible"]]), order(pairs[r["occluded"]]), int(tris[r["visible"]].sum())


def args_of(input_count, visible_count):
    """the argument triple beside a culled list: groupsX mirrors the count; a culler with nothing to cull leaves zeros"""
    return [visible_count, 1, 1] if input_count else [0, 0, 0]
