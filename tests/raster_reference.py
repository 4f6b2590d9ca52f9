"""NumPy restatement of the rasteriser over the meshlet draw lists (a helper, like the other
*_reference.py files): vertices, the fast path's conditions, the clipper, snapping, coverage, depth, ties and the counts of
prosper_pt_get_raster_info - one float32 operation per rounding, in the order pt_raster.hip fixes.

The draw order does not matter: a pixel keeps the greatest key, (depth bits << 32) | ~(ordinal * 128 + triangle)."""
import numpy as np

import culling_reference as CR
from particles_reference import fma
from prosper_amd import meshlets as M

F = np.float32
I = np.int64
SMALL_PIXELS, MEDIUM_SIDE = 32, 64  # pt_raster.hip's size classes: they decide who walks a box, and the `queued` count
NO_ID = 0xFFFFFFFF


def guard_band(width, height):
    return F(F(65536.0) / F(max(width, height)) - F(2.0))


class View:
    def __init__(self, camera, width=None, height=None):
        self.w2c = CR.mat4_of(camera.worldToCamera)
        self.c2c = CR.mat4_of(camera.cameraToClip)
        self.width = int(camera.resolution[0]) if width is None else width
        self.height = int(camera.resolution[1]) if height is None else height
        self.G = guard_band(self.width, self.height)


def to_clip(view, m2w, positions):
    """`m2w` float32 [3, 4]: the three rows of the affine; `positions` float32 [n, 3] -> clip float32 [n, 4]"""
    p = np.asarray(positions, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        w = [fma(p[:, 2], m2w[r, 2], fma(p[:, 1], m2w[r, 1], fma(p[:, 0], m2w[r, 0], m2w[r, 3]))) for r in range(3)]
        W, C = view.w2c, view.c2c
        cam = [fma(W[k, 2], w[2], fma(W[k, 1], w[1], fma(W[k, 0], w[0], W[k, 3]))) for k in range(4)]
        clip = [fma(C[r, 3], cam[3], fma(C[r, 2], cam[2], fma(C[r, 1], cam[1], (C[r, 0] * cam[0]).astype(F)))) for r in range(4)]
    return np.stack(clip, axis=1).astype(F)


def plane_distances(view, clip):
    """float32 [n, 6]: near (z <= w), far (z >= 0), x <= G w, x >= -G w, y <= G w, y >= -G w; inside is >= 0"""
    c = np.asarray(clip, F).reshape(-1, 4)
    x, y, z, w = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    G = view.G
    with np.errstate(all="ignore"):
        return np.stack([(w - z).astype(F), z, fma(G, w, -x), fma(G, w, x), fma(G, w, -y), fma(G, w, y)], axis=1).astype(F)


def snap(view, clip):
    """-> (X, Y int64 in 1/256 pixel, d = z / w float32, ok)"""
    c = np.asarray(clip, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        fx = ((c[:, 0] / c[:, 3]) * F(0.5) + F(0.5)) * F(view.width)
        fy = ((c[:, 1] / c[:, 3]) * F(0.5) + F(0.5)) * F(view.height)
        sx, sy = np.rint(fx * F(256.0)), np.rint(fy * F(256.0))
        ok = (np.abs(sx) <= F(8388608.0)) & (np.abs(sy) <= F(8388608.0))
        d = (c[:, 2] / c[:, 3]).astype(F)
    X = np.where(ok, sx, 0).astype(I)
    Y = np.where(ok, sy, 0).astype(I)
    return X, Y, d, ok


def is_fast(clip, ok):
    c = np.asarray(clip, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return (c[:, 3] > 0) & (c[:, 2] >= 0) & (c[:, 2] <= c[:, 3]) & ok


def area2(X, Y):
    """twice the area in framebuffer coordinates, y down: negative is the front"""
    return int((X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]))


def box(X, Y, width, height):
    px0, py0 = max((int(min(X)) + 127) >> 8, 0), max((int(min(Y)) + 127) >> 8, 0)
    px1, py1 = min((int(max(X)) - 128) >> 8, width - 1), min((int(max(Y)) - 128) >> 8, height - 1)
    return px0, py0, px1, py1


def cover(X, Y, d, a2, bx):
    """Coverage of the box's pixels by a front-facing triangle (a2 < 0) under the top-left rule, and the depth
    -> (py, px index arrays, depth float32) of the fragments that pass 0 < depth <= 1"""
    px0, py0, px1, py1 = bx
    px, py = np.meshgrid(np.arange(px0, px1 + 1, dtype=I), np.arange(py0, py1 + 1, dtype=I))
    sx, sy = px * 256 + 128, py * 256 + 128
    X, Y = [int(v) for v in X], [int(v) for v in Y]
    f, inside = [], np.ones(px.shape, bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ex, ey = X[b] - X[a], Y[b] - Y[a]
        fe = ey * (sx - X[a]) - ex * (sy - Y[a])
        inside &= (fe > 0) | ((fe == 0) & (ey > 0 or (ey == 0 and ex < 0)))
        f.append(fe)
    two_a = F(-a2)
    with np.errstate(all="ignore"):
        l1, l2 = f[2].astype(F) / two_a, f[0].astype(F) / two_a
        depth = fma(l2, F(d[2]) - F(d[0]), fma(l1, F(d[1]) - F(d[0]), F(d[0]))).astype(F)
        inside &= (depth > 0) & (depth <= 1)
    return py[inside], px[inside], depth[inside]


def clip_polygon(view, tri_clip):
    """Sutherland-Hodgman over the six planes in float32; a crossing is cut from the inside vertex towards the outside one
    -> float32 [n, 4], n = 0 or 3 .. 9"""
    poly = [np.asarray(v, F) for v in tri_clip]
    for k in range(6):
        out = []
        dist = [plane_distances(view, v)[0, k] for v in poly]
        for i in range(len(poly)):
            j = i + 1 if i + 1 < len(poly) else 0
            a, b, da, db = poly[i], poly[j], dist[i], dist[j]
            ina, inb = bool(da >= 0), bool(db >= 0)
            if ina:
                out.append(a)
            if ina != inb:
                s, e, ds, de = (a, b, da, db) if ina else (b, a, db, da)
                with np.errstate(all="ignore"):
                    t = F(ds / F(ds - de))
                    out.append(np.asarray(fma(t, (e - s).astype(F), s), F))
        poly = out[:10] if len(out) >= 3 else []
        if not poly:
            break
    return np.array(poly, F).reshape(-1, 4)


def mesh_uvs(world, mesh):
    """float64 [n, 2]: the mesh's texCoord0 as the buffer holds it (fp16), zeros without one"""
    md, info = world.metadatas[mesh], world.mesh_infos[mesh]
    if md.texCoord0sOffset == 0xFFFFFFFF:
        return np.zeros((info.vertexCount, 2))
    words = world._buffer_words_of(md.bufferIndex)
    return words[md.texCoord0sOffset:md.texCoord0sOffset + info.vertexCount].view(np.float16).reshape(-1, 2).astype(np.float64)


TEXEL_MARGIN = 0.02  # of a texel: a float64 uv this far from a texel's border names the texel the float32 code names


def mask_discards(world, material, clip3, uv3, px, py, width, height):
    """gbuffer.frag:61-63 for a MASK material: sampleMaterial's alpha is 0 where the RAW alpha * factor is below the cutoff
    (not the any-hit's sampleAlpha, which takes alpha through sRGB -> linear).  The decision, not the bits: the pixel
    centre's perspective-correct barycentrics on the ORIGINAL triangle in float64, the uv, and - for a NEAREST sampler
    with REPEAT wrap, the only kind restated - the texel, asserted to lie TEXEL_MARGIN clear of its borders.
    -> bool array over the fragments (py, px)"""
    from prosper_amd import structs as S
    m = world.materials[material]
    if m.alphaMode != S.ALPHA_MODE_MASK:
        return np.zeros(len(px), bool)
    factor = float(m.baseColorFactor.w)
    tex, samp = m.baseColorTextureSampler & 0xFFFFFF, m.baseColorTextureSampler >> 24
    if tex == 0:
        return np.full(len(px), F(F(1.0) * F(factor)) < F(m.alphaCutoff))
    mag, min_, ws, wt = world.samplers[samp]
    assert (mag, min_, ws, wt) == (S.FILTER_NEAREST, S.FILTER_NEAREST, S.WRAP_REPEAT, S.WRAP_REPEAT)
    texels = world.textures[tex]
    th, tw = texels.shape[:2]
    c = np.asarray(clip3, np.float64)[:, [0, 1, 3]]  # homogeneous 2-D: (x, y, w)
    P = np.stack([(px + 0.5) / width * 2.0 - 1.0, (py + 0.5) / height * 2.0 - 1.0, np.ones(len(px))], axis=1)
    lam = np.stack([np.linalg.det(np.stack([P, np.broadcast_to(c[(k + 1) % 3], P.shape), np.broadcast_to(c[(k + 2) % 3], P.shape)], axis=1))
                    for k in range(3)], axis=1)
    lam /= lam.sum(axis=1, keepdims=True)
    uv = lam @ np.asarray(uv3, np.float64)
    tu, tv = uv[:, 0] * tw, uv[:, 1] * th
    for t in (tu, tv):
        frac = t - np.floor(t)
        assert ((frac > TEXEL_MARGIN) & (frac < 1.0 - TEXEL_MARGIN)).all(), "a pixel's uv lies on a texel border: the scene is not what the restatement can decide"
    a = texels[np.floor(tv).astype(I) % th, np.floor(tu).astype(I) % tw, 3]
    raw = (a.astype(F) / F(255.0)) * F(factor)
    return raw < F(m.alphaCutoff)


def meshlet_base(world):
    """the ordinal of every draw instance's meshlet 0: the prefix sum of the meshlet counts of the draw instances before it
    (every instance the generator can emit entries for: a mesh with meshlets has indices, so these are the instances
    recordGenerateList counts)"""
    base, total = [], 0
    for mi, mesh, mat in CR.draw_instances_of(world):
        base.append(total)
        total += world.mesh_infos[mesh].meshletCount
    return base


def rasterise(world, camera, pairs, keys=None, m2w=None):
    """Draws the list `pairs` [(drawInstanceIndex, meshletIndex)] -> dict(keys uint64 [h, w], counts).  `keys`: the image
    to draw on top of (None: cleared)."""
    view = View(camera)
    width, height = view.width, view.height
    keys = np.zeros((height, width), np.uint64) if keys is None else keys.copy()
    counts = dict(triangles=0, culledBackface=0, culledZeroArea=0, culledOutside=0, clipped=0, queued=0, fragments=0)
    f = world.freeze()
    dis = CR.draw_instances_of(world)
    base = meshlet_base(world)
    m2w = CR.transforms_of(world) if m2w is None else m2w
    cache = {}

    def emit(py, px, depth, low, mask=None):
        if mask is not None and len(py):
            keep = ~mask_discards(world, mask[0], mask[1], mask[2], px, py, width, height)
            py, px, depth = py[keep], px[keep], depth[keep]
        counts["fragments"] += len(py)
        k = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(~low & 0xFFFFFFFF)
        keys[py, px] = np.maximum(keys[py, px], k)

    for di, mi in np.asarray(pairs, I).reshape(-1, 2).tolist():
        inst, mesh, material = dis[di]
        if mesh not in cache:
            md, info = world.metadatas[mesh], world.mesh_infos[mesh]
            cache[mesh] = (world.mesh_geometry(mesh)[0], M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info))
        positions, built = cache[mesh]
        uvs = mesh_uvs(world, mesh)
        vo, to, vc, tc = (int(v) for v in built["meshlets"][mi])
        vidx = built["vertices"][vo:vo + vc].astype(I)
        clip = to_clip(view, m2w[inst], positions[vidx])
        X, Y, d, ok = snap(view, clip)
        fast = is_fast(clip, ok)
        outcode = ~(plane_distances(view, clip) >= 0)
        tris = built["triangles"][to:to + 3 * tc].reshape(-1, 3).astype(I)
        for t, (a, b, c) in enumerate(tris.tolist()):
            counts["triangles"] += 1
            low = (base[di] + mi) * 128 + t
            v = [a, b, c]
            mask = (material, clip[v], uvs[vidx[v]])
            if fast[v].all():
                a2 = area2(X[v], Y[v])
                if a2 == 0:
                    counts["culledZeroArea"] += 1
                    continue
                if a2 > 0:
                    counts["culledBackface"] += 1
                    continue
                bx = box(X[v], Y[v], width, height)
                if bx[0] > bx[2] or bx[1] > bx[3]:
                    counts["culledOutside"] += 1
                    continue
                bw, bh = bx[2] - bx[0] + 1, bx[3] - bx[1] + 1
                if bw * bh > SMALL_PIXELS and (bw > MEDIUM_SIDE or bh > MEDIUM_SIDE):
                    counts["queued"] += 1
                emit(*cover(X[v], Y[v], d[v], a2, bx), low, mask)
                continue
            if outcode[v].all(axis=0).any():  # all three vertices beyond one plane
                counts["culledOutside"] += 1
                continue
            counts["queued"] += 1
            poly = clip_polygon(view, clip[v])
            if len(poly):
                PX, PY, pd, pok = snap(view, poly)
                if not pok.all():
                    poly = poly[:0]
            if not len(poly):
                counts["culledOutside"] += 1
                continue
            counts["clipped"] += 1
            for k in range(1, len(poly) - 1):  # the fan from the polygon's first vertex
                w = [0, k, k + 1]
                a2 = area2(PX[w], PY[w])
                if a2 >= 0:
                    continue
                bx = box(PX[w], PY[w], width, height)
                if bx[0] > bx[2] or bx[1] > bx[3]:
                    continue
                emit(*cover(PX[w], PY[w], pd[w], a2, bx), low, mask)
    return dict(keys=keys, counts=counts)


def decode(world, keys):
    """-> (ids uint32 [h, w, 3], depth float32 [h, w]) as prosper_pt_read_raster_visibility gives them"""
    base = np.array(meshlet_base(world), I)
    has = np.array([world.mesh_infos[mesh].meshletCount > 0 and world.mesh_infos[mesh].indexCount > 0
                    for _, mesh, _ in CR.draw_instances_of(world)])
    low = (~keys & np.uint64(0xFFFFFFFF)).astype(I)
    ordinal = low >> 7
    # the last draw instance whose base is not above the ordinal
    d = np.searchsorted(base, ordinal, side="right") - 1
    ids = np.stack([d, ordinal - base[d], low & 127], axis=2).astype(np.uint32)
    ids[keys == 0] = NO_ID
    assert has[d[keys != 0]].all()
    return ids, (keys >> np.uint64(32)).astype(np.uint32).view(F)


def _canonical(a, b, c):
    """the rotation of a triangle that starts at its smallest index: the winding is kept"""
    k = min(range(3), key=lambda i: (a, b, c)[i])
    return ((a, b, c), (b, c, a), (c, a, b))[k]


def triangle_map(indices, built):
    """meshlet triangle -> geometry triangle: a meshlet triangle's three global vertex indices are looked up, rotation-
    invariant, among the index buffer's triangles; duplicates take the lowest match.  `indices` uint32 [3 n], `built` what
    meshlets.read_meshlets gives -> [int64 [triangleCount] per meshlet].  A triangle with no match is a ValueError."""
    first = {}
    for g, tri in enumerate(np.asarray(indices, I).reshape(-1, 3).tolist()):
        first.setdefault(_canonical(*tri), g)
    out = []
    for vo, to, vc, tc in built["meshlets"].tolist():
        verts = built["vertices"][vo:vo + vc].astype(I)
        local = built["triangles"][to:to + 3 * tc].reshape(-1, 3).astype(I)
        row = []
        for t in verts[local].tolist():
            key = _canonical(*t)
            if key not in first:
                raise ValueError("meshlet triangle %r is not in the index buffer" % (t,))
            row.append(first[key])
        out.append(np.array(row, I))
    return out


def geometry_ids(world, ids):
    """the id image with its meshlet triangle mapped to the geometry triangle -> int64 [h, w, 2] of (drawInstance,
    primitive), -1 where nothing is drawn"""
    f = world.freeze()
    dis = CR.draw_instances_of(world)
    maps = {}
    out = np.full(ids.shape[:2] + (2,), -1, I)
    for py, px in zip(*np.nonzero(ids[..., 0] != NO_ID)):
        di, mi, t = (int(v) for v in ids[py, px])
        mesh = dis[di][1]
        if mesh not in maps:
            md, info = world.metadatas[mesh], world.mesh_infos[mesh]
            maps[mesh] = triangle_map(world.mesh_geometry(mesh)[1], M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info))
        out[py, px] = (di, maps[mesh][mi][t])
    return out
