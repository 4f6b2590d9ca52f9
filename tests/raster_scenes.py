"""Designed scenes of the rasteriser's tests (a helper, like culling_scenes.py).

S1, made for a 48 x 32 image seen from the origin down -z with a vertical field of view of 90 degrees: on the plane
z = -1 pixel centre (c, r) lies at x = (c + 0.5) / 16 - 1.5, y = 1 - (r + 0.5) / 16, both exact in fp16."""
import numpy as np

import culling_scenes as CS
from prosper_amd import meshlets as M
from prosper_amd import scenes
from prosper_amd import world as W

F = np.float32
S1_EXTENT = (48, 32)


def centre(c, r, z=-1.0):
    """the point of the plane `z` that projects onto pixel centre (c, r) of the 48 x 32 image"""
    s = -z
    return ((c + 0.5) / 16.0 - 1.5) * s, (1.0 - (r + 0.5) / 16.0) * s, z


def _attach(world, mesh, groups):
    """meshlets of our own choosing: `groups` = [(vertex indices, [local triangles])]"""
    positions, _ = world.mesh_geometry(mesh)
    meshlets, vertices, tri_bytes, bounds = [], [], bytearray(), []
    for verts, tris in groups:
        assert len(verts) <= M.MAX_VERTICES and len(tris) <= M.MAX_TRIANGLES
        meshlets.append((len(vertices), len(tri_bytes), len(verts), len(tris)))
        vertices += list(verts)
        for t in tris:
            tri_bytes += bytes(t)
        tri_bytes += b"\0" * (-len(tri_bytes) % 4)
        bounds.append(M.meshlet_bounds(positions[np.array(verts)], np.array(tris).reshape(-1, 3)))
    m = np.array(meshlets, np.uint32).reshape(-1, 4)
    size = ((int(m[-1, 1]) + int(m[-1, 3]) + 3) & ~3) * 3
    t = np.zeros(max(size, len(tri_bytes)), np.uint8)
    t[:len(tri_bytes)] = np.frombuffer(bytes(tri_bytes), np.uint8)
    t = np.concatenate([t, np.zeros(-t.size % 4, np.uint8)])
    world.attach_meshlets(mesh, dict(meshlets=m, bounds=np.array(bounds, np.uint32).reshape(-1, 5), vertices=np.array(vertices, np.uint32),
                                     triangles=t))


MASK_ALPHA = np.array([[255, 0, 255, 0], [0, 255, 0, 255], [160, 160, 160, 160], [100, 100, 100, 100]], np.uint8)
"""The MASK quad's 4 x 4 alpha texels: two rows of 0 and 255; a row of 160, where sampleMaterial keeps the fragment
(160 / 255 = 0.63 >= the cutoff 0.5) and the any-hit's sampleAlpha would drop it (sRGB -> linear: 0.35); a row of 100,
below the cutoff either way."""


def _mesh(world, material, points, triangles, groups=None, **kw):
    """a mesh whose index buffer holds `triangles`, every triangle a meshlet of its own unless `groups` says otherwise"""
    points = np.array(points, F)
    mesh = world.add_mesh(points, np.array(triangles, np.uint32).reshape(-1), material,
                          normals=np.tile(np.array([[0, 0, 1]], F), (len(points), 1)), **kw)
    if groups is None:
        groups = [(list(t), [(0, 1, 2)]) for t in triangles]
    _attach(world, mesh, groups)
    return mesh


def s1_world():
    """-> (world, dict of the draw instances by name)"""
    w = scenes.World()
    m = w.add_material(base_color=(0.7, 0.7, 0.7, 1.0), metallic=0.0, roughness=0.8)
    names = {}

    def place(name, mesh, transform=None):
        w.add_instance(w.add_model([(mesh, m)]), np.eye(4) if transform is None else transform)
        names[name] = len(w.model_instances) - 1

    # two triangles sharing the diagonal (4, 4) - (12, 12), which runs through pixel centres; every vertex on a centre;
    # one meshlet of two triangles
    quad = [centre(4, 4), centre(4, 12), centre(12, 12), centre(12, 4)]  # counter-clockwise seen from +z (y up)
    place("pair", _mesh(w, m, quad, [(0, 1, 2), (0, 2, 3)], groups=[([0, 1, 2, 3], [(0, 1, 2), (0, 2, 3)])]))
    # a sliver thinner than a pixel, a zero-area triangle, a back-facing one: three meshlets of one triangle
    a, b, c = centre(20.8, 3.3, -1.5), centre(21.0, 14.7, -1.5), centre(21.3, 3.4, -1.5)
    z0, z1 = centre(25, 5), centre(29, 9)
    zmid = tuple((p + q) / 2 for p, q in zip(z0, z1))
    back = [centre(30, 4), centre(36, 4), centre(30, 10)]  # clockwise seen from +z
    place("odd", _mesh(w, m, [a, b, c, z0, zmid, z1] + back, [(0, 1, 2), (3, 4, 5), (6, 7, 8)]))
    # crossing the near plane; reaching far outside the guard band; straddling and beyond the far plane
    near = [(0.4, -0.6, -1.0), (-0.4, -0.6, -1.0), (0.0, -0.2, 0.5)]
    guard = [(-0.2, 0.3, -2.0), (30000.0, 0.2, -2.0), (-0.2, 0.9, -2.0)]
    far = [(-40.0, -30.0, -50.0), (40.0, -30.0, -50.0), (0.0, 20.0, -150.0)]
    beyond = [(-40.0, -30.0, -120.0), (40.0, -30.0, -120.0), (0.0, 20.0, -150.0)]
    behind = [(-1.0, -1.0, 2.0), (1.0, -1.0, 2.0), (0.0, 1.0, 3.0)]
    place("clipped", _mesh(w, m, near + guard + far + beyond + behind, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(5)],
                           force_u32_indices=True))  # u32 meshlet vertices
    # one triangle over the whole image, behind everything else
    place("cover", _mesh(w, m, [(-100.0, -60.0, -20.0), (100.0, -60.0, -20.0), (0.0, 140.0, -20.0)], [(0, 1, 2)]))
    # a meshlet of 64 vertices and 124 triangles: an 8 x 8 grid's 98 triangles and, again, the other diagonal's of 13 quads
    # (coplanar with what they overlap: ties inside a meshlet)
    grid = [centre(14 + 1.25 * i, 16 + 1.25 * j, -1.25) for j in range(8) for i in range(8)]
    tris = []
    for j in range(7):
        for i in range(7):
            v = j * 8 + i
            tris += [(v, v + 8, v + 9), (v, v + 9, v + 1)]
    for q in range(13):
        v = (q // 7) * 8 + q % 7
        tris += [(v, v + 8, v + 1), (v + 1, v + 8, v + 9)]
    assert len(tris) == 124
    full = _mesh(w, m, grid, tris, groups=[(list(range(64)), tris)])
    place("full", full)
    # the same quad twice in one place: two draw instances, equal depths, the lower one wins
    dup = _mesh(w, m, [centre(38, 18, -1.1), centre(38, 26, -1.1), centre(45, 26, -1.1), centre(45, 18, -1.1)], [(0, 1, 2), (0, 2, 3)])
    place("dup0", dup)
    place("dup1", dup)
    # a non-uniform scale, and a negative one that turns a clockwise quad to the front
    place("stretched", full, W.translate((-0.9, 0.4, -1.5)) @ W.scale((0.5, 1.5, 1.0)))
    cw = _mesh(w, m, [(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.5, 0.5, 0.0), (0.0, 0.5, 0.0)], [(0, 2, 1), (0, 3, 2)])
    place("mirrored", cw, W.translate((1.6, -1.2, -2.0)) @ W.scale((-1.0, 1.0, 1.0)))
    place("mirrored_away", cw, W.translate((2.6, -1.2, -2.0)))  # the same quad unmirrored: back-facing
    # a MASK quad over pixels 30..45 x 2..13 (its corners on pixel corners: every texel is 4 x 3 pixels and every centre lies
    # an eighth of a texel or more inside one), nearest-sampled, in front of a farther opaque quad
    from prosper_amd import structs as S
    rgba = np.full((4, 4, 4), 200, np.uint8)
    rgba[..., 3] = MASK_ALPHA
    tex = w.add_texture(rgba)
    nearest = w.add_sampler(mag=S.FILTER_NEAREST, min_=S.FILTER_NEAREST)
    masked = w.add_material(base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.0, roughness=0.6, alpha_mode=S.ALPHA_MODE_MASK, alpha_cutoff=0.5,
                            base_tex=(tex, nearest))
    corners = [centre(29.5, 1.5), centre(29.5, 13.5), centre(45.5, 13.5), centre(45.5, 1.5)]
    quad_uv = np.array([(0, 0), (0, 1), (1, 1), (1, 0)], F)
    mq = _mesh(w, masked, corners, [(0, 1, 2), (0, 2, 3)], groups=[([0, 1, 2, 3], [(0, 1, 2), (0, 2, 3)])], uvs=quad_uv)
    w.add_instance(w.add_model([(mq, masked)]), np.eye(4))
    names["mask"] = len(w.model_instances) - 1
    behind = [centre(28, 0, -1.4), centre(28, 15, -1.4), centre(47, 15, -1.4), centre(47, 0, -1.4)]
    place("behind_mask", _mesh(w, m, behind, [(0, 1, 2), (0, 2, 3)]))
    w.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 0.0, 0.0))
    return w, names


def s1_camera(width=S1_EXTENT[0], height=S1_EXTENT[1]):
    return CS.camera_at(width=width, height=height)


def list_world(count):
    """`count` meshlets of one triangle each in front of the camera (count 0: one, under a BLEND material, which the
    OPAQUE list leaves out)"""
    from prosper_amd import structs as S
    w = scenes.World()
    opaque = w.add_material(base_color=(0.8, 0.8, 0.8, 1.0))
    blend = w.add_material(base_color=(0.2, 0.2, 0.8, 0.5), alpha_mode=S.ALPHA_MODE_BLEND)
    n = max(count, 1)
    rng = np.random.default_rng(count)
    points, tris = [], []
    for k in range(n):
        x, y, z = rng.uniform(-1.2, 1.2), rng.uniform(-0.8, 0.8), -rng.uniform(1.0, 3.0)
        points += [(x * -z, y * -z, z), (x * -z + 0.2, y * -z, z), (x * -z, y * -z + 0.2, z)]
        tris.append((3 * k, 3 * k + 1, 3 * k + 2))
    mat = opaque if count else blend
    mesh = _mesh(w, mat, points, tris)
    w.add_instance(w.add_model([(mesh, mat)]))
    w.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 5.0, 0.0))
    return w


# ---- the sweep's scenes (tests/test_raster_sweep_cpu.py states what each has to reach) ----

SWEEP_EXTENT = (96, 80)  # 3 x 3 tiles of 32 x 32, the last row of tiles half as high


def _half(points):
    """the positions as a mesh's buffer holds them (fp16), finite"""
    p = np.asarray(points, np.float64).astype(np.float16).astype(F)
    assert np.isfinite(p).all()
    return p


def _facing(p):
    """the triangle's front looks at the eye at the origin: counter-clockwise seen from there"""
    p = np.asarray(p, np.float64)
    return float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), -p[0])) > 0.0


def _materials(world, n):
    return [world.add_material(base_color=(0.8 - 0.1 * k, 0.5 + 0.1 * k, 0.4, 1.0), metallic=0.0, roughness=0.6 + 0.1 * k) for k in range(n)]


def _light(world):
    world.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 3.0, 0.0))


def _queue_kind(view, points):
    """what the rasteriser does with a front-facing triangle at SWEEP_EXTENT: 0 queued unclipped, 1 clipped by the near plane
    alone, 2 by the guard band alone, 3 by both; None: anything else"""
    import raster_reference as R
    clip = R.to_clip(view, np.eye(4, dtype=F)[:3], points)
    X, Y, _, ok = R.snap(view, clip)
    if R.is_fast(clip, ok).all():
        bx = R.box(X, Y, view.width, view.height)
        side = max(bx[2] - bx[0], bx[3] - bx[1]) + 1
        return 0 if R.area2(X, Y) < 0 and min(bx[2] - bx[0], bx[3] - bx[1]) >= 0 and side > R.MEDIUM_SIDE else None
    out = ~(R.plane_distances(view, clip) >= 0)
    if out.all(axis=0).any() or out[:, 1].any() or len(R.clip_polygon(view, clip)) < 3:
        return None
    # (a vertex behind the eye is outside everything: the guard band's kinds are told by the vertices in front of it)
    return (1 if out[:, 0].any() else 0) + (2 if out[clip[:, 3] > 0, 2:].any() else 0)


def _queue_group(rng, count):
    """Up to 124 queue-class triangles over a pool of 64 vertices: 22 points near the image's left edge and 22 near its right
    one at depths of 0.4 to 30, 10 behind the near plane and far above the view, 10 far beyond the guard band.  A
    triangle's kind is its index modulo 4 (_queue_kind): a wedge across the whole image; two neighbours of one side and a
    point behind the near plane; two and a point beyond the guard band; one of each, starting far away because it is wide.
    What such a triangle shows of itself is a thin band near the depth of its side points: many triangles win pixels.
    -> (points fp16 [64, 3], triangles)"""
    import raster_reference as R
    assert count <= M.MAX_TRIANGLES
    view = R.View(CS.camera_at(width=SWEEP_EXTENT[0], height=SWEEP_EXTENT[1]))
    aspect = SWEEP_EXTENT[0] / SWEEP_EXTENT[1]
    side = []
    for sign in (-1.0, 1.0):
        d = 10.0 ** rng.uniform(-0.4, 1.45, 22)
        side.append(np.stack([sign * rng.uniform(0.8, 1.1, 22) * aspect * d, rng.uniform(-0.95, 0.95, 22) * d, -d], axis=1))
    behind = np.stack([rng.uniform(-1.0, 1.0, 10), rng.uniform(20.0, 60.0, 10), rng.uniform(0.0, 0.5, 10)], axis=1)
    d = 10.0 ** rng.uniform(-0.4, 1.45, 10)
    far = rng.uniform(40000.0, 60000.0, 10) * rng.choice([-1.0, 1.0], 10)
    along_x = rng.random(10) < 0.5
    far = np.where(along_x, far, np.abs(far))  # (above, like the points behind: a triangle of both never passes the eye's front)
    guard = np.stack([np.where(along_x, far, rng.uniform(-1.0, 1.0, 10) * d), np.where(along_x, rng.uniform(-1.0, 1.0, 10) * d, far), -d], axis=1)
    points = _half(np.concatenate(side + [behind, guard]))
    height = points[:44, 1] / -points[:44, 2]  # where a side's point lies along its edge of the image
    far_half = [int(i) for i in np.argsort(points[:44, 2])[:22]]

    def neighbour(i):
        """another point of i's side, among the two nearest to it along the edge"""
        same = [j for j in range(22 * (i // 22), 22 * (i // 22) + 22) if j != i]
        same.sort(key=lambda j: abs(height[j] - height[i]))
        return same[int(rng.integers(0, 2))]

    tris = []
    while len(tris) < count:
        kind = len(tris) % 4
        i = int(rng.integers(0, 44))
        if kind == 0:
            t = [i, neighbour(i), int(rng.integers(0, 22)) + (22 if i < 22 else 0)]
        elif kind == 1:
            t = [i, neighbour(i), 44 + int(rng.integers(0, 10))]
        elif kind == 2:
            t = [i, neighbour(i), 54 + int(rng.integers(0, 10))]
        else:
            i = far_half[int(rng.integers(0, len(far_half)))]
            t = [i, 44 + int(rng.integers(0, 10)), 54 + int(rng.integers(0, 10))]
        if not _facing(points[t]):
            t = [t[0], t[2], t[1]]
        if tuple(t) not in tris and _queue_kind(view, points[t]) == kind:
            tris.append(tuple(t))
    return points, tris


def queue_world(n, grouped):
    """`n` triangles that all go to the queue at SWEEP_EXTENT, a quarter each of: unclipped with a box side above 64 pixel
    centres; crossing the near plane; reaching beyond the guard band; both.  Steeply tilted wedges at depths of 0.4 to 30, so
    that many of them win pixels.  grouped False: a meshlet per triangle; True: meshlets of up to 124 triangles over 64
    vertices, so that a wave appends up to 64 records in one ballot, in both rounds.  The first 124 triangles are one mesh
    under one material, the rest another under another."""
    rng = np.random.default_rng(1000 + n)
    w = scenes.World()
    mats = _materials(w, 2)
    for k, at in enumerate(range(0, n, M.MAX_TRIANGLES)):
        points, tris = _queue_group(rng, min(M.MAX_TRIANGLES, n - at))
        material = mats[min(k, 1)]
        mesh = _mesh(w, material, points, tris, groups=[(list(range(64)), tris)] if grouped else None)
        w.add_instance(w.add_model([(mesh, material)]))
    _light(w)
    return w


_ZOO = []


def _zoo_triangles():
    """The seeded search of clip_zoo_world, made once: -> [(points fp16 [3, 3], polygon size, fan triangles skipped)]"""
    import raster_reference as R
    if _ZOO:
        return _ZOO
    rng = np.random.default_rng(77)
    view = R.View(CS.camera_at(width=SWEEP_EXTENT[0], height=SWEEP_EXTENT[1]))
    identity = np.eye(4, dtype=F)[:3]
    by_size, skipping = {}, []
    wanted = {4: 3, 5: 3, 6: 3, 7: 3, 8: 1, 9: 1}
    for attempt in range(4000):  # the fixed budget; 8 and 9 vertices are looked for over its first 800 attempts only
        full = len(skipping) >= 4 and all(len(by_size.get(s, [])) >= wanted[s] for s in (4, 5, 6, 7))
        if full and (attempt >= 800 or any(s >= 8 for s in by_size)):
            break
        if attempt % 4 == 3 and len(skipping) < 4:
            # a vertex a few fp16 steps behind the near plane: two cuts that snap onto each other
            d = rng.uniform(0.5, 4.0)
            p = np.array([(rng.uniform(-1, 1) * d, rng.uniform(-1, 1) * d, -d), (rng.uniform(-1, 1) * d, rng.uniform(-1, 1) * d, -d),
                          (rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), -CS.NEAR + rng.uniform(0.0, 3e-4))])
        else:
            scale = 10.0 ** rng.uniform(2.5, 4.5)
            p = rng.normal(size=(3, 3)) * [scale, scale, 1.0] + [0.0, 0.0, -0.3]
        p = np.clip(p, -60000.0, 60000.0).astype(np.float16).astype(F)
        if not _facing(p):
            p = p[::-1].copy()
        clip = R.to_clip(view, identity, p)
        X, Y, _, ok = R.snap(view, clip)
        out = ~(R.plane_distances(view, clip) >= 0)
        if R.is_fast(clip, ok).all() or out.all(axis=0).any():
            continue
        # a plane adds a vertex at the most, and only where it separates the triangle's vertices
        most = 3 + int((out.any(axis=0) & ~out.all(axis=0)).sum())
        if len(skipping) >= 4 and not any(len(by_size.get(s, [])) < n for s, n in wanted.items() if s <= most):
            continue
        poly = R.clip_polygon(view, clip)
        if len(poly) < 4:
            continue
        PX, PY, _, pok = R.snap(view, poly)
        if not pok.all():
            continue
        areas = [R.area2(PX[[0, k, k + 1]], PY[[0, k, k + 1]]) for k in range(1, len(poly) - 1)]
        drawn, skipped = sum(a < 0 for a in areas), sum(a >= 0 for a in areas)
        if drawn == 0:
            continue
        if skipped and len(skipping) < 4:
            skipping.append((p, len(poly), skipped))
        elif not skipped and len(by_size.setdefault(len(poly), [])) < wanted[len(poly)]:
            by_size[len(poly)].append((p, len(poly), 0))
    _ZOO.extend([t for s in sorted(by_size) for t in by_size[s]] + skipping)
    return _ZOO


def clip_zoo_world():
    """Triangles whose clipped polygons at SWEEP_EXTENT have 4, 5, 6 and 7 vertices (three each; 8 or 9 where the search's
    budget finds one), and four whose fan holds a triangle that snaps to zero or positive area next to ones that are drawn.
    A meshlet per triangle."""
    w = scenes.World()
    (m,) = _materials(w, 1)
    found = _zoo_triangles()
    points = np.concatenate([p for p, _, _ in found])
    mesh = _mesh(w, m, points, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(found))])
    w.add_instance(w.add_model([(mesh, m)]))
    _light(w)
    return w


def _pack(rng, tris):
    """consecutive triangles into meshlets of random size from 1 to 124, of at most 64 vertices -> groups for _attach"""
    groups, at = [], 0
    while at < len(tris):
        want = int(rng.integers(1, M.MAX_TRIANGLES + 1))
        verts, local = [], []
        while at < len(tris) and len(local) < want:
            new = [v for v in dict.fromkeys(tris[at]) if v not in verts]
            if len(verts) + len(new) > M.MAX_VERTICES:
                break
            verts += new
            local.append(tuple(verts.index(v) for v in tris[at]))
            at += 1
        groups.append((verts, local))
    return groups


def _soup_mesh(rng, world, material, count, **kw):
    """`count` triangles in strips of 1 to 6 that share their vertices, in a frustum-shaped volume down -z:
    screen size log-uniform from a tenth of a pixel to several tiles, any orientation, either winding; of twelve strips one is
    pulled through the near plane, one beyond the guard band, one lies wholly outside, one has coincident vertices"""
    points, tris = [], []
    while len(tris) < count:
        d = 10.0 ** rng.uniform(-0.3, 1.2)
        size = d * 10.0 ** rng.uniform(-2.2, 0.7)
        c = np.array([rng.uniform(-1.3, 1.3) * d, rng.uniform(-1.0, 1.0) * d, -d])
        kind = int(rng.integers(0, 12))
        if kind == 2:
            c[int(rng.integers(0, 2))] = rng.choice([-1.0, 1.0]) * (3.0 * d + 4.0 * size)
        a = rng.uniform(0.0, 2.0 * np.pi)
        tilt = min(1.0, 0.2 * d / size)  # (a strip of several tiles keeps clear of the near plane unless it is pulled there)
        u = np.array([np.cos(a), np.sin(a), rng.uniform(-0.5, 0.5) * tilt]) * size
        v = np.array([-np.sin(a), np.cos(a), rng.uniform(-0.5, 0.5) * tilt]) * size
        k = int(rng.integers(1, 7))
        strip = [c + u * (j // 2) + v * (j % 2) + rng.uniform(-0.15, 0.15, 3) * size * [1.0, 1.0, tilt] for j in range(k + 2)]
        if kind == 0:
            strip[int(rng.integers(0, k + 2))][2] = rng.uniform(0.0, 1.0)
        if kind == 1:
            strip[int(rng.integers(0, k + 2))][:2] *= 1e4
        if kind == 3:
            strip[-1] = strip[-3].copy()  # the last triangle has no area, under any transform
        base = len(points)
        flip = rng.random() < 0.35
        points += [np.clip(p, -60000.0, 60000.0) for p in strip]
        for j in range(k):
            t = (base + j, base + j + 1, base + j + 2)
            tris.append((t[1], t[0], t[2]) if (j % 2 == 1) != flip else t)
    tris = tris[:count]
    return _mesh(world, material, _half(points), tris, groups=_pack(rng, tris), **kw)


def soup_world(seed):
    """Two meshes of triangle strips of every size class (_soup_mesh), one with u16 and one with u32 meshlet vertices, in
    meshlets of random size; five draw instances: the first mesh as it is, mirrored, and as it is once more (equal depths
    across draw instances at every pixel); the second under a non-uniform scale and under a rotation.  -> (world, names)"""
    rng = np.random.default_rng(seed)
    w = scenes.World()
    mats = _materials(w, 3)
    first = _soup_mesh(rng, w, mats[0], 125)
    second = _soup_mesh(rng, w, mats[1], 105, force_u32_indices=True)
    names = {}
    for name, mesh, material, transform in (
            ("plain", first, mats[0], W.translate((0.1, -0.05, -0.2))),
            ("mirrored", first, mats[1], W.translate((-0.2, 0.1, 0.1)) @ W.scale((-1.0, 1.0, 1.0))),
            ("stretched", second, mats[1], W.scale((1.3, 0.7, 1.1))),
            ("duplicate", first, mats[0], W.translate((0.1, -0.05, -0.2))),
            ("turned", second, mats[2], W.rotate_z(0.8) @ W.rotate_y(0.15))):
        w.add_instance(w.add_model([(mesh, material)]), transform)
        names[name] = len(w.model_instances) - 1
    _light(w)
    return w, names


def graded_floor_world(columns=(8, 1, 1, 1, 1) * 3, nz=28, below=0.06, nearest=0.06, ratio=1.2, half=(2.4, 1.0), roll=0.3):
    """One indexed planar grid of nx x nz quads `below` the eye: its rows are graded geometrically in distance, from `nearest`
    (behind the near plane, 0.1) on - queue class where the floor enters the image, a thirtieth of a pixel deep at the far end -
    and the floor is turned about the vertical, so that an image row crosses rows of the grid of several classes.  No jitter:
    no triangle folds under the fp16 rounding.  Meshlets by the builder."""
    w = scenes.World()
    (m,) = _materials(w, 1)
    nx = len(columns)
    edges = np.concatenate([[0.0], np.cumsum(columns)]) / float(sum(columns))
    points = []
    for z in -nearest * ratio ** np.arange(nz + 1):
        reach = half[0] + half[1] * abs(z)
        points += [(reach * (2.0 * x - 1.0), -below, z) for x in edges]
    tris = []
    for j in range(nz):
        for i in range(nx):
            v = j * (nx + 1) + i
            a, b, c, d = v, v + 1, v + nx + 2, v + nx + 1  # a, b on the nearer row
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 else [(a, b, d), (b, c, d)]
    points = np.array(points, F)
    mesh = w.add_mesh(points, np.array(tris, np.uint32).reshape(-1), m, normals=np.tile(np.array([[0, 1, 0]], F), (len(points), 1)))
    w.add_instance(w.add_model([(mesh, m)]), W.rotate_z(roll))
    _light(w)
    w.add_meshlets()
    return w


def scan_world():
    """Four large BLEND triangles, tilted in depth along both image axes and overlapping only partly, in front of an opaque
    backdrop: a pixel holds 0 to 4 layers, and no two neighbouring pixels the same keys.  They reach past the image's last
    rows, where the scan's last blocks lie.  Made for a camera at the origin looking down -z (any extent)."""
    from prosper_amd import structs as S
    w = scenes.World()
    tris = [[(-2.6, -2.4, -1.6), (3.4, -2.9, -2.9), (-1.9, 2.2, -2.3)],
            [(3.0, 2.6, -1.4), (-3.1, 2.9, -2.6), (2.4, -3.3, -3.2)],
            [(-0.3, 3.1, -1.9), (-2.2, -3.4, -3.4), (2.3, -3.0, -1.5)],
            [(-3.6, 0.4, -2.7), (1.9, -1.4, -1.7), (1.2, 2.7, -3.6)]]
    for k, p in enumerate(tris):
        mat = w.add_material(base_color=(0.3 + 0.2 * k, 0.8 - 0.15 * k, 0.4, 0.3 + 0.15 * k), metallic=0.0, roughness=0.5, alpha_mode=S.ALPHA_MODE_BLEND)
        p = _half(p)
        mesh = _mesh(w, mat, p if _facing(p) else p[::-1], [(0, 1, 2)])
        w.add_instance(w.add_model([(mesh, mat)]))
    _backdrop(w)
    _light(w)
    return w


def _backdrop(world):
    """one far opaque quad over the whole view, so that the scene has an opaque list too"""
    m = world.add_material(base_color=(0.5, 0.5, 0.5, 1.0), metallic=0.0, roughness=0.8)
    mesh = _mesh(world, m, [(-400.0, -400.0, -90.0), (400.0, -400.0, -90.0), (400.0, 400.0, -90.0), (-400.0, 400.0, -90.0)], [(0, 1, 2), (0, 2, 3)])
    world.add_instance(world.add_model([(mesh, m)]))


def blend_variant(world):
    """the same geometry under BLEND materials without a texture (alpha 0.3, 0.5, 0.7, ...), in front of one far opaque
    backdrop: for the layer modes.  Changes `world` and returns it."""
    from prosper_amd import structs as S
    for k, m in enumerate(world.materials[1:]):
        m.alphaMode = S.ALPHA_MODE_BLEND
        m.baseColorFactor.w = 0.3 + 0.2 * (k % 3)
    _backdrop(world)
    world._frozen = None
    return world


def mask_variant(world):
    """the same geometry under MASK materials without a texture, cutoff 0.5: the first, third, ... with an alpha factor of
    0.75 (every fragment kept), the others of 0.25 (every fragment discarded).  Changes `world` and returns it."""
    from prosper_amd import structs as S
    for k, m in enumerate(world.materials[1:]):
        m.alphaMode = S.ALPHA_MODE_MASK
        m.alphaCutoff = 0.5
        m.baseColorFactor.w = 0.25 if k % 2 else 0.75
    world._frozen = None
    return world


def closed_world(n=5):
    """A closed, outward-facing object in front of the camera: a cube of n x n quads per face pushed out onto a sphere of
    radius 1.5 at z = -3.6 (every vertex is shared by index, so the fp16 rounding opens no crack), and a smaller plain cube
    beside it.  No pixel's nearest surface is a back face.  Meshlets by the greedy builder."""
    w = scenes.World()
    m = w.add_material(base_color=(0.7, 0.6, 0.5, 1.0), metallic=0.0, roughness=0.7)

    def cube(n, round_):
        index, points, tris = {}, [], []

        def vertex(p):
            key = tuple(int(round(c * n)) for c in p)
            if key not in index:
                q = np.array(p, np.float64) * 2.0 - 1.0
                if round_:
                    q = q / np.linalg.norm(q)
                index[key] = len(points)
                points.append(tuple(q))
            return index[key]

        # per face: the fixed axis and its value, the two running axes ordered so that (u, v, outward) is right-handed
        for axis, value, (ua, va) in ((0, 1, (1, 2)), (0, 0, (2, 1)), (1, 1, (2, 0)), (1, 0, (0, 2)), (2, 1, (0, 1)), (2, 0, (1, 0))):
            for j in range(n):
                for i in range(n):
                    def at(di, dj):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[ua], p[va] = float(value), (i + di) / n, (j + dj) / n
                        return vertex(p)
                    a, b, c, d = at(0, 0), at(1, 0), at(1, 1), at(0, 1)
                    tris += [(a, b, c), (a, c, d)]
        return np.array(points, F), np.array(tris, np.uint32)

    for round_, n_, transform in ((True, n, W.translate((-0.9, 0.1, -3.6)) @ W.rotate_y(0.4) @ W.scale(1.5)),
                                  (False, 2, W.translate((2.0, -0.4, -3.0)) @ W.rotate_y(0.7) @ W.scale(0.7))):
        points, tris = cube(n_, round_)
        normals = points / np.linalg.norm(points, axis=1, keepdims=True)
        mesh = w.add_mesh(points, tris.reshape(-1), m, normals=normals.astype(F))
        w.add_instance(w.add_model([(mesh, m)]), transform)
    w.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 3.0, 0.0))
    w.add_meshlets()
    return w
