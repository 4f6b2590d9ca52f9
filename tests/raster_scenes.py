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
