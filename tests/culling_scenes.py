"""Designed scenes of the culling tests (a helper, like debug_view_scene.py): meshes of one triangle per meshlet whose bounds
words the test writes itself - the culler reads nothing else of a meshlet but its triangle count - and the depths their
pyramids are made from."""
import math

import numpy as np

from prosper_amd import scenes, structs as S
from prosper_amd import world as W

F = np.float32
WIDTH, HEIGHT = 96, 64
FOV = math.radians(90.0)
NEAR, FAR = 0.1, 100.0


def camera_at(eye=(0.0, 0.0, 0.0), target=(0.0, 0.0, -1.0), width=WIDTH, height=HEIGHT):
    from prosper_amd import rt_reference
    cam = rt_reference.Camera()
    cam.set_parameters(FOV, NEAR, FAR)
    cam.look_at(eye, target, (0.0, 1.0, 0.0))
    cam.update_resolution(width, height)
    u, _ = cam.update_buffer()
    cam.close()
    return u


def depth_of(camera, view_z):
    """the non-linear depth of a point at view-space z (negative in front of the camera), float64 -> float32"""
    m = np.array([[getattr(camera.cameraToClip.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], np.float64)
    clip = m @ np.array([0.0, 0.0, view_z, 1.0])
    return F(clip[2] / clip[3])


def bounds_word(center, radius, axis_s8=(0, 0, 0), cutoff_s8=127):
    w = np.empty(5, np.uint32)
    w[:3] = np.asarray(center, F).view(np.uint32)
    w[3] = np.array([radius], F).view(np.uint32)[0]
    w[4] = (int(axis_s8[0]) & 0xFF) | ((int(axis_s8[1]) & 0xFF) << 8) | ((int(axis_s8[2]) & 0xFF) << 16) | ((int(cutoff_s8) & 0xFF) << 24)
    return w


def add_designed_mesh(world, bounds, material, triangles_per_meshlet=None):
    """A mesh of len(bounds) meshlets: meshlet k has bounds[k] and (k % 3) + 1 small triangles of its own (or what
    `triangles_per_meshlet` says), far below the scene where no camera of the tests looks."""
    n = len(bounds)
    tcount = [(k % 3) + 1 for k in range(n)] if triangles_per_meshlet is None else list(triangles_per_meshlet)
    positions, indices, meshlets, vertices, tri_bytes = [], [], [], [], bytearray()
    for k in range(n):
        base = len(positions)
        x = 0.01 * (k % 50)
        positions += [(x, -900.0, 0.0), (x + 0.005, -900.0, 0.0), (x, -900.0, 0.005), (x + 0.005, -900.0, 0.005), (x, -900.0, 0.01)]
        local = [(0, 1, 2), (1, 3, 2), (2, 3, 4)][:tcount[k]]
        meshlets.append((len(vertices), len(tri_bytes), 5, tcount[k]))
        vertices += list(range(base, base + 5))
        for t in local:
            indices += [base + t[0], base + t[1], base + t[2]]
            tri_bytes += bytes(t)
        tri_bytes += b"\0" * (-len(tri_bytes) % 4)
    mesh = world.add_mesh(np.array(positions, F), np.array(indices, np.uint32), material,
                          normals=np.tile(np.array([[0, 1, 0]], F), (len(positions), 1)))
    m = np.array(meshlets, np.uint32).reshape(-1, 4)
    size = ((int(m[-1, 1]) + int(m[-1, 3]) + 3) & ~3) * 3
    t = np.zeros(max(size, len(tri_bytes)), np.uint8)
    t[:len(tri_bytes)] = np.frombuffer(bytes(tri_bytes), np.uint8)
    world.attach_meshlets(mesh, dict(meshlets=m, bounds=np.array(bounds, np.uint32).reshape(n, 5), vertices=np.array(vertices, np.uint32),
                                     triangles=t))
    return mesh


def ulps(x, k):
    x = F(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
    return x


def sweep_bounds(camera):
    """-> (bounds words [n, 5], labels): hand-set object-space bounds for an instance at the identity, a camera at the
    origin looking down -z"""
    out, labels = [], []

    def add(label, *a, **k):
        out.append(bounds_word(*a, **k))
        labels.append(label)

    planes = {n: np.array([getattr(camera, n).x, getattr(camera, n).y, getattr(camera, n).z, getattr(camera, n).w], np.float64)
              for n in ("nearPlane", "farPlane", "leftPlane", "rightPlane", "bottomPlane", "topPlane")}
    mid = np.array([0.0, 0.0, -10.0])
    radius = 0.5
    for name, pl in planes.items():
        sd_mid = pl[:3] @ mid + pl[3]
        for k in (-3, -1, 0, 1, 3):  # the centre a few ulps of the step either side of signedDistance = -radius
            t = float(ulps(sd_mid + radius, k))
            add("plane %s ulps %+d" % (name, k), mid - pl[:3] * t, radius)
        for margin in (-0.25, 0.25):
            add("plane %s margin %+.2f" % (name, margin), mid - pl[:3] * (sd_mid + radius + margin), radius)
    # the cone, axis pointing away from the eye: hidden while cutoff * 10 + 0.5 <= 10
    for cutoff in (0, 100, 119, 120, 121, 122, 126, 127):
        add("cone cutoff %d" % cutoff, (0.0, 0.0, -10.0), 0.5, (0, 0, -127), cutoff)
    for k in (-2, -1, 0, 1, 2):  # cutoff 0: hidden while radius <= 10 exactly
        add("cone at %+d" % k, (0.0, 0.0, -10.0), ulps(10.0, k), (0, 0, -127), 0)
    add("cone towards the eye", (0.0, 0.0, -10.0), 0.5, (0, 0, 127), 20)
    add("cone sideways", (2.0, 1.0, -10.0), 0.5, (127, 0, 0), 20)
    add("cone zero axis", (0.0, 0.0, -10.0), 0.5, (0, 0, 0), 0)
    # the eye inside the sphere, the sphere behind the eye, straddling the near plane
    add("eye inside", (0.0, 0.0, -1.0), 5.0)
    add("behind the eye", (0.0, 0.0, 3.0), 1.0)
    add("straddles near", (0.0, 0.0, -0.05), 0.3)
    add("touches near from behind", (0.0, 0.0, 0.15), 0.3)
    # footprints from under a pixel to past the top level, in front of and behind a wall at z = -5, left and right
    for r in (0.0005, 0.004, 0.02, 0.06, 0.12, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
        for x in (-4.0, 0.3, 4.0):
            add("behind r %g x %g" % (r, x), (x, 0.5, -12.0), r)
        add("in front r %g" % r, (-1.0, 0.2, -2.0 - r), min(r, 1.5))
    # centres off the screen whose spheres still reach into the frustum: the gather reads the border
    for x, y in ((16.5, 0.0), (-16.5, 0.0), (0.0, 11.0), (0.0, -11.0), (16.0, 10.5)):
        for r in (1.6, 2.5):
            add("off screen %g %g r %g" % (x, y, r), (x, y, -10.0), r)
    return np.array(out, np.uint32), labels


def wall_depth(camera, left_columns=WIDTH, wall_z=-5.0, width=WIDTH, height=HEIGHT):
    """a depth image: a wall at view z `wall_z` over the first `left_columns` columns, sky (0) right of it"""
    d = np.zeros((height, width), F)
    d[:, :left_columns] = depth_of(camera, wall_z)
    return d


def sweep_world(camera, sizes=(1, 15, 16, 17)):
    """The sweep's scene: the hand-set bounds dealt over meshes of `sizes` meshlets (the rest in one more mesh), each mesh an
    instance at the identity; the occlusion cases again under a uniform scale 2 (a mesh of 130 meshlets), a negative uniform scale, a non-uniform
    scale and on an instance a transform update will move; an OPAQUE, a MASK and a BLEND material; one mesh more that is
    never loaded.  -> (world, dict of what the tests need)"""
    w = scenes.World()
    opaque = w.add_material(base_color=(0.8, 0.8, 0.8, 1.0))
    mask = w.add_material(base_color=(0.8, 0.2, 0.2, 1.0), alpha_mode=S.ALPHA_MODE_MASK)
    blend = w.add_material(base_color=(0.2, 0.2, 0.8, 0.5), alpha_mode=S.ALPHA_MODE_BLEND)
    bounds, labels = sweep_bounds(camera)
    at, k = 0, 0
    for n in list(sizes) + [len(bounds) - sum(sizes)]:
        assert n > 0
        mesh = add_designed_mesh(w, bounds[at:at + n], opaque)
        w.add_instance(w.add_model([(mesh, (opaque, mask)[k % 2])]))
        at += n
        k += 1
    assert at == len(bounds)
    occl = np.array([b for b, l in zip(bounds, labels) if l.startswith(("behind r", "in front r", "off screen"))], np.uint32)
    half = occl.copy()
    half[:, :4] = (occl[:, :4].copy().view(F) * F(0.5)).view(np.uint32)  # under scale 2 the same world-space spheres
    flipped = occl.copy()
    flipped[:, :3] = (-(occl[:, :3].copy().view(F) / F(1.5))).astype(F).view(np.uint32)
    flipped[:, 3] = (occl[:, 3].copy().view(F) / F(1.5)).astype(F).view(np.uint32)
    shifted = occl.copy()
    extra = {}
    for name, b, transform, material in (
            ("scaled", np.tile(half, (3, 1))[:130], W.scale(2.0), opaque),
            ("negative", flipped, W.scale(-1.5), mask),
            ("non_uniform", occl, W.scale((1.0, 2.0, 1.0)), opaque),
            ("moved", shifted, W.translate((40.0, 0.0, 0.0)), opaque),  # starts outside the frustum; the update brings it in
            ("blend", occl[:20], np.eye(4), blend)):
        mesh = add_designed_mesh(w, b, material)
        w.add_instance(w.add_model([(mesh, material)]), transform)
        extra[name] = len(w.model_instances) - 1
    # a model with an opaque and a blend sub-mesh, and a mesh that never arrives
    m1, m2 = add_designed_mesh(w, occl[:5], opaque), add_designed_mesh(w, occl[5:12], blend)
    w.add_instance(w.add_model([(m1, opaque), (m2, blend)]))
    missing = add_designed_mesh(w, occl[:9], opaque)
    w.add_instance(w.add_model([(missing, opaque)]))
    w.add_point_light((1.0, 1.0, 1.0), 100.0, (0.0, 5.0, 0.0))
    return w, dict(labels=labels, labelled_meshes=len(sizes) + 1, instances=extra, missing_mesh=missing)


# ---- the property test's scene ----

def property_world(cells=42, tile=7):
    """A wall quad at z = -5 over the left of the view; behind it, at z = -12, a plane of cells x cells quads that extends past
    the wall to the right, its index buffer running tile by tile (7 x 7 quads are 64 vertices: the greedy scan makes every
    tile a meshlet, so the meshlets are compact); the same mesh again wholly behind the wall, wholly outside the frustum, and facing away over the sky
    above everything.  Meshlets by meshlets.py.  -> (world, dict of the instances' indices)"""
    w = scenes.World()
    m = w.add_material(base_color=(0.7, 0.7, 0.7, 1.0), metallic=0.0, roughness=0.8)
    wall = scenes._add(w, scenes.quad((-20.0, -20.0, -5.0), (0.5, -20.0, -5.0), (0.5, 20.0, -5.0), (-20.0, 20.0, -5.0)), m)
    xs, ys = np.linspace(-9.0, 9.0, cells + 1), np.linspace(-4.0, 4.0, cells + 1)
    p = np.array([(x, y, 0.0) for y in ys for x in xs], F)
    idx = []
    for tj in range(0, cells, tile):
        for ti in range(0, cells, tile):
            for j in range(tj, tj + tile):
                for i in range(ti, ti + tile):
                    a = j * (cells + 1) + i
                    idx += [a, a + 1, a + cells + 1, a + 1, a + cells + 2, a + cells + 1]  # counter-clockwise seen from +z
    plane = w.add_mesh(p, np.array(idx, np.uint32), m, normals=np.tile(np.array([[0, 0, 1]], F), (len(p), 1)))
    names = {}
    for name, mesh, t in (("wall", wall, np.eye(4)),
                          ("plane", plane, W.translate((0.0, 0.0, -12.0))),
                          ("hidden", plane, W.translate((-6.0, 0.0, -13.0)) @ W.scale(0.08)),
                          ("outside", plane, W.translate((60.0, 0.0, -12.0))),
                          ("away", plane, W.translate((4.0, 7.5, -11.0)) @ W.rotate_y(math.pi) @ W.scale(0.25))):
        w.add_instance(w.add_model([(mesh, m)]), t)
        names[name] = len(w.model_instances) - 1
    w.add_point_light((1.0, 1.0, 1.0), 500.0, (0.0, 0.0, 0.0))
    w.add_meshlets()
    return w, names


def owners(world, camera, width=WIDTH, height=HEIGHT, margin=1e-4):
    """Ground truth from neither the culler nor its restatement: every triangle of every draw instance against every pixel
    centre in float64, the nearest surface wins; a pixel counts for its triangle's meshlet only where it is clear of the
    triangle's edges and of the next surface's depth by `margin` (barycentrics and depth), and the triangle faces the camera
    (a surface facing away still hides what lies behind it: the traced depth holds it).  -> set of (drawInstance, meshlet)"""
    from prosper_amd import meshlets as M
    f = world.freeze()
    c2c = np.array([[getattr(camera.cameraToClip.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], np.float64)
    w2c = np.array([[getattr(camera.worldToCamera.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], np.float64)
    clip_from_world = c2c @ w2c
    px = (np.arange(width) + 0.5)[None, :]
    py = (np.arange(height) + 0.5)[:, None]
    best = np.zeros((height, width))      # reverse Z: the sky is 0
    second = np.zeros((height, width))
    owner = np.full((height, width, 2), -1, np.int64)
    clear = np.zeros((height, width), bool)
    for di, (mi, mesh, _) in enumerate([(d.modelInstanceIndex, d.meshIndex, d.materialIndex) for d in f["draw_instances"][:f["draw_instance_count"]]]):
        positions, indices = world.mesh_geometry(mesh)
        md, info = world.metadatas[mesh], world.mesh_infos[mesh]
        built = M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info)
        meshlet_of = np.repeat(np.arange(info.meshletCount), built["meshlets"][:, 3])
        m4 = np.asarray(world.model_instances[mi][1], np.float64).astype(np.float32).astype(np.float64)
        pw = np.concatenate([positions.astype(np.float64), np.ones((len(positions), 1))], axis=1) @ m4.T
        clip = pw @ clip_from_world.T
        assert (clip[:, 3] > 0).all()  # nothing of the scene crosses the eye's plane
        ndc = clip[:, :3] / clip[:, 3:4]
        sx, sy = (ndc[:, 0] * 0.5 + 0.5) * width, (ndc[:, 1] * 0.5 + 0.5) * height
        for t, (a, b, c) in enumerate(indices.reshape(-1, 3).tolist()):
            area = (sx[b] - sx[a]) * (sy[c] - sy[a]) - (sx[c] - sx[a]) * (sy[b] - sy[a])
            if area == 0:
                continue
            w0 = ((sx[b] - px) * (sy[c] - py) - (sx[c] - px) * (sy[b] - py)) / area
            w1 = ((sx[c] - px) * (sy[a] - py) - (sx[a] - px) * (sy[c] - py)) / area
            w2 = 1.0 - w0 - w1
            inside = (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
            if not inside.any():
                continue
            z = w0 * ndc[a, 2] + w1 * ndc[b, 2] + w2 * ndc[c, 2]  # z / w is affine in screen space
            nearer = inside & (z > best)
            second = np.where(nearer, best, np.where(inside & (z > second), z, second))
            best = np.where(nearer, z, best)
            owner[nearer] = (di, meshlet_of[t])
            # Vulkan's y points down: a counter-clockwise triangle in the world has a negative area here
            clear = np.where(nearer, (w0 > margin) & (w1 > margin) & (w2 > margin) & (area < 0), clear)
    counted = clear & (best - second > margin)
    return {tuple(o) for o in owner[counted].tolist()}, best
