"""Triangle sets for the linear-BVH tests (tests/test_lbvh_cpu.py, tests/test_gpu_hierarchy.py): (n, 3, 3) float32
vertices, made once.  Every coordinate is a binary16 value so that a scene made of a set holds exactly these triangles."""
import numpy as np


def _half(v):
    return np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


def _around(centroids, size=0.0625, seed=1):
    """One small triangle around every centroid (the box centre is the centroid up to rounding)."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centroids, np.float32).reshape(-1, 1, 3)
    offsets = rng.uniform(-size, size, (len(c), 3, 3)).astype(np.float32)
    return _half(c + offsets)


def _random(n, seed):
    rng = np.random.default_rng(seed)
    return _around(rng.uniform(-4.0, 4.0, (n, 3)), seed=seed + 100)


def _identical(n):
    one = _half([[0.5, 0.25, -1.0], [1.5, 0.25, -1.0], [0.5, 1.25, -2.0]])
    return np.repeat(one[None], n, axis=0)


def _degenerate(kind, n=97, seed=7):
    """All centroids on a line / in a plane / in one point: congruent triangles moved by exactly representable steps."""
    rng = np.random.default_rng(seed)
    one = _half([[0.0, 0.0, 0.0], [0.25, 0.0, 0.125], [0.0, 0.25, 0.125]])
    steps = np.zeros((n, 3), np.float32)
    if kind in ("line", "plane"):
        steps[:, 0] = rng.integers(0, 64, n) * 0.125
    if kind == "plane":
        steps[:, 2] = rng.integers(0, 64, n) * 0.125
    return _half(one[None] + steps[:, None, :])


def _spread(n=120, seed=11):
    """Coordinates from 2^-20 to 2^10 (binary16 holds 2^-24 .. 65504)."""
    rng = np.random.default_rng(seed)
    magnitude = np.exp2(rng.uniform(-20.0, 10.0, (n, 1, 3))).astype(np.float32)
    sign = rng.choice(np.array([-1.0, 1.0], np.float32), (n, 1, 3))
    jitter = rng.uniform(0.75, 1.25, (n, 3, 3)).astype(np.float32)
    return _half(magnitude * sign * jitter)


def _soup(n=3000, seed=23):
    """Clusters of small triangles, a few large ones across them, some exact duplicates."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-8.0, 8.0, (12, 3))
    c = centres[rng.integers(0, 12, n)] + rng.normal(0.0, 0.5, (n, 3))
    v = _around(c, size=0.05, seed=seed + 1)
    big = rng.choice(n, 20, replace=False)
    v[big] = _around(c[big], size=6.0, seed=seed + 2)
    copies = rng.choice(n, 60, replace=False)
    v[copies] = v[(copies + 1) % n]
    return v


def deep_comb(copies=512):
    """The deepest tree a few hundred triangles give: one centroid per code bit, on the three axes in geometric sequence
    (cell 2^k of one axis, 0 of the others), so that every split of the radix tree takes one triangle off; the two
    triangles that fix the centroid bounds at cells 0 and 2^21 - 1; and `copies` identical triangles in cell 0, whose
    balanced subtree hangs below the last split.  Coordinates are cells * 2^-6 +- 2^-7, exact in fp32 (NOT in
    binary16: this set is for the statement and for flat triangles given as they are)."""
    cells = [(0, 0, 0)] * copies + [((1 << 21) - 1,) * 3]
    for k in range(21):
        for axis in range(3):
            cell = [0, 0, 0]
            cell[axis] = 1 << k
            cells.append(tuple(cell))
    c = np.array(cells, np.float64) * 2.0 ** -6
    d = 2.0 ** -7
    one = np.array([[-d, -d, 0.0], [d, -d, 0.0], [0.0, d, 0.0]])  # its box is centred on the centroid
    return (c[:, None, :] + one[None]).astype(np.float32)


def sets():
    out = {"n%d" % n: _random(n, seed=n) for n in (0, 1, 2, 4, 5, 64, 65, 257)}
    out["identical9"] = _identical(9)
    out["identical70"] = _identical(70)
    for kind in ("line", "plane", "point"):
        out[kind] = _degenerate(kind)
    out["spread"] = _spread()
    out["soup"] = _soup()
    return out


def world_of(vertices):
    """A one-instance scene that holds exactly these triangles, in this order."""
    from prosper_amd.world import World
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    world = World()
    material = world.add_material(base_color=(0.8, 0.7, 0.6, 1.0))
    if len(v):  # (no triangles: no geometry at all)
        mesh = world.add_mesh(v, np.arange(len(v), dtype=np.uint32), material)
        world.add_instance(world.add_model([(mesh, material)]))
    world.set_directional_light((1.0, 1.0, 1.0), 3.0, (-0.3, -1.0, -0.2))
    lo, hi = (v.min(axis=0), v.max(axis=0)) if len(v) else (np.zeros(3), np.ones(3))
    centre, reach = 0.5 * (lo + hi), float(np.max(hi - lo)) + 1.0
    world.camera = dict(eye=tuple(centre + np.array([0.3, 0.4, 1.0]) * reach), target=tuple(centre), up=(0.0, 1.0, 0.0),
                        fov=0.9, zN=0.01 * reach, zF=10.0 * reach)
    return world
