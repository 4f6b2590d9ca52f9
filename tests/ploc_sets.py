"""Triangle sets for the PLOC tests (tests/test_ploc_cpu.py, tests/test_gpu_hierarchy_ploc.py): the linear tests' sets
(tests/lbvh_sets.py), three more sizes, and the sizes around the cluster count T from which the GPU build finishes in one
workgroup: T (no round outside that launch), T + 1 (one) and 2 T + 1 (several); and the nested comb, whose PLOC tree sits
on the traversal's stack limit or is refused (tests/test_gpu_hierarchy_refusal.py)."""
import numpy as np

import lbvh_sets
from prosper_amd import ploc

T = ploc.SINGLE_WORKGROUP_CLUSTERS
# the sizes of the nested comb around the stack limit (lbvh.MAX_STACK_BOUND = 96): with the PLOC method and one triangle
# per leaf the stack bound of nested_comb(n) is n
COMB_SIZES = (96, 97, 101)
COMB_MESH = np.float32([[-1.0, 0.0, 0.0625], [1.0, 0.0625, 0.0625], [0.0, 0.0625, 0.0625]])


def comb_scales(n):
    return np.exp2(np.arange(n, dtype=np.float64) - n // 2)


def nested_comb(n):
    """n triangles (-s, 0, s/16), (s, 1/16, s/16), (0, 1/16, s/16), s = 2^(k - n // 2): every box contains the smaller
    ones in x and y, every triangle lies in its own plane z = s/16 (closest hits are unique), every value is exact in
    fp32.  Clustering merges the two smallest, then their union with the next one, and so on: a comb of depth n - 1."""
    s = comb_scales(n)[:, None, None]
    return (COMB_MESH[None].astype(np.float64) * np.concatenate([s, np.ones_like(s), s], axis=2)).astype(np.float32)


def comb_world(n, extra_quad=False):
    """nested_comb(n) as a scene: one mesh of binary16 vertices (COMB_MESH) and n instances of one model, instance k scaled
    (s, 1, s) - the flatten kernel writes exactly nested_comb(n), in this order.  extra_quad: an ordinary mesh of its own
    model ahead of the comb (mesh 0, instance 0; the comb is mesh 1).  The camera looks along +z at the comb's axis x = 0
    from a height where the ray through the axis pierces every triangle and every box; the near plane lies in front of the
    smallest triangles' planes (the path tracer's rays start at the eye and are not clipped by it anyway)."""
    from prosper_amd.world import World, scale
    world = World()
    material = world.add_material(base_color=(0.8, 0.7, 0.6, 1.0))
    if extra_quad:
        quad = np.float32([[-0.03125, 0.0625, 0.25], [0.03125, 0.0625, 0.25], [0.03125, 0.078125, 0.25], [-0.03125, 0.078125, 0.25]])
        mesh = world.add_mesh(quad, np.uint32([0, 1, 2, 0, 2, 3]), material, normals=np.float32([[0.0, 0.0, -1.0]] * 4))
        world.add_instance(world.add_model([(mesh, material)]))
    # (normals towards the eye and the light: without any a hit shades to nothing)
    mesh = world.add_mesh(COMB_MESH, np.arange(3, dtype=np.uint32), material, normals=np.float32([[0.0, 0.0, -1.0]] * 3))
    model = world.add_model([(mesh, material)])
    for s in comb_scales(n):
        world.add_instance(model, scale((s, 1.0, s)))
    world.set_directional_light((1.0, 1.0, 1.0), 3.0, (0.125, -0.25, 1.0))  # from -z, a little from above
    world.camera = dict(eye=(0.0, 0.046875, -0.25), target=(0.0, 0.046875, 1.0), up=(0.0, 1.0, 0.0), fov=0.2,
                        zN=2.0 ** -6, zF=2.0 ** 20)
    return world


def sets():
    out = dict(lbvh_sets.sets())
    for n in (3, 513, 1025):
        out["n%d" % n] = lbvh_sets._random(n, seed=n)
    for name, n in (("t", T), ("t_plus_1", T + 1), ("two_t_plus_1", 2 * T + 1)):
        out[name] = lbvh_sets._random(n, seed=9000 + n)
    return out
