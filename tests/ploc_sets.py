"""Triangle sets for the PLOC tests (tests/test_ploc_cpu.py, tests/test_gpu_hierarchy_ploc.py): the linear tests' sets
(tests/lbvh_sets.py), three more sizes, and the sizes around the cluster count T from which the GPU build finishes in one
workgroup: T (no round outside that launch), T + 1 (one) and 2 T + 1 (several)."""
import lbvh_sets
from prosper_amd import ploc

T = ploc.SINGLE_WORKGROUP_CLUSTERS


def sets():
    out = dict(lbvh_sets.sets())
    for n in (3, 513, 1025):
        out["n%d" % n] = lbvh_sets._random(n, seed=n)
    for name, n in (("t", T), ("t_plus_1", T + 1), ("two_t_plus_1", 2 * T + 1)):
        out[name] = lbvh_sets._random(n, seed=9000 + n)
    return out
