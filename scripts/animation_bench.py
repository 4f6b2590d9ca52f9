#!/usr/bin/env python3
"""What a frame's animation update costs on one MI355X: prints one JSON object.

The animated fixture (tests/golden/animated_scene.gltf) scaled to 1 000 and 10 000 nodes in chains of depth 8 - every
second level animated by two of the fixture's channels, the leaf carrying one of its meshes - and per size

  sample_ms, hierarchy_ms    the two animation kernels alone, between events on the stream (medians)
  animate_refit_ms           prosper_pt_animate(PROSPER_PT_UPDATE_NOW) to an idle device: the kernels, the world triangles
                             and the refit (host clock around the call and a device synchronise)
  parent_numpy_ms            the path a caller had before: the NumPy restatement (tests/animation_reference.py) of both
                             kernels on the host ...
  parent_update_refit_ms     ... and prosper_pt_update_transforms_async(PROSPER_PT_UPDATE_NOW) of its table, to an idle device

    python scripts/animation_bench.py [--out profiles/f15_animation_bench.json] [--sizes 1000,10000]
"""
import argparse
import copy
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

DEPTH = 8


def scaled_scene(fixture, node_count):
    """(world, tables): node_count // DEPTH chains on a grid, one mesh instance at the end of each."""
    import animation_reference as R
    from prosper_amd import animation, gltf, structs as S
    from prosper_amd.world import translate
    base_world, base = gltf.load_gltf(fixture), animation.load_animations(fixture)
    usable = [c for c in base.channels if float(np.abs(R.channel_values(base, c)).max()) < 5.0]  # (without the decoy)
    chains = node_count // DEPTH
    side = int(np.ceil(np.sqrt(chains)))
    world = copy.copy(base_world)
    world._frozen = None
    world.model_instances = []
    nodes, channels = [], []
    for c in range(chains):
        world.add_instance(c % len(base_world.models), translate((3.0 * (c % side), 0.0, 3.0 * (c // side))))
        for level in range(DEPTH):
            n = S.AnimationNode()
            n.parent = S.ANIMATION_NONE if level == 0 else len(nodes) - 1
            n.modelInstance = c if level == DEPTH - 1 else S.ANIMATION_NONE
            n.pointLight = n.spotLight = S.ANIMATION_NONE
            n.translation[:] = (3.0 * (c % side), 0.0, 3.0 * (c // side)) if level == 0 else (0.125, 0.0625 * level, 0.0)
            n.rotation[:] = (0.0, float(np.float32(np.sin(0.15))), 0.0, float(np.float32(np.cos(0.15))))
            n.scale[:] = (1.0, 1.25, 0.75) if level == 1 else (1.0, 1.0, 1.0)
            n.flags = S.NODE_HAS_TRANSLATION | (S.NODE_HAS_ROTATION if level % 2 else 0) | (S.NODE_HAS_SCALE if level == 1 else 0)
            if level % 2 == 0:
                k = (c * (DEPTH // 2) + level // 2) * 2
                for source in (usable[k % len(usable)], usable[(k + 1) % len(usable)]):
                    ch = S.AnimationChannel.from_buffer_copy(source)  # (the fixture's key times and values, shared)
                    ch.node = len(nodes)
                    channels.append(ch)
            nodes.append(n)
    return world, animation.AnimationTables(nodes, channels, base.times, base.values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--parent-iterations", type=int, default=3)
    args = ap.parse_args()
    import animation_reference as R
    from prosper_amd import capi, structs as S
    hip = C.CDLL("libamdhip64.so")  # the runtime the library already uses
    fixture = os.path.join(ROOT, "tests", "golden", "animated_scene.gltf")
    ctx = capi.Context(0)
    result = {"fixture": "tests/golden/animated_scene.gltf", "chainDepth": DEPTH, "iterations": args.iterations,
              "parentIterations": args.parent_iterations, "sizes": []}
    for node_count in (int(v) for v in args.sizes.split(",")):
        world, tables = scaled_scene(fixture, node_count)
        n = len(world.model_instances)
        ctx.upload_scene(world)
        ctx.set_animations(tables)
        end = tables.end_time
        for k in range(3):  # (code objects, the second and third scene version, the pinned read-back)
            ctx.animate(0.1 * (k + 1), now=True)
        assert hip.hipDeviceSynchronize() == 0
        sample, hierarchy, whole = [], [], []
        for k in range(args.iterations):
            t = (0.037 * (k + 1)) % end
            t0 = time.perf_counter()
            ctx.animate(t, now=True)
            assert hip.hipDeviceSynchronize() == 0
            whole.append((time.perf_counter() - t0) * 1e3)
            st = ctx.animation_state()
            sample.append(st.sampleMs)
            hierarchy.append(st.hierarchyMs)
        levels = ctx.hierarchy_state().levels
        base_table = np.frombuffer(world.freeze()["transforms"], np.float32).reshape(-1, 2, 3, 4)[:n].copy()
        none4, none24 = np.zeros(4, np.float32), np.zeros((1, 2, 4), np.float32)
        host, update = [], []
        for k in range(args.parent_iterations):
            t = (0.211 * (k + 1)) % end
            t0 = time.perf_counter()
            table = R.outputs(tables, R.hierarchy(tables, R.evaluate_trs(tables, t)), base_table, none4, none4[None], none24)[0]
            staged = (S.ModelInstanceTransforms * n)()
            C.memmove(staged, np.ascontiguousarray(table).ctypes.data, table.nbytes)
            host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            capi._check(capi.lib().prosper_pt_update_transforms_async(ctx._h, C.cast(staged, C.c_void_p), n, S.UPDATE_NOW, None))
            assert hip.hipDeviceSynchronize() == 0
            update.append((time.perf_counter() - t0) * 1e3)
        result["sizes"].append({
            "nodes": len(tables.nodes), "chains": n, "modelInstances": n, "triangles": int(ctx.scene_stats().triangleCount),
            "targets": len(R.resolve_targets(tables)), "refitLaunches": int(levels) + 1,
            "sample_ms": round(statistics.median(sample), 4), "hierarchy_ms": round(statistics.median(hierarchy), 4),
            "animate_refit_ms": round(statistics.median(whole), 4), "animate_refit_ms_min": round(min(whole), 4),
            "parent_numpy_ms": round(statistics.median(host), 2),
            "parent_update_refit_ms": round(statistics.median(update), 4)})
    ctx.close()
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
