#!/usr/bin/env python3
"""The GPU hierarchy build (prosper_pt_build_hierarchy_gpu) beside the host builder, on
S-sponza-class (C3), C4 and the FlightHelmet fixture: device milliseconds per stage (events) and the wall time of the call,
for the linear method and the PLOC method (with its round counts); the host's prosper_pt_rebuild_hierarchy on the same
state with every instance moved, interleaved with them; the frame time at 1920x1080 x 8 spp on one chain under the host
tree, under the linear tree at leaf sizes 1, 2 and 4 and under the PLOC tree at radii 8, 16 and 32 and the same leaf sizes,
interleaved, with the run-to-run spread of every one of them; and the drift scenario of scripts/drift_rebuild_bench.py with
the host builder, the GPU builder and the GPU builder's PLOC method.  One JSON object on stdout
(profiles/f26_ploc_bench.json; profiles/f24_gpu_hierarchy_bench.json is the run before the method axis); run on the GPU box.
With --sites the build sites of DESIGN.md f27 instead (profiles/f27_gpu_build_sites_bench.json): uploads with the first tree
from the host and from the GPU builder, alternating; stage slot 0 of those uploads (the fused launch) beside slot 0 of
synchronous GPU rebuilds of the same scene; and the drift scenario with the re-split as a background GPU generation.

    python scripts/gpu_hierarchy_bench.py [--scenes c3,c4,helmet] [--repeats 5] [--rounds 5] [--no-drift] [--sites]"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, flight_helmet, scenes, structs as S  # noqa: E402
from prosper_amd.rt_reference import Camera  # noqa: E402
from prosper_amd.world import translate  # noqa: E402

hip = ctypes.CDLL("libamdhip64.so")
W, H, SPP = 1920, 1080, 8
FLAGS = S.PC_FLAG_ACCUMULATE | S.PC_FLAG_CLAMP_INDIRECT | S.PC_FLAG_IBL | S.PC_FLAG_SKIP_HISTORY


def moved(base, offset, which=None):
    world = copy.copy(base)
    world._frozen = None
    world.model_instances = list(base.model_instances)
    for i in (range(len(world.model_instances)) if which is None else which):
        model, m = world.model_instances[i]
        world.model_instances[i] = (model, translate(offset) @ m)
    world.freeze()
    return world


def wall_ms(call):
    hip.hipDeviceSynchronize()
    t0 = time.perf_counter()
    call()
    hip.hipDeviceSynchronize()
    return (time.perf_counter() - t0) * 1e3


def frame_ms(ctx, cam, focal, ibl, repeats):
    """(device ms from events, wall ms) of one 8-spp frame: the median of `repeats` after one warm-up."""
    start, stop = ctypes.c_void_p(), ctypes.c_void_p()
    hip.hipEventCreate(ctypes.byref(start))
    hip.hipEventCreate(ctypes.byref(stop))
    pc = S.ReferencePC(0, FLAGS if ibl else FLAGS & ~S.PC_FLAG_IBL, 1, 1e-5, 1.0, focal, 3, 4)
    device, wall = [], []
    for k in range(repeats + 1):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        hip.hipEventRecord(start, None)
        ctx.render(pc, cam, W, H, frames=SPP)
        hip.hipEventRecord(stop, None)
        hip.hipEventSynchronize(stop)
        ms = ctypes.c_float()
        hip.hipEventElapsedTime(ctypes.byref(ms), start, stop)
        if k:
            device.append(ms.value)
            wall.append((time.perf_counter() - t0) * 1e3)
    hip.hipEventDestroy(start)
    hip.hipEventDestroy(stop)
    return statistics.median(device), statistics.median(wall)


PLOC_RADII, LEAF_SIZES = (8, 16, 32), (1, 2, 4)


def select(ctx, tree):
    """`tree` is host, gpu_leafL (the linear method) or ploc_rR_leafL: selects method and leaf size, builds."""
    if tree == "host":
        capi.debug(leafSize=None)
        ctx.rebuild_hierarchy()
        return
    parts = tree.split("_")
    capi.debug(leafSize=int(parts[-1][4:]))
    if parts[0] == "ploc":
        ctx.set_gpu_hierarchy_method(S.GPU_HIERARCHY_PLOC, int(parts[1][1:]))
    else:
        ctx.set_gpu_hierarchy_method(S.GPU_HIERARCHY_LINEAR)
    ctx.build_hierarchy_gpu()


def bench_scene(name, base, repeats, rounds):
    out = {"triangles": base.triangle_count(), "instances": len(base.model_instances)}
    ibl = base.skybox is not None
    cam, focal = Camera.from_world(base, W, H).update_buffer()
    ctx = capi.Context(0, flags=S.CREATE_SINGLE_CHAIN)
    ctx.upload_scene(base)
    out["host_upload_bvh_ms"] = ctx.scene_stats().bvhBuildSeconds * 1e3
    # ---- builds: every instance moved before each one, host and GPU interleaved ----
    poses = [moved(base, (0.01 * (k + 1), 0.0, 0.0)) for k in range(2)]
    methods = {"gpu": (S.GPU_HIERARCHY_LINEAR, 0), "ploc": (S.GPU_HIERARCHY_PLOC, 0)}  # (each with its default leaf size)
    host_wall = []
    gpu = {m: {"wall": [], "total": [], "stages": [], "how": None} for m in methods}
    for k in range(repeats + 1):
        ctx.update_transforms(poses[k % 2])
        ms = wall_ms(ctx.rebuild_hierarchy)
        if k:  # (the first round allocates)
            host_wall.append(ms)
        for i, (m, (method, radius)) in enumerate(methods.items()):
            ctx.update_transforms(poses[(k + 1 + i) % 2])
            ctx.set_gpu_hierarchy_method(method, radius)
            g = wall_ms(ctx.build_hierarchy_gpu)
            info, how = ctx.hierarchy_build_info(), ctx.gpu_hierarchy_method_info()
            if k:
                gpu[m]["wall"].append(g)
                gpu[m]["total"].append(info.totalMs)
                gpu[m]["stages"].append(list(info.stageMs))
                gpu[m]["how"] = {"leafSize": info.leafSize, "radius": how.radius, "rounds": how.rounds,
                                 "rounds_in_one_workgroup": how.finishRounds}
    out["host_rebuild_all_moved_wall_ms"] = {"median": statistics.median(host_wall), "runs": host_wall}
    for m, runs in gpu.items():
        out["%s_build_wall_ms" % m] = {"median": statistics.median(runs["wall"]), "runs": runs["wall"]}
        out["%s_build_device_ms" % m] = {"median": statistics.median(runs["total"]), "runs": runs["total"]}
        out["%s_build_stage_ms" % m] = {n: statistics.median(s[i] for s in runs["stages"]) for i, n in enumerate(S.HIERARCHY_BUILD_STAGE_NAMES)}
        out["%s_build" % m] = runs["how"]
    # ---- frame time under each tree, interleaved; one figure per round (the median of its repeats), the spread between
    #      the rounds is the run-to-run spread of that measurement ----
    ctx.update_transforms(base)
    names = ["host"] + ["gpu_leaf%d" % leaf for leaf in LEAF_SIZES] + \
            ["ploc_r%d_leaf%d" % (radius, leaf) for radius in PLOC_RADII for leaf in LEAF_SIZES]
    frames = {tree: [] for tree in names}
    trees = {}
    for rnd in range(rounds):
        for tree in frames:
            select(ctx, tree)
            info, how = ctx.hierarchy_build_info(), ctx.gpu_hierarchy_method_info()
            trees[tree] = {"nodes": info.nodeCount, "levels": info.levels, "stackBound": info.stackBound, "rounds": how.rounds,
                           "rounds_in_one_workgroup": how.finishRounds}
            frames[tree].append(frame_ms(ctx, cam, focal, ibl, repeats))
    capi.debug(leafSize=None)
    ctx.set_gpu_hierarchy_method(S.GPU_HIERARCHY_LINEAR)
    table = out["frame_1920x1080x8spp_one_chain"] = {
        tree: dict(trees[tree], device_ms=statistics.median(d for d, _ in runs), wall_ms=statistics.median(w for _, w in runs),
                   device_ms_runs=[d for d, _ in runs], spread_ms=max(d for d, _ in runs) - min(d for d, _ in runs))
        for tree, runs in frames.items()}
    host = table["host"]["device_ms"]
    for tree in frames:
        table[tree]["ratio_to_host"] = table[tree]["device_ms"] / host
    # PLOC counts as faster to trace than the linear tree only where its frame is lower by more than the spread of either
    linear = min((t for t in names if t.startswith("gpu_")), key=lambda t: table[t]["device_ms"])
    best = min((t for t in names if t.startswith("ploc_")), key=lambda t: table[t]["device_ms"])
    spread = max(table[linear]["spread_ms"], table[best]["spread_ms"])
    out["ploc_against_linear"] = {
        "best_linear": linear, "best_ploc": best, "linear_ms": table[linear]["device_ms"], "ploc_ms": table[best]["device_ms"],
        "spread_ms": spread, "ratio": table[best]["device_ms"] / table[linear]["device_ms"],
        "ploc_is_faster": table[linear]["device_ms"] - table[best]["device_ms"] > spread}
    ctx.close()
    return out


def spread(runs):
    return max(runs) - min(runs)


def bench_uploads(base, repeats):
    """prosper_pt_upload_scene with the first tree from the host (sites 0: the path as it was) and from the GPU builder
    (site UPLOAD) under both methods, alternating on one context after one warm-up upload each; then, on the same context,
    synchronous GPU rebuilds of the same scene, whose stage slot 0 is lbvh_bounds_kernel's where a sited upload's is the
    fused launch's."""
    variants = {"host": (0, S.GPU_HIERARCHY_LINEAR), "gpu_linear": (S.GPU_BUILD_SITE_UPLOAD, S.GPU_HIERARCHY_LINEAR),
                "gpu_ploc": (S.GPU_BUILD_SITE_UPLOAD, S.GPU_HIERARCHY_PLOC)}
    view = base.view()
    lib = capi.lib()
    ctx = capi.Context(0, flags=S.CREATE_SINGLE_CHAIN)
    runs = {v: {"wall": [], "build": [], "bvh": [], "stages": []} for v in variants}
    for k in range(repeats + 1):
        for v, (sites, method) in variants.items():
            ctx.set_gpu_hierarchy_sites(sites)
            ctx.set_gpu_hierarchy_method(method)
            ms = wall_ms(lambda: capi._check(lib.prosper_pt_upload_scene(ctx._h, ctypes.byref(view))))
            stats, info = ctx.scene_stats(), ctx.hierarchy_build_info()
            assert info.builder == (S.BUILDER_GPU if sites else S.BUILDER_HOST)
            if k:  # (the first upload of each variant allocates; the first of the process is slower still)
                runs[v]["wall"].append(ms)
                runs[v]["build"].append(stats.buildSeconds * 1e3)
                runs[v]["bvh"].append(stats.bvhBuildSeconds * 1e3)
                runs[v]["stages"].append(list(info.stageMs))
    out = {}
    for v, r in runs.items():
        out[v] = {"upload_wall_ms": {"median": statistics.median(r["wall"]), "spread": spread(r["wall"]), "runs": r["wall"]},
                  "buildSeconds_ms": {"median": statistics.median(r["build"]), "spread": spread(r["build"])},
                  "bvhBuildSeconds_ms": {"median": statistics.median(r["bvh"]), "spread": spread(r["bvh"])}}
        if v != "host":
            out[v]["stage_ms"] = {n: statistics.median(st[i] for st in r["stages"]) for i, n in enumerate(S.HIERARCHY_BUILD_STAGE_NAMES)}
            out[v]["fused_launch_ms"] = {"median": statistics.median(st[0] for st in r["stages"]), "spread": spread([st[0] for st in r["stages"]])}
            gap = out["host"]["upload_wall_ms"]["median"] - out[v]["upload_wall_ms"]["median"]
            out[v]["faster_than_host_upload"] = gap > max(out["host"]["upload_wall_ms"]["spread"], out[v]["upload_wall_ms"]["spread"])
            out[v]["upload_wall_ms_saved"] = gap
    # slot 0 of synchronous rebuilds of the same scene in the same run: reset + lbvh_bounds_kernel
    ctx.set_gpu_hierarchy_sites(0)
    ctx.set_gpu_hierarchy_method(S.GPU_HIERARCHY_LINEAR)
    ctx.upload_scene(base)
    slot0 = []
    for k in range(repeats + 1):
        ctx.build_hierarchy_gpu()
        if k:
            slot0.append(ctx.hierarchy_build_info().stageMs[0])
    out["synchronous_rebuild_bounds_stage_ms"] = {"median": statistics.median(slot0), "spread": spread(slot0)}
    ctx.close()
    return out


def drift(builder, steps=240, threshold=1.3, method=S.GPU_HIERARCHY_LINEAR, sites=0):
    """scripts/drift_rebuild_bench.py's loop with `builder` selected: 1-spp frames, three in flight, three instances moved
    every frame.  The measure is read when the host has waited for the device anyway (every third frame).  sites: the GPU
    builder's build sites (DRIFT: the re-split as a background generation from the GPU builder)."""
    base = scenes.sponza_class()
    cam, focal = Camera.from_world(base, W, H).update_buffer()
    ctx = capi.Context(0)
    ctx.upload_scene(base)
    ctx.set_hierarchy_builder(builder)
    ctx.set_gpu_hierarchy_method(method)
    ctx.set_gpu_hierarchy_sites(sites)
    poses = [moved(base, (0.12 * k, 0.016 * k, 0.032 * k), which=(3, 5, 7)) for k in range(steps)]
    times, update_ms, above = [], [], 0
    seen = []  # (frame, geometryInstalls, geometryBuildRunning) wherever the state is read
    t0 = time.perf_counter()
    for k, world in enumerate(poses):
        t1 = time.perf_counter()
        ctx.update_transforms(world)
        update_ms.append((time.perf_counter() - t1) * 1e3)
        ctx.render(S.ReferencePC(0, FLAGS, 1 + k, 1e-5, 1.0, focal, 3, 4), cam, W, H, frames=1, flags=S.RENDER_PIPELINED)
        if k % 3 == 2:
            hip.hipDeviceSynchronize()
            times.append((time.perf_counter() - t0) * 1e3 / 3)
            hs = ctx.hierarchy_state()
            if hs.costRatio > threshold:
                above += 3
            seen.append((k, hs.geometryInstalls, hs.geometryBuildRunning))
            t0 = time.perf_counter()
    hip.hipDeviceSynchronize()
    ctx.finish_mesh_updates()
    hs = ctx.hierarchy_state()
    out = {"frames": steps, "median_frame_ms": statistics.median(times), "worst_frame_ms": max(times),
           "worst_update_call_ms": max(update_ms), "median_update_call_ms": statistics.median(update_ms),
           "frames_above_cost_threshold": above, "rebuilds": hs.rebuilds, "refits": hs.refits,
           "geometryInstalls": hs.geometryInstalls, "cost_ratio_at_end": hs.costRatio}
    # a background generation: the frames from the first reading that saw it running to the first that saw it installed
    # (the state is read every third frame: each figure is exact to three frames; None: it was installed at the end)
    waits, started = [], None
    for (k, installs, running), (_, before, _) in zip(seen[1:], seen):
        if running and started is None:
            started = k
        if installs > before:
            waits.append(k - started if started is not None else 0)
            started = k if running else None
    out["frames_from_trigger_to_install"] = waits
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="c3,c4,helmet")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds over the trees of the frame-time table")
    ap.add_argument("--no-drift", action="store_true")
    ap.add_argument("--sites", action="store_true", help="the build sites (DESIGN.md f27) in place of the builds and frame times")
    args = ap.parse_args()
    make = {"c3": scenes.sponza_class, "c4": lambda: scenes.sponza_class(lights=True, foliage=True),
            "helmet": lambda: flight_helmet.load_fixture()}
    result = {"what": "GPU hierarchy build (linear method, PLOC method) beside the host builder; frames 1920x1080 x 8 spp, one chain, all bounces",
              "scenes": {}}
    if args.sites:
        result["what"] = "GPU builder's build sites: uploads with the first tree from the host / the GPU builder, the fused launch, the drift scenario"
        for name in args.scenes.split(","):
            result["scenes"][name] = dict(bench_uploads(make[name](), args.repeats), triangles=make[name]().triangle_count())
            print("%s done" % name, file=sys.stderr)
        if not args.no_drift:
            rows = {"host_builder": dict(builder=S.BUILDER_HOST), "gpu_builder": dict(builder=S.BUILDER_GPU),
                    "gpu_builder_ploc": dict(builder=S.BUILDER_GPU, method=S.GPU_HIERARCHY_PLOC),
                    "gpu_background_linear": dict(builder=S.BUILDER_HOST, sites=S.GPU_BUILD_SITE_DRIFT),
                    "gpu_background_ploc": dict(builder=S.BUILDER_HOST, sites=S.GPU_BUILD_SITE_DRIFT, method=S.GPU_HIERARCHY_PLOC)}
            result["drift_scenario"] = {row: drift(**how) for row, how in rows.items()}
        print(json.dumps(result, indent=1))
        return
    for name in args.scenes.split(","):
        result["scenes"][name] = bench_scene(name, make[name](), args.repeats, args.rounds)
        print("%s done" % name, file=sys.stderr)
    if not args.no_drift:
        result["drift_scenario"] = {"host_builder": drift(S.BUILDER_HOST), "gpu_builder": drift(S.BUILDER_GPU),
                                    "gpu_builder_ploc": drift(S.BUILDER_GPU, method=S.GPU_HIERARCHY_PLOC)}
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
