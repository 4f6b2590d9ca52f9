#!/usr/bin/env python3
"""The visibility system's stages on S-cornell (C2's scene), sponza_class (C3), sponza_class with the sun,
1024 punctual lights and foliage (C4) and the FlightHelmet fixture, each with meshlets added (World.add_meshlets).

The pyramid (prosper_pt_hiz_downsample) at 1920x1080 and at 3840x2160 over the pixel-centre traced G-buffer's depth of the
same context: a sample is the device time between two events around `--batch` back-to-back calls on one stream, divided by
the batch (one call is a few microseconds, the order of an event's own resolution).  `GBps` counts the depth read once and
every level of the pyramid (which covers bit_ceil(extent)) written once.

The culling stages at 1920x1080: the generator, the first-phase culler and the second-phase culler are the device times
between the events the library records around their kernels (prosper_pt_get_cull_stage_ms), of a first phase against the
previous frame's pyramid and a second phase against this frame's; `cull_gbuffer_us` is the whole prosper_pt_cull_gbuffer
- first phase, pyramid, second phase - on the second of two frames (the first leaves the pyramid it culls against),
between two events on the stream.  `meshlets` reports the counts in (generated), drawn by each phase and occluded after
the first.  Every figure is the median over `--repeats` samples after warm-up, the pyramid's with the 10th and 90th
percentile beside it; `gbuffer_ms` of the same run is the yardstick.  Prints one JSON object.

    python scripts/culling_bench.py [--repeats 20] [--batch 20] [--scenes c2,c3,c4,fh]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, flight_helmet, scenes, structs as S  # noqa: E402
from prosper_amd.rt_reference import Camera  # noqa: E402

SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell(with_skybox=True)),
    "c3": ("sponza_class", lambda: scenes.sponza_class()),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}
SIZES = ((1920, 1080), (3840, 2160))


def bench_scene(torch, key, repeats, batch):
    name, make = SCENES[key]
    world = make()
    meshlets = world.add_meshlets()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        st = torch.cuda.current_stream().cuda_stream
        out = {"scene": name, "repeats": repeats, "batch": batch, "meshlets_built": meshlets, "sizes": {}}
        for width, height in SIZES:
            cam, _ = Camera.from_world(world, width, height).update_buffer()

            def trace():
                # (Context.trace_gbuffer would read the targets back; the entry itself only enqueues)
                capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, 0, C.byref(cam), width, height, None, C.c_void_p(st)))

            def timed(fn, calls):
                samples = []
                for i in range(repeats + 3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        fn()
                    b.record()
                    b.synchronize()
                    if i >= 3:
                        samples.append(a.elapsed_time(b) / calls)
                return [float(np.percentile(samples, q)) for q in (50, 10, 90)]

            gbuffer_ms = timed(trace, 1)[0]
            us = [1000.0 * v for v in timed(lambda: ctx.hiz_downsample(width, height, slot=0, stream=st), batch)]
            info = ctx.hiz_info(0)
            depth = ctx.read_gbuffer()[2]
            # the depth read once and every level of the pyramid written once; the pyramid covers bit_ceil(extent)
            levels = [ctx.hiz_device_ptr(0, l)[1:] for l in range(info.levelCount)]
            nbytes = 4 * (width * height + sum(lw * lh for lw, lh in levels))
            out["sizes"]["%dx%d" % (width, height)] = {
                "levels": info.levelCount, "launches": info.launches, "miss_share": float((depth == 0).mean()),
                "hiz_downsample_us": {"median": us[0], "p10": us[1], "p90": us[2]},
                "hiz_downsample_GBps": nbytes / (us[0] * 1e-6) / 1e9, "gbuffer_ms": gbuffer_ms,
                "farthest_depth": float(ctx.read_hiz_level(0, info.levelCount - 1)[0, 0]),
            }
        out["culling_1920x1080"] = bench_culling(torch, ctx, world, repeats, st)
        return out
    finally:
        ctx.close()


def bench_culling(torch, ctx, world, repeats, st, width=1920, height=1080):
    cam, _ = Camera.from_world(world, width, height).update_buffer()

    def trace():
        capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, 0, C.byref(cam), width, height, None, C.c_void_p(st)))

    trace()
    ctx.hiz_downsample(width, height, slot=0, stream=st)  # the previous frame's pyramid: the same view
    ctx.hiz_downsample(width, height, slot=1, stream=st)
    stages = {"generator": [], "first_phase_culler": [], "second_phase_culler": []}
    for i in range(repeats + 3):
        ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, hiz_slot=0, stream=st)
        ctx.cull_second_phase(cam, 1, stream=st)
        ms = ctx.cull_stage_ms()
        if i >= 3:
            for k, v in zip(stages, ms):
                stages[k].append(1000.0 * v)
    counts = {}
    for key, which in (("in", S.DRAW_LIST_GENERATED), ("drawn_first_phase", S.DRAW_LIST_FIRST_PHASE),
                       ("occluded_after_first_phase", S.DRAW_LIST_SECOND_PHASE_INPUT), ("drawn_second_phase", S.DRAW_LIST_SECOND_PHASE)):
        n = C.c_uint32()
        capi._check(capi.lib().prosper_pt_read_draw_list(ctx._h, which, C.byref(n), None, 0, None, C.c_void_p(st)))
        counts[key] = n.value
    stats = ctx.draw_stats()
    counts["drawn"] = stats.drawnMeshletCount
    counts["rasterized_triangles"], counts["total_triangles"] = stats.rasterizedTriangleCount, stats.totalTriangleCount
    # the whole sequence on the second of two frames
    whole = []
    for i in range(repeats + 3):
        trace()
        ctx.cull_gbuffer(cam, stream=st)  # (the frame before: leaves the pyramid)
        trace()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.cull_gbuffer(cam, stream=st)
        b.record()
        b.synchronize()
        if i >= 3:
            whole.append(1000.0 * a.elapsed_time(b))
    after = ctx.draw_stats()
    return {"stage_us": {k: float(np.median(v)) for k, v in stages.items()}, "cull_gbuffer_us": float(np.median(whole)),
            "meshlets": counts, "cull_gbuffer_drawn": after.drawnMeshletCount}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--scenes", default="c2,c3,c4,fh")
    args = ap.parse_args()
    import torch
    results = [bench_scene(torch, k, args.repeats, args.batch) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "culling", "device": torch.cuda.get_device_name(0), "stages": ["hiz_downsample", "generator", "first_phase_culler", "second_phase_culler", "cull_gbuffer"], "scenes": results}))


if __name__ == "__main__":
    main()
