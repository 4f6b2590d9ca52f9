#!/usr/bin/env python3
"""The rasteriser over the meshlet draw lists at 1920x1080 on S-cornell (C2's scene), sponza_class (C3),
sponza_class with the sun, 1024 punctual lights and foliage (C4) and the FlightHelmet fixture, each with meshlets added
(World.add_meshlets).

Per scene, in steady state (the second frame on, so that the first phase has the previous frame's pyramid):
  `raster_gbuffer_ms`  the whole prosper_pt_raster_gbuffer (the sequence below, then the resolve), `resolve_ms` the resolve alone
                   (prosper_pt_raster_resolve into the context's targets), between two events on the stream;
  `visibility_ms`  the whole prosper_pt_raster_visibility - both culling phases, both draws, the depth and its pyramids -
                   between two events on the stream, with a static camera and with a camera that steps sideways;
  `stage_ms`       the device time of the meshlet kernel and of the tile pass of each of the two draws, between the events
                   the library records around them (prosper_pt_get_raster_info);
  `unculled_ms`    first phase + one cleared draw of the GENERATED list, and that draw's two kernels;
  `gbuffer_ms`     prosper_pt_trace_gbuffer with PROSPER_PT_GBUFFER_OPAQUE_ONLY, alternating with the above in the same process:
                   the yardstick.
Every figure is the median over `--repeats` samples after three of warm-up.  A scene the rasteriser refuses is reported with
the refusal.  Prints ONE JSON object.

    python scripts/raster_gbuffer_bench.py [--repeats 20] [--scenes c2,c3,c4,fh]
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
WIDTH, HEIGHT = 1920, 1080
OPAQUE_ONLY = 1 << 2
COUNTS = ("triangles", "culledBackface", "culledZeroArea", "culledOutside", "clipped", "queued", "fragments", "queueOverflow")


def draw_of(d):
    return None if not d.valid else dict({k: getattr(d, k) for k in COUNTS}, meshlets_ms=d.meshletsMs, large_ms=d.largeMs)


def bench_scene(torch, key, repeats):
    name, make = SCENES[key]
    world = make()
    meshlets = world.add_meshlets()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        st = torch.cuda.current_stream().cuda_stream
        out = {"scene": name, "repeats": repeats, "meshlets_built": meshlets, "extent": [WIDTH, HEIGHT]}
        host = Camera.from_world(world, WIDTH, HEIGHT)
        cam, _ = host.update_buffer()

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        def trace():
            capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, OPAQUE_ONLY, C.byref(cam), WIDTH, HEIGHT, None, C.c_void_p(st)))

        def unculled():
            ctx.cull_first_phase(cam, S.CULL_MODE_OPAQUE, stream=st)
            ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True, stream=st)

        try:
            ctx.raster_visibility(cam, stream=st)
        except capi.ProsperPtError as e:
            out["refused"] = str(e)
            out["gbuffer_ms"] = float(np.median([timed(trace) for _ in range(repeats + 3)][3:]))
            return out
        desc = S.VelocityGBufferDesc()  # context-owned targets

        def raster_gbuffer():
            capi._check(capi.lib().prosper_pt_raster_gbuffer(ctx._h, 0, C.byref(cam), C.byref(desc), C.c_void_p(st)))

        def resolve():
            capi._check(capi.lib().prosper_pt_raster_resolve(ctx._h, 0, C.byref(cam), C.byref(desc), C.c_void_p(st)))

        samples = {"static": [], "gbuffer": [], "unculled": [], "raster_gbuffer": [], "resolve": []}
        stages = {"first_meshlets": [], "first_large": [], "second_meshlets": [], "second_large": [], "unculled_meshlets": [], "unculled_large": []}
        for i in range(repeats + 3):
            t_vis = timed(lambda: ctx.raster_visibility(cam, stream=st))
            info = ctx.raster_info()
            t_resolve = timed(resolve)
            t_whole = timed(raster_gbuffer)
            t_trace = timed(trace)
            t_un = timed(unculled)
            un = ctx.raster_info()
            ctx.raster_visibility(cam, stream=st)  # (the unculled draw replaced the lists; the kept pyramid stands)
            if i >= 3:
                samples["static"].append(t_vis)
                samples["gbuffer"].append(t_trace)
                samples["raster_gbuffer"].append(t_whole)
                samples["resolve"].append(t_resolve)
                samples["unculled"].append(t_un)
                for k, d in (("first", info.draw[0]), ("second", info.draw[1])):
                    stages[k + "_meshlets"].append(d.meshletsMs)
                    stages[k + "_large"].append(d.largeMs)
                stages["unculled_meshlets"].append(un.draw[0].meshletsMs)
                stages["unculled_large"].append(un.draw[0].largeMs)
        out["visibility_ms"] = {"static": float(np.median(samples["static"]))}
        out["gbuffer_ms"] = float(np.median(samples["gbuffer"]))
        out["raster_gbuffer_ms"] = float(np.median(samples["raster_gbuffer"]))
        out["resolve_ms"] = float(np.median(samples["resolve"]))
        out["unculled_ms"] = float(np.median(samples["unculled"]))
        out["stage_ms"] = {k: float(np.median(v)) for k, v in stages.items()}
        out["static_draws"] = [draw_of(info.draw[0]), draw_of(info.draw[1])]
        out["unculled_draw"] = draw_of(un.draw[0])
        stats = ctx.draw_stats()
        out["drawn_meshlets"], out["total_meshlets"] = stats.drawnMeshletCount, stats.totalMeshletCount
        # a camera that steps sideways by 1 % of the scene's distance every frame
        eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z])
        right = np.array([cam.cameraToWorld.col[0].x, cam.cameraToWorld.col[0].y, cam.cameraToWorld.col[0].z])
        fwd = -np.array([cam.cameraToWorld.col[2].x, cam.cameraToWorld.col[2].y, cam.cameraToWorld.col[2].z])
        step, moving, second = 0.01 * max(float(np.linalg.norm(eye)), 1.0), [], []
        for i in range(repeats + 3):
            e = eye + right * step * (i + 1)
            host.look_at(tuple(e), tuple(e + fwd), (0.0, 1.0, 0.0))
            moved, _ = host.update_buffer()
            t = timed(lambda: ctx.raster_visibility(moved, stream=st))
            if i >= 3:
                moving.append(t)
                second.append(ctx.read_draw_list(S.DRAW_LIST_SECOND_PHASE, stream=st)[0].shape[0])
        out["visibility_ms"]["camera_step"] = float(np.median(moving))
        out["second_phase_meshlets_camera_step"] = float(np.median(second))
        host.close()
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="c2,c3,c4,fh")
    args = ap.parse_args()
    import torch
    results = [bench_scene(torch, k, args.repeats) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "raster_gbuffer", "device": torch.cuda.get_device_name(0),
                      "stages": ["raster_visibility", "meshlets kernel", "tile pass", "unculled draw", "traced gbuffer"], "scenes": results}))


if __name__ == "__main__":
    main()
