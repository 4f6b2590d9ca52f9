#!/usr/bin/env python3
"""The forward opaque pass at 1920x1080 on S-cornell (C2's scene), sponza_class (C3), sponza_class with
the sun, 1024 punctual lights and foliage (C4) and the FlightHelmet fixture, each with meshlets added (World.add_meshlets).

Per scene and for ibl 0 and 1, in steady state (the second frame on, so that the first phase has the previous frame's
pyramid), between two events on the stream, alternating in one process:
  `raster_forward_ms`     the whole prosper_pt_raster_forward (both culling phases, both draws, the pyramids, the shade);
  `forward_shade_ms`      prosper_pt_raster_forward_shade alone over the image as drawn (the lists of the last clustering
                          serve), and `forward_kernel_ms`, the device time of its kernel between the library's own events
                          (prosper_pt_get_forward_opaque_info);
  `raster_deferred_ms`    the yardstick: prosper_pt_raster_gbuffer + prosper_pt_deferred_shading over its targets;
  `resolve_shading_ms`    the yardstick's two passes after the draws: prosper_pt_raster_resolve + prosper_pt_deferred_shading
                          (which clusters the lights on every call; `cluster_ms` is prosper_pt_cluster_lights alone).
`ratio` = forward_shade_ms / (resolve_shading_ms - cluster_ms): the shade against what it replaces.  Every figure is the
median over `--repeats` samples after three of warm-up.  A scene the rasteriser refuses is reported with the refusal.
Prints ONE JSON object and writes it to --out (default profiles/f19_forward_opaque_bench.json).

    python scripts/forward_opaque_bench.py [--repeats 20] [--scenes c2,c3,c4,fh] [--out FILE]
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
        host.close()

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        try:
            ctx.raster_visibility(cam, stream=st)
        except capi.ProsperPtError as e:
            out["refused"] = str(e)
            return out
        ctx.generate_ibl(stream=st)
        lib = capi.lib()
        gdesc, fdesc = S.VelocityGBufferDesc(), S.ForwardOpaqueDesc()  # context-owned targets

        def shading(ibl):
            g, _, _ = ctx.gbuffer_device_ptrs()
            ctx.deferred_shading_device(cam, WIDTH, HEIGHT, g.albedoRoughness, g.normalMetallic, g.nonLinearDepth, ibl=ibl, stream=st)

        def raster_deferred(ibl):
            capi._check(lib.prosper_pt_raster_gbuffer(ctx._h, 0, C.byref(cam), C.byref(gdesc), C.c_void_p(st)))
            shading(ibl)

        def resolve_shading(ibl):
            capi._check(lib.prosper_pt_raster_resolve(ctx._h, 0, C.byref(cam), C.byref(gdesc), C.c_void_p(st)))
            shading(ibl)

        def forward(entry, ibl):
            pc = S.ForwardPC(0, ibl, 0)
            capi._check(entry(ctx._h, C.byref(pc), C.byref(cam), C.byref(fdesc), C.c_void_p(st)))

        for ibl in (0, 1):
            keys = ("raster_forward_ms", "forward_shade_ms", "forward_kernel_ms", "raster_deferred_ms", "resolve_shading_ms", "cluster_ms")
            samples = {k: [] for k in keys}
            for i in range(repeats + 3):
                t = {}
                t["raster_forward_ms"] = timed(lambda: forward(lib.prosper_pt_raster_forward, ibl))
                t["forward_shade_ms"] = timed(lambda: forward(lib.prosper_pt_raster_forward_shade, ibl))
                info = ctx.forward_opaque_info()  # (the events above were waited for: it has landed)
                t["forward_kernel_ms"] = info.shadeMs
                t["raster_deferred_ms"] = timed(lambda: raster_deferred(ibl))
                t["resolve_shading_ms"] = timed(lambda: resolve_shading(ibl))
                t["cluster_ms"] = timed(lambda: ctx.cluster_lights(cam, WIDTH, HEIGHT, stream=st))
                if i >= 3:
                    for k in keys:
                        samples[k].append(t[k])
            r = {k: float(np.median(v)) for k, v in samples.items()}
            r["shaded_pixels"] = int(info.shadedPixels)
            r["ratio"] = r["forward_shade_ms"] / max(r["resolve_shading_ms"] - r["cluster_ms"], 1e-6)
            out["ibl_%d" % ibl] = r
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="c2,c3,c4,fh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f19_forward_opaque_bench.json"))
    args = ap.parse_args()
    import torch
    results = []
    for k in args.scenes.split(","):
        results.append(bench_scene(torch, k, args.repeats))
        print("%s done" % SCENES[k][0], file=sys.stderr, flush=True)
    text = json.dumps({"bench": "forward_opaque", "device": torch.cuda.get_device_name(0),
                       "stages": ["raster_forward", "forward shade", "raster_gbuffer + deferred shading", "resolve + deferred shading"],
                       "scenes": results})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
