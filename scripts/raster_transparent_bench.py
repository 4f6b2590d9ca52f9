#!/usr/bin/env python3
"""The rasterised transparent pass at 1920x1080 on S-cornell (C2's scene), sponza_class with the sun, 1024
punctual lights and foliage (C4) and the FlightHelmet fixture, each with meshlets added (World.add_meshlets), beside the
traced pass over the same depth in the same process, alternating.

Per scene, over the depth of a steady-state prosper_pt_raster_forward frame, between two events on the stream:
  `raster_call_ms`   the whole prosper_pt_raster_forward_transparent: the TRANSPARENT first phase, count, scan, the host's
                     wait for the total, fill, the resolve;
  `count_ms`, `scan_ms`, `fill_ms`, `resolve_ms`   its stages between the library's own events
                     (prosper_pt_get_raster_transparent_info), and `kernels_ms` their sum;
  `host_wait_ms`     raster_call_ms - kernels_ms: the culling phase and what the stream idles while the host reads the total
                     and grows the buffer;
  `traced_ms`        the yardstick: prosper_pt_forward_transparent over the same depth and image, its device time
                     (prosper_pt_get_transparent_info).
`ratio` = raster_call_ms / traced_ms, `kernel_ratio` = kernels_ms / traced_ms.  Every figure is the median over `--repeats`
samples after three of warm-up; both passes work in place, so each sample blends over the previous one's image (the work
does not depend on the image).  Prints ONE JSON object and writes it to --out (default
profiles/f20_raster_transparent_bench.json).

    python scripts/raster_transparent_bench.py [--repeats 10] [--scenes c2,c4,fh] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, flight_helmet, scenes  # noqa: E402
from prosper_amd.rt_reference import Camera  # noqa: E402

SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell(with_skybox=True)),
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
            for _ in range(2):  # the second frame has the first one's pyramid
                ctx.raster_forward(cam, stream=st)
        except capi.ProsperPtError as e:
            out["refused"] = str(e)
            return out
        keys = ("raster_call_ms", "count_ms", "scan_ms", "fill_ms", "resolve_ms", "kernels_ms", "host_wait_ms", "traced_ms")
        samples = {k: [] for k in keys}
        for i in range(repeats + 3):
            t = {}
            t["raster_call_ms"] = timed(lambda: ctx.raster_forward_transparent(cam, stream=st))
            info = ctx.raster_transparent_info()  # (the events above were waited for: it has landed)
            t["count_ms"], t["scan_ms"], t["fill_ms"], t["resolve_ms"] = info.countMs, info.scanMs, info.fillMs, info.resolveMs
            t["kernels_ms"] = info.countMs + info.scanMs + info.fillMs + info.resolveMs
            t["host_wait_ms"] = t["raster_call_ms"] - t["kernels_ms"]
            ctx.forward_transparent(cam, WIDTH, HEIGHT, stream=st)  # over the forward frame's depth: the context's last
            tinfo = ctx.transparent_info()
            t["traced_ms"] = tinfo.ms
            if i >= 3:
                for k in keys:
                    samples[k].append(t[k])
        r = {k: float(np.median(v)) for k, v in samples.items()}
        r.update(fragments=int(info.fragments), covered_pixels=int(info.coveredPixels), shaded_layers=int(info.shadedLayers),
                 max_layers=int(info.maxLayers), traced_covered_pixels=int(tinfo.coveredPixels), traced_layers=int(tinfo.totalLayers),
                 traced_max_layers=int(tinfo.maxLayers))
        stats = ctx.draw_stats()
        r.update(drawn_meshlets=int(stats.drawnMeshletCount), total_meshlets=int(stats.totalMeshletCount))
        r["ratio"] = r["raster_call_ms"] / max(r["traced_ms"], 1e-6)
        r["kernel_ratio"] = r["kernels_ms"] / max(r["traced_ms"], 1e-6)
        out.update(r)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f20_raster_transparent_bench.json"))
    args = ap.parse_args()
    import torch
    results = []
    for k in args.scenes.split(","):
        results.append(bench_scene(torch, k, args.repeats))
        print("%s done" % SCENES[k][0], file=sys.stderr, flush=True)
    text = json.dumps({"bench": "raster_transparent", "device": torch.cuda.get_device_name(0),
                       "stages": ["count", "scan", "fill", "resolve"], "yardstick": "prosper_pt_forward_transparent", "scenes": results})
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
