"""Clustered lighting and deferred shading at 1920x1080 (prosper's default lighting of its G-buffer:
LightClustering::record + DeferredShading::record) on S-cornell (C2's scene), the C4 scene (sponza_class with the sun
and 512 + 512 punctual lights) and the FlightHelmet fixture.

The G-buffer is the product's ray-traced one at the pixel centres (prosper_pt_trace_gbuffer into device buffers).  Timed
with device events around `--repeats` launches after warm-up, the median per launch:
  cluster_ms         prosper_pt_cluster_lights alone
  deferred_ms        prosper_pt_deferred_shading over the device G-buffer: clustering + shading
  shade_ms           deferred_ms - cluster_ms (the shading kernel's share; the entry has no shading-only form)
  traced_ms          prosper_pt_deferred_shading with PROSPER_PT_DEFERRED_TRACE_GBUFFER: G-buffer + clustering + shading
  restir_record_ms   the yardstick: prosper_pt_restir_di_record over the same G-buffer, spatial reuse on
The clustering's shape is reported too: mean point / spot entries per cluster, clusters that overflow the 128 + 128
entries, and the entries dropped.  Prints one JSON object.

    python scripts/deferred_shading_bench.py [--repeats 60] [--scenes c2,c4,fh]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, flight_helmet, scenes, structs as S  # noqa: E402
from prosper_amd.rt_reference import Camera  # noqa: E402

SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell()),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}


def median_ms(torch, fn, repeats):
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in events:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in events]))


def bench_scene(torch, key, repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        cam, _ = Camera.from_world(world, width, height).update_buffer()
        gb = [torch.empty((height, width, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        gb.append(torch.empty((height, width), dtype=torch.float32, device="cuda"))
        ptrs = tuple(x.data_ptr() for x in gb)
        st = torch.cuda.current_stream().cuda_stream
        ctx.trace_gbuffer(cam, width, height, jitter=False, targets=ptrs, stream=st)
        pc = S.RestirTracePC(0, 1, 1)  # skipHistory
        stages = {
            "cluster": lambda: ctx.cluster_lights(cam, width, height, stream=st),
            "deferred": lambda: ctx.deferred_shading_device(cam, width, height, *ptrs, stream=st),
            "traced": lambda: ctx.deferred_shading_traced(cam, width, height, stream=st),
            "restir_record": lambda: ctx.restir_di_record_device(pc, cam, width, height, *ptrs, spatial_reuse=True,
                                                                 stream=st),
        }
        for fn in stages.values():  # warm-up (allocations, code object load)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: median_ms(torch, fn, repeats) for k, fn in stages.items()}
        ctx.cluster_lights(cam, width, height, stream=st)
        cl = ctx.read_light_clusters(st)
        packed = cl["pointers"][..., 1]
        points, spots = packed >> 16, packed & 0xFFFF
        return {"scene": name, "width": width, "height": height, "repeats": repeats,
                "point_lights": world.point_lights.count, "spot_lights": world.spot_lights.count,
                "clusters": int(packed.size), "cluster_ms": ms["cluster"], "deferred_ms": ms["deferred"],
                "shade_ms": ms["deferred"] - ms["cluster"], "traced_ms": ms["traced"],
                "restir_record_ms": ms["restir_record"],
                "mean_points_per_cluster": float(points.mean()), "mean_spots_per_cluster": float(spots.mean()),
                "overflowing_clusters": cl["overflowing"], "dropped_entries": cl["dropped"]}
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    result = {"bench": "deferred_shading", "configs": {}}
    for key in args.scenes.split(","):
        result["configs"][key] = bench_scene(torch, key, args.repeats, args.width, args.height)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
