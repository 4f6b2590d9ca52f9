#!/usr/bin/env python3
"""The forward transparent pass at 1920x1080 (prosper_pt_forward_transparent) on S-cornell (C2's scene),
the C4 scene (sponza_class with the sun, 1024 punctual lights and the BLEND foliage) and the FlightHelmet fixture.

Per scene, in one process:
  gbuffer_ms / gbuffer_opaque_only_ms   the pixel-centre traced G-buffer with the stochastic any-hit and with
                                        PROSPER_PT_GBUFFER_OPAQUE_ONLY, launched alternately, device events around each
  transparent_ms / transparent_ibl_ms   the pass with ibl 0 and 1 over the opaque-only G-buffer's depth and the shaded,
                                        sky-filled image, the context's clustering reused: the library's own device time
                                        (prosper_pt_get_transparent_info)
  transparent_reclustered_ms            the same call after a light update, which makes it cluster the lights first;
                                        recluster_ms is the difference to transparent_ms
  layers                                covered share, mean layers per covered pixel, the deepest pixel, the histogram of
                                        layer counts (from the pass's debug read-back, taken outside the timed launches)
  per_traversal                         transparent_ms over gbuffer_ms: one peel is one primary traversal, so this is the
                                        pass's cost in G-buffer traces
Every time is the median over `--repeats` launches after three warm-up launches.  The pass works in place, so the image
changes from launch to launch; its layers, and with them the work, do not.  Prints one JSON object.

    python scripts/transparent_bench.py [--repeats 30] [--scenes c2,c4,fh] [--size 1920x1080]
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
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}


class Events:
    """Device events of the HIP runtime the library runs on, on the null stream (which the entries are given)."""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")

    def timed(self, fn):
        a, b, ms = C.c_void_p(), C.c_void_p(), C.c_float()
        assert self.hip.hipEventCreate(C.byref(a)) == 0 and self.hip.hipEventCreate(C.byref(b)) == 0
        assert self.hip.hipEventRecord(a, None) == 0
        fn()
        assert self.hip.hipEventRecord(b, None) == 0 and self.hip.hipEventSynchronize(b) == 0
        assert self.hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        self.hip.hipEventDestroy(a)
        self.hip.hipEventDestroy(b)
        return ms.value


def bench_scene(events, key, repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        ctx.generate_ibl()
        hcam = Camera.from_world(world, width, height)
        cam, _ = hcam.update_buffer()

        def gbuffer(flags):
            # (Context.trace_gbuffer would read the targets back; the entry itself only enqueues)
            capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, flags, C.byref(cam), width, height, None, None))

        times = {"stochastic": [], "opaque_only": []}
        for i in range(repeats + 3):
            for kind, flags in (("stochastic", 0), ("opaque_only", S.GBUFFER_OPAQUE_ONLY)):
                ms = events.timed(lambda: gbuffer(flags))
                if i >= 3:
                    times[kind].append(ms)

        # the frame up to the pass: opaque-only G-buffer (the last one traced), shading, sky
        inp, _, _ = ctx.gbuffer_device_ptrs()
        ctx.deferred_shading_device(cam, width, height, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
        ctx.skybox_fill(cam, width, height)

        def run(ibl):
            ctx.forward_transparent(cam, width, height, ibl=ibl)
            return ctx.transparent_info()

        passes = {0: [], 1: []}
        for i in range(repeats + 3):
            for ibl in (0, 1):
                info = run(ibl)
                assert info.reclustered == 0
                if i >= 3:
                    passes[ibl].append(info.ms)
        reclustered = []
        first = world.point_lights.lights[0] if world.point_lights.count else None
        for i in range(repeats + 3):
            # a light update that changes the bytes and (nearly) nothing else
            if first is not None:
                first.radianceAndRadius.x = float(np.nextafter(np.float32(first.radianceAndRadius.x), np.float32(np.inf)))
            else:
                world.directional.irradiance.x = float(np.nextafter(np.float32(world.directional.irradiance.x), np.float32(np.inf)))
            ctx.update_lights(world)
            info = run(0)
            assert info.reclustered == 1
            if i >= 3:
                reclustered.append(info.ms)

        ctx.set_transparent_debug_layers(1)  # the counts are whole whatever the number of layers kept
        info = run(0)
        counts, _ = ctx.read_transparent_layers()
        ctx.set_transparent_debug_layers(0)
        assert (info.coveredPixels, info.totalLayers, info.maxLayers) == ((counts > 0).sum(), counts.sum(), counts.max())
        covered = counts[counts > 0]
        gb, tr = float(np.median(times["stochastic"])), float(np.median(passes[0]))
        return {
            "scene": name, "width": width, "height": height, "repeats": repeats,
            "triangles": int(ctx.scene_stats().triangleCount),
            "gbuffer_ms": gb, "gbuffer_opaque_only_ms": float(np.median(times["opaque_only"])),
            "opaque_only_over_stochastic": float(np.median(times["opaque_only"])) / gb,
            "transparent_ms": tr, "transparent_ibl_ms": float(np.median(passes[1])),
            "transparent_reclustered_ms": float(np.median(reclustered)),
            "recluster_ms": float(np.median(reclustered)) - tr,
            "per_traversal": tr / gb,
            "layers": {
                "covered_share": float((counts > 0).mean()),
                "mean_per_covered_pixel": float(covered.mean()) if covered.size else 0.0,
                "mean_per_pixel": float(counts.mean()),
                "max": int(counts.max()),
                "histogram": np.bincount(counts.ravel()).tolist(),
            },
        }
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    events = Events()
    results = [bench_scene(events, k, args.repeats, w, h) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "forward_transparent", "scenes": results}))


if __name__ == "__main__":
    main()
