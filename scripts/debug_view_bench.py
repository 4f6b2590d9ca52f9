#!/usr/bin/env python3
"""The inspection passes at 1920x1080 (prosper_pt_debug_lines, prosper_pt_texture_debug, prosper_pt_texture_readback;
DESIGN.md f16) on S-cornell (C2's scene), the C4 scene (sponza_class with lights and foliage) and the FlightHelmet fixture.

Per scene, in one process, three line sets:
  scene     what prosper draws: the axes of the scene's own lights (prosper_pt_read_lights) and the frustum of the
            scene's camera
  axes_1024 the axes of 1024 point lights (C4's light count) spread over the view: 3072 lines of length 0.2
  max_short DebugLines::sMaxLineCount = 100 000 segments of length 0.2 spread over the view
Before each measured call the frame up to the pass is made again (traced G-buffer, deferred shading, sky), since the
pass writes the illumination and the depth.  ms: median (_mean, _max) device time of the two kernels over the measured
calls, the library's own events (prosper_pt_get_debug_lines_info).
  texture_debug     the viewer into a 1920x1080 RGBA8 device image over "illumination" (RGBA32F) and "depth" (R32F), nearest
                    and bilinear, and zoomed with the magnifier: us per call, the median of `repeats` batches of 10 calls
                    between two events on the stream
  texture_readback  one record (the one-lane kernel and the 16-byte copy to pinned memory), the same way, one call a batch
Prints one JSON object.

    python scripts/debug_view_bench.py [--repeats 20] [--scenes c2,c4,fh] [--size 1920x1080]

PROSPER_PT_LIB selects another build of the library, e.g. the measurement build with one lane per line that the
product's wave-per-line mapping was compared with; "library" names it.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, debug_geometry as G, flight_helmet, scenes  # noqa: E402
from prosper_amd.rt_reference import Camera  # noqa: E402

SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell(with_skybox=True)),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}


def spread_points(cam, n, seed):
    """n world positions inside the view, 2 to 20 units in front of the camera (a segment of 0.2 is then about 95 to 9
    pixels long at 1080 rows): random clip-space points through clipToWorld"""
    rng = np.random.default_rng(seed)
    m = G.mat4(cam.clipToWorld).astype(np.float64)
    p = G.mat4(cam.cameraToClip).astype(np.float64)
    d = rng.uniform(2.0, 20.0, n)
    z = (p[2, 2] * -d + p[2, 3]) / (p[3, 2] * -d + p[3, 3])
    clip = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), z, np.ones(n)], 1)
    p = clip @ m.T
    return (p[:, :3] / p[:, 3:4]).astype(np.float32)


def short_segments(cam, n, seed):
    a = spread_points(cam, n, seed)
    d = np.random.default_rng(seed + 1).normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * G.DEBUG_LINE_LENGTH).astype(np.float32)
    colour = np.tile(np.array(G.DEBUG_RED, np.float32), (n, 1))
    return np.concatenate([a, a + d, colour], 1)


class Events:
    """two HIP events on the null stream, the runtime the library itself uses"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time_us(self, call, calls):
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(calls):
            call()
        assert self.hip.hipEventRecord(self.b, None) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3 / calls

    def close(self):
        self.hip.hipEventDestroy(self.a)
        self.hip.hipEventDestroy(self.b)


def bench_viewer(ctx, width, height, repeats):
    from prosper_amd import structs as S
    ev = Events()
    target = C.c_void_p()
    assert ev.hip.hipMalloc(C.byref(target), C.c_size_t(width * height * 4)) == 0
    try:
        def view(name, flags, bilinear, cursor=(0.0, 0.0)):
            return lambda: ctx.texture_debug(name, (width, height), (0.0, 1.0), 0, flags, cursor, bilinear, device_ptr=target.value,
                                             to_host=False)
        rgb, mag = S.TEXTURE_DEBUG_CHANNEL_RGB, S.TEXTURE_DEBUG_ZOOM | S.TEXTURE_DEBUG_MAGNIFIER
        cases = {"illumination_nearest": view("illumination", rgb, False), "illumination_bilinear": view("illumination", rgb, True),
                 "illumination_bilinear_zoom_magnifier": view("illumination", rgb | mag, True, (0.4, 0.6)),
                 "depth_nearest": view("depth", 0, False), "depth_bilinear": view("depth", 0, True)}
        viewer = {}
        for name, call in cases.items():
            call()
            us = np.array([ev.time_us(call, 10) for _ in range(repeats)])
            viewer[name] = {"us": float(np.median(us)), "us_max": float(us.max())}

        def record():
            ctx.texture_readback("depth", width / 2, height / 2)
        us = []
        for _ in range(repeats + 1):
            us.append(ev.time_us(record, 1))
            assert ctx.try_texture_readback() is not None
        us = np.array(us[1:])
        return viewer, {"us": float(np.median(us)), "us_max": float(us.max())}
    finally:
        ev.hip.hipFree(target)
        ev.close()


def bench_scene(key, repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        cam, _ = Camera.from_world(world, width, height).update_buffer()

        def frame():
            capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, 0, C.byref(cam), width, height, None, None))
            inp, _, _ = ctx.gbuffer_device_ptrs()
            ctx.deferred_shading_device(cam, width, height, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
            ctx.skybox_fill(cam, width, height)

        _, points, spots = ctx.read_lights()
        sets = {
            "scene": np.concatenate([G.light_axes_from_buffers(points, spots),
                                     G.frustum_lines(G.frustum_corners(cam), (1.0, 1.0, 1.0))]),
            "axes_1024": G.light_axes(spread_points(cam, 1024, 7), []),
            "max_short": short_segments(cam, G.DebugLines.sMaxLineCount, 11),
        }
        out = {"scene": name, "width": width, "height": height, "repeats": repeats,
               "point_lights": int(points.count), "spot_lights": int(spots.count), "sets": {}}
        for set_name, lines in sets.items():
            ms, info = [], None
            for _ in range(repeats + 1):  # the first call allocates
                frame()
                ctx.debug_lines(lines, cam, width, height)
                info = ctx.debug_lines_info()
                ms.append(info.ms)
            ms = np.array(ms[1:], np.float64)
            out["sets"][set_name] = {
                "lines": int(len(lines)), "fragments_written": int(info.fragmentsWritten),
                "lines_clipped_away": int(info.linesClippedAway), "ms": float(np.median(ms)), "ms_mean": float(ms.mean()),
                "ms_max": float(ms.max()),
            }
        frame()
        out["texture_debug"], out["texture_readback"] = bench_viewer(ctx, width, height, repeats)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(k, args.repeats, w, h) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "debug_view", "library": os.path.relpath(capi.LIB_PATH, ROOT), "scenes": results}))


if __name__ == "__main__":
    main()
