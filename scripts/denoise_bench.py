#!/usr/bin/env python3
"""The spatiotemporal denoiser at 1920x1080 (prosper_pt_denoise) on S-cornell (C2's scene), the C4 scene
(sponza_class with the sun and 1024 punctual lights) and the FlightHelmet fixture, beside the 1-spp render of the same
frame.  The pass is new: there is no earlier version to be faster than.

Per scene: the velocity G-buffer is traced once (a still camera: every geometry texel reads its history), one 1-spp
frame is rendered and kept in a device copy, and the denoise runs in place with every input NULL, the image restored
from the copy before each call (outside the timed stages).  Each stage's time is the device time between the events the
library records around it (prosper_pt_get_denoise_info): the median over `--repeats` calls after warm-up, with the
minimum, the maximum and the 10th / 90th percentiles as the spread.  The whole measurement runs `--rounds` times in the
same process; the medians of every round are reported, their difference is the run-to-run spread.  `bytes` is what a
stage must move at the least (each image it reads or writes once, 16 bytes per record), `gb_per_s` that over the median
time and `hbm_fraction` that over the 8.0 TB/s HBM3E peak: how far a stage is from the time its bytes alone would take.
`render_1spp_ms` is prosper_pt_render of one frame between events on the stream.  Prints one JSON object.

    python scripts/denoise_bench.py [--repeats 40] [--rounds 2] [--scenes c2,c4,fh]
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
HBM_PEAK_GB_PER_S = 8000.0
STAGES = ("temporal", "variance", "atrous0", "atrous1", "atrous2", "atrous3", "atrous4")


def stage_bytes(pc, pixels):
    """The least each stage must move with a history of 4 frames or more, bytes: every image once."""
    rec = 16
    temporal = (rec + (rec if pc.demodulate else 0) + rec + 4 + 8) + 4 * rec + 4 * rec  # inputs, the history read, the new one written
    if pc.feedbackIteration >= pc.iterations:
        temporal += rec
    out = {"temporal": temporal * pixels, "variance": 2 * rec * pixels}  # the flag and the length decide: nothing else is read
    for i in range(pc.iterations):
        b = 4 * rec  # image, guide A, guide B in; image out
        if i == pc.feedbackIteration:
            b += rec
        if i + 1 == pc.iterations:
            b += (rec if pc.demodulate else 0) + 2 * rec  # the albedo, the input's alpha, the HDR image
        out["atrous%d" % i] = b * pixels
    return out


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "p10": float(np.quantile(v, 0.1)),
            "p90": float(np.quantile(v, 0.9))}


def bench_scene(torch, key, repeats, rounds, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, width, height)
        cam, focal = hcam.update_buffer()
        st = torch.cuda.current_stream().cuda_stream
        pixels = width * height
        flags = S.PC_FLAG_ACCUMULATE | S.PC_FLAG_CLAMP_INDIRECT | S.PC_FLAG_SKIP_HISTORY | S.PC_FLAG_IBL
        render_pc = S.ReferencePC(0, flags, 1, 1e-5, 1.0, focal, 3, 4)
        ctx.trace_gbuffer_velocity(cam, width, height, stream=st)
        ctx.render(render_pc, cam, width, height, stream=st)
        ptr, _ = ctx.hdr_device_ptr()
        keep = torch.empty(pixels * 4, dtype=torch.float32, device="cuda")
        hip = C.CDLL("libamdhip64.so")

        def restore():
            assert hip.hipMemcpyAsync(C.c_void_p(ptr), C.c_void_p(keep.data_ptr()), C.c_size_t(pixels * 16), 3, C.c_void_p(st)) == 0
        assert hip.hipMemcpyAsync(C.c_void_p(keep.data_ptr()), C.c_void_p(ptr), C.c_size_t(pixels * 16), 3, C.c_void_p(st)) == 0

        def timed(fn):
            for _ in range(3):
                fn()
            ev = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize()
            return spread([a.elapsed_time(b) for a, b in ev])

        pc = S.DenoisePC.default()
        need = stage_bytes(pc, pixels)
        out = {"scene": name, "width": width, "height": height, "repeats": repeats, "rounds": []}
        for _ in range(rounds):
            r = {"render_1spp_ms": timed(lambda: ctx.render(render_pc, cam, width, height, stream=st))}
            ctx.denoise_release_history()
            times = {k: [] for k in STAGES + ("total",)}
            for i in range(repeats + 6):
                restore()
                ctx.denoise(pc, cam, width, height, stream=st)
                info = ctx.denoise_info()
                if i >= 6:  # (the history is longer than 4 frames: the steady state of a still camera)
                    assert info.ignoredHistory == 0 and info.noHistoryPixels == 0
                    for k, ms in zip(STAGES, [info.temporalMs, info.varianceMs] + list(info.atrousMs)):
                        times[k].append(ms)
                    times["total"].append(info.totalMs)
            r["history_pixels"] = int(info.historyPixels)
            r["stages"] = {}
            for k in STAGES:
                if k not in need:
                    continue
                s = spread(times[k])
                s.update(bytes=need[k], gb_per_s=need[k] / s["median"] * 1e-6)
                s["hbm_fraction"] = s["gb_per_s"] / HBM_PEAK_GB_PER_S
                r["stages"][k] = s
            r["denoise_total_ms"] = spread(times["total"])
            r["denoise_bytes"] = sum(need.values())
            r["denoise_hbm_fraction"] = r["denoise_bytes"] / r["denoise_total_ms"]["median"] * 1e-6 / HBM_PEAK_GB_PER_S
            r["denoise_over_render"] = r["denoise_total_ms"]["median"] / r["render_1spp_ms"]["median"]
            out["rounds"].append(r)
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(torch, k, args.repeats, args.rounds, w, h) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "denoise", "device": torch.cuda.get_device_name(0), "hbm_peak_gb_per_s": HBM_PEAK_GB_PER_S,
                      "scenes": results}))


if __name__ == "__main__":
    main()
