#!/usr/bin/env python3
"""The traced G-buffer at 1920x1080 with material textures sampled at LOD 0 and through their mip chains
(prosper_pt_set_texture_lod), on the C3 scene (sponza_class: 75 x 1024^2 textures), the C4 scene (the same
with 1024 punctual lights and alpha foliage) and the FlightHelmet fixture.

Per scene, four contexts' worth of numbers: a context created WITHOUT PROSPER_PT_CREATE_TEXTURE_MIPS (`plain`: what the
parent commit runs) and one created with it, with LOD off (`lod_off`: must cost what `plain` costs), on with bias 0
(`lod_on`) and on with prosper's TAA bias of -1 (`lod_on_bias_-1`); each for prosper_pt_trace_gbuffer through the pixel
centres (`gbuffer_ms`) and prosper_pt_trace_gbuffer_velocity with the camera's jitter (`velocity_gbuffer_ms`).  A time is
the median over `--repeats` launches, after warm-up, of the device time between two events on the stream.  `upload_s`
is prosper_pt_upload_scene's own figure with and without chains (generation is part of it), `mip_texel_bytes` what the
chains hold.  `uv_footprint_mean` / `_median`: over the hit pixels, the larger of the two uv forward differences' lengths (times a
texture's extent it is rho; log2 of that is lambda at bias 0).
The forward transparent pass follows the same state; it is not timed here.  Prints ONE JSON object.

    python scripts/texture_lod_bench.py [--repeats 40] [--scenes c3,c4,fh]
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
    "c3": ("sponza_class", lambda: scenes.sponza_class()),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}


def bench_context(torch, world, flags, modes, repeats, width, height):
    ctx = capi.Context(0, flags=flags)
    try:
        ctx.upload_scene(world)
        stats = ctx.scene_stats()
        out = {"upload_s": stats.uploadSeconds, "texture_s": stats.textureSeconds}
        if flags & S.CREATE_TEXTURE_MIPS:
            out["mip_texel_bytes"] = int(ctx.texture_mips_info(0).mipTexelBytes)
        hcam = Camera.from_world(world, width, height)
        cam, _ = hcam.update_buffer()
        cam = S.CameraUniforms.from_buffer_copy(bytes(cam))
        hcam.set_jitter(True)
        hcam.end_frame()
        jittered, _ = hcam.update_buffer()
        jittered = S.CameraUniforms.from_buffer_copy(bytes(jittered))
        st = torch.cuda.current_stream().cuda_stream
        lib = capi.lib()
        desc = S.VelocityGBufferDesc()

        def check(rc):
            assert rc == 0, lib.prosper_pt_last_error().decode()

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
            return float(np.median([a.elapsed_time(b) for a, b in ev]))

        for label, enabled, bias in modes:
            if enabled is not None:
                ctx.set_texture_lod(enabled, bias)
            out[label] = {
                "gbuffer_ms": timed(lambda: check(lib.prosper_pt_trace_gbuffer(ctx._h, 0, 1, 0, C.byref(cam), width, height, None, C.c_void_p(st)))),
                "velocity_gbuffer_ms": timed(lambda: check(lib.prosper_pt_trace_gbuffer_velocity(
                    ctx._h, 0, 1, 0, C.byref(jittered), width, height, C.byref(desc), C.c_void_p(st)))),
            }
        if flags & S.CREATE_TEXTURE_MIPS:
            ctx.set_texture_lod(True, 0.0)
            ctx.set_texture_lod_debug(True)
            _, _, depth = ctx.trace_gbuffer(cam, width, height, jitter=False, stream=st)
            d = ctx.read_texture_lod_derivatives(width, height, stream=st).astype(np.float64)
            ctx.set_texture_lod_debug(False)
            hit = (depth > 0) & np.isfinite(d).all(axis=-1)
            rho = np.maximum(np.hypot(d[..., 0], d[..., 1]), np.hypot(d[..., 2], d[..., 3]))[hit]
            out["uv_footprint_mean"] = float(rho.mean()) if rho.size else None
            out["uv_footprint_median"] = float(np.median(rho)) if rho.size else None
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--scenes", default="c3,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = []
    for key in args.scenes.split(","):
        name, make = SCENES[key]
        world = make()
        r = {"scene": name, "width": w, "height": h, "repeats": args.repeats}
        r["without_flag"] = bench_context(torch, world, 0, [("plain", None, 0.0)], args.repeats, w, h)
        r["with_flag"] = bench_context(torch, world, S.CREATE_TEXTURE_MIPS, [("lod_off", False, 0.0), ("lod_on", True, 0.0), ("lod_on_bias_-1", True, -1.0),
                                                                          ("lod_off_again", False, 0.0)], args.repeats, w, h)
        results.append(r)
    print(json.dumps({"bench": "texture_lod", "device": torch.cuda.get_device_name(0), "scenes": results}))


if __name__ == "__main__":
    main()
