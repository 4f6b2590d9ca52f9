#!/usr/bin/env python3
"""The temporal anti-aliasing resolve at 1920x1080: the two kernels of prosper_pt_taa_resolve, `resolve` and `expand`,
on S-cornell (C2's scene), the C4 scene (sponza_class with the sun and 1024 punctual lights) and the FlightHelmet
fixture, for prosper's default variant (Catmull-Rom, Variance, Closest, luminance weighting) and the cheapest one
(bilinear, None, Center, no weighting).

The input is the traced, shaded and sky-filled image with the traced G-buffer's depth; the velocity is a constant
sub-pixel shift (0.3, -0.2 texels), so every texel reads its history.  The resolve runs in place (the image is restored
from a device copy before every launch, outside the timed stages) and, for `resolve_writes_hdr_ms`, from the copy as a
separate input, where `resolve` writes the HDR image itself and `expand` is skipped.  Each stage's time is the device
time between the events the library records around it (prosper_pt_get_taa_info), the median over `--repeats` launches
after warm-up.  `bytes` is what a stage must move (each image once), `gb_per_s` that over the time.  Bloom's `compose`
and depth of field's `combine`, two full-image passes of the existing code, are timed in the same run as yardsticks.
`gbuffer_ms` and `velocity_gbuffer_ms` are prosper_pt_trace_gbuffer through the pixel centres and
prosper_pt_trace_gbuffer_velocity with the camera's jitter and the scene's transforms as the previous frame's, between
events on the stream; their difference is what the velocity target costs.  Prints one JSON object.

    python scripts/taa_bench.py [--repeats 60] [--scenes c2,c4,fh]
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
from prosper_amd.rt_reference import Camera, DepthOfField  # noqa: E402

SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell(with_skybox=True)),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}
VARIANTS = (("default", S.TaaPC.default()),
            ("cheapest", S.TaaPC.default(0, S.TAA_CLIPPING_NONE, S.TAA_VELOCITY_CENTER, 0)))


def stage_bytes(pc, pixels):
    """What the two kernels must move in place: illumination, history, velocity and (Closest) depth in, history out;
    history in, HDR image out."""
    resolve = pixels * (16 + 8 + 8 + (4 if pc.velocitySampling == S.TAA_VELOCITY_CLOSEST else 0) + 8)
    return resolve, pixels * (8 + 16)


def bench_scene(torch, key, repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, width, height)
        cam, _ = hcam.update_buffer()
        st = torch.cuda.current_stream().cuda_stream
        pixels = width * height
        ctx.deferred_shading_traced(cam, width, height, stream=st)
        ctx.skybox_fill(cam, width, height, stream=st)
        ptr, _ = ctx.hdr_device_ptr()
        keep = torch.empty(pixels * 4, dtype=torch.float32, device="cuda")
        velocity = torch.empty((height, width, 2), dtype=torch.float32, device="cuda")
        velocity[..., 0] = 2.0 * 0.3 / width
        velocity[..., 1] = -2.0 * 0.2 / height
        hip = C.CDLL("libamdhip64.so")

        def copy(dst, src):
            assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(pixels * 16), 3, C.c_void_p(st)) == 0
        copy(keep.data_ptr(), ptr)
        out = {"scene": name, "width": width, "height": height, "repeats": repeats}

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

        lib = capi.lib()
        hcam.set_jitter(True)
        hcam.end_frame()
        jittered, _ = hcam.update_buffer()
        jittered = S.CameraUniforms.from_buffer_copy(bytes(jittered))
        transforms = world.freeze()["transforms"]
        desc = S.VelocityGBufferDesc()
        desc.previousTransforms = C.cast(transforms, C.c_void_p)
        desc.previousTransformCount = len(transforms)

        def check(rc):
            assert rc == 0, lib.prosper_pt_last_error().decode()
        out["gbuffer_ms"] = timed(lambda: check(lib.prosper_pt_trace_gbuffer(ctx._h, 0, 1, 0, C.byref(cam), width, height, None, C.c_void_p(st))))
        out["velocity_gbuffer_ms"] = timed(lambda: check(lib.prosper_pt_trace_gbuffer_velocity(
            ctx._h, 0, 1, 0, C.byref(jittered), width, height, C.byref(desc), C.c_void_p(st))))
        out["gbuffer_ms_again"] = timed(lambda: check(lib.prosper_pt_trace_gbuffer(ctx._h, 0, 1, 0, C.byref(cam), width, height, None, C.c_void_p(st))))
        hcam.set_jitter(False)
        for label, pc in VARIANTS:
            ctx.taa_release_history()
            stages, separate = {"resolve": [], "expand": []}, []
            for i in range(repeats + 3):
                copy(ptr, keep.data_ptr())
                ctx.taa_resolve(pc, width, height, velocity_ptr=velocity.data_ptr(), stream=st)
                info = ctx.taa_info()
                if i >= 3:
                    assert info.ignoredHistory == 0
                    stages["resolve"].append(info.resolveMs)
                    stages["expand"].append(info.expandMs)
            for i in range(repeats + 3):
                ctx.taa_resolve(pc, width, height, velocity_ptr=velocity.data_ptr(), illumination_ptr=keep.data_ptr(), stream=st)
                if i >= 3:
                    separate.append(ctx.taa_info().resolveMs)
            resolve_ms, expand_ms = float(np.median(stages["resolve"])), float(np.median(stages["expand"]))
            resolve_bytes, expand_bytes = stage_bytes(pc, pixels)
            out[label] = {
                "resolve_ms": resolve_ms, "expand_ms": expand_ms, "in_place_ms": resolve_ms + expand_ms,
                "resolve_writes_hdr_ms": float(np.median(separate)),
                "resolve_bytes": resolve_bytes, "expand_bytes": expand_bytes,
                "resolve_gb_per_s": resolve_bytes / resolve_ms * 1e-6, "expand_gb_per_s": expand_bytes / expand_ms * 1e-6,
            }
        # the yardsticks: bloom's compose and depth of field's combine over the same image
        compose, combine = [], []
        copy(ptr, keep.data_ptr())
        bloom_pc = S.BloomPC.default(threshold=float(np.quantile(ctx.read_hdr()[..., :3].max(axis=-1), 0.7)))
        dof = DepthOfField(ctx)
        for i in range(repeats + 3):
            copy(ptr, keep.data_ptr())
            ctx.bloom(bloom_pc, width, height, stream=st)
            if i >= 3:
                compose.append(ctx.bloom_info().composeMs)
        for i in range(repeats + 3):
            copy(ptr, keep.data_ptr())
            dof.record(hcam, width, height, stream=st)
            if i >= 3:
                combine.append(ctx.dof_info().combineMs)
        out["bloom_compose_ms"] = float(np.median(compose))
        out["dof_combine_ms"] = float(np.median(combine))
        out["yardstick_ms"] = out["bloom_compose_ms"] + out["dof_combine_ms"]
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    args = ap.parse_args()
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(torch, k, args.repeats, w, h) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "taa", "device": torch.cuda.get_device_name(0), "scenes": results}))


if __name__ == "__main__":
    main()
