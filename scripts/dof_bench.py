#!/usr/bin/env python3
"""Depth of field at 1920x1080: the seven passes of render::dof::DepthOfField (prosper_pt_depth_of_field) stage by stage,
on S-cornell (C2's scene), the C4 scene (sponza_class with the sun and 1024 punctual lights) and the FlightHelmet
fixture.

The input is the traced, shaded and sky-filled image: the pixel-centre G-buffer, deferred shading and
prosper_pt_skybox_fill of the same context; depth of field then runs in place over the traced depth (the image is
restored from a device copy before every launch, outside the timed stages).  The focus lies at the median depth of the
hit texels and the aperture gives the far background a circle of `--coc` half-resolution texels (12 by default), so the
nearer half of the hits lies in front of the focus and the other half and the sky behind it: both layers are active,
and `foreground_tiles` / `background_tiles` say on how many tiles.  Each stage's time is the device time between the
events the library records around it (prosper_pt_get_dof_info), the median over `--repeats` launches after warm-up;
`deferred_shading_ms` (trace + clustering + shading) and `gbuffer_ms` of the same run are the yardsticks.  Prints one
JSON object.

    python scripts/dof_bench.py [--repeats 60] [--scenes c2,c4,fh] [--coc 12]
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
STAGES = ("setupMs", "reduceMs", "flattenMs", "dilateMs", "gatherForegroundMs", "gatherBackgroundMs",
          "filterForegroundMs", "filterBackgroundMs", "combineMs")


def bench_scene(torch, key, repeats, width, height, coc):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        c = world.camera
        hcam = Camera.from_world(world, width, height)
        cam, focal = hcam.update_buffer()
        ctx.deferred_shading_traced(cam, width, height)
        depth = ctx.read_gbuffer()[2]
        hit = depth != 0
        c2c = np.frombuffer(bytes(cam.cameraToClip), np.float32).reshape(4, 4).T.astype(np.float64)
        linear = c2c[2, 3] / (depth[hit].astype(np.float64) + c2c[2, 2])  # distance along the view direction
        focus = float(np.median(linear))
        aperture = coc / ((width + 1) // 2) * 0.035 * (focus - focal) / focal
        hcam.set_parameters(c["fov"], c["zN"], c["zF"], aperture, focus)
        cam, _ = hcam.update_buffer()
        st = torch.cuda.current_stream().cuda_stream

        def timed(fn):
            ev = []
            for _ in range(repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in ev]))

        for _ in range(3):
            ctx.deferred_shading_traced(cam, width, height, stream=st)
        shading_ms = timed(lambda: ctx.deferred_shading_traced(cam, width, height, stream=st))
        # (Context.trace_gbuffer would read the targets back; the entry itself only enqueues)
        gbuffer_ms = timed(lambda: capi._check(capi.lib().prosper_pt_trace_gbuffer(
            ctx._h, 0, 0, 0, C.byref(cam), width, height, None, C.c_void_p(st))))
        ctx.deferred_shading_traced(cam, width, height, stream=st)
        fill_ms = timed(lambda: ctx.skybox_fill(cam, width, height, stream=st))
        ptr, nbytes = ctx.hdr_device_ptr()
        keep = torch.empty(width * height * 4, dtype=torch.float32, device="cuda")
        hip = C.CDLL("libamdhip64.so")

        def restore():
            assert hip.hipMemcpyAsync(C.c_void_p(ptr), C.c_void_p(keep.data_ptr()), C.c_size_t(width * height * 16), 3,
                                      C.c_void_p(st)) == 0
        assert hip.hipMemcpyAsync(C.c_void_p(keep.data_ptr()), C.c_void_p(ptr), C.c_size_t(width * height * 16), 3,
                                  C.c_void_p(st)) == 0
        dof = DepthOfField(ctx)
        inputs = S.DofInputs(None, None, 1, 0)
        pc = dof.record_inputs(hcam, width, height, inputs, stream=st)
        tiles = ctx.read_dof_stage(S.DOF_DILATED_TILE_MIN_MAX).astype(np.float32)
        per_stage = {k: [] for k in STAGES}
        whole = []
        for i in range(repeats + 3):
            restore()
            dof.record_inputs(hcam, width, height, inputs, stream=st)
            info = ctx.dof_info()
            if i >= 3:
                for k in STAGES:
                    per_stage[k].append(getattr(info, k))
                whole.append(sum(getattr(info, k) for k in STAGES))
        out = {
            "scene": name, "width": width, "height": height, "repeats": repeats,
            "focus_distance": focus, "aperture_diameter": aperture,
            "max_background_coc": pc.maxBackgroundCoC, "max_coc": pc.maxCoC, "gather_radius": pc.gatherRadius,
            "miss_share": float(1.0 - hit.mean()),
            "foreground_tiles": float((tiles[..., 0] <= -0.5).mean()),
            "background_tiles": float((tiles[..., 1] >= 1.0).mean()),
            "both_layers_active": bool((tiles[..., 0] <= -0.5).any() and (tiles[..., 1] >= 1.0).any()),
            "stage_ms": {k[:-2]: float(np.median(v)) for k, v in per_stage.items()},
            "depth_of_field_ms": float(np.median(whole)),
            "deferred_shading_ms": shading_ms, "gbuffer_ms": gbuffer_ms, "skybox_fill_ms": fill_ms,
        }
        return out
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--coc", type=float, default=12.0, help="the far background's circle in half-resolution texels")
    args = ap.parse_args()
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(torch, k, args.repeats, w, h, args.coc) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "depth_of_field", "device": torch.cuda.get_device_name(0), "scenes": results}))


if __name__ == "__main__":
    main()
