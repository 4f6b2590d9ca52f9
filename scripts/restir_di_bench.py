"""ReSTIR-DI at 1920x1080: the three passes of RtDirectIllumination::record (initial reservoirs, spatial reuse, trace)
and the whole record, on S-cornell (C2's scene), the C4 scene (sponza_class with the sun and 1024 punctual lights) and
the FlightHelmet fixture.

The ray-traced G-buffer (prosper_pt_trace_gbuffer) is timed too: `gbuffer_ms` jittered and at the pixel centres,
`record_traced_ms` the record that traces it first (spatial reuse on and off), and the yardstick
`render_1spp_1bounce_ms`, one prosper_pt_render frame with maxBounces = 1 (the same primary trace and surface, plus
NEE, a shadow ray and the accumulation), launched alternately with the G-buffer in the same process.

The G-buffer comes from the product's own debug views of the primary hits at 1 spp (Position, ShadingNormal, Albedo,
Roughness, Metallic), depth by projecting the positions with worldToClip, as tests/test_restir_di.py does.  Each stage is
timed alone with device events around `--repeats` launches after warm-up, the median of the per-launch times; the
record with spatial reuse on and off.  Prints one JSON object.

    python scripts/restir_di_bench.py [--repeats 60] [--scenes c2,c4,fh]
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

HBM_ROOF_GBS = 8000.0
SCENES = {
    "c2": ("S-cornell", lambda: scenes.cornell()),
    "c4": ("sponza_class lights+foliage", lambda: scenes.sponza_class(lights=True, foliage=True)),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture()),
}


def gbuffer(ctx, cam, focal, width, height):
    """Albedo/roughness, normal/metallic, non-linear depth from the debug draw types (gbuffer.frag's encodings)."""
    def view(name):
        pc = S.ReferencePC(S.DrawType[name], S.PC_FLAG_SKIP_HISTORY, 1, 1e-5, 1.0, focal, 3, 1)
        ctx.render(pc, cam, width, height)
        return ctx.read_hdr()[..., :3].astype(np.float64)
    pos, raw_n, alb = view("Position"), view("ShadingNormal"), view("Albedo")
    rough, metal = view("Roughness")[..., 0], view("Metallic")[..., 0]
    hit = raw_n.sum(axis=-1) > 0.0
    n = np.where(hit[..., None], raw_n * 2.0 - 1.0, np.array([0.0, 0.0, 1.0]))
    n = n / np.abs(n).sum(axis=-1, keepdims=True)  # signedOctEncode
    ey = n[..., 1] * 0.5 + 0.5
    enc = np.stack([n[..., 0] * 0.5 + ey, n[..., 0] * -0.5 + ey, np.clip(n[..., 2] * 1e30, 0.0, 1.0)], axis=-1)
    c2c = np.frombuffer(bytes(cam.cameraToClip), np.float32).reshape(4, 4).T.astype(np.float64)
    w2c = np.frombuffer(bytes(cam.worldToCamera), np.float32).reshape(4, 4).T.astype(np.float64)
    clip = np.concatenate([pos, np.ones(pos.shape[:2] + (1,))], axis=-1) @ (c2c @ w2c).T
    depth = np.where(hit, clip[..., 2] / np.where(clip[..., 3] == 0, 1.0, clip[..., 3]), 0.0).astype(np.float32)
    ar = np.concatenate([alb, np.maximum(rough, 0.05)[..., None]], axis=-1).astype(np.float32)
    nm = np.stack([enc[..., 0], enc[..., 1], metal, enc[..., 2]], axis=-1).astype(np.float32)
    return ar, nm, depth


def median_ms(torch, fn, repeats):
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in events:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in events]))


def alternating_median_ms(torch, fns, repeats):
    """Every function timed once per round, the rounds back to back: the median per function."""
    events = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            events[k].append((a, b))
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) for a, b in ev])) for k, ev in events.items()}


def bench_scene(torch, key, repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        cam, focal = Camera.from_world(world, width, height).update_buffer()
        ar, nm, depth = gbuffer(ctx, cam, focal, width, height)
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ar, nm, depth)]
        ptrs = [x.data_ptr() for x in t]
        res0 = torch.empty((height, width, 2), dtype=torch.float32, device="cuda")
        res1 = torch.empty_like(res0)
        pc = S.RestirTracePC(0, 1, 1)  # skipHistory
        st = torch.cuda.current_stream().cuda_stream
        stages = {
            "initial": lambda: ctx.restir_di_resample_device(S.RESTIR_INITIAL, 1, cam, width, height, *ptrs,
                                                             out_ptr=res0.data_ptr(), stream=st),
            "spatial": lambda: ctx.restir_di_resample_device(S.RESTIR_SPATIAL, 1, cam, width, height, *ptrs,
                                                             res_ptr=res0.data_ptr(), out_ptr=res1.data_ptr(), stream=st),
            "trace": lambda: ctx.restir_di_trace_device(pc, cam, width, height, *ptrs, res1.data_ptr(), stream=st),
            "record_spatial_on": lambda: ctx.restir_di_record_device(pc, cam, width, height, *ptrs, spatial_reuse=True,
                                                                  stream=st),
            "record_spatial_off": lambda: ctx.restir_di_record_device(pc, cam, width, height, *ptrs, spatial_reuse=False,
                                                                   stream=st),
        }
        for fn in stages.values():  # warm-up (allocations, code object load)
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: median_ms(torch, fn, repeats) for k, fn in stages.items()}
        # the ray-traced G-buffer into caller-owned targets, against one 1-bounce frame of the path tracer
        gb = [torch.empty_like(x) for x in t]
        targets = tuple(x.data_ptr() for x in gb)
        render_pc = S.ReferencePC(0, S.PC_FLAG_SKIP_HISTORY | S.PC_FLAG_ACCUMULATE, 1, 1e-5, 1.0, focal, 3, 1)
        yard = {
            "gbuffer_jitter": lambda: ctx.trace_gbuffer(cam, width, height, frame_index=1, jitter=True, targets=targets,
                                                        stream=st),
            "gbuffer_centre": lambda: ctx.trace_gbuffer(cam, width, height, frame_index=1, jitter=False, targets=targets,
                                                        stream=st),
            "render_1spp_1bounce": lambda: ctx.render(render_pc, cam, width, height, stream=st),
        }
        traced = {
            "spatial_on": lambda: ctx.restir_di_record_traced(pc, cam, width, height, spatial_reuse=True, stream=st),
            "spatial_off": lambda: ctx.restir_di_record_traced(pc, cam, width, height, spatial_reuse=False, stream=st),
        }
        for fn in list(yard.values()) + list(traced.values()):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        yard_ms = alternating_median_ms(torch, yard, repeats)
        traced_ms = {k: median_ms(torch, fn, repeats) for k, fn in traced.items()}
        px = width * height
        lit = float((ctx.read_restir_reservoirs(st)[..., 0].copy().view(np.int32) >= 0).mean())
        # algorithmic bytes: G-buffer 16 + 16 + 4 B, reservoirs 8 B in / out, HDR 16 B; the spatial pass's neighbour
        # reads (up to 25 depth + normal pairs and 5 reservoirs) are L2 traffic and not counted
        nbytes = {"initial": 44 * px, "spatial": 52 * px, "trace": 60 * px}
        out = {"scene": name, "width": width, "height": height,
               "lights": 1 + world.point_lights.count + world.spot_lights.count, "repeats": repeats,
               "pixels_with_a_light": lit, "ms": ms, "algorithmic_bytes": nbytes,
               "gbuffer_ms": {"jitter": yard_ms["gbuffer_jitter"], "centre": yard_ms["gbuffer_centre"]},
               "render_1spp_1bounce_ms": yard_ms["render_1spp_1bounce"], "record_traced_ms": traced_ms}
        out["GBps"] = {k: nbytes[k] / (ms[k] * 1e-3) / 1e9 for k in nbytes}
        out["share_of_hbm_roof"] = {k: out["GBps"][k] / HBM_ROOF_GBS for k in nbytes}
        return out
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
    result = {"bench": "restir_di", "configs": {}}
    for key in args.scenes.split(","):
        result["configs"][key] = bench_scene(torch, key, args.repeats, args.width, args.height)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
