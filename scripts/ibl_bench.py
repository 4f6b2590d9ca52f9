"""Image-based lighting: ImageBasedLighting::recordGeneration's three passes and deferred shading with and without the
IBL term at 1920x1080, on the C3 scene (sponza_class: the sun and the 512^2 sky_cube) and the FlightHelmet fixture.

  generation          per pass (irradiance, radiance, lut), the device time prosper_pt_get_ibl_info reports for one
                      prosper_pt_generate_ibl (events around each pass, borders included), median over `--gen-repeats`
                      generations; also the whole call timed with device events
  lookups             the work of each pass, from its sizes: environment lookups of the irradiance and radiance passes
                      as the GLSL writes them and as the kernels make them (mip 0 is one lookup per texel), LUT samples
  deferred_ms         prosper_pt_deferred_shading over the pixel-centre traced G-buffer (device pointers), ibl = 0 and
                      ibl = 1, median over `--repeats` launches (device events)
Prints one JSON object.

    python scripts/ibl_bench.py [--repeats 60] [--gen-repeats 5] [--scenes c3,fh]
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
    "c3": ("sponza_class", lambda: scenes.sponza_class()),
    "fh": ("FlightHelmet", lambda: flight_helmet.load_fixture(sky_size=512)),
}
IRR, RAD, MIPS, LUT, SAMPLES = 64, 512, 10, 512, 1024


def lookups():
    rad_texels = sum(6 * (RAD >> m) ** 2 for m in range(MIPS))
    mip0 = 6 * RAD * RAD
    return {"irradiance_lookups": 6 * IRR * IRR * 64 * 128,
            "radiance_texels": rad_texels,
            "radiance_lookups_glsl": rad_texels * SAMPLES,
            "radiance_lookups": (rad_texels - mip0) * SAMPLES + mip0,
            "lut_samples": LUT * LUT * SAMPLES}


def median_ms(torch, fn, repeats):
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in events:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in events]))


def bench_scene(torch, key, repeats, gen_repeats, width, height):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        st = torch.cuda.current_stream().cuda_stream
        ctx.generate_ibl(stream=st)  # warm-up: allocation, code object load
        torch.cuda.synchronize()
        passes = {"irradiance": [], "radiance": [], "lut": []}
        for _ in range(gen_repeats):
            ctx.generate_ibl(stream=st)
            info = ctx.ibl_info()
            passes["irradiance"].append(info.irradianceMs)
            passes["radiance"].append(info.radianceMs)
            passes["lut"].append(info.lutMs)
        generate_ms = median_ms(torch, lambda: ctx.generate_ibl(stream=st), gen_repeats)
        cam, _ = Camera.from_world(world, width, height).update_buffer()
        gb = [torch.empty((height, width, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        gb.append(torch.empty((height, width), dtype=torch.float32, device="cuda"))
        ptrs = tuple(x.data_ptr() for x in gb)
        ctx.trace_gbuffer(cam, width, height, jitter=False, targets=ptrs, stream=st)
        stages = {
            "ibl0": lambda: ctx.deferred_shading_device(cam, width, height, *ptrs, stream=st, ibl=0),
            "ibl1": lambda: ctx.deferred_shading_device(cam, width, height, *ptrs, stream=st, ibl=1),
        }
        for fn in stages.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: median_ms(torch, fn, repeats) for k, fn in stages.items()}
        return {"scene": name, "sky_size": int(world.skybox.shape[1]), "width": width, "height": height,
                "repeats": repeats, "gen_repeats": gen_repeats,
                "irradiance_ms": float(np.median(passes["irradiance"])),
                "radiance_ms": float(np.median(passes["radiance"])), "lut_ms": float(np.median(passes["lut"])),
                "generate_ms": generate_ms, "deferred_ibl0_ms": ms["ibl0"], "deferred_ibl1_ms": ms["ibl1"],
                "ibl_term_ms": ms["ibl1"] - ms["ibl0"]}
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--gen-repeats", type=int, default=5)
    ap.add_argument("--scenes", default="c3,fh")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    result = {"bench": "ibl", "work": lookups(), "configs": {}}
    for key in args.scenes.split(","):
        result["configs"][key] = bench_scene(torch, key, args.repeats, args.gen_repeats, args.width, args.height)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
