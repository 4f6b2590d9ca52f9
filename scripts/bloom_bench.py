#!/usr/bin/env python3
"""Bloom at 1920x1080: the passes of render::bloom::Bloom's multi-resolution blur (prosper_pt_bloom) stage by stage, at
half and at quarter resolution, on S-cornell (C2's scene), the C4 scene (sponza_class with the sun and 1024 punctual
lights) and the FlightHelmet fixture.

The input is the traced, shaded and sky-filled image: the pixel-centre G-buffer, deferred shading and
prosper_pt_skybox_fill of the same context; bloom then runs in place (the image is restored from a device copy before
every launch, outside the timed stages).  The threshold is chosen per scene as the `--lit` quantile (0.7 by default) of
the image's brightest channel, so that highlights are non-zero on about 30 % of the texels; `lit_share` is the share of
level 0 of the highlights that is non-zero, measured.  The streak's cost does not depend on it.  Each stage's time is
the device time between the events the library records around it (prosper_pt_get_bloom_info), the median over
`--repeats` launches after warm-up; `streak_ms` is the horizontal pass of level 1, which carries the streak.
`deferred_shading_ms` (trace + clustering + shading) of the same run is the yardstick.

`--technique fft` times the FFT technique (prosper_pt_bloom_fft) on the same images instead: the stages of
a call that keeps the kernel's DFT, the stages that remake it (`regenerateKernel`, fewer launches), the bytes per
second of the two row launches (dim^2 texels of 16 bytes read and written; the forward one reads 8-byte texels) and of the
fused middle (the image read and written, the kernel's DFT read), and `transform_alone`: one 2-D transform in place at every dim from 256
to 4096.  The default run and its JSON are as they were.

`--compare-lib PATH` times the same passes once more in a child process that loads another build of the library
(PROSPER_PT_LIB), e.g. one with another streak kernel, and adds its `streak_ms` and whether the streak pass's output
bytes are the same.  Prints one JSON object.

    python scripts/bloom_bench.py [--repeats 60] [--scenes c2,c4,fh] [--compare-lib build/variants/lib_x.so --compare-label x]
    python scripts/bloom_bench.py --technique fft [--repeats 60] [--scenes c2,c4,fh]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

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
SCALES = (("half", S.BLOOM_HALF), ("quarter", S.BLOOM_QUARTER))


def stage_times(info):
    first = info.firstLevel
    out = {"separate": info.separateMs, "reduce": info.reduceMs, "compose": info.composeMs}
    for n in range(3):
        out["blur_horizontal_level%d" % (first + n)] = info.blurHorizontalMs[n]
        out["blur_vertical_level%d" % (first + n)] = info.blurVerticalMs[n]
    return out


FFT_STAGES = ("separate", "generate", "prepare", "kernel_fft", "forward_fft", "convolution", "inverse_fft", "compose")


def fft_stage_times(info):
    return dict(zip(FFT_STAGES, (info.separateMs, info.generateMs, info.prepareMs, info.kernelFftMs, info.forwardFftMs,
                                 info.convolutionMs, info.inverseFftMs, info.composeMs)))


def bench_fft(ctx, copy_back, threshold, scale, repeats, width, height, st):
    """The FFT technique at one resolution scale: medians of the kept-kernel call, and of the one that remakes the kernel."""
    kept, remade, whole = {}, {}, []
    for regenerate, n, into in ((1, min(repeats, 5) + 1, remade), (0, repeats + 3, kept)):
        pc = S.BloomFftPC.default(threshold, scale, 1, regenerate)
        for i in range(n):
            copy_back()
            ctx.bloom_fft(pc, width, height, stream=st)
            info = ctx.bloom_fft_info()
            if i >= (1 if regenerate else 3):
                times = fft_stage_times(info)
                for k, v in times.items():
                    into.setdefault(k, []).append(v)
                if not regenerate:
                    whole.append(sum(times.values()))
    kept = {k: float(np.median(v)) for k, v in kept.items()}
    remade = {k: float(np.median(v)) for k, v in remade.items()}
    texels = info.dim * info.dim
    # forward_fft and inverse_fft are the row launches alone (fp16 texels in on the way forward); the middle, timed as
    # the convolution, reads the image and the kernel's DFT and writes the image
    moved = {"forward_fft": texels * (8 + 16), "convolution": texels * 48, "inverse_fft": texels * 32}
    highlights = ctx.read_bloom_fft_stage(S.BLOOM_FFT_HIGHLIGHTS, stream=st)
    return {
        "dim": info.dim, "kernel_dim": info.kernelDim, "convolution_scale": info.convolutionScale, "fused": info.fused,
        "lit_share": float(highlights[..., :3].any(axis=-1).mean()),
        "stage_ms": kept, "bloom_ms": float(np.median(whole)),
        "kernel_remade_stage_ms": {k: remade[k] for k in ("generate", "prepare", "kernel_fft")},
        "transform_tb_per_s": {k: moved[k] / (kept[k] * 1e-3) / 1e12 for k in moved},
        "kernel_fft_tb_per_s": texels * 64 / (remade["kernel_fft"] * 1e-3) / 1e12,
        "output_crc32": zlib.crc32(ctx.read_hdr().tobytes()),
    }


def bench_scene(torch, key, repeats, width, height, lit, technique="blur"):
    name, make = SCENES[key]
    world = make()
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        cam, _ = Camera.from_world(world, width, height).update_buffer()
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
        ctx.deferred_shading_traced(cam, width, height, stream=st)
        fill_ms = timed(lambda: ctx.skybox_fill(cam, width, height, stream=st))
        image = ctx.read_hdr()
        threshold = float(np.quantile(image[..., :3].max(axis=-1), lit))
        ptr, _ = ctx.hdr_device_ptr()
        keep = torch.empty(width * height * 4, dtype=torch.float32, device="cuda")
        hip = C.CDLL("libamdhip64.so")

        def copy(dst, src):
            assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(width * height * 16), 3, C.c_void_p(st)) == 0
        copy(keep.data_ptr(), ptr)
        out = {"scene": name, "width": width, "height": height, "repeats": repeats, "threshold": threshold,
               "deferred_shading_ms": shading_ms, "skybox_fill_ms": fill_ms}
        for label, scale in SCALES:
            if technique == "fft":
                out[label] = bench_fft(ctx, lambda: copy(ptr, keep.data_ptr()), threshold, scale, repeats, width, height, st)
                continue
            pc = S.BloomPC.default(threshold=threshold, resolution_scale=scale)
            per_stage, whole = {}, []
            for i in range(repeats + 3):
                copy(ptr, keep.data_ptr())
                ctx.bloom(pc, width, height, stream=st)
                info = ctx.bloom_info()
                if i >= 3:
                    times = stage_times(info)
                    for k, v in times.items():
                        per_stage.setdefault(k, []).append(v)
                    whole.append(sum(times.values()))
            level0 = ctx.read_bloom_stage(S.BLOOM_HIGHLIGHTS, 0, stream=st)
            streak_out = ctx.read_bloom_stage(S.BLOOM_HORIZONTAL, 1, stream=st)
            stage_ms = {k: float(np.median(v)) for k, v in per_stage.items()}
            out[label] = {
                "working_extent": [info.workingWidth, info.workingHeight], "streak_half_width": info.streakHalfWidth,
                "lit_share": float(level0[..., :3].any(axis=-1).mean()),
                "stage_ms": stage_ms, "streak_ms": stage_ms["blur_horizontal_level1"], "bloom_ms": float(np.median(whole)),
                "streak_output_crc32": zlib.crc32(streak_out.tobytes()),
            }
        return out
    finally:
        ctx.close()


def bench_transform_alone(torch, repeats):
    """prosper_pt_bloom_fft_transform in place on a device image at every dim it takes: a row and a column launch, each
    reading and writing dim^2 texels of 16 bytes."""
    ctx = capi.Context(0)
    try:
        st = torch.cuda.current_stream().cuda_stream
        out = {}
        for dim in (256, 512, 1024, 2048, 4096):
            image = torch.randn(dim * dim * 4, dtype=torch.float32, device="cuda")
            ev = []
            for i in range(repeats + 3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = capi.lib().prosper_pt_bloom_fft_transform(ctx._h, dim, 0, C.c_void_p(image.data_ptr()), C.c_void_p(image.data_ptr()),
                                                               1, C.c_void_p(st))
                assert rc == 0
                b.record()
                ev.append((a, b))
            torch.cuda.synchronize()
            ms = float(np.median([a.elapsed_time(b) for a, b in ev[3:]]))
            out[str(dim)] = {"ms": ms, "tb_per_s": dim * dim * 64 / (ms * 1e-3) / 1e12}
        return out
    finally:
        ctx.close()


def main_fft(args):
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(torch, k, args.repeats, w, h, args.lit, "fft") for k in args.scenes.split(",")]
    print(json.dumps({"bench": "bloom_fft", "device": torch.cuda.get_device_name(0), "scenes": results,
                      "transform_alone": bench_transform_alone(torch, args.repeats)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=60)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--lit", type=float, default=0.7, help="the quantile of the brightest channel that becomes the threshold")
    ap.add_argument("--label", default="row_staged", help="what to call the streak kernel of the library this process loads")
    ap.add_argument("--technique", default="blur", choices=("blur", "fft"), help="fft: prosper_pt_bloom_fft instead of prosper_pt_bloom")
    ap.add_argument("--compare-lib", default=None, help="another build of the library, timed in a child process")
    ap.add_argument("--compare-label", default="other")
    args = ap.parse_args()
    if args.technique == "fft":
        return main_fft(args)
    compare = None
    if args.compare_lib:
        env = dict(os.environ, PROSPER_PT_LIB=os.path.abspath(args.compare_lib))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--scenes", args.scenes,
                                "--size", args.size, "--lit", str(args.lit), "--label", args.compare_label],
                               env=env, capture_output=True, text=True, check=True)
        compare = json.loads(child.stdout.strip().splitlines()[-1])
    import torch
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(torch, k, args.repeats, w, h, args.lit) for k in args.scenes.split(",")]
    if compare:
        for mine, other in zip(results, compare["scenes"]):
            for label, _ in SCALES:
                mine[label]["streak_ms_by_kernel"] = {args.label: mine[label]["streak_ms"], args.compare_label: other[label]["streak_ms"]}
                mine[label]["bloom_ms_by_kernel"] = {args.label: mine[label]["bloom_ms"], args.compare_label: other[label]["bloom_ms"]}
                mine[label]["streak_outputs_identical"] = mine[label]["streak_output_crc32"] == other[label]["streak_output_crc32"]
    print(json.dumps({"bench": "bloom", "device": torch.cuda.get_device_name(0), "streak_kernel": args.label,
                      "compared_with": args.compare_label if compare else None, "scenes": results}))


if __name__ == "__main__":
    main()
