#!/usr/bin/env python3
"""prosper_pt_compress_texture on square RGBA8 images of 1024, 2048 and 4096 texels a side with full mip
chains, and on every texture of the FlightHelmet fixture (64 x 64).

Per case: `call_ms`, the host clock around the whole call (source up, tiling, mip generation, encoding, payload back; the
call ends in a stream synchronise), and the three stages of it between events on the stream (`prepare_ms`, `encode_ms` =
the encode kernels of all levels, `readback_ms`; prosper_pt_get_compress_texture_timing) - each the median over
`--repeats` calls after warm-up, with the minimum beside it.  `mtexels_per_s` is level 0's texel count over `encode_ms`.
`psnr_db` is decode(encode) of level 0 against the source over all four channels (bc7.decode_image; null for an exact
round trip), `modes` the histogram of the chosen modes over all levels.  `host_encode_1024_s` is bc7.encode_image on the
host for the 1024 x 1024 image's level 0: the only path a caller had.  The images are seeded: smooth regions, noise and
an opaque half, so that every candidate is chosen somewhere.  Prints ONE JSON object.

    python scripts/bc7_encode_bench.py [--repeats 20] [--sizes 1024,2048,4096] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import bc7, capi, flight_helmet, structs as S  # noqa: E402


def test_image(size, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float32) / size
    img = np.stack([0.5 + 0.5 * np.sin(9 * x + 3 * y), x * y, 0.5 + 0.5 * np.cos(14 * y), 0.3 + 0.7 * x], axis=2)
    img = img * 255.0 + rng.normal(0.0, 3.0, img.shape)
    img[size // 2:, : size // 2] = rng.integers(0, 256, (size - size // 2, size // 2, 4))       # a quarter of noise
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[: size // 2, :, 3] = 255                                                                  # an opaque half
    return img


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return None if mse == 0.0 else float(10.0 * np.log10(255.0 ** 2 / mse))


def mode_histogram(levels):
    first = np.concatenate([np.frombuffer(l, np.uint8).reshape(-1, 16)[:, 0] for l in levels]).astype(np.int64)
    mode = np.log2(first & -first).astype(np.int64)
    return {str(m): int((mode == m).sum()) for m in (4, 5, 6)}


def bench_case(ctx, img, srgb, repeats):
    h, w = img.shape[:2]
    for _ in range(3):
        fmt, levels = ctx.compress_texture(img, srgb=srgb, mips=True)
    call, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.compress_texture(img, srgb=srgb, mips=True)
        call.append((time.perf_counter() - t0) * 1e3)
        stages.append(ctx.compress_texture_timing())
    stages = np.array(stages)
    out = {"width": w, "height": h, "srgb": bool(srgb), "levels": len(levels), "format": "BC7" if fmt == S.FORMAT_BC7_UNORM else "RGBA8",
           "call_ms": float(np.median(call)), "call_ms_min": float(np.min(call))}
    for k, name in enumerate(("prepare_ms", "encode_ms", "readback_ms")):
        out[name] = float(np.median(stages[:, k]))
        out[name + "_min"] = float(stages[:, k].min())
    if fmt == S.FORMAT_BC7_UNORM:
        out["mtexels_per_s"] = w * h / out["encode_ms"] / 1e3
        out["psnr_db"] = psnr(bc7.decode_image(levels[0], w, h), img)
        out["modes"] = mode_histogram(levels)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--no-host", action="store_true", help="skip the host encode of the 1024 x 1024 image")
    args = ap.parse_args()
    import torch
    ctx = capi.Context(0)
    try:
        result = {"bench": "bc7_encode", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "images": [], "flight_helmet": []}
        for size in (int(v) for v in args.sizes.split(",")):
            result["images"].append(bench_case(ctx, test_image(size, size), True, args.repeats))
        world = flight_helmet.load_fixture(sky_size=0)
        for index, t in enumerate(world.textures):
            t = np.asarray(t)
            if index == 0 or t.shape[0] < 4:
                continue
            r = bench_case(ctx, t, False, args.repeats)
            r["texture"] = index
            result["flight_helmet"].append(r)
        if not args.no_host:
            img = test_image(1024, 1024)
            t0 = time.perf_counter()
            payload = bc7.encode_image(img)
            result["host_encode_1024_s"] = time.perf_counter() - t0
            result["host_equals_gpu_1024"] = payload == ctx.compress_texture(img, mips=False)[1][0]
    finally:
        ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
