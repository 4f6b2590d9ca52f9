#!/usr/bin/env python3
"""prosper_pt_prepare_mesh on the meshes of the FlightHelmet fixture and of C3 (scenes.sponza_class()):
tangents generated (the sources are handed over without theirs), meshlets on.

The source streams are what the world's buffers hold, decoded: fp16 positions and uvs, snorm10 normals.  Per scene,
summed over its meshes: `call_ms`, the host clock around the whole call (source up, kernels, partition, blob and tangents
back; the call ends in a stream synchronise), and its stages (prosper_pt_get_prepare_mesh_timing: `tangents_ms`,
`pack_ms`, `bounds_ms`, `readback_ms` between events on the stream, `meshlet_host_ms` the partition on the host's clock)
- each mesh's figure the median over `--repeats` calls after warm-up, the sums of the minima beside them.  `host_s` is
the path a caller had before: tangents.generate_tangents + mesh_cache.pack_cache(with_meshlets=True, ordered=True) in
NumPy, once per mesh, with its two parts apart (`host_tangents_s`, `host_pack_s`); `equal` says that both paths gave the
same header, blob and tangents for every mesh.  `largest` repeats the figures for the scene's largest mesh alone.
Prints ONE JSON object.

    python scripts/mesh_prepare_bench.py [--repeats 20] [--scenes flight_helmet,c3] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prosper_amd import capi, flight_helmet, mesh_cache, scenes, structs as S, tangents as T  # noqa: E402

SCENES = {"flight_helmet": lambda: flight_helmet.load_fixture(sky_size=0), "c3": lambda: scenes.sponza_class()}
STAGES = ("tangents_ms", "pack_ms", "meshlet_host_ms", "bounds_ms", "readback_ms")


def mesh_source(world, index):
    """positions, indices, normals, uvs of a loaded mesh as float32 / uint32 (its tangents are left behind)"""
    md, info = world.metadatas[index], world.mesh_infos[index]
    positions, indices = world.mesh_geometry(index)
    words = world._buffer_words_of(md.bufferIndex)
    n = info.vertexCount
    normals = uvs = None
    if md.normalsOffset != S.ABSENT:
        w = words[md.normalsOffset:md.normalsOffset + n]
        fields = [(w << np.uint32(22 - s)).view(np.int32) >> 22 for s in (0, 10, 20)]
        normals = np.maximum(np.stack(fields, axis=1).astype(np.float32) / np.float32(511), np.float32(-1))
    if md.texCoord0sOffset != S.ABSENT:
        uvs = words[md.texCoord0sOffset:md.texCoord0sOffset + n].view(np.float16).reshape(n, 2).astype(np.float32)
    return dict(positions=positions, indices=indices, normals=normals, uvs=uvs)


def bench_mesh(ctx, src, repeats, host):
    args = dict(normals=src["normals"], uvs=src["uvs"], generate_tangents=src["normals"] is not None, meshlets=True)
    for _ in range(2):
        header, blob, tangents = ctx.prepare_mesh(src["positions"], src["indices"], **args)
    call, stages = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ctx.prepare_mesh(src["positions"], src["indices"], **args)
        call.append((time.perf_counter() - t0) * 1e3)
        stages.append(ctx.prepare_mesh_timing())
    stages = np.array(stages)
    out = {"vertices": int(header["vertexCount"]), "triangles": int(header["indexCount"]) // 3, "meshlets": int(header["meshletCount"]),
           "blob_bytes": int(header["blobByteCount"]), "tangents_generated": tangents is not None,
           "call_ms": float(np.median(call)), "call_ms_min": float(np.min(call))}
    for k, name in enumerate(STAGES):
        out[name] = float(np.median(stages[:, k]))
        out[name + "_min"] = float(stages[:, k].min())
    if host:
        t0 = time.perf_counter()
        want = None
        if tangents is not None:
            want = T.generate_tangents(src["positions"], src["normals"], src["uvs"], src["indices"])
        t1 = time.perf_counter()
        wh, wb = mesh_cache.pack_cache(src["positions"], src["indices"], src["normals"], want, src["uvs"], with_meshlets=True, ordered=True)
        t2 = time.perf_counter()
        out.update(host_tangents_s=t1 - t0, host_pack_s=t2 - t1, host_s=t2 - t0)
        out["equal"] = bool(header == dict(wh, blobByteCount=int(wb.size) * 4) and np.array_equal(blob, wb) and
                            (want is None or want.tobytes() == tangents.tobytes()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--scenes", default="flight_helmet,c3")
    ap.add_argument("--no-host", action="store_true", help="skip the NumPy path")
    args = ap.parse_args()
    import torch
    ctx = capi.Context(0)
    try:
        result = {"bench": "mesh_prepare", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "scenes": {}}
        for name in args.scenes.split(","):
            world = SCENES[name]()
            meshes = [bench_mesh(ctx, mesh_source(world, i), args.repeats, not args.no_host)
                      for i, info in enumerate(world.mesh_infos) if info.indexCount]
            total = {"meshes": len(meshes)}
            for key in meshes[0]:
                if key == "equal":
                    total[key] = all(m[key] for m in meshes)
                elif key != "tangents_generated":
                    total[key] = type(meshes[0][key])(sum(m[key] for m in meshes))
            total["tangents_generated"] = sum(1 for m in meshes if m["tangents_generated"])
            total["largest"] = max(meshes, key=lambda m: m["triangles"])
            result["scenes"][name] = total
    finally:
        ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
