#!/usr/bin/env python3
"""The particle system at 1920x1080 (prosper_pt_particles) on S-cornell (C2's scene), the C4 scene
(sponza_class with lights and foliage) and the FlightHelmet fixture, with prosper's pool of 500 000 slots.

Per scene, in one process: a reset step makes one emitter per vertex of the source draw instance (the one whose mesh has
the most vertices), `--warmup` steps at dt = 1/60 without render let the live count settle (a child lives 4 s = 240
steps; an emitter spawns every 0.1 s, so the pool settles at 41 particles per emitter or, when that is more than the pool
holds, full with spawns refused), then `--repeats` whole steps are measured.  Before each measured step the frame up to
the pass is made again (traced G-buffer, deferred shading, sky), since render writes the illumination and the depth.

  stage_ms        median (_mean, _max) device time per stage over the measured steps: the library's own events
                  (prosper_pt_get_particles_info); init runs in the reset step only (reset_step_ms has it), later its
                  interval is the gap between two event records
  per_step_mean   live, granted, refused, freed and fragments per measured step: the emitters spawn in phase, every
                  sixth step (spawning_steps of the measured ones), and their children die in phase too
  bytes, gbps     the bytes each stage's kernels ask for under those mean counts, and that over the stage's mean time:
                    decay     20 B per slot (position_lifetime, mask), 20 B per freed slot
                    simulate  16 B per slot, 20 + 32 B more per live slot, 32 B more per emitter, 164 B per child
                              (staged, read back, written to its slot, its freelist entry)
                    render    16 B per slot, 4 B more per live slot; 8 B per pixel for the keys, 36 B per written pixel
                  (records are 64 B apart, so the memory system moves whole lines: this is the demand, not DRAM traffic)
Prints one JSON object.

    python scripts/particles_bench.py [--repeats 30] [--warmup 300] [--scenes c2,c4,fh] [--size 1920x1080] [--slots 0]
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
DT = 1.0 / 60.0
STAGES = ("decay", "init", "simulate", "render")
NO_RENDER = S.PARTICLES_DECAY | S.PARTICLES_INIT | S.PARTICLES_SIMULATE


def stage_ms(info):
    return [info.decayMs, info.initMs, info.simulateMs, info.renderMs]


def bench_scene(key, repeats, warmup, width, height, slots):
    name, make = SCENES[key]
    world = make()
    f = world.freeze()
    counts = [world.mesh_infos[f["draw_instances"][i].meshIndex].vertexCount for i in range(f["draw_instance_count"])]
    source = int(np.argmax(counts))
    pool = slots or S.MAX_PARTICLE_COUNT
    ctx = capi.Context(0)
    try:
        ctx.upload_scene(world)
        hcam = Camera.from_world(world, width, height)
        cam, _ = hcam.update_buffer()

        def frame():
            capi._check(capi.lib().prosper_pt_trace_gbuffer(ctx._h, 0, 0, 0, C.byref(cam), width, height, None, None))
            inp, _, _ = ctx.gbuffer_device_ptrs()
            ctx.deferred_shading_device(cam, width, height, inp.albedoRoughness, inp.normalMetallic, inp.nonLinearDepth)
            ctx.skybox_fill(cam, width, height)

        def step(k, stages, reset=0):
            ctx.particles(S.ParticlesPC(slots, source, reset, DT, k, k % 64), stages, cam, width, height)
            return ctx.particles_info()

        frame()
        info = step(1, S.PARTICLES_ALL, reset=1)
        assert info.initRecorded == 1
        emitters, reset_ms = info.liveCount - info.grantedSpawns, stage_ms(info)
        history = []
        for k in range(2, 2 + warmup):
            info = step(k, NO_RENDER)
            history.append(info.liveCount)
        rows, before = [], info.liveCount
        for k in range(2 + warmup, 2 + warmup + repeats):
            frame()
            info = step(k, S.PARTICLES_ALL)
            freed = before + info.grantedSpawns - info.liveCount
            rows.append(stage_ms(info) + [info.liveCount, info.grantedSpawns, info.refusedSpawns, freed, info.fragmentsWritten])
            before = info.liveCount
        rows = np.array(rows, np.float64)
        ms, mean = rows[:, :4], rows.mean(axis=0)
        live, granted, refused, freed, fragments = mean[4:]
        pixels = width * height
        demand = {
            "decay": 20 * pool + 20 * freed,
            "init": 0,
            "simulate": 16 * pool + 52 * live + 32 * emitters + 164 * granted,
            "render": 16 * pool + 4 * live + 8 * pixels + 36 * fragments,
        }

        def per_stage(v):
            return dict(zip(STAGES, (float(x) for x in v)))
        return {
            "scene": name, "width": width, "height": height, "repeats": repeats, "warmup_steps": warmup, "dt": DT,
            "slots": pool, "source_draw_instance": source, "emitters": int(emitters),
            "reset_step_ms": per_stage(reset_ms),
            "stage_ms": per_stage(np.median(ms, axis=0)), "stage_ms_mean": per_stage(ms.mean(axis=0)),
            "stage_ms_max": per_stage(ms.max(axis=0)),
            "step_ms": float(np.median(ms.sum(axis=1))),
            "per_step_mean": {"live": float(live), "granted": float(granted), "refused": float(refused), "freed": float(freed),
                              "fragments": float(fragments)},
            "live_min_max": [int(rows[:, 4].min()), int(rows[:, 4].max())],
            "spawning_steps": int((rows[:, 5] + rows[:, 6] > 0).sum()),
            "live_settled": bool(len(history) >= 240 and max(history[-240:]) == max(history[-120:])),
            "live_during_warmup": [int(v) for v in history[::max(1, len(history) // 10)]],
            "bytes": {k: int(v) for k, v in demand.items()},
            "gbps": {k: (float(demand[k] / (ms[:, i].mean() * 1e-3) / 1e9) if ms[:, i].mean() > 0 else 0.0)
                     for i, k in enumerate(STAGES)},
        }
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--scenes", default="c2,c4,fh")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--slots", type=int, default=0, help="maxParticleCount; 0: prosper's 500 000")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.lower().split("x"))
    results = [bench_scene(k, args.repeats, args.warmup, w, h, args.slots) for k in args.scenes.split(",")]
    print(json.dumps({"bench": "particles", "scenes": results}))


if __name__ == "__main__":
    main()
