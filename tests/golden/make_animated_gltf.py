#!/usr/bin/env python3
"""Writes tests/golden/animated_scene.gltf: a hand-made animated glTF for the keyframe animation.

Twelve nodes, three meshes of at most 12 triangles, one camera, a point, a spot and a directional light, authored to hold

  * a chain of depth 4: carousel (animated) -> arm (static, non-uniform scale) -> wrist (animated) -> blade (static, mesh);
  * Step, Linear and CubicSpline on each of translation, rotation and scale;
  * a channel with one key (sun), a channel whose first key is at 0.5 s (lamp / bob), repeated key times (rig, lamp);
  * one sampler shared by two nodes (lamp and bob), two channels on one target (bob's translation: the later one wins);
  * a node whose static rotation is inside the 1e-3 threshold but animated (wrist);
  * a non-uniform scale above a rotation (arm above wrist), which makes normalToWorld differ from modelToWorld;
  * every light and the camera below an animated node (rig); one mesh instance under no animated node (floor);
  * rotation key pairs for every branch of slerp: one with a negative dot, one of two identical quaternions whose
    self-dot is exactly 1, the rest at least 0.3 rad apart.

Everything is authored here; nothing comes from the reference."""
import base64
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return [float(x) for x in np.float32(np.append(a * math.sin(angle / 2), math.cos(angle / 2)))]


def main():
    buf = bytearray()
    views, accessors = [], []

    def add(data, ctype, kind, **extra):
        data = np.ascontiguousarray(data)
        while len(buf) % 4:
            buf.append(0)
        views.append({"buffer": 0, "byteOffset": len(buf), "byteLength": data.nbytes})
        buf.extend(data.tobytes())
        a = {"bufferView": len(views) - 1, "componentType": ctype, "count": int(data.shape[0]), "type": kind}
        a.update(extra)
        accessors.append(a)
        return len(accessors) - 1

    def mesh(positions, triangles, material):
        p = np.asarray(positions, np.float32)
        t = np.asarray(triangles, np.uint16)
        # flat shading: one vertex per corner, the face normal on each
        corners = p[t.reshape(-1)]
        n = np.cross(corners[1::3] - corners[0::3], corners[2::3] - corners[0::3])
        n = np.repeat(n / np.linalg.norm(n, axis=1, keepdims=True), 3, axis=0).astype(np.float32)
        a_pos = add(corners, 5126, "VEC3", min=[float(x) for x in corners.min(0)], max=[float(x) for x in corners.max(0)])
        a_nrm = add(n, 5126, "VEC3")
        a_idx = add(np.arange(corners.shape[0], dtype=np.uint16), 5123, "SCALAR")
        return {"primitives": [{"attributes": {"POSITION": a_pos, "NORMAL": a_nrm}, "indices": a_idx, "material": material}]}

    # blade: a pyramid (6 triangles); floor: a quad (2); bob: an octahedron (8)
    blade = mesh([[-0.4, 0, -0.4], [0.4, 0, -0.4], [0.4, 0, 0.4], [-0.4, 0, 0.4], [0, 0.9, 0]],
                 [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [0, 2, 1], [0, 3, 2]], 0)
    floor = mesh([[-5, 0, 5], [5, 0, 5], [5, 0, -5], [-5, 0, -5]], [[0, 1, 2], [0, 2, 3]], 1)
    bob = mesh([[0.5, 0, 0], [-0.5, 0, 0], [0, 0.5, 0], [0, -0.5, 0], [0, 0, 0.5], [0, 0, -0.5]],
               [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], 2)

    samplers, channels = [], []

    def sampler(times, values, interpolation, kind):
        t = np.asarray(times, np.float32)
        a_in = add(t, 5126, "SCALAR", min=[float(t.min())], max=[float(t.max())])
        a_out = add(np.asarray(values, np.float32), 5126, kind)
        samplers.append({"input": a_in, "output": a_out, "interpolation": interpolation})
        return len(samplers) - 1

    def channel(smp, node, path):
        channels.append({"sampler": smp, "target": {"node": node, "path": path}})

    CAROUSEL, ARM, WRIST, BLADE, FLOOR, RIG, LAMP, SPOT, BOB, SUN, CAMERA, MAST = range(12)

    # carousel: cubic-spline translation, linear rotation through every slerp branch
    channel(sampler([0.0, 1.0, 2.0],
                    [[0, 0, 0], [0, 0, 0], [0.5, 0.25, 0],        # in-tangent, value, out-tangent
                     [0.25, 0, 0.5], [0.5, 0.5, 0.25], [0, -0.5, 0.25],
                     [0, 0.25, 0], [-0.25, 0.25, 0.5], [0, 0, 0]], "CUBICSPLINE", "VEC3"), CAROUSEL, "translation")
    half = [0.5, 0.5, 0.5, 0.5]  # its dot with itself is exactly 1: the mix branch
    flipped = [-x for x in quat([1, 0, 1], 1.4)]  # the same rotation as its negation: a negative dot with its neighbours
    channel(sampler([0.0, 0.4, 0.8, 1.2, 1.6, 2.0],
                    [[0, 0, 0, 1], quat([0, 1, 0], 0.8), flipped, half, half, quat([0, 1, 0], 2.4)], "LINEAR", "VEC4"),
            CAROUSEL, "rotation")
    # wrist: cubic-spline rotation (normalised), linear scale
    channel(sampler([0.0, 0.75, 2.0],
                    [[0, 0, 0, 0], quat([0, 0, 1], 0.3), [0.1, 0, 0.2, -0.05],
                     [0.05, 0.1, 0, 0], quat([1, 0, 0], 1.1), [0, -0.1, 0.1, 0.05],
                     [0, 0.05, 0.05, 0], quat([0, 1, 1], 0.7), [0, 0, 0, 0]], "CUBICSPLINE", "VEC4"), WRIST, "rotation")
    channel(sampler([0.0, 1.0, 2.0], [[1, 1, 1], [1.5, 0.75, 1.25], [0.5, 1.0, 2.0]], "LINEAR", "VEC3"), WRIST, "scale")
    # rig: step translation over repeated key times, step scale
    channel(sampler([0.0, 1.0, 1.0, 2.0], [[0, 0, 0], [0.25, 0, 0], [0.25, 0.125, 0], [0, 0.125, -0.25]], "STEP", "VEC3"),
            RIG, "translation")
    channel(sampler([0.25, 1.25], [[1, 1, 1], [1.25, 1.25, 1.25]], "STEP", "VEC3"), RIG, "scale")
    # lamp and bob share a sampler: linear translation, first key at 0.5 s, a repeated key time
    shared = sampler([0.5, 1.0, 1.0, 2.5], [[0, 2.5, 0.5], [0.5, 3.0, 0.5], [0.5, 2.0, 1.0], [-0.5, 2.5, 0.0]], "LINEAR", "VEC3")
    channel(shared, LAMP, "translation")
    # bob: an earlier channel on the same target loses to the shared sampler; cubic-spline scale
    channel(sampler([0.0, 2.0], [[9, 9, 9], [-9, -9, -9]], "LINEAR", "VEC3"), BOB, "translation")
    channel(shared, BOB, "translation")
    channel(sampler([0.0, 2.0],
                    [[0, 0, 0], [1, 1, 1], [0.5, -0.25, 0.25],
                     [-0.25, 0.5, 0], [1.5, 0.5, 1.25], [0, 0, 0]], "CUBICSPLINE", "VEC3"), BOB, "scale")
    # spot: step rotation; sun: a channel with one key
    channel(sampler([0.0, 0.9, 1.8], [quat([1, 0, 0], -1.0), quat([1, 0, 0.5], -1.3), quat([1, 0.5, 0], -0.7)], "STEP", "VEC4"),
            SPOT, "rotation")
    channel(sampler([1.0], [quat([1, 0, 0.25], -0.9)], "LINEAR", "VEC4"), SUN, "rotation")

    tiny = quat([0, 0, 1], 0.0008)  # euler angles under the 1e-3 threshold: dropped as a static component, animated anyway
    nodes = [
        {"name": "carousel", "children": [ARM, BOB], "translation": [0.0, 0.0, -0.5]},
        {"name": "arm", "children": [WRIST], "translation": [1.5, 0.25, 0.0], "scale": [1.0, 2.0, 0.5]},
        {"name": "wrist", "children": [BLADE], "rotation": tiny},
        {"name": "blade", "mesh": 0, "translation": [0.0, 0.5, 0.0], "rotation": quat([0, 0, 1], 0.5)},
        {"name": "floor", "mesh": 1, "translation": [0.0, -1.0, 0.0]},
        {"name": "rig", "children": [LAMP, SPOT, SUN, CAMERA, MAST]},
        {"name": "lamp", "translation": [0.0, 2.5, 0.5], "extensions": {"KHR_lights_punctual": {"light": 0}}},
        {"name": "spot", "translation": [1.0, 3.0, 2.0], "rotation": quat([1, 0, 0], -1.0),
         "extensions": {"KHR_lights_punctual": {"light": 1}}},
        {"name": "bob", "mesh": 2, "translation": [-1.0, 0.5, 0.0]},
        {"name": "sun", "rotation": quat([1, 0, 0], -0.8), "extensions": {"KHR_lights_punctual": {"light": 2}}},
        {"name": "camera", "camera": 0, "translation": [0.0, 1.5, 7.0], "rotation": quat([1, 0, 0], -0.15)},
        {"name": "mast", "translation": [0.0, 1.0, 0.0]},
    ]
    doc = {
        "asset": {"version": "2.0", "generator": "tests/golden/make_animated_gltf.py"},
        "extensionsUsed": ["KHR_lights_punctual"],
        "extensions": {"KHR_lights_punctual": {"lights": [
            {"type": "point", "color": [1.0, 0.8, 0.6], "intensity": 300.0},
            {"type": "spot", "color": [0.7, 0.8, 1.0], "intensity": 600.0, "range": 20.0,
             "spot": {"innerConeAngle": 0.4, "outerConeAngle": 0.8}},
            {"type": "directional", "color": [1.0, 0.95, 0.9], "intensity": 2.0},
        ]}},
        "buffers": [None],
        "bufferViews": views,
        "accessors": accessors,
        "materials": [
            {"name": "blade", "pbrMetallicRoughness": {"baseColorFactor": [0.9, 0.3, 0.2, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.5}},
            {"name": "floor", "pbrMetallicRoughness": {"baseColorFactor": [0.6, 0.6, 0.6, 1.0], "metallicFactor": 0.0, "roughnessFactor": 0.9}},
            {"name": "bob", "pbrMetallicRoughness": {"baseColorFactor": [0.2, 0.5, 0.9, 1.0], "metallicFactor": 0.5, "roughnessFactor": 0.3}},
        ],
        "meshes": [blade, floor, bob],
        "cameras": [{"type": "perspective", "perspective": {"yfov": 0.9, "znear": 0.05, "zfar": 60.0}}],
        "nodes": nodes,
        "animations": [{"name": "all", "samplers": samplers, "channels": channels}],
        "scenes": [{"nodes": [CAROUSEL, FLOOR, RIG]}],
        "scene": 0,
    }
    doc["buffers"][0] = {"byteLength": len(buf), "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(buf)).decode("ascii")}
    with open(os.path.join(HERE, "animated_scene.gltf"), "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote animated_scene.gltf (%d buffer bytes)" % len(buf))


if __name__ == "__main__":
    main()
