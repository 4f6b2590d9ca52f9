"""glTF nodes and animations -> the tables of `prosper_pt_set_animations`.

What the reference keeps of a glTF's node tree and animations (`src/scene/WorldData.cpp:960-1122` loadAnimations,
`:1124-1362` loadScenes, `:1364-1456` gatherScene) as flat tables:

  * nodes in prosper's scene-node order: a root takes the next index, and when a node comes off the LIFO stack its
    children take the next indices together - so a parent always precedes its child;
  * that walk pops nodes in the order `gltf.load_gltf` pops them, so a node's model instance and light indices are the
    ones `load_gltf` assigned (model instances, point and spot lights count up as their nodes come off the stack);
  * the node that carries glTF camera 0 (if perspective) is the CAMERA node, the last directional light's node the
    DIRECTIONAL_LIGHT one (`load_gltf`: the last sun in traversal order wins);
  * per node its static translation / rotation / scale and which of them the reference keeps (`gltf.node_trs`);
  * one channel per glTF channel whose target is a translation, rotation or scale of a node of the scene, in file order
    (the last one on a (node, path) wins), with its sampler's key times, values, interpolation and the input accessor's
    min / max.

`load_gltf` itself is untouched: this module reads the same file a second time.
"""
import ctypes as C

import numpy as np

from . import structs as S
from .gltf import GltfError, _Document, node_trs

_PATHS = {"translation": S.ANIMATION_PATH_TRANSLATION, "rotation": S.ANIMATION_PATH_ROTATION, "scale": S.ANIMATION_PATH_SCALE}
_INTERPOLATIONS = {"STEP": S.ANIMATION_STEP, "LINEAR": S.ANIMATION_LINEAR, "CUBICSPLINE": S.ANIMATION_CUBICSPLINE}


class AnimationTables:
    """nodes: list of structs.AnimationNode; channels: list of structs.AnimationChannel; times / values: float32 arrays;
    gltf_nodes: the glTF node index of every scene node."""

    def __init__(self, nodes, channels, times, values, gltf_nodes=None):
        self.nodes = list(nodes)
        self.channels = list(channels)
        self.times = np.ascontiguousarray(times, np.float32).reshape(-1)
        self.values = np.ascontiguousarray(values, np.float32).reshape(-1)
        self.gltf_nodes = list(gltf_nodes) if gltf_nodes is not None else list(range(len(self.nodes)))

    @property
    def end_time(self):
        return max([float(c.endTimeS) for c in self.channels], default=0.0)

    def desc(self):
        """A prosper_pt_animation_desc over arrays this object keeps alive."""
        self._nodes = (S.AnimationNode * max(1, len(self.nodes)))(*self.nodes)
        self._channels = (S.AnimationChannel * max(1, len(self.channels)))(*self.channels)
        d = S.AnimationDesc()
        d.struct_size = C.sizeof(S.AnimationDesc)
        d.nodeCount = len(self.nodes)
        d.nodes = C.cast(self._nodes, C.c_void_p)
        d.channelCount = len(self.channels)
        d.channels = C.cast(self._channels, C.c_void_p)
        d.timeCount = int(self.times.size)
        d.times = self.times.ctypes.data
        d.valueCount = int(self.values.size)
        d.values = self.values.ctypes.data
        return d


def load_animations(path, scene=None):
    """The AnimationTables of `path` (.gltf or .glb) for the scene `gltf.load_gltf(path, scene=scene)` loads."""
    d = _Document(path)
    doc = d.doc
    gltf_nodes = doc.get("nodes", [])
    lights = doc.get("extensions", {}).get("KHR_lights_punctual", {}).get("lights", [])
    scenes = doc.get("scenes", [])
    roots = scenes[doc.get("scene", 0) if scene is None else scene].get("nodes", []) if scenes else []

    nodes, source = [], []  # scene nodes, and the glTF node each one came from

    def new_node(parent):
        n = S.AnimationNode()
        n.parent, n.modelInstance, n.pointLight, n.spotLight = parent, S.ANIMATION_NONE, S.ANIMATION_NONE, S.ANIMATION_NONE
        nodes.append(n)
        source.append(None)
        return len(nodes) - 1

    instances = points = spots = 0
    camera_node = sun_node = None
    for root in roots:
        stack = [(root, new_node(S.ANIMATION_NONE))]
        while stack:
            index, scene_index = stack.pop()
            g = gltf_nodes[index]
            source[scene_index] = index
            for child in g.get("children", []):
                stack.append((child, new_node(scene_index)))
            n = nodes[scene_index]
            (t, r, s), (has_t, has_r, has_s) = node_trs(g)
            n.translation[:], n.rotation[:], n.scale[:] = [float(x) for x in t], [float(x) for x in r], [float(x) for x in s]
            n.flags = ((S.NODE_HAS_TRANSLATION if has_t else 0) | (S.NODE_HAS_ROTATION if has_r else 0) |
                       (S.NODE_HAS_SCALE if has_s else 0))
            if "mesh" in g:
                n.modelInstance = instances
                instances += 1
            if g.get("camera") == 0 and camera_node is None and doc["cameras"][0].get("type") == "perspective":
                camera_node = scene_index
            light_index = g.get("extensions", {}).get("KHR_lights_punctual", {}).get("light")
            if light_index is not None:
                kind = lights[light_index]["type"]
                if kind == "directional":
                    sun_node = scene_index
                elif kind == "point":
                    n.pointLight = points
                    points += 1
                elif kind == "spot":
                    n.spotLight = spots
                    spots += 1
    if camera_node is not None:
        nodes[camera_node].flags |= S.NODE_CAMERA
    if sun_node is not None:
        nodes[sun_node].flags |= S.NODE_DIRECTIONAL_LIGHT
    scene_node_of = {g: i for i, g in enumerate(source)}

    channels, times, values = [], [], []
    time_floats = value_floats = 0
    for anim in doc.get("animations", []):
        for ch in anim.get("channels", []):
            target = ch.get("target", {})
            if target.get("path") not in _PATHS or target.get("node") not in scene_node_of:
                continue  # morph-target weights, and nodes of other scenes
            smp = anim["samplers"][ch["sampler"]]
            interpolation = _INTERPOLATIONS.get(smp.get("interpolation", "LINEAR"))
            if interpolation is None:
                raise GltfError("unsupported animation interpolation '%s'" % smp.get("interpolation"))
            accessor = doc["accessors"][smp["input"]]
            t = d.floats(smp["input"]).reshape(-1)
            v = d.floats(smp["output"])
            path = _PATHS[target["path"]]
            if v.shape[1] != (4 if path == S.ANIMATION_PATH_ROTATION else 3):
                raise GltfError("animation output of a %s channel is %d floats wide" % (target["path"], v.shape[1]))
            if v.shape[0] != t.size * (3 if interpolation == S.ANIMATION_CUBICSPLINE else 1):
                raise GltfError("animation output count does not match its key times")
            c = S.AnimationChannel()
            c.node, c.path, c.interpolation = scene_node_of[target["node"]], path, interpolation
            c.timeOffset, c.keyCount, c.valueOffset, c.valueWidth = time_floats, int(t.size), value_floats, int(v.shape[1])
            # (the reference asserts that the input accessor carries min and max, WorldData.cpp:1047-1054)
            c.startTimeS = float(np.float32(accessor["min"][0])) if "min" in accessor else float(t.min())
            c.endTimeS = float(np.float32(accessor["max"][0])) if "max" in accessor else float(t.max())
            channels.append(c)
            times.append(t)
            values.append(v.reshape(-1))
            time_floats += int(t.size)
            value_floats += int(v.size)
    return AnimationTables(nodes, channels, np.concatenate(times) if times else np.zeros(0, np.float32),
                           np.concatenate(values) if values else np.zeros(0, np.float32), source)
