"""Meshlets in an uploaded scene (World.add_meshlets): the sections ride along in the geometry buffers the
library uploads as they are, and nothing that exists reads them - the traced G-buffer is the same to the bit."""
import numpy as np
import pytest

from conftest import same_bits
from prosper_amd import meshlets as M, scenes

pytestmark = pytest.mark.gpu


def test_a_scene_with_meshlets_uploads_and_traces_as_before(gpu_ctx, oracle):
    w, h = 96, 64
    plain = scenes.cornell(with_skybox=True)
    c = plain.camera
    cam = oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], w, h)[0]
    gpu_ctx.upload_scene(plain)
    want = gpu_ctx.trace_gbuffer(cam, w, h)
    world = scenes.cornell(with_skybox=True)
    added = world.add_meshlets()
    assert added >= len(world.metadatas) and all(i.meshletCount > 0 for i in world.mesh_infos)
    f = world.freeze()
    assert f["geometry_buffers"][0].size > plain.freeze()["geometry_buffers"][0].size
    for md, info in zip(world.metadatas, world.mesh_infos):
        got = M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info)
        assert int(got["meshlets"][:, 3].sum()) * 3 == info.indexCount  # every triangle of the mesh, once
    gpu_ctx.upload_scene(world)
    got = gpu_ctx.trace_gbuffer(cam, w, h)
    for a, b in zip(got, want):
        assert same_bits(a, b).all()
    assert (want[2] > 0).any()
