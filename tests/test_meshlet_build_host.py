"""The host partition of prosper_pt_prepare_mesh (prosper_amd/csrc/meshlet_build.cpp) as a stand-alone
program built with AddressSanitizer + UBSan: its bytes against prosper_amd.meshlets.build_meshlets.  CPU only; nothing
is preloaded and no code loaded into Python is sanitised."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from prosper_amd import meshlets as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def strip(triangles, ring=None):
    """(i, i+1, i+2); over `ring` vertices that it wraps around, or over triangles + 2 of its own"""
    i = np.arange(triangles)
    tri = np.stack([i, i + 1, i + 2], axis=1)
    if ring:
        return ring, (tri % ring).astype(np.uint32)
    return triangles + 2, tri.astype(np.uint32)


def soup(triangles):
    return 3 * triangles, np.arange(3 * triangles, dtype=np.uint32).reshape(-1, 3)


def fan(triangles, rim):
    i = np.arange(triangles)
    return rim + 1, np.stack([np.zeros_like(i), 1 + i % rim, 1 + (i + 1) % rim], axis=1).astype(np.uint32)


# name -> (vertex count, triangles [m, 3]); the meshlet count each must give is in EXPECTED
CASES = {
    "one_triangle": (3, np.array([[0, 1, 2]], np.uint32)),
    "strip_exactly_64_vertices": strip(62),
    "strip_65_vertices": strip(63),
    "strip_exactly_124_triangles": strip(124, ring=20),
    "strip_125_triangles": strip(125, ring=20),
    "soup_vertex_limit_first": soup(50),
    "fan_triangle_limit_first": fan(300, rim=40),
    "soup_257_meshlets": soup(257 * 21),
    "soup_past_65535_vertices": soup(21846),
    "repeated_index": (70, np.array([[i, i, i + 1] for i in range(69)], np.uint32)),
}
EXPECTED = {"one_triangle": 1, "strip_exactly_64_vertices": 1, "strip_65_vertices": 2, "strip_exactly_124_triangles": 1,
            "strip_125_triangles": 2, "soup_vertex_limit_first": 3, "fan_triangle_limit_first": 3, "soup_257_meshlets": 257,
            "soup_past_65535_vertices": 1041, "repeated_index": 2}


def partition_of(built):
    return (np.asarray(built["meshlets"], np.uint32).tobytes(), np.asarray(built["vertices"], np.uint32).tobytes(),
            np.asarray(built["triangles"], np.uint8).tobytes())


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("meshlet_build") / "meshlet_build_main")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "prosper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "meshlet_build_main.cpp"),
                           os.path.join(ROOT, "prosper_amd", "csrc", "meshlet_build.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_partition_equals_build_meshlets(program, tmp_path, name):
    vertex_count, tri = CASES[name]
    assert tri.max() < vertex_count
    if name == "soup_past_65535_vertices":
        assert vertex_count > 0xFFFF
    src, dst = str(tmp_path / "mesh.bin"), str(tmp_path / "meshlets.bin")
    with open(src, "wb") as f:
        f.write(np.array([vertex_count, len(tri)], np.uint32).tobytes() + tri.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    out = subprocess.run([program, src, dst], env=env, capture_output=True, text=True, timeout=120)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-2000:]
    assert "runtime error" not in text and "Sanitizer" not in text, text[-2000:]
    data = open(dst, "rb").read()
    n, nv, nt = np.frombuffer(data, np.uint32, 3)
    got = (data[12:12 + 16 * n], data[12 + 16 * n:12 + 16 * n + 4 * nv], data[12 + 16 * n + 4 * nv:])
    assert len(got[2]) == nt
    # (the bounds are not the partition's business: any positions do)
    want = M.build_meshlets(np.zeros((vertex_count, 3), np.float32), tri)
    assert n == len(want["meshlets"]) == EXPECTED[name]
    assert got == partition_of(want)
