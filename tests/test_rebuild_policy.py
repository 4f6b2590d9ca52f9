"""prosper_amd/csrc/pt_rebuild_policy.hpp alone: what a transform update or an animation does about a tree its refits have
degraded.  tests/rebuild_policy_main.cpp walks the function over every input on a CPU; the table is written out here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLD, BELOW, ABOVE = "1.3", "1.0", "1.6"


def table(moved, always_rebuild, drift_site, gpu_builder, build_running, above):
    """The policy, row by row, in order (`above`: the cost ratio exceeds the threshold; equal does not)."""
    if moved and always_rebuild:
        return "Synchronous"
    if not moved or not above:
        return "None"
    if drift_site:
        return "None" if build_running else "Background"
    if gpu_builder:
        return "Synchronous"
    return "None" if build_running else "Background"


@pytest.fixture(scope="module")
def decisions(tmp_path_factory):
    """{(moved, alwaysRebuild, driftSite, gpuBuilder, buildRunning, ratio): decision} from the header's own function, built
    for the host under AddressSanitizer + UBSan."""
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path_factory.mktemp("rebuild_policy") / "rebuild_policy")
    subprocess.check_call([
        gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
        "-I", os.path.join(ROOT, "prosper_amd", "csrc"), os.path.join(ROOT, "tests", "rebuild_policy_main.cpp"), "-o", exe])
    out = subprocess.run([exe, THRESHOLD, BELOW, ABOVE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout + out.stderr)[-3000:]
    got = {}
    for line in out.stdout.splitlines():
        *key, decision = line.split()
        got[tuple(int(k) for k in key)] = decision
    return got


def test_the_policy_is_the_table_on_every_input(decisions):
    assert len(decisions) == 32 * 3
    for key, decision in sorted(decisions.items()):
        *flags, ratio = key
        assert decision == table(*(bool(f) for f in flags), above=ratio == 2), key


def test_always_rebuild_needs_a_moved_instance(decisions):
    """The debug option takes the synchronous path only for an update that moves something: an unchanged table stays a
    no-op whatever the ratio, the sites, the builder and a running build are."""
    rows = [k for k in decisions if k[0] == 0 and k[1] == 1]
    assert len(rows) == 8 * 3
    assert all(decisions[k] == "None" for k in rows)
