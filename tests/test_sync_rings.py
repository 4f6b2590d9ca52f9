"""The fence, the version ring and the pinned staging ring behind the scene updates of the frame loop
(prosper_amd/csrc/pt_sync.hpp) on a CPU: tests/sync_rings_main.cpp drives them against fakes of the HIP entry points the
header calls - which versions a ring visits, which waits are enqueued and which are not, when the host waits for a staging
buffer, what a failure between next() and commit() leaves behind; the stream owner and the launch timeline of a timed
render (which events it records, what it drops beyond its capacity, how its intervals add up per stage, what a creation
that failed half way gives back); that every event, pinned buffer and stream is given back once.
A stand-alone program built with the host compiler, without the HIP runtime, under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sync_rings_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the host C++ compiler (g++) is needed"
    exe = str(tmp_path / "sync_rings")
    subprocess.check_call([
        gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
        "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "prosper_amd", "csrc"),
        "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "sync_rings_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=60)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-4000:]
    assert "runtime error" not in text and "Sanitizer" not in text, text[-4000:]
    assert "sync rings ok" in text
