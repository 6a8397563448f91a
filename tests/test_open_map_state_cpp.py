"""The open map's rows of the handle's resident state (direct_amd/csrc/resident_state.h) on the CPU:
tests/cpp/test_open_map_state.cpp builds the header with plain g++ under AddressSanitizer and UBSan and runs as a program of its
own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_open_map_state_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_open_map_state")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "cpp", "test_open_map_state.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
