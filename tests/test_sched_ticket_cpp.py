"""The ticket arithmetic of the ticket-scheduled hot kernel (direct_amd/csrc/sched_ticket.h) on the CPU:
tests/cpp/test_sched_ticket.cpp replays every launch shape B in {1, 3, 64} x n in {1, 2, 20} x tail in {0, 8}, whole-trip
and half-trip tickets, as a program of its own built with AddressSanitizer and UBSan.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sched_ticket_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_sched_ticket")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests", "cpp", "test_sched_ticket.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
