"""Compile a C++ program around the headers of direct_amd/csrc with g++, exchange one binary file with it, unpack what it wrote -
TEST INFRASTRUCTURE of the harness modules (tests/*_harness.py).  Every harness compiles through compile_program, so the flags are
written once; the corridor harnesses also share the file exchange and the unpacking."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# -ffp-contract=off: the headers' multiply-adds are explicit fma() calls and nothing else may be fused, whatever the host's
# instruction set (the kernels are compiled with contraction switched off per function)
FLAGS = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"]


def compile_program(workdir, name, source, extra=(), tail=(), exe=None):
    """writes <workdir>/<name>.cpp and compiles it -> the executable's path (<workdir>/<exe or name>).  extra: flags in front of
    the include path; tail: flags behind the output file"""
    src, exe = os.path.join(str(workdir), name + ".cpp"), os.path.join(str(workdir), exe or name)
    with open(src, "w") as f:
        f.write(source)
    subprocess.check_call(FLAGS + list(extra) + ["-I", os.path.join(ROOT, "direct_amd", "csrc"), src, "-o", exe] + list(tail))
    return exe


def exchange(harness, ints, doubles, arrays):
    """harness: (workdir, executable).  Writes in.bin - `ints` as int32, `doubles` as float64, then every array in its own dtype -,
    runs `executable in.bin out.bin` -> the bytes of out.bin, which is removed"""
    d, exe = harness
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    with open(fin, "wb") as f:
        np.array(ints, np.int32).tofile(f)
        np.array(doubles, np.float64).tofile(f)
        for a in arrays:
            np.ascontiguousarray(a).tofile(f)
    subprocess.check_call([exe, fin, fout])
    with open(fout, "rb") as f:
        raw = f.read()
    os.remove(fout)
    return raw


def unpack(raw, layout):
    """layout: (key, dtype, shape) in file order -> dict of arrays; every byte of `raw` must be consumed"""
    out, off = {}, 0
    for k, dt, shape in layout:
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        out[k], off = np.frombuffer(raw[off:off + n], dt).reshape(shape).copy(), off + n
    assert off == len(raw), (off, len(raw))
    return out
