"""hz::DevBuf / hz::PinBuf (huygens_amd/csrc/hz_buf.h), the owners of every handle's device and
pinned buffers, checked on the host: tests/cpp/devbuf_host.cpp defines counting stand-ins for the
four HIP allocation calls (with a switch that fails the next allocation) and links no HIP
runtime.  The case that matters most: a failed growth leaves the buffer empty, so a later,
smaller request allocates again instead of handing a null pointer to a kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "devbuf_host.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
        "-I", os.path.join(ROOT, "include")]


def build_and_run(exe, extra):
    r = subprocess.run(BASE + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode == 0:
        assert "warning" not in r.stderr, r.stderr[-3000:]
        run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        return r, run
    return r, None


def test_devbuf_host_program(tmp_path):
    r, run = build_and_run(tmp_path / "devbuf_host", ["-O1"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "devbuf ok" in run.stdout and "live 0" in run.stdout, run.stdout


def test_devbuf_host_program_sanitized(tmp_path):
    # a stand-alone host program, nothing preloaded: double frees, leaks (LeakSanitizer, where the
    # platform has it) and use after move show up here
    r, run = build_and_run(tmp_path / "devbuf_host_san",
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "devbuf ok" in run.stdout and "live 0" in run.stdout, run.stdout
