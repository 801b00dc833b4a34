"""hz::Stream / hz::Event / hz::ProfEvents / hz::check_handle (huygens_amd/csrc/hz_stream.h), the
owners of every handle's stream, ordering events and profile timers, checked on the host:
tests/cpp/stream_host.cpp defines counting stand-ins for the HIP stream and event calls (with a
switch that fails the next creation) and links no HIP runtime.  What it pins: a private stream is
destroyed exactly once and a borrowed one never, under both null-stream policies of set_stream;
a failed creation leaves an object that destroys nothing; the timing pool hands out live events
across its growth steps and sums complete groups only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "stream_host.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
        "-I", os.path.join(ROOT, "include")]


def build_and_run(exe, extra):
    r = subprocess.run(BASE + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode == 0:
        assert "warning" not in r.stderr, r.stderr[-3000:]
        run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        return r, run
    return r, None


def test_stream_host_program(tmp_path):
    r, run = build_and_run(tmp_path / "stream_host", ["-O1"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "stream ok" in run.stdout and "live 0" in run.stdout, run.stdout


def test_stream_host_program_sanitized(tmp_path):
    # a stand-alone host program, nothing preloaded: every stand-in stream and event is a heap
    # block, so a double destroy, a leak (LeakSanitizer, where the platform has it) and a use
    # after move show up here
    r, run = build_and_run(tmp_path / "stream_host_san",
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "stream ok" in run.stdout and "live 0" in run.stdout, run.stdout
