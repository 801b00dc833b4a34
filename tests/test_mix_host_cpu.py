"""hz::mix_plan (huygens_amd/csrc/hz_mixplan.h), the time-segment plan of every bank engine's
mixdown launch, and hz::allow_lds (hz_lds.h), the one owner of a kernel's dynamic-LDS limit,
checked on the host: tests/cpp/mix_host.cpp restates the plan's formula over a grid of groups,
lengths, tiles and targets (no empty segment, n_pad covers n), and defines a counting stand-in for
hipFuncSetAttribute (with a switch that fails the next call); no HIP runtime is linked.  What it
pins for allow_lds: one runtime call per (device, kernel), none on a repeat with an equal or
smaller size, one more when the size grows, a failure reported as HZ_E_HIP and retried, and eight
threads asking for one pair at once producing exactly one call."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mix_host.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
        "-I", os.path.join(ROOT, "include")]


def build_and_run(exe, extra):
    r = subprocess.run(BASE + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode == 0:
        assert "warning" not in r.stderr, r.stderr[-3000:]
        run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        return r, run
    return r, None


def check(r, run):
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "mix ok: 252 plans" in run.stdout, run.stdout   # 7 groups x 2 tiles x 6 lengths x 3 targets


def skip_without_runtime(r, names):
    if r.returncode != 0 and any(n in r.stderr for n in names):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])


def test_mix_host_program(tmp_path):
    check(*build_and_run(tmp_path / "mix_host", ["-O1"]))


def test_mix_host_program_sanitized(tmp_path):
    # a stand-alone host program, nothing preloaded
    r, run = build_and_run(tmp_path / "mix_host_san",
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    skip_without_runtime(r, ("asan", "ubsan", "sanitize"))
    check(r, run)


def test_mix_host_program_thread_sanitized(tmp_path):
    # the threaded case under ThreadSanitizer: the repeat path takes no lock, so its loads and the
    # slow path's stores must be ordered by the atomics alone
    r, run = build_and_run(tmp_path / "mix_host_tsan", ["-O1", "-g", "-fsanitize=thread"])
    skip_without_runtime(r, ("tsan", "sanitize"))
    check(r, run)
