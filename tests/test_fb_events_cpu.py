"""Filterbank events on the host (no GPU): the event compiler of hz_fb_process_events
(huygens_amd/csrc/hz_fb_events.h) through tests/cpp/fb_events_host.cpp -- a stand-alone program with
its own main, plain g++, no HIP runtime, nothing preloaded, built once plain and once with
-fsanitize=address,undefined -- and the numpy twin of the kernel's per-lane arithmetic
(tests/fb_events_model.py) against the oracle driven through the same events as setter calls
between process() pieces."""
import os
import subprocess

import numpy as np
import pytest

from fb_events_model import compile_rows, lane_track, positions_events, run_events_split
from oracle import OracleFilterbank, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fb_events_host.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include")]


def build_and_run(exe, extra):
    r = subprocess.run(BASE + extra + [SRC, "-o", str(exe)], capture_output=True, text=True)
    if r.returncode == 0:
        assert "warning" not in r.stderr, r.stderr[-3000:]
        return r, subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    return r, None


def check(r, run):
    assert r.returncode == 0, r.stderr[-3000:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "fb_events ok: 23 cases" in run.stdout, run.stdout


def test_event_compiler_host_program(tmp_path):
    check(*build_and_run(tmp_path / "fb_events_host", ["-O1"]))


def test_event_compiler_host_program_sanitized(tmp_path):
    # a stand-alone host program, nothing preloaded
    r, run = build_and_run(tmp_path / "fb_events_host_san",
                           ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0 and any(n in r.stderr for n in ("asan", "ubsan", "sanitize")):
        pytest.skip("sanitizer runtime not installed: " + r.stderr.strip().splitlines()[-1])
    check(r, run)


@pytest.mark.parametrize("kp,kg", [(0.05, 0.3), (0.0, 0.01)])
def test_lane_arithmetic_matches_oracle_state(kp, kg):
    """The kernel's formula, before a GPU is involved: rows compiled from the events, each lane's
    closed-form seed and stepped recurrence (lane_track), against the oracle's smoother state after
    the split run -- at the call's end (get_state) and, through shorter runs, at samples on both
    sides of every kind of position."""
    N, n = 37, 3000
    rng = np.random.default_rng(1)
    fwd = rng.uniform(-1, 1, (N, 3))
    back = np.tile([-1.2, 0.5], (N, 1))
    boost0 = rng.uniform(0.5, 1.5, N)
    sp, sg = lib().orc_relaxation(kp), lib().orc_relaxation(kg)
    events = positions_events(N, n)

    def oracle_pg(stop):
        o = OracleFilterbank(2, N, kp, kg)
        for b in range(N):
            o.coefficients(b, fwd[b], back[b])
        o.boost(boost0)
        o.open()
        o.process(rng.uniform(-1, 1, 40))   # smoothers under way: the call starts mid-ramp
        pg0 = o.get_state()[-2 * N:].reshape(N, 2).copy()
        x = np.zeros(stop)
        run_events_split(o, x, [e for e in events if e[0] < stop])
        return pg0, o.get_state()[-2 * N:].reshape(N, 2)

    pg0, pg_end = oracle_pg(n)
    table = compile_rows(events, n, 0, N, sp, sg, boost0, np.ones(N), pg0)
    assert sorted(table) == list(range(N))   # band -1 events: every band has rows
    assert len(table[7]) == 3 and table[7][1][1] == 3.0    # equal `at` collapsed, the last BOOST wins
    assert len(table[4]) == 6 and len(table[20]) == 2
    track = {b: (lane_track(table[b], 0, sp, n), lane_track(table[b], 1, sg, n)) for b in range(N)}
    for b in range(N):
        for which in (0, 1):
            ref = pg_end[b, which]
            assert abs(track[b][which][n - 1] - ref) <= 1e-12 * max(1.0, abs(ref)), (b, which)
            assert abs(table[b][-1][3 + which] - ref) <= 1e-12 * max(1.0, abs(ref)), (b, which)   # the end row
        # the end row's targets are the ones staged for the next call (events at n included)
        assert table[b][-1][2] == 0.5 and table[b][-1][1] == (4.0 if b == 5 else table[b][-2][1])
    for stop in (1, 2, 16, 17, 18, 21, 501, 1024, 1025, 1026, 2048):
        _, pg = oracle_pg(stop)
        for b in (0, 3, 4, 5, 7, 20, N - 1):
            for which in (0, 1):
                got, ref = track[b][which][stop - 1], pg[b, which]
                assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), (stop, b, which, got, ref)
    if kp == 0.0:   # an instant pre-amp: pre == pin from the event's own sample on
        assert track[4][0][15] == 2.0 and track[4][0][16] == 2.0 and track[4][0][17] == 0.3
