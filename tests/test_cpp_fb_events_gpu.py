"""GPU: tests/cpp/fb_events_dropin.cpp -- the MIDI instrument of the reference's
tests/filterbank.cpp (process_midi, 217-252) over include/soundmath/filterbank.h with its setter
calls turned into the events of process(in, out, n, ev, nev): a score of note-ons and note-offs on
9 keys x 4 courses, block by block, on Filterbank<double> and FFilterbank<double, 36, 2>.  The
program dumps its input and events; both outputs are replayed through the oracle with the events
applied as setter calls between process() pieces."""
import os
import subprocess

import numpy as np
import pytest

from fb_events_model import run_events_split
from oracle import OracleFilterbank, rel_err
from test_cpp_cpu import LIB, ROOT

pytestmark = pytest.mark.gpu
PI = 3.14159265359
BANDS = 36


def build(exe):
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "fb_events_dropin.cpp"), "-o", str(exe), "-L", LIB, "-lhuygens_hip",
           f"-Wl,-rpath,{LIB}", "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_midi_score_as_events(gpu_lib, tmp_path):
    exe = tmp_path / "fb_events_dropin"
    r = build(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    p = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "fb_events_dropin ok: 112 events" in p.stdout, p.stdout + p.stderr

    def load(name):
        return np.fromfile(os.path.join(tmp_path, name + ".bin"), dtype=np.float64)
    x, flat = load("fbev_x"), load("fbev_events").reshape(-1, 4)
    events = [(int(a), int(b), int(k), float(v)) for a, b, k, v in flat]
    assert len(x) == 6 * 1024 and len({e[0] for e in events}) == 13
    o = OracleFilterbank(2, BANDS, 0.05, 0.3)
    for i in range(BANDS):
        g, R, th = 0.01 * (i % 7 + 1), 0.995, 2 * PI * (i + 1) / 90.0
        o.coefficients(i, [g, 0, -g], [-2 * R * np.cos(th), R * R])
    o.distortion(1)   # &softclip, width 0.125
    want = run_events_split(o, x, events)
    assert np.max(np.abs(want)) > 1e-3   # the notes sound
    assert rel_err(load("fbev_y"), want) < 1e-9
    assert rel_err(load("fbev_yf"), want) < 1e-9
