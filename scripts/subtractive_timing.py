"""Timings of Subtractive<double, 2> for DESIGN.md 4.8.

    python scripts/subtractive_timing.py [--out FILE]

  reference program   7 x 7 x 2, resonance 0.999995, k 1, a physics step every 32 samples,
                      128-sample blocks (2.667 ms of audio): host clock around process(), which
                      ends in a stream synchronise (uploads and copies included), median of 5 runs of
                      200 blocks after 100 warm-up blocks; kernel split from profile_read()
  scaled bank         64 x 64 x 2, 48,000 samples in one process_device() call on device buffers,
                      alternating with the per-sample resonant stream route over the same count of
                      band-samples: hz_fb_process_tv_device(RESONANT), 4096 bands, a device-resident
                      [48000][4096] frequency stream, run twice for two channels (its stream is
                      neither produced nor uploaded inside the timed window); medians of 5
One JSON object.  Needs a gfx950 device; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from huygens_amd import GRAV_TRUNC, Filterbank, Subtractive
    from huygens_amd.filterbank import TV_RESONANT

    out = {}
    rng = np.random.default_rng(0)

    g = Subtractive(7, 7, 0.7, 0.999995, 1.0, 1.0, channels=2)
    g.physics_every(32, GRAV_TRUNC)
    for p, a in ((48, 1.0), (55.3, 0.6), (60.1, 0.8)):
        g.makenote(p, a)
    x = rng.standard_normal((2, 128))
    for _ in range(100):
        g.process(x)
    runs = []
    for _ in range(5):
        ts = []
        for _ in range(200):
            t0 = time.perf_counter()
            g.process(x)
            ts.append(time.perf_counter() - t0)
        runs.append(statistics.median(ts) * 1e3)
    out["ref_block_ms_runs"] = runs
    out["ref_block_ms"] = statistics.median(runs)
    g.profile(True)
    for _ in range(200):
        g.process(x)
    out["ref_kernel_ms_per_block"] = dict(zip(("physics", "coefficients", "resonators", "reduce"),
                                              (m / 200 for m in g.profile_read())))
    g.profile(False)

    V, O, n = 64, 64, 48000
    s = Subtractive(V, O, 0.9, 0.99999, 1.0, 0.1, channels=2)
    s.physics_every(32, GRAV_TRUNC)
    for i in range(V):   # small masses: the gravity of 4096 particles stays bounded
        s.makenote(30.0 + 0.83 * i, 0.002 + 0.002 * ((i * 7) % 5) / 5)
    xin = torch.from_numpy(rng.standard_normal((2, n))).cuda()
    yout = torch.zeros_like(xin)
    fb = Filterbank(2, V * O)
    fb.boost(np.ones(V * O))
    fb.open()
    freqs = torch.from_numpy(np.geomspace(40.0, 20000.0, V * O)).cuda()
    wobble = torch.sin(torch.arange(n, device="cuda", dtype=torch.float64)[:, None] * 1e-3)
    stream = (freqs[None, :] * (1 + 0.01 * wobble)).contiguous()
    y1 = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def run_sub():
        t0 = time.perf_counter()
        s.process_device(xin.data_ptr(), yout.data_ptr(), n)
        s.positions()   # synchronises the handle's stream
        return time.perf_counter() - t0

    def run_tv():
        t0 = time.perf_counter()
        for k in range(2):
            fb.process_tv_device(xin[k].data_ptr(), y1.data_ptr(), n, TV_RESONANT, stream.data_ptr(), 0.99999)
        fb.synchronize()
        return time.perf_counter() - t0

    run_sub()
    run_tv()
    a, b = [], []
    for _ in range(5):
        a.append(run_sub())
        b.append(run_tv())
    s.profile(True)
    run_sub()
    out["scaled_kernel_ms"] = dict(zip(("physics", "coefficients", "resonators", "reduce"), s.profile_read()))
    s.profile(False)
    out["scaled_sub_s_runs"], out["scaled_tv_s_runs"] = a, b
    out["scaled_sub_s"], out["scaled_tv_s"] = statistics.median(a), statistics.median(b)
    out["scaled_band_samples_per_s_sub"] = V * O * 2 * n / out["scaled_sub_s"]
    out["scaled_band_samples_per_s_tv"] = V * O * 2 * n / out["scaled_tv_s"]
    s.physics_every(0, GRAV_TRUNC)
    run_sub()
    out["scaled_sub_physics_off_s"] = statistics.median(run_sub() for _ in range(5))
    out["scaled_output_finite"] = bool(torch.isfinite(yout).all().item())
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
