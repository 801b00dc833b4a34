"""Timings of the heterodyne engine's three chains for DESIGN.md 4.4.

    python scripts/het_chains_timing.py [--out FILE]

One MI355X, one session, warm, medians of 5 alternating runs.  Chains: HARM (tests/harmbank.cpp,
Slidebank order 4), PHASE at order 4 (like for like) and at phasebank.cpp's order 1, STICKS
(tests/oscbank.cpp: 3 + 1 Stickbanks, gate 0.001).  Two sizes:
  small  the reference programs' own: 48 channels, process() on host arrays in blocks of their
         BSIZE (32; oscbank.cpp 64), 200 calls per run, host clock around the calls
  wide   262,144 channels (C8's bank), process_device() over 48,000 samples, 2 calls per run: the
         host clock ends in a synchronise, the chain kernel's time comes from profile_read()
Reported: samples/s (small), channel-samples/s from the kernel time and from the host clock
(wide).  One JSON object.  Needs a gfx950 device; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDE_N, WIDE_S, WIDE_CALLS = 262144, 48000, 2
SMALL_N, SMALL_CALLS = 48, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from bench_rows import c8_bank
    from huygens_amd import Heterodyne, StickChain, phasebank

    def opened(h, fa, fs):
        idx = np.arange(fa.size)
        h.freqmod(0, idx, fa)
        h.freqmod(1, idx, fs)
        h.open(0)
        h.open(1)
        return h

    def chains(N, fa, fs, radii, kw):
        r1 = radii   # the same radii at either order: the arithmetic does not depend on them
        return {
            "harm_o4": lambda: opened(Heterodyne(N, 4, radii, **kw), fa, fs),
            "phase_o4": lambda: opened(Heterodyne(N, 4, radii, chain="phase", **kw), fa, fs),
            "phase_o1": lambda: opened(Heterodyne(N, 1, r1, chain="phase", **kw), fa, fs),
            "sticks_3_1": lambda: opened(StickChain(N, 3, 1, -0.999, 0.001, 0.0, kw["gain"]), fa, fs),
        }

    rng = np.random.default_rng(8)
    out = {}

    # small: the programs' own sizes
    n, fa, fs, radii = phasebank()
    kw = dict(thresh=0.0005, ratio=0.2, width=2400, stick_order=1, stick_rad=-0.9, dry=0.0, gain=3.0)
    hs = {k: make() for k, make in chains(n, fa, fs, radii, kw).items()}
    runs = {k: [] for k in hs}
    for rep in range(6):   # the first pass warms
        for k, h in hs.items():
            b = 64 if k.startswith("sticks") else 32
            x = 0.2 * rng.standard_normal(b)
            t0 = time.perf_counter()
            for _ in range(SMALL_CALLS):
                h.process(x)
            if rep:
                runs[k].append(SMALL_CALLS * b / (time.perf_counter() - t0))
    out["small"] = {k: {"channels": n, "block": 64 if k.startswith("sticks") else 32,
                        "samples_per_s": statistics.median(v), "samples_per_s_runs": v} for k, v in runs.items()}
    for h in hs.values():
        h.close()

    # wide: 262,144 channels
    fa, radii, kw = c8_bank(WIDE_N)
    x = torch.from_numpy(0.2 * rng.standard_normal(WIDE_S)).cuda()
    y = torch.empty_like(x)
    hs = {k: make() for k, make in chains(WIDE_N, fa, -2 * fa, radii, kw).items()}
    host, kern = {k: [] for k in hs}, {k: [] for k in hs}
    for h in hs.values():
        h.profile(True)
    for rep in range(6):
        for k, h in hs.items():
            h.profile_read()
            t0 = time.perf_counter()
            for _ in range(WIDE_CALLS):
                h.process_device(x.data_ptr(), y.data_ptr(), WIDE_S)
            h.synchronize()
            dt = time.perf_counter() - t0
            ms, _, cs = h.profile_read()
            if rep:
                host[k].append(cs / dt)
                kern[k].append(cs / (ms / 1e3))
    out["wide"] = {k: {"channels": WIDE_N, "samples_per_call": WIDE_S,
                       "kernel_channel_samples_per_s": statistics.median(kern[k]),
                       "host_channel_samples_per_s": statistics.median(host[k]),
                       "kernel_runs": kern[k], "host_runs": host[k]} for k in hs}
    base = out["wide"]["harm_o4"]["kernel_channel_samples_per_s"]
    for k in hs:
        out["wide"][k]["kernel_vs_harm_o4"] = out["wide"][k]["kernel_channel_samples_per_s"] / base
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
