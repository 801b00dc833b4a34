"""Timings of Delaybank.process_tv (per-sample tap streams) for DESIGN.md 4.9.

    python scripts/delay_tv_timing.py [--out FILE]

Two banks, one MI355X, one session, warm, medians of 5 alternating runs; a run is the mean of a
few calls on a host clock that ends in a stream synchronise, the kernels come from profile_read():
  ambi   12 lines, S = 1, ring 48,001, double: tests/ambi.cpp's bank, a forward tap sweeping
         between 900 and 1,500 samples, no feedback (null back streams)
  c5     64 lines, S = 3, ring 96,001, float: C5's bank (forward {0, 1}, feedback
         {10000 + 37 k, .5}, {20000 + 53 k, .5}) as a stream that repeats its taps
per call length 32, 1,024 and 48,000:
  (a) process_tv with host streams and process_tv_device with device streams
  (b) process() / process_device() with the equivalent static taps: the same gathers, no stream
and once per bank:
  (c) the only route without the stream entry: modulate_* on every tap, then a one-sample
      process(), over 1,000 samples
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

SIZES = ((32, 200), (1024, 50), (48000, 4))   # call length, calls per run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    from huygens_amd import Delaybank

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()

    def bank_ambi():
        b = Delaybank(12, 1, 48000, np.float64)

        def streams(n, t0=0):
            t = (t0 + np.arange(n))[None, None, :]
            l = np.arange(12)[:, None, None]
            d = 12.0 + 3.0 * np.sin(2 * np.pi * 37.0 * t / 48000 + l)   # distance, as sqrt(d2)
            return (d / 0.01).astype(np.uint32), (1.0 / (d * d)).astype(np.float64), None, None
        return b, streams

    def bank_c5():
        b = Delaybank(64, 3, 96000, np.float32)
        ft, bt = np.zeros((64, 3), np.uint32), np.zeros((64, 3), np.uint32)
        fg, bg = np.zeros((64, 3), np.float32), np.zeros((64, 3), np.float32)
        for k in range(64):
            b.coefficients(k, [(0, 1.0)], [(10000 + 37 * k, 0.5), (20000 + 53 * k, 0.5)])
            fg[k, 0] = 1.0
            bt[k, :2], bg[k, :2] = (10000 + 37 * k, 20000 + 53 * k), 0.5

        def streams(n, t0=0):
            return tuple(np.repeat(a[:, :, None], n, axis=2) for a in (ft, fg, bt, bg))
        return b, streams

    out = {}
    rng = np.random.default_rng(0)
    for name, make in (("ambi", bank_ambi), ("c5", bank_c5)):
        b, streams = make()
        dt = b.dtype
        res = {}
        for n, calls in SIZES:
            x = (0.1 * rng.standard_normal(n)).astype(dt)
            s = streams(n)
            if s[2] is None:   # (b)'s static taps: the stream's first row
                for k in range(b.lines):
                    b.coefficients(k, [(int(s[0][k, 0, 0]), float(s[1][k, 0, 0]))], [])
            xd, yd = dev(x), torch.zeros(b.lines * n, dtype=torch.float64 if dt == np.float64 else torch.float32,
                                         device="cuda")
            sd = [None if a is None else dev(a) for a in s]
            ptr = [None if a is None else a.data_ptr() for a in sd]
            torch.cuda.synchronize()

            def tv_host():
                b.process_tv(x, *s)

            def tv_dev():
                b.process_tv_device(xd.data_ptr(), yd.data_ptr(), n, *ptr)
                b.synchronize()

            def st_host():
                b.process(x)

            def st_dev():
                b.process_device(xd.data_ptr(), yd.data_ptr(), n)
                b.synchronize()

            routes = {"tv_host": tv_host, "tv_device": tv_dev, "static_host": st_host, "static_device": st_dev}
            for f in routes.values():   # warm: buffers grown, kernels loaded
                f()
                f()
            runs = {k: [] for k in routes}
            for _ in range(5):
                for k, f in routes.items():
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        f()
                    runs[k].append((time.perf_counter() - t0) / calls * 1e3)
            r = {"calls_per_run": calls}
            for k in routes:
                r[k + "_ms_runs"] = runs[k]
                r[k + "_ms"] = statistics.median(runs[k])
                r[k + "_us_per_sample"] = r[k + "_ms"] * 1e3 / n
            b.profile(True)
            for k in ("tv_device", "static_device"):
                for _ in range(calls):
                    routes[k]()
                ms, _ = b.profile_read()
                r[k + "_kernel_ms"] = ms / calls
            b.profile(False)
            r["tv_over_static_host"] = r["tv_host_ms"] / r["static_host_ms"]
            r["tv_over_static_device"] = r["tv_device_ms"] / r["static_device_ms"]
            r["tv_over_static_kernels"] = r["tv_device_kernel_ms"] / r["static_device_kernel_ms"]
            res[str(n)] = r

        # (c) modulate_* per tap and a one-sample process() per sample, 1,000 samples
        n = 1000
        x = (0.1 * rng.standard_normal(n)).astype(dt)
        s = streams(n)

        def loop():
            t0 = time.perf_counter()
            for t in range(n):
                for l in range(b.lines):
                    for i in range(b.sparsity):
                        b.modulate_forward(l, i, (s[0][l, i, t], s[1][l, i, t]))
                        if s[2] is not None:
                            b.modulate_back(l, i, (s[2][l, i, t], s[3][l, i, t]))
                b.process(x[t:t + 1])
            return (time.perf_counter() - t0) / n * 1e6
        loop()
        lr = [loop() for _ in range(5)]
        res["per_sample_loop_us_per_sample_runs"] = lr
        res["per_sample_loop_us_per_sample"] = statistics.median(lr)
        res["tv_beats_loop"] = {str(nn): {k: res[str(nn)][k + "_us_per_sample"] < res["per_sample_loop_us_per_sample"]
                                          for k in ("tv_host", "tv_device")} for nn, _ in SIZES}
        out[name] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
