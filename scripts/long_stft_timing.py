"""Timings of the long-frame STFT engine (frames above 8192 points) for DESIGN.md 4.10.

    python scripts/long_stft_timing.py [--out FILE]

One MI355X, one session, warm, medians of 5 runs.  (N, laps) = (16384, 4), (32768, 2) and
(262144, 16), each over 2^21 samples of the C4 input (white noise + 8 sinusoids, real), device
pointers in and out, one call on a handle that has already run one such call:
  static    StaticSTFT(N, laps, long_frames=True): four launches per internal block
  identity  Fourier(PROC_IDENTITY, N, laps, long_frames=True): three launches
per case and engine: the wall time of the call (host clock, ends in a stream synchronise), the
frame-pass and overlap-add times from profile_read(), samples/s, the real-time factor at 48 kHz,
and the bytes a frame moves through device memory against the algorithmic minimum (read N real
samples, write N complex ones: 24 N bytes).
Yardstick, same device and session: torch.fft.fft followed by torch.fft.ifft (rocFFT) over the
same [frames, N] complex128 batch -- the two transforms alone, no window, gate or overlap-add.
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

CASES = ((16384, 4), (32768, 2), (262144, 16))
SAMPLES = 1 << 21
RUNS = 5


def c4_signal(n, seed=3):
    import numpy as np
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    x = 0.1 * rng.standard_normal(n)
    for k in range(1, 9):
        x += 0.5 * np.sin(2 * np.pi * 220 * k ** 1.5 * t)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from huygens_amd.stft import PROC_IDENTITY, Fourier, StaticSTFT, frames_before

    x = torch.from_numpy(c4_signal(SAMPLES)).cuda()
    y = torch.empty_like(x)
    out = {"samples": SAMPLES, "runs": RUNS, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N, laps in CASES:
        frames = frames_before(N, laps, SAMPLES)
        res = {"frames": frames, "min_bytes_per_frame": 24 * N}
        engines = {"static": (lambda: StaticSTFT(N, laps, long_frames=True), 128 * N),
                   "identity": (lambda: Fourier(PROC_IDENTITY, N, laps, long_frames=True), 96 * N)}
        for name, (make, bytes_per_frame) in engines.items():
            def call():
                f = make()   # a fresh handle, warmed by one call (buffers grown, kernels loaded)
                f.process_block_device(x.data_ptr(), 0, y.data_ptr(), 0, SAMPLES)
                f.synchronize()
                torch.cuda.synchronize()
                before = f.frames()[0]
                f.profile(True)
                t0 = time.perf_counter()
                f.process_block_device(x.data_ptr(), 0, y.data_ptr(), 0, SAMPLES)
                f.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                frame_ms, ola_ms, blocks = f.profile_read()
                assert abs(f.frames()[0] - before - frames) <= 2 * laps   # the second 2^21 samples
                f.close()
                return wall, frame_ms, ola_ms, blocks
            call()
            call()
            runs = [call() for _ in range(RUNS)]
            wall = statistics.median(r[0] for r in runs)
            r = {"wall_ms_runs": [q[0] for q in runs], "wall_ms": wall,
                 "frame_pass_ms": statistics.median(q[1] for q in runs),
                 "overlap_add_ms": statistics.median(q[2] for q in runs),
                 "blocks": runs[0][3],
                 "samples_per_s": SAMPLES / (wall * 1e-3),
                 "realtime_factor_48k": SAMPLES / (wall * 1e-3) / 48000.0,
                 "bytes_per_frame": bytes_per_frame,
                 "bytes_over_minimum": bytes_per_frame / (24 * N)}
            r["frame_pass_us_per_frame"] = r["frame_pass_ms"] * 1e3 / frames
            r["frame_pass_gb_per_s"] = bytes_per_frame * frames / (r["frame_pass_ms"] * 1e-3) / 1e9
            res[name] = r

        z = torch.randn(frames, N, dtype=torch.complex128, device="cuda")

        def pair():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = torch.fft.ifft(torch.fft.fft(z, dim=1), dim=1)
            torch.cuda.synchronize()
            del w
            return (time.perf_counter() - t0) * 1e3
        pair()
        pair()
        pr = [pair() for _ in range(RUNS)]
        res["rocfft_pair_ms_runs"] = pr
        res["rocfft_pair_ms"] = statistics.median(pr)
        for name in engines:
            res[name]["frame_pass_over_rocfft_pair"] = res[name]["frame_pass_ms"] / res["rocfft_pair_ms"]
        del z
        out["cases"][f"{N}x{laps}"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
