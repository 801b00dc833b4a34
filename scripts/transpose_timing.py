"""Timings of the spectral transposer (PROC_TRANSPOSE) for DESIGN.md 4.11.

    python scripts/transpose_timing.py [--out FILE]

One MI355X, one session, warm, medians of 5 runs, the method of scripts/long_stft_timing.py:
(N, laps) = (4096, 4), (16384, 4), (32768, 2) and (262144, 16), each over 2^21 samples of the C4
input (white noise + 8 sinusoids, real), device pointers in and out, one call on a handle that has
already run one such call.  Per shape:
  static       StaticSTFT(N, laps, long_frames=True), the gated engine: the yardstick (four launches
               above 8192; at or below it real input takes the two-frames-per-transform kernel)
  identity     Fourier(PROC_IDENTITY, ...)
  transpose_2, transpose_0.5   Fourier(PROC_TRANSPOSE, ..., params=(r, 0))
  host_2       the path the device processor replaces: the scatter loop as a C function pointer
               (tests/cpp/transpose_host_proc.cpp) through the host-processor path, which this
               feature leaves as it was
with the wall time of the call (host clock, ends in a stream synchronise) and the frame-pass and
overlap-add times from profile_read().  One JSON object.  Needs a gfx950 device and g++.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CASES = ((4096, 4), (16384, 4), (32768, 2), (262144, 16))
SAMPLES = 1 << 21
RUNS = 5


def host_proc_lib(tmp):
    so = os.path.join(tmp, "libtranspose_host_proc.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "transpose_host_proc.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.transpose_host_setup.argtypes = [C.c_int, C.c_double]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from huygens_amd._lib import check, load
    from huygens_amd.stft import PROC_IDENTITY, PROC_TRANSPOSE, Fourier, StaticSTFT, frames_before
    from long_stft_timing import c4_signal

    tmp = tempfile.mkdtemp()
    hp = host_proc_lib(tmp)

    def host_handle(N, laps, r):
        hp.transpose_host_setup(N, r)
        f = Fourier(PROC_IDENTITY, N, laps, long_frames=True)
        check(load().hz_stft_set_processor(f._h, C.cast(hp.transpose_host_proc, C.c_void_p)))
        return f

    x = torch.from_numpy(c4_signal(SAMPLES)).cuda()
    y = torch.empty_like(x)
    yi = torch.empty_like(x)
    out = {"samples": SAMPLES, "runs": RUNS, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N, laps in CASES:
        frames = frames_before(N, laps, SAMPLES)
        res = {"frames": frames}
        engines = {"static": lambda: StaticSTFT(N, laps, long_frames=True),
                   "identity": lambda: Fourier(PROC_IDENTITY, N, laps, long_frames=True),
                   "transpose_2": lambda: Fourier(PROC_TRANSPOSE, N, laps, long_frames=True, params=(2.0, 0.0)),
                   "transpose_0.5": lambda: Fourier(PROC_TRANSPOSE, N, laps, long_frames=True, params=(0.5, 0.0)),
                   "host_2": lambda: host_handle(N, laps, 2.0)}
        for name, make in engines.items():
            def call():
                f = make()   # a fresh handle, warmed by one call (buffers grown, kernels loaded)
                f.process_block_device(x.data_ptr(), 0, y.data_ptr(), yi.data_ptr(), SAMPLES)
                f.synchronize()
                torch.cuda.synchronize()
                f.profile(True)
                t0 = time.perf_counter()
                f.process_block_device(x.data_ptr(), 0, y.data_ptr(), yi.data_ptr(), SAMPLES)
                f.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                frame_ms, ola_ms, blocks = f.profile_read()
                f.close()
                return wall, frame_ms, ola_ms, blocks
            call()
            runs = [call() for _ in range(RUNS)]
            res[name] = {"wall_ms_runs": [q[0] for q in runs], "wall_ms": statistics.median(q[0] for q in runs),
                         "frame_pass_ms": statistics.median(q[1] for q in runs),
                         "overlap_add_ms": statistics.median(q[2] for q in runs), "blocks": runs[0][3]}
        for name in ("transpose_2", "transpose_0.5"):
            res[name]["frame_pass_over_static"] = res[name]["frame_pass_ms"] / res["static"]["frame_pass_ms"]
            res[name]["frame_pass_over_identity"] = res[name]["frame_pass_ms"] / res["identity"]["frame_pass_ms"]
        res["host_over_device_wall"] = res["host_2"]["wall_ms"] / res["transpose_2"]["wall_ms"]
        out["cases"][f"{N}x{laps}"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
