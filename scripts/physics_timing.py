"""Time per 1024-sample block of Additive with physics at period 2 (the reference program's rate:
24,000 steps per second), against the real-time budget 1024 / 48000 = 21.33 ms.

    python scripts/physics_timing.py [--out FILE]

Per size: warm-up blocks, then the median over several timed blocks of
  block_ms    host clock around fill(1024), which ends in a stream synchronise (uploads included)
  physics_ms  HIP events around the physics kernels of the block (min_steps_kernel / min_step_kernel)
  audio_ms    HIP events around add_track_kernel + add_reduce_kernel
One JSON line per size.  Needs a gfx950 device; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOCK, PERIOD, BUDGET_MS = 1024, 2, 1024 / 48000 * 1e3
SINGLE_GROUP_MAX = 256   # the engine's default path split (hz_add_tune_physics)

# (voices, overtones, warm-up blocks, timed blocks, tune_physics or None)
CASES = [
    (10, 7, 3, 15, None),          # tests/additive.cpp
    (16, 64, 3, 9, None),          # 1024 particles: per-step path by default
    (16, 64, 3, 9, (1024, 256)),   # the same bank forced onto the one-workgroup path (its upper edge)
    (64, 256, 1, 3, None),         # 16384 particles, 1.3e8 pair terms per step
]


def run(V, O, warm, timed, tune):
    from huygens_amd import GRAV_TRUNC, Additive
    a = Additive(V, O, 0.75, 1.0)
    if tune:
        a.tune_physics(*tune)
    for v in range(V):   # neighbouring voices 0.3 semitone apart: inside the gravity cutoff
        a.makenote(36 + 0.3 * v, 0.5 + 0.5 * (v % 2))
    a.physics_every(PERIOD, GRAV_TRUNC)
    for _ in range(warm):
        a.fill(BLOCK)
    block, phys, audio = [], [], []
    for _ in range(timed):
        a.profile(True)
        t0 = time.perf_counter()
        a.fill(BLOCK)
        block.append((time.perf_counter() - t0) * 1e3)
        p, s = a.physics_profile_read()
        phys.append(p)
        audio.append(s)
    a.profile(False)
    med = statistics.median
    return dict(voices=V, overtones=O, particles=V * O, path="one_group" if V * O <= (tune[0] if tune else SINGLE_GROUP_MAX) else "per_step",
                period=PERIOD, block=BLOCK, blocks_timed=timed, block_ms=round(med(block), 4),
                block_ms_min=round(min(block), 4), block_ms_max=round(max(block), 4),
                physics_ms=round(med(phys), 4), audio_ms=round(med(audio), 4), budget_ms=round(BUDGET_MS, 3),
                real_time=med(block) < BUDGET_MS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for c in CASES:
        lines.append(json.dumps(run(*c)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
