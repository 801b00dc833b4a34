"""Timings of Filterbank.process_events_device (boost / mix events inside one block call) for
DESIGN.md 3.12.

    python scripts/fb_events_timing.py [--out FILE] [--notes 0,16,128,1024]

The C2 recipe on one MI355X, one session, warm: 4096 bands, order 2 (f_i = 0.5 (i + 1) SR / 4096,
R = 0.999), k_p = 0.1, k_g = 1, 480,000 samples resident on the device, without a distortion and
with softclip.  A score of 0, 16, 128 or 1024 notes spread evenly over the call; a note is nine
neighbouring bands x (BOOST + MIX), alternately on (1, gain) and off (0, 0) as the reference's
MIDI handler sets them (tests/filterbank.cpp:231-245).  Per score size, the median of five
alternating runs on a host clock that ends in a stream synchronise:
  (a) one process_events_device call
  (b) the split loop through process_device and the setters: a call per piece between notes --
      what a caller had to do before events, hence the baseline
  (c) (0 notes) process_device with set_path(GENERAL)
and the kernel-time split of (a) and (b) from profile_read().  (a) and (b) start from the same
state (set_state) and their outputs are compared.  One JSON object.  Needs a gfx950 device; there
is no fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, SAMPLES = 4096, 480_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--notes", default="0,16,128,1024")
    args = ap.parse_args()

    import numpy as np
    import torch

    from golden.spec_numpy import resonant_coefficients, white_noise_f32
    from huygens_amd import EV_BOOST, EV_MIX, Filterbank
    from huygens_amd._lib import HZ_DIST_NONE, HZ_DIST_SOFTCLIP, HZ_FB_PATH_AUTO, HZ_FB_PATH_GENERAL

    fwd, back = resonant_coefficients(N, 0.999, 1.0)
    x = white_noise_f32(SAMPLES, seed=1)
    xd = torch.from_numpy(x).cuda()
    ya, yb = torch.zeros_like(xd), torch.zeros_like(xd)
    gains = 0.5 + 0.5 * np.random.default_rng(0).uniform(size=N)

    def score(notes):
        """-> [(at, [(band, kind, value), ...])]: the setters of each note"""
        out = []
        for i in range(notes):
            at = (i * SAMPLES) // notes + 37
            key = (i * 131) % (N // 9)
            on = (i // (N // 9)) % 2 == 0
            out.append((at, [(9 * key + j, k, (1.0 if k == EV_BOOST else gains[9 * key + j]) if on else 0.0)
                             for j in range(9) for k in (EV_BOOST, EV_MIX)]))
        return out

    out = {"bands": N, "samples": SAMPLES}
    for dist, dname in ((HZ_DIST_NONE, "none"), (HZ_DIST_SOFTCLIP, "softclip")):
        fb = Filterbank(2, N, 0.1, 1.0)
        for b in range(N):
            fb.coefficients(b, fwd[b], back[b])
        fb.boost(np.ones(N))
        fb.open()
        fb.distortion(dist)
        fb.process(x[:20000])   # smoothers converged, buffers grown
        start = fb.get_state()
        res = {}
        for notes in [int(v) for v in args.notes.split(",")]:
            sc = score(notes)
            events = [(at, band, kind, value) for at, sets in sc for band, kind, value in sets]

            def reset():
                fb.boost(np.ones(N))
                fb.open()
                fb.set_state(start)

            def one_call():
                fb.process_events_device(xd.data_ptr(), ya.data_ptr(), SAMPLES, events)
                fb.synchronize()

            def split_loop():
                pos = 0
                for at, sets in sc:
                    if at > pos:
                        fb.process_device(xd.data_ptr() + 8 * pos, yb.data_ptr() + 8 * pos, at - pos)
                        pos = at
                    for band, kind, value in sets:
                        (fb.boost if kind == EV_BOOST else fb.mix)(band, value)
                fb.process_device(xd.data_ptr() + 8 * pos, yb.data_ptr() + 8 * pos, SAMPLES - pos)
                fb.synchronize()

            def general():
                fb.set_path(HZ_FB_PATH_GENERAL)
                fb.process_device(xd.data_ptr(), yb.data_ptr(), SAMPLES)
                fb.synchronize()
                fb.set_path(HZ_FB_PATH_AUTO)

            routes = {"events_call": one_call, "split_loop": split_loop}
            if notes == 0:
                routes["general_path"] = general
            for f in routes.values():   # warm
                reset()
                f()
            runs = {k: [] for k in routes}
            for _ in range(5):
                for k, f in routes.items():
                    reset()
                    fb.synchronize()
                    t0 = time.perf_counter()
                    f()
                    runs[k].append((time.perf_counter() - t0) * 1e3)
            r = {"events": len(events)}
            for k in routes:
                r[k + "_ms_runs"] = runs[k]
                r[k + "_ms"] = statistics.median(runs[k])
            for k, f in routes.items():   # kernel times: segment pre-pass, mix, reduce, launches
                reset()
                fb.profile(True)
                f()
                r[k + "_kernels"] = dict(zip(("segment_ms", "mix_ms", "reduce_ms", "launches"), fb.profile_read()))
                fb.profile(False)
            d = (ya - yb).abs().max().item() / yb.abs().max().item()
            r["events_vs_split_rel_err"] = d
            r["events_over_split"] = r["events_call_ms"] / r["split_loop_ms"]
            res[str(notes)] = r
        out[dname] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
