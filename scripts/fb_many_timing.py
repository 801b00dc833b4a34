"""hz_fb_process_many against the per-handle loop on the program's shape (tests/filterbanks.cpp:
8 channels x 864 bands, order 2, &softclip), buffers resident on the device.

    python scripts/fb_many_timing.py [--loop-only] [--package-root DIR] [--json FILE]

Per call length (256, 1024, 4096, 48,000 samples): (a) one process_many_device call, (b) the loop of
eight process_device calls, each handle on its own stream.  A run is `reps` calls back to back from
the same start state (set_state before it, outside the clock), timed from the host clock to the
synchronisation of every handle's stream; the routes alternate and each figure is the median of five
runs, per call.  A second figure per route is one call alone on an idle device (the audio callback's
case), call to synchronisation: the median of 20 calls per run, then of the five runs.  The
per-launch kernel times come from hz_fb_profile_read in a run of their own.
--loop-only measures (b) alone, with a package that has no process_many (--package-root: the parent
commit's tree), to show that the loop has not moved."""
import argparse
import json
import os
import statistics
import sys
import time

LENGTHS = [(256, 50), (1024, 50), (4096, 20), (48000, 5)]
H, N = 8, 864


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import numpy as np
    import torch
    import huygens_amd
    from huygens_amd import Filterbank
    from huygens_amd._lib import HZ_DIST_SOFTCLIP
    from golden.spec_numpy import resonant_coefficients

    fwd, back = resonant_coefficients(N, 0.999, 1.0)
    gs = []
    for k in range(H):
        g = Filterbank(2, N)
        for b in range(N):
            g.coefficients(b, fwd[b], back[b])
        g.boost(np.full(N, 1.0 + 0.1 * k))
        g.open()
        g.distortion(HZ_DIST_SOFTCLIP, None)
        gs.append(g)
    nmax = max(n for n, _ in LENGTHS)
    xt = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (H, nmax))).cuda()
    yt = torch.zeros_like(xt)
    torch.cuda.synchronize()
    row = 8 * nmax

    def many(n):
        huygens_amd.process_many_device(gs, xt.data_ptr(), nmax, yt.data_ptr(), nmax, n)

    def loop(n):
        for j, g in enumerate(gs):
            g.process_device(xt.data_ptr() + j * row, yt.data_ptr() + j * row, n)

    def sync():
        for g in gs:
            g.synchronize()

    loop(64)   # staged setters uploaded, buffers grown
    sync()
    start = [g.get_state() for g in gs]
    routes = [("loop", loop)] if args.loop_only else [("many", many), ("loop", loop)]

    def run(fn, n, reps):
        for g, s in zip(gs, start):
            g.set_state(s)
        fn(n)   # (slab growth and first-launch costs outside the clock)
        sync()
        for g, s in zip(gs, start):
            g.set_state(s)
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(n)
        sync()
        return (time.perf_counter() - t0) / reps

    def run_single(fn, n):
        ts = []
        for _ in range(20):
            t0 = time.perf_counter()
            fn(n)
            sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts)

    rows = []
    for n, reps in LENGTHS:
        times = {name: [] for name, _ in routes}
        single = {name: [] for name, _ in routes}
        for _ in range(5):
            for name, fn in routes:
                times[name].append(run(fn, n, reps))
            for name, fn in routes:
                single[name].append(run_single(fn, n))
        rec = {"n": n, "reps": reps}
        for name, fn in routes:
            rec[name + "_us"] = 1e6 * statistics.median(times[name])
            rec[name + "_us_runs"] = [round(1e6 * t, 2) for t in times[name]]
            rec[name + "_single_us"] = 1e6 * statistics.median(single[name])
            # kernel times per launch sequence (events cost a few us each: a run of its own)
            prof = gs if name == "loop" else gs[:1]
            for g in prof:
                g.profile(True)
            for g, s in zip(gs, start):
                g.set_state(s)
            for _ in range(reps):
                fn(n)
            sync()
            seg = mix = red = 0.0
            launches = 0
            for g in prof:
                s_, m_, r_, c_ = g.profile_read()
                seg, mix, red, launches = seg + s_, mix + m_, red + r_, launches + c_
                g.profile(False)
            rec[name + "_launches_per_call"] = launches / reps
            rec[name + "_kernel_us_per_call"] = {"segment": 1e3 * seg / reps, "mix": 1e3 * mix / reps,
                                                 "reduce": 1e3 * red / reps}
        if not args.loop_only:
            rec["loop_over_many"] = rec["loop_us"] / rec["many_us"]
        rows.append(rec)
        print(json.dumps(rec), flush=True)
    print("\n| n | " + " | ".join(f"{name} us/call" for name, _ in routes) + " | " +
          " | ".join(f"{name} alone us" for name, _ in routes) + " | launches/call | kernel us/call (segment + mix + reduce) |")
    print("|---|" + "---|" * (2 * len(routes) + 2))
    for rec in rows:
        ks = " vs ".join("{segment:.1f} + {mix:.1f} + {reduce:.1f}".format(**rec[name + "_kernel_us_per_call"]) for name, _ in routes)
        ls = " vs ".join(f"{rec[name + '_launches_per_call']:.0f}" for name, _ in routes)
        print(f"| {rec['n']} | " + " | ".join(f"{rec[name + '_us']:.1f}" for name, _ in routes) + " | " +
              " | ".join(f"{rec[name + '_single_us']:.1f}" for name, _ in routes) + f" | {ls} | {ks} |")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
