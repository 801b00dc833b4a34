"""SHA-256 of the outputs of a fixed case table, for comparing two builds of the library bit for bit.

    HZ_LIB_PATH=/path/to/libhuygens_hip.so python scripts/mixdown_bits.py --out FILE [--hash-dir DIR]

The cases are small shapes that reach every branch of the mixdown skeleton (hz_mix.h, hz_mixplan.h)
and every kernel whose dynamic-LDS limit hz::allow_lds raises: Oscbank (1, 300 and 16384 active, a
third inactive, mix and per-band outputs), Additive (one group: the direct store; several groups;
after endnote), Sinusoids, Bowl in double and float (short and long reduce), Subtractive (two
channels), the general Filterbank engine with softclip (N = 64: time segments and the segment
carry), the LTI engine, a gated STFT at N = 8192, Cosine(8192), one long frame at N = 16384 and a
Freezer at N = 8192.  Inputs come from fixed numpy seeds; the Freezer's libc rand() is seeded.
--hash-dir adds the files of a directory (bench.py --dump-outputs).  One JSON object
{case: sha256}; two runs agree when every hash is equal.  Needs a gfx950 device.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def resonators(N, R):
    """N two-pole band-passes, centres spread over (0, pi)"""
    w = np.pi * (np.arange(N) + 0.5) / (N + 1)
    g = (1 - R * R) / 2
    fwd = np.stack([np.full(N, g), np.zeros(N), np.full(N, -g)], axis=1)
    back = np.stack([-2 * R * np.cos(w), np.full(N, R * R)], axis=1)
    return fwd, back


def cases():
    from huygens_amd import Additive, Bowl, Cosine, Filterbank, Freezer, Oscbank, Sinusoids, Subtractive
    from huygens_amd._lib import HZ_DIST_SOFTCLIP, HZ_FB_PATH_GENERAL, HZ_FB_RESP_OFF
    from huygens_amd.stft import StaticSTFT

    # ---- Oscbank
    for N, keep in ((1, 1), (300, 1), (16384, 1), (300, 3)):
        for n in (1, 1024, 1025, 5000):
            if N == 16384 and n not in (1024, 5000):
                continue
            rng = np.random.default_rng(N + keep)
            o = Oscbank(N)
            for i, hz in enumerate(rng.uniform(20.0, 20000.0, N)):
                o.freqmod(i, hz)
            o.activate([i for i in range(N) if keep == 1 or i % keep])   # keep 3: a third inactive
            per_band = N <= 300
            a = o.fill(n, per_band)
            b = o.fill(n, per_band)   # a second call: the advanced phasors
            yield f"osc_N{N}_keep{keep}_n{n}", sha(*(a if per_band else (a,)), *(b if per_band else (b,)))
            o.close()

    # ---- Additive / Sinusoids
    for V, O in ((1, 5), (3, 130), (2, 200)):
        for n in (2048, 2049, 7000):
            a = Additive(V, O, 0.7, 1.0)
            for v in range(V):
                a.makenote(48.0 + 7 * v, 0.5)
            yield f"add_V{V}_O{O}_n{n}", sha(a.fill(n), a.fill(n))
            a.close()
    a = Additive(3, 130, 0.7, 1.0)
    for v in range(3):
        a.makenote(48.0 + 7 * v, 0.5)
    first = a.fill(2049)
    a.endnote(55.0)
    yield "add_V3_O130_endnote", sha(first, a.fill(7000))
    a.close()
    s = Sinusoids(110.0, 5, 0.7)
    first = s.fill(2049)
    s.fundmod(220.0)
    s.decaymod(0.5)
    yield "sin_O5", sha(first, s.fill(7000))
    s.close()

    # ---- Bowl
    for dtype in (np.float64, np.float32):
        for M, n, groups in ((5, 7000, 1), (303, 1024, 256), (303, 30000, 256)):
            rng = np.random.default_rng(M)
            f = np.exp(rng.uniform(np.log(20.0), np.log(16000.0), M))
            amp = rng.uniform(1e-4, 5e-2, M)
            d = rng.uniform(0.05, 15.0, M)
            b = Bowl(M, f, amp, d, dtype)
            b.set_target_groups(groups)
            yield f"bowl_{np.dtype(dtype).name}_M{M}_n{n}", sha(b.fill(n), b.fill(n), b.render(n))
            b.close()

    # ---- Subtractive: 2 channels, 20 voices x 4 overtones = 2 groups of 64 filters
    for n in (300, 5000):
        su = Subtractive(20, 4, 0.7, channels=2)
        for v in range(6):
            su.makenote(40.0 + 5 * v, 0.5)
        x = np.random.default_rng(n).uniform(-1, 1, (2, n))
        yield f"sub_n{n}", sha(su.process(x), su.process(x))
        su.close()

    # ---- Filterbank: the general engine with softclip, then the LTI engine
    for N in (64, 512):
        fwd, back = resonators(N, 0.999)
        fb = Filterbank(2, N, 0.1, 1.0)
        for k in range(N):
            fb.coefficients(k, fwd[k], back[k])
        fb.boost(np.ones(N))
        fb.open()
        fb.distortion(HZ_DIST_SOFTCLIP)
        fb.set_path(HZ_FB_PATH_GENERAL)
        x = np.random.default_rng(N).uniform(-1, 1, 5000)
        y0, y1 = fb.process(x), fb.process(x)
        yield f"fb_general_softclip_N{N}", sha(y0, y1)
        fb.close()
    fwd, back = resonators(256, 0.999)
    fb = Filterbank(2, 256, 0.001, 0.001)
    fb.set_response(HZ_FB_RESP_OFF)
    for k in range(256):
        fb.coefficients(k, fwd[k], back[k])
    fb.boost(np.ones(256))
    fb.open()
    rng = np.random.default_rng(256)
    ys, paths = [], []
    for n in (4096, 4096, 100000):   # the first call starts unconverged: the general engine
        ys.append(fb.process(rng.uniform(-1, 1, n)))
        paths.append(fb.last_path())
    yield "fb_lti_N256_paths_" + "".join(map(str, paths)), sha(*ys)
    fb.close()

    # ---- the transforms
    x = np.random.default_rng(8192).standard_normal(5 * 8192 + 3)
    x[::2] += np.sin(2 * np.pi * 1000 * np.arange(x[::2].size) / 48000)
    f = StaticSTFT(8192, 4)
    yield "stft_static_N8192", sha(*f.process_block(x))
    f.close()
    c = Cosine(8192)
    c.inp[:] = x[:8192]
    c.forward()
    fw = c.out.copy()
    c.out[:] = x[8192:16384]
    c.backward()
    yield "cosine_N8192", sha(fw, c.inp)
    c.close()
    f = StaticSTFT(16384, 4, long_frames=True)
    yield "stft_static_long_N16384", sha(*f.process_block(x[:2 * 16384]))
    f.close()
    C.CDLL(None).srand(C.c_uint(7))
    z = Freezer(8192, 4)
    yield "freezer_N8192", sha(z.process(x[:40000], [(20000, 1), (35000, 0)]))
    z.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--hash-dir", default="")
    args = ap.parse_args()
    try:  # one HIP runtime per process: torch-ROCm's first (huygens_amd/_lib.py)
        import torch  # noqa: F401
    except Exception:
        pass
    table = {}
    for name, digest in cases():
        table[name] = digest
        print(name, digest[:16], flush=True)
    if args.hash_dir:
        for fn in sorted(os.listdir(args.hash_dir)):
            with open(os.path.join(args.hash_dir, fn), "rb") as fh:
                table["dump/" + fn] = hashlib.sha256(fh.read()).hexdigest()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(table, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
