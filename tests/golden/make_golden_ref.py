"""Fixtures made by the reference itself (run: python tests/golden/make_golden_ref.py).

TEST INFRASTRUCTURE.  Unlike the other make_golden_*.py, nothing here restates the reference:
the fixed case table below is run through oracle/_ref/hz_ref_dump (the reference's own headers,
compiled by `make -C oracle ref`) and every tests/golden/ref_<class>_<case>.npz holds the case
(parameters, ev_* schedule, input signal) beside what the reference computed for it, tagged
made_by="reference".  Data only.  A file whose arrays would not change is left untouched, so a
second run leaves the tree as it was.

The cases are the smallest that reach the branches where a restatement or a kernel goes wrong;
each says which below.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_driver as R  # noqa: E402

SR = R.SR


def cases():
    out = {}
    # scalars: k = 0 (the early return), k < 0 (fmax(0, k): a division by zero), the defaults in use
    out["scalars_all"] = dict(
        cls="scalars",
        relaxation_x=np.array([0.0, 2.0 / SR, 0.0001, 0.001, 0.01, 0.1, 1.0, 10.0, -1.0]),
        mtof_x=np.array([0.0, 21.0, 36.5, 60.0, 69.0, 69.25, 100.0, 127.0, -12.0]),
        ftom_x=np.array([8.175798915643707, 27.5, 261.6255653005986, 440.0, 441.0, 1234.5, 16000.0]),
        dbtoa_x=np.array([-96.0, -60.0, -8.0, -3.0, -0.5, 0.0, 6.0, 20.0]))
    # waves: outside [0, 1), 0.5 exactly (square's zero), negatives for the limiter
    out["wave_shapes"] = dict(cls="wave", phase=np.array(
        [-100.0, -3.7, -1.25, -0.5, -0.1, 0.0, 1e-9, 0.1, 0.25, 0.4999999999999999, 0.5, 0.5000000000000001, 0.75,
         0.999, 1.0, 1.5, 2.3, 7.125, 100.0]))
    # Oscillator / Synth: phasemod(0.3), the ambiguous phasemod(0.5), a negative offset, freqmod steps, reset;
    # the default relaxation time and Additive's
    osc_ev = [(300, R.PHASEMOD, 0.3), (800, R.PHASEMOD, 0.5), (1300, R.PHASEMOD, -0.4), (1700, R.FREQMOD, 660.0),
              (2200, R.FREQMOD, 110.0), (2700, R.RESET, 220.0), (2900, R.PHASEMOD, -1.75)]
    for name, k in (("k2sr", 2.0 / SR), ("k1e4", 0.0001)):
        out["oscillator_" + name] = dict(cls="oscillator", f=440.0, phi=0.1, k=k, n=3200, **R.events(osc_ev))
    out["synth_mods"] = dict(cls="synth", f=-330.0, phi=0.25, k=0.0001, n=3200, **R.events(osc_ev))
    # frequency steps alone, phase 0, default k: what Sinusoids(f, 1, 1, 1, k=0) must equal
    out["synth_freqsteps"] = dict(cls="synth", f=220.0, phi=0.0, k=2.0 / SR, n=3000, **R.events(
        [(500, R.FREQMOD, 330.0), (1500, R.FREQMOD, 55.0), (2500, R.FREQMOD, 1760.0)]))
    # Sinusoids: each modulator stepped once, slow and default relaxation
    sin_ev = [(1000, R.FUNDMOD, 330.0), (2000, R.DECAYMOD, 0.5), (3000, R.HARMMOD, 1.1)]
    out["sinusoids_o5_slow"] = dict(cls="sinusoids", fund=220.0, O=5, decay=0.7, harm=1.0, k=0.01, n=4096,
                                    **R.events(sin_ev))
    out["sinusoids_o7_inharm"] = dict(cls="sinusoids", fund=110.0, O=7, decay=1.0, harm=1.3, k=2.0 / SR, n=4096,
                                      **R.events(sin_ev))
    # Additive 3 x 5: three notes, a fourth that steals the nearest voice, an endnote whose release tail (k = 0.1 s,
    # 4800 samples) outlasts the run so amplitudes[i] keeps ticking with active[i] == 0, request() into the freed
    # voice, release(); decay 1.0 is the `normalization = overtones` branch
    add_ev = [(0, R.MAKENOTE, 60.0, 1.0), (0, R.MAKENOTE, 67.0, 0.5), (300, R.MAKENOTE, 72.0, 0.8),
              (1200, R.MAKENOTE, 65.0, 0.9), (2000, R.ENDNOTE, 60.0), (2600, R.REQUEST, 330.0, 0.6),
              (3300, R.RELEASE, 1.0)]
    for name, decay, harm in (("d07_h10", 0.7, 1.0), ("d10_h13", 1.0, 1.3)):
        out["additive_v3o5_" + name] = dict(cls="additive", V=3, O=5, decay=decay, harm=harm, k=0.1, n=4096,
                                            **R.events(add_ev))
    # Delay: sparsity 3, time 50 (ring 51): taps at 0, at `time`, beyond it (77, 64: the unsigned wrap of the ring
    # index), a zero-time feedback tap (dropped), modulate_forward, modulate_back mid-run incl. a zero-time one,
    # ten bare tick()s
    rng = np.random.default_rng(20)
    for lines in (1, 3):
        ft = np.array([[0, 50, 77 + k] for k in range(lines)])
        fg = np.array([[1.0, 0.5, -0.25 + 0.0625 * k] for k in range(lines)])
        bt = np.array([[0, 13 + 5 * k, 64] for k in range(lines)])
        bg = np.array([[0.4, 0.3, -0.2] for k in range(lines)])
        ev = [(600, R.MOD_FORWARD, 5.0, -0.5, 1), (1000, R.MOD_BACK, 21.0, 0.25, ((lines - 1) << 16) | 1),
              (1000, R.MOD_BACK, 0.0, 0.7, 2), (1500, R.BARE_TICKS, 10.0, 0.0, 0)]
        x64 = rng.standard_normal((1, 2000))
        for tag, dt in (("d", np.float64), ("f", np.float32)):
            out[f"delay_l{lines}_{tag}"] = dict(cls="delay", is_float=int(dt == np.float32), lines=lines, S=3, time=50,
                                                n=2000, x=x64.astype(dt), ft=ft, fg=fg, bt=bt, bg=bg, **R.events(ev))
    # Bowl: 5 modes and 67 (past one 64-lane wavefront); 3000 samples as n // 3, 1, the rest; trigger() mid-run
    for M in (5, 67):
        r = np.random.default_rng(M)
        out[f"bowl_m{M}"] = dict(cls="bowl", M=M, n=3000, f=np.exp(r.uniform(np.log(20.0), np.log(16000.0), M)),
                                 a=r.uniform(1e-4, 5e-2, M), d=r.uniform(0.05, 15.0, M),
                                 seg=np.array([1000, 1, 1999]), **R.events([(1700, R.TRIGGER, 0.0)]))
    # Granulator, polyphony 4: speeds 1, 2, -1; offset 0.001 < size (speed - 1): the clamp; a grain of exactly 750
    # samples (ends at ticks == sizes) and one of 484.8; a fifth request refused; size == 0; a voice reused
    req = [(10, 0.0, 1.0 / 64, 1.0, 0.8, 0.0), (10, 0.001, 0.0101, 2.0, 0.5, 0.0), (50, 0.02, 0.02, -1.0, 0.7, 0.0),
           (60, 0.0, 0.03, 1.0, 0.3, 0.0), (70, 0.0, 0.01, 1.0, 1.0, 0.0), (80, 0.0, 0.0, 1.0, 1.0, 0.0),
           (1000, 0.0, 0.005, 2.0, 0.9, 0.0)]
    out["granulator_p4"] = dict(cls="granulator", P=4, size=4000, n=3000, x=np.random.default_rng(4).standard_normal(3000),
                                ev_t=np.array([r[0] for r in req], dtype=np.int64),
                                ev_kind=np.full(len(req), R.GRAIN, dtype=np.int64),
                                ev_par=np.array([r[1:] for r in req]))
    return out


def same(path, d):
    if not os.path.exists(path):
        return False
    with np.load(path, allow_pickle=False) as z:
        if sorted(z.files) != sorted(d):
            return False
        for k in d:
            a, b = z[k], np.asarray(d[k])
            if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                return False
    return True


def main():
    if not R.available():
        sys.exit("oracle/_ref/hz_ref_dump is missing: make -C oracle ref (needs the reference's sources)")
    for name, case in cases().items():
        d = dict(case, made_by="reference", **R.reference(case))
        path = os.path.join(HERE, f"ref_{name}.npz")
        if same(path, d):
            print("unchanged", name)
        else:
            np.savez(path, **d)
            print("wrote", name)


if __name__ == "__main__":
    main()
