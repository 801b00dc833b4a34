"""Cases for oracle/_ref/hz_ref_dump, the reference's own classes compiled from its headers
(oracle/ref/hz_ref_dump.cpp, `make -C oracle ref`).  TEST INFRASTRUCTURE.

A case is a dict of numpy arrays and scalars: the parameters, the event schedule in the
ev_t / ev_kind / ev_a / ev_b layout of oracle_osc.run_note_events (ev_i: an integer operand,
where a class needs one), the input signal where there is one.  reference(case) encodes it (every
floating-point value as a C hex float), runs the binary in a child process and returns the
outputs; the run_* helpers drive an oracle binding or a HIP engine through the same case,
split into several calls at the event times.  tests/golden/ref_*.npz are such cases with the
reference's outputs stored beside them (make_golden_ref.py), so the tests that read them need
neither the binary nor the reference.
"""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref", "hz_ref_dump")
SR = 48000

MAKENOTE, ENDNOTE, REQUEST, RELEASE = 0, 1, 2, 3
FUNDMOD, DECAYMOD, HARMMOD = 10, 11, 12
FREQMOD, PHASEMOD, RESET = 20, 21, 22
MOD_FORWARD, MOD_BACK, BARE_TICKS = 30, 31, 32
GRAIN = 40
TRIGGER = 50

SCALARS = ("relaxation", "mtof", "ftom", "dbtoa")
WAVES = ("saw", "triangle", "square", "phasor", "cycle", "hann", "halfhann", "limiter")


def available() -> bool:
    return os.access(BIN, os.X_OK)


def hx(v) -> str:
    return float(v).hex()


def events(evs):
    """[(t, kind, a[, b[, i]])] -> the ev_* arrays"""
    evs = [tuple(e) + (0.0,) * (5 - len(e)) for e in evs]
    return dict(ev_t=np.array([e[0] for e in evs], dtype=np.int64),
                ev_kind=np.array([e[1] for e in evs], dtype=np.int64),
                ev_a=np.array([e[2] for e in evs], dtype=np.float64),
                ev_b=np.array([e[3] for e in evs], dtype=np.float64),
                ev_i=np.array([int(e[4]) for e in evs], dtype=np.int64))


def split_points(case, extra=()):
    n = int(case["n"])
    return sorted({int(t) for t in case["ev_t"].tolist() if t < n} | {int(t) for t in extra if 0 < t < n})


def _events_at(case, t):
    for e in np.argsort(case["ev_t"], kind="stable"):
        if int(case["ev_t"][e]) == t:
            i = int(case["ev_i"][e]) if "ev_i" in case else 0
            yield int(case["ev_kind"][e]), i, float(case["ev_a"][e]), float(case["ev_b"][e])


def _ops(case, word="run", extra=()):
    n, pos, lines = int(case["n"]), 0, []
    for t in split_points(case, extra) + [n]:
        if t > pos:
            lines.append(f"{word} {t - pos}")
            pos = t
        if t >= n:
            break
        for kind, i, a, b in _events_at(case, t):
            lines.append(f"ev {kind} {i} {hx(a)} {hx(b)}")
    lines.append("end")
    return "\n".join(lines)


def _dump(sub, text):
    with tempfile.TemporaryDirectory() as d:
        case, out = os.path.join(d, "case.txt"), os.path.join(d, "out.f64")
        with open(case, "w") as f:
            f.write(text + "\n")
        subprocess.run([BIN, sub, case, out], check=True, timeout=120)
        return np.fromfile(out, dtype="<f8")


def _arr(v):
    return " ".join(hx(x) for x in np.asarray(v, dtype=np.float64).ravel())


def reference(case) -> dict:
    """The reference's outputs for a case (needs oracle/_ref/hz_ref_dump)."""
    cls = str(case["cls"])
    if cls == "scalars":
        return {fn + "_y": _dump("scalars", f"{len(case[fn + '_x'])}\n" +
                                 "\n".join(f"{fn} {hx(x)}" for x in case[fn + "_x"])) for fn in SCALARS}
    if cls == "wave":
        p = case["phase"]
        return dict(y=_dump("wave", f"{len(p)}\n{_arr(p)}").reshape(len(WAVES), len(p)))
    if cls in ("oscillator", "synth"):
        return dict(y=_dump(cls, f"{hx(case['f'])} {hx(case['phi'])} {hx(case['k'])}\n" + _ops(case)))
    if cls == "sinusoids":
        head = f"{hx(case['fund'])} {int(case['O'])} {hx(case['decay'])} {hx(case['harm'])} {hx(case['k'])}\n"
        return dict(y=_dump(cls, head + _ops(case)))
    if cls == "additive":
        head = f"{int(case['V'])} {int(case['O'])} {hx(case['decay'])} {hx(case['harm'])} {hx(case['k'])}\n"
        return dict(y=_dump(cls, head + _ops(case)))
    if cls == "delay":
        x = case["x"]
        lines, n = int(case["lines"]), int(case["n"])
        text = [f"{int(case['is_float'])} {lines} {int(case['S'])} {int(case['time'])} {x.shape[0]} {n}", _arr(x)]
        for k in range(lines):
            for t, g in ((case["ft"][k], case["fg"][k]), (case["bt"][k], case["bg"][k])):
                text.append(f"{len(t)} " + " ".join(f"{int(a)} {hx(b)}" for a, b in zip(t, g)))
        y = _dump(cls, "\n".join(text) + "\n" + _ops(case)).reshape(lines, n)
        return dict(y=y.astype(np.float32) if int(case["is_float"]) else y)
    if cls == "bowl":
        head = f"{int(case['M'])} {len(case['f'])}\n{_arr(case['f'])}\n{_arr(case['a'])}\n{_arr(case['d'])}\n"
        cuts = np.cumsum(case["seg"]).tolist()
        return dict(y_render=_dump(cls, head + _ops(case)),
                    y_fill=_dump(cls, head + _ops(case, "fill", cuts)).astype(np.float32))
    if cls == "granulator":
        x, par = case["x"], case["ev_par"]
        text = [f"{int(case['P'])} {int(case['size'])} {len(x)}", _arr(x), str(len(par))]
        text += [f"{int(t)} {_arr(p)}" for t, p in zip(case["ev_t"], par)]
        o = _dump(cls, "\n".join(text))
        return dict(y=o[:len(x)], voices=o[len(x):].astype(np.int32))
    raise ValueError(cls)


# ---- driving an oracle binding or a HIP engine through a case --------------------------------

def run_delay(bank_cls, case):
    """Delaybank-like class (coefficients / modulate_* / tick / process): -> y [lines, n]"""
    from oracle_delay import bank_from_golden
    b = bank_from_golden(bank_cls, case)
    x, n = case["x"], int(case["n"])
    out = np.zeros((int(case["lines"]), n), dtype=x.dtype)
    pos = 0
    for t in split_points(case) + [n]:
        if t > pos:
            out[:, pos:t] = b.process(x[:, pos:t] if x.shape[0] > 1 else x[0, pos:t])
            pos = t
        if t >= n:
            break
        for kind, i, a, g in _events_at(case, t):
            if kind == MOD_FORWARD:
                b.modulate_forward(i >> 16, i & 0xFFFF, (int(a), g))
            elif kind == MOD_BACK:
                b.modulate_back(i >> 16, i & 0xFFFF, (int(a), g))
            elif kind == BARE_TICKS:
                b.tick(int(a))
    return out


def run_bowl(bowl, case, method):
    """Bowl-like object; method 'render' or 'fill', called per segment of case['seg'] and at
    the trigger() events."""
    n = int(case["n"])
    out = np.zeros(n, dtype=np.float32 if method == "fill" else np.float64)
    pos = 0
    for t in split_points(case, np.cumsum(case["seg"]).tolist()) + [n]:
        if t > pos:
            out[pos:t] = getattr(bowl, method)(t - pos)
            pos = t
        if t >= n:
            break
        for kind, _, _, _ in _events_at(case, t):
            if kind == TRIGGER:
                bowl.trigger()
    return out


def grain_requests(case, lo=0, hi=None):
    hi = int(case["n"]) if hi is None else hi
    return [(int(t) - lo,) + tuple(float(v) for v in p) for t, p in zip(case["ev_t"], case["ev_par"]) if lo <= t < hi]


def run_granulator(gran, case, blocks=None):
    """Granulator-like object with process(x, requests) -> (y, voices), in blocks."""
    x, n = case["x"], int(case["n"])
    ys, vs, pos = [], [], 0
    for b in (blocks or [n]):
        y, v = gran.process(x[pos:pos + b], grain_requests(case, pos, pos + b))
        ys.append(y)
        vs.extend(int(k) for k in v)
        pos += b
    assert pos == n
    return np.concatenate(ys), np.array(vs, dtype=np.int32)


# ---- seeded random cases (tests/test_ref_live_cpu.py), in the ranges of the pinned table ------

def _osc_events(rng, n, count):
    evs = []
    for t in sorted(rng.integers(1, n, count).tolist()):
        kind = int(rng.choice([FREQMOD, FREQMOD, PHASEMOD, PHASEMOD, RESET]))
        if kind == PHASEMOD:
            a = float(rng.choice([0.3, 0.5, -0.25, rng.uniform(-2, 2)]))
        else:
            a = float(rng.uniform(20.0, 4000.0))
        evs.append((t, kind, a))
    return evs


def random_case(cls, rng):
    if cls in ("oscillator", "synth"):
        n = int(rng.integers(500, 2000))
        k = float(rng.choice([2.0 / SR, 0.0001, rng.uniform(1e-5, 1e-2)]))
        return dict(cls=cls, f=float(rng.uniform(-3000, 3000)), phi=float(rng.uniform(-0.2, 0.9)), k=k, n=n,
                    **events(_osc_events(rng, n, 8)))
    if cls == "sinusoids":
        n = int(rng.integers(500, 2000))
        evs = [(int(rng.integers(1, n)), kind, float(rng.uniform(*r)))
               for kind, r in ((FUNDMOD, (50, 800)), (DECAYMOD, (0.3, 1.0)), (HARMMOD, (0.8, 1.4)))]
        return dict(cls=cls, fund=float(rng.uniform(50, 800)), O=int(rng.integers(1, 12)),
                    decay=float(rng.choice([0.7, 1.0, rng.uniform(0.3, 0.99)])),
                    harm=float(rng.choice([1.0, 1.3])), k=float(rng.choice([2.0 / SR, 0.001, 0.01])), n=n,
                    **events(sorted(evs)))
    if cls == "additive":
        n, V = int(rng.integers(800, 2500)), int(rng.integers(2, 5))
        pitches = rng.permutation(np.arange(36, 96))[:V + 3].astype(float)
        evs = [(int(rng.integers(0, n // 4)), MAKENOTE, float(p), float(rng.uniform(0.1, 1.0))) for p in pitches[:V]]
        evs.append((int(rng.integers(n // 4, n // 2)), MAKENOTE, float(pitches[V]), 0.7))       # steals a voice
        evs.append((int(rng.integers(n // 2, 3 * n // 4)), ENDNOTE, float(pitches[0]), 0.0))
        evs.append((int(rng.integers(n // 2, 3 * n // 4)), RELEASE, float(rng.integers(-1, V)), 0.0))
        evs.append((int(rng.integers(3 * n // 4, n)), REQUEST, float(rng.uniform(100, 900)), float(rng.uniform(0.1, 1))))
        return dict(cls=cls, V=V, O=int(rng.integers(2, 8)), decay=float(rng.choice([0.7, 1.0])),
                    harm=float(rng.choice([1.0, 1.3])), k=float(rng.choice([0.1, 0.01, 0.001])), n=n,
                    **events(sorted(evs)))
    if cls == "delay":
        is_float = int(rng.integers(0, 2))
        lines, S, time, n = int(rng.choice([1, 3])), 3, int(rng.choice([50, 7, 200])), int(rng.integers(500, 2000))
        dt = np.float32 if is_float else np.float64
        x = rng.standard_normal((int(rng.choice([1, lines])), n)).astype(dt)
        gain = lambda lim: float(dt(rng.uniform(-lim, lim)))   # noqa: E731
        ft = rng.integers(0, 2 * time + 3, (lines, S))
        bt = rng.integers(0, 2 * time + 3, (lines, S))
        evs = []
        for t in sorted(rng.integers(1, n, 4).tolist()):
            kind = int(rng.choice([MOD_FORWARD, MOD_BACK, BARE_TICKS]))
            line_tap = (int(rng.integers(0, lines)) << 16) | int(rng.integers(0, S))
            if kind == BARE_TICKS:
                evs.append((t, kind, float(rng.integers(0, 2 * time + 5)), 0.0, 0))
            else:
                evs.append((t, kind, float(rng.integers(0, 2 * time + 3)), gain(0.3), line_tap))
        return dict(cls=cls, is_float=is_float, lines=lines, S=S, time=time, n=n, x=x, ft=ft, bt=bt,
                    fg=np.array([[gain(1.0) for _ in range(S)] for _ in range(lines)]),
                    bg=np.array([[gain(0.3) for _ in range(S)] for _ in range(lines)]), **events(evs))
    if cls == "bowl":
        M, n = int(rng.choice([1, 5, 67, int(rng.integers(2, 130))])), int(rng.integers(300, 1500))
        count = int(rng.choice([M, max(1, M - 2), M + 3]))   # the constructor's resize pads with zeros or cuts
        return dict(cls=cls, M=M, n=n, f=np.exp(rng.uniform(np.log(20.0), np.log(16000.0), count)),
                    a=rng.uniform(1e-4, 5e-2, count), d=rng.uniform(0.05, 15.0, count),
                    seg=np.array([n // 3, 1, n - n // 3 - 1]), **events([(int(rng.integers(1, n)), TRIGGER, 0.0)]))
    if cls == "granulator":
        P, size, n = int(rng.choice([1, 4, 16])), int(rng.choice([37, 500, 4000])), int(rng.integers(500, 2000))
        at = sorted(rng.integers(0, n, 12).tolist())
        par = [(float(rng.uniform(0, 2 * size / SR)), float(rng.choice([0.0, rng.uniform(0.02, 8.0) / 1000.0])),
                float(rng.choice([1.0, 2.0, -1.0, rng.uniform(-2, 3)])), float(rng.uniform(0, 1)), 0.0) for _ in at]
        return dict(cls=cls, P=P, size=size, n=n, x=rng.standard_normal(n), ev_t=np.array(at, dtype=np.int64),
                    ev_kind=np.full(len(at), GRAIN, dtype=np.int64), ev_par=np.array(par))
    raise ValueError(cls)


# ---- the C oracle's outputs for a case, through the existing Oracle* bindings ------------------

def oracle_outputs(case) -> dict:
    """What oracle/hz_oracle*.c computes for a case, keyed like reference()."""
    from oracle import lib
    from oracle_bowl import OracleBowl
    from oracle_delay import OracleDelaybank
    from oracle_gran import OracleGranulator
    from oracle_osc import (OracleAdditive, OracleOscillator, OracleSinusoids, oracle_dbtoa, oracle_wave,
                            run_note_events)
    cls = str(case["cls"])
    if cls == "scalars":
        fns = dict(relaxation=lib().orc_relaxation, mtof=lib().orc_mtof, ftom=lib().orc_ftom, dbtoa=oracle_dbtoa)
        return {fn + "_y": np.array([fns[fn](float(x)) for x in case[fn + "_x"]]) for fn in SCALARS}
    if cls == "wave":
        return dict(y=np.array([[oracle_wave(w, float(p)) for p in case["phase"]] for w in range(len(WAVES))]))
    if cls in ("oscillator", "synth"):
        o = OracleOscillator(float(case["f"]), float(case["phi"]), float(case["k"]), wave=cls == "synth")
        return dict(y=run_note_events(o, case))
    if cls == "sinusoids":
        o = OracleSinusoids(float(case["fund"]), int(case["O"]), float(case["decay"]), float(case["harm"]),
                            float(case["k"]))
        return dict(y=run_note_events(o, case))
    if cls == "additive":
        o = OracleAdditive(int(case["V"]), int(case["O"]), float(case["decay"]), float(case["harm"]), float(case["k"]))
        return dict(y=run_note_events(o, case))
    if cls == "delay":
        return dict(y=run_delay(OracleDelaybank, case))
    if cls == "bowl":
        mk = lambda: OracleBowl(int(case["M"]), case["f"], case["a"], case["d"], np.float64)   # noqa: E731
        return dict(y_render=run_bowl(mk(), case, "render"), y_fill=run_bowl(mk(), case, "fill"))
    if cls == "granulator":
        n = int(case["n"])
        y, v = run_granulator(OracleGranulator(int(case["size"]), int(case["P"])), case, [n // 3, 1, n - n // 3 - 1])
        return dict(y=y, voices=v)
    raise ValueError(cls)


def bit_equal(a, b) -> bool:
    """same dtype, shape and bits (so NaNs and signed zeros count)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def max_abs_diff(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b), initial=0.0))
