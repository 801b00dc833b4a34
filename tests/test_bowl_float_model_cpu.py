"""CPU proofs under tests/test_bowl_modes_gpu.py: everything its cases rest on, from the float
restatement (OracleBowl) and the numpy model of the kernels (bowl_float_model.py) alone.

The per-mode bound  |y - reference| <= 3e-7 a_i  (bowl_float_model.PER_MODE), derived:
  * each side rounds its sample to float32 once at the end: 2 x 2^-24 |y| <= 1.2e-7 a_i;
  * the decay's exponent is the reference's float32 one at a chunk's first sample and stepped
    from there, which moves the term by < 2.5e-8 a_i (hz_bowl.hip's header);
  * the wave value is rounded to float32 on both sides, from doubles that differ by the
    reference's own double argument (a few 1e-9 at late counters) and the polynomial's 1.35e-11,
    so the two roundings may fall to different sides: one float32 spacing of a value <= 1, scaled
    by the decay, <= 1.2e-7 a_i.
Together 2.65e-7 a_i < 3e-7 a_i.  Measured on the cases below (printed): <= 1.15e-7 a_i.

1. one-hot banks equal single-mode banks, bit for bit (the GPU cases' references are M = 1);
2. model against restatement for every GPU case, under the bound, and every compared window
   visible (visibility.assert_visible: the hot mode's peak >= 1000 x the bound);
3. sin2pi_ref restated, against long double;
4. the plan restatement: the literals of bowl_mode_cases.py, the constants in the sources, and
   what the hot modes are;
5. mutants of the model that pass the old mixdown check and fail the per-mode one.
"""
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest

import bowl_float_model as bm
import bowl_mode_cases as bc
import visibility as vz
from oracle import rel_err
from oracle_bowl import OracleBowl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORTH_STAR = 1e-5   # the old check: mixdown against the restatement, relative to the mix's peak


def ref_single(fad, start, calls):
    """the restatement of one mode from counter `start` over the calls, concatenated"""
    f, a, d = fad
    o = OracleBowl(1, [f], [a], [d], np.float32)
    o.seek(start)
    return o.fill(int(sum(calls)))


def check_mode(fad, start, calls, chunk, windows=None):
    """model against restatement under the bound, every window visible -> error / a_i"""
    ref = ref_single(fad, start, calls)
    mod = bm.model_fill([fad[0]], [fad[1]], [fad[2]], calls, chunk, n0=start)
    a32 = float(np.float32(fad[1]))
    for lo, hi in windows or [(0, len(ref))]:
        vz.assert_visible(vz.component_visibility(np.max(np.abs(ref[lo:hi])), a32), bm.PER_MODE)
    err = bm.per_mode_error(mod, ref, fad[1])
    assert err <= bm.PER_MODE, "mode %r from %d: model off by %.3e a_i" % (fad, start, err)
    return err


# ---- 1. one-hot == single mode ----------------------------------------------------------------------

@pytest.mark.parametrize("start", [0, 479_000, bc.STUCK - 100])
def test_one_hot_bank_is_the_single_mode_bit_for_bit(start):
    M, n = 7, 400
    for i in range(M):
        fad = bc.mode_of(M, i)
        if start:
            fad = (fad[0], fad[1], 0.003)
        f, a, d = bc.one_hot(M, i, fad)
        o = OracleBowl(M, f, a, d, np.float32)
        o.seek(start)
        full, single = o.fill(n), ref_single(fad, start, [n])
        assert np.array_equal(full.view(np.uint32), single.view(np.uint32))
        assert np.max(np.abs(single)) > 0


# ---- 2. the bound and the visibility of every GPU case ----------------------------------------------

@pytest.mark.parametrize("M", bc.FILL_M)
def test_fill_cases_bound_and_visibility(M):
    hot = sorted(set().union(*(bc.fill_hot(M, g) for g in bc.FILL_GROUPS)))
    worst = max(check_mode(bc.mode_of(M, i), 0, bc.FILL_CALLS, bm.K_L, bc.FILL_WINDOWS) for i in hot)
    print("fill M = %d, %d hot modes: model - restatement <= %.3e a_i" % (M, len(hot), worst))


@pytest.mark.parametrize("start", bc.LATE_STARTS)
def test_late_cases_bound_and_visibility(start):
    calls = [bc.LATE_WINDOW, 1000]
    worst = max(check_mode(m, start, calls, bm.K_L) for m in bc.late_modes(start))
    print("late counter %d: model - restatement <= %.3e a_i" % (start, worst))
    for M in bc.LATE_M:   # the all-hot banks: the old mixdown bound, and the reference's constant
        f, a, d = bc.late_bank(M)
        o = OracleBowl(M, f, a, d, np.float32)
        o.seek(start)
        ref = o.fill(sum(calls))
        mod = bm.model_fill(f, a, d, calls, bm.K_L, n0=start)
        assert rel_err(mod, ref) < NORTH_STAR
        if start + bc.LATE_WINDOW > bc.STUCK:
            k = bc.STUCK - start
            assert np.all(ref[k:] == ref[k]) and np.all(mod[k:] == mod[k]) and ref[k] != 0


@pytest.mark.parametrize("M", bc.CHAIN_M)
def test_chain_cases_bound_and_visibility(M):
    runs = [(0, bc.CHAIN_BLOCKS, False)]
    if M in bc.CHAIN_LATE_M:
        runs += [(bc.CHAIN_LATE, bc.CHAIN_BLOCKS, True), (bc.CHAIN_STUCK_START, bc.CHAIN_STUCK_BLOCKS, True)]
    for start, blocks, late in runs:
        worst = max(check_mode(bc.chain_mode(M, i, late), start, blocks, bm.CHAIN_SPW) for i in bc.chain_hot(M))
        print("chain M = %d from %d: model - restatement <= %.3e a_i" % (M, start, worst))


def test_stuck_counter_is_constant_in_reference_and_model():
    """From the first sample at 2^24 on the reference repeats one value; so does the model, in a
    call the counter sticks in and in one that starts stuck.  The kernels' stepped decay alone
    (stuck=False, the engine before stuck_sum) does not: the issue's sawtooth, 1.9e-7 / 2.8e-7 / 4.5e-9 a."""
    start, n, k = bc.STUCK - 3000, 6000, 3000
    for d, saw in ((0.001, 1.9e-7), (1 / 350, 2.8e-7), (0.02, 4.5e-9)):
        ref = ref_single((440.0, 0.03, d), start, [n + 100])
        assert np.all(ref[k:] == ref[k])
        for chunk in (bm.K_L, bm.CHAIN_SPW):
            mod = bm.model_fill([440.0], [0.03], [d], [n, 100], chunk, n0=start)
            assert np.all(mod[k:] == mod[k])
            assert bm.per_mode_error(mod, ref, 0.03) <= bm.PER_MODE
        old = bm.model_fill([440.0], [0.03], [d], [n], bm.K_L, n0=start, stuck=False)
        dev = bm.per_mode_error(old[k:], ref[k:n], 0.03)
        assert 0.9 * saw < dev < 1.1 * saw and not np.all(old[k:] == old[k])
        assert np.array_equal(old[:k], bm.model_fill([440.0], [0.03], [d], [n], bm.K_L, n0=start)[:k])


# ---- 3. sin2pi_ref ----------------------------------------------------------------------------------

def test_sin2pi_ref_against_long_double():
    """|sin2pi_ref(p) - sin(2 PI p)| < 1.4e-11 (the kernel comment's bound) over float32 p across
    [0, 2^24 * 16000 / 48000] and on to 2^24, where p has a spacing of 0.5 and of 1.  PI is the
    reference's: the double nearest 3.14159265359.  The reference value is sinl of the exactly
    reduced argument: 2 PI p = 2 pi (r + p e) with r = p - round(p) exact and e = PI / pi - 1 from
    50 digits, so that the long double's own rounding of a 1e8 rad argument (1e-11) does not enter.
    kE is that e as a literal, in the kernel and in the model: the quotient formed in double,
    3.14159265359 / M_PI - 1.0, is 0.2 % off, which is 4.7e-9 in the sine at p = 5.6e6; with the
    literal the polynomial's 1.35e-11 is what remains."""
    getcontext().prec = 60
    pi50 = Decimal("3.14159265358979323846264338327950288419716939937510")
    e50 = Decimal(3.14159265359) / pi50 - 1          # Decimal(float) is the double's exact value
    e = np.longdouble(str(e50))
    two_pi = np.longdouble(2) * np.longdouble(str(pi50))
    assert bm.K_E == float(e50) and abs(3.14159265359 / np.pi - 1.0 - bm.K_E) > 1e-16
    m = re.search(r"constexpr double kE = ([0-9.e+-]+);", _src("hz_bowl.hip"))
    assert m and float(m.group(1)) == bm.K_E
    rng = np.random.default_rng(11)
    top = 2.0 ** 24 * 16000 / 48000
    ps = [rng.uniform(0, 4, 20000), rng.uniform(0, top, 20000), rng.uniform(2.0 ** 22, top, 5000),
          rng.uniform(2.0 ** 23, 2.0 ** 24, 5000), np.exp(rng.uniform(np.log(1e-3), np.log(top), 20000)),
          np.arange(0, 64) / 8.0, 2.0 ** 22 + np.arange(0, 64) / 2.0, 2.0 ** 23 + np.arange(0, 64)]
    worst = 0.0
    for p in ps:
        p = p.astype(np.float32)
        pl = p.astype(np.longdouble)
        want = np.sin(two_pi * ((pl - np.rint(pl)) + pl * e))
        worst = max(worst, float(np.max(np.abs(bm.sin2pi_ref(p).astype(np.longdouble) - want))))
    print("sin2pi_ref: max error %.3e" % worst)
    assert worst < 1.4e-11
    sp = np.spacing(np.float32([2.0 ** 22, 2.0 ** 23]))
    assert sp[0] == 0.5 and sp[1] == 1.0 and 2.0 ** 22 < top


# ---- 4. the plan ------------------------------------------------------------------------------------

def _src(name):
    with open(os.path.join(ROOT, "huygens_amd", "csrc", name)) as fh:
        return fh.read()


def test_plan_constants_are_the_sources():
    bowl, mix = _src("hz_bowl.hip"), _src("hz_mix.h")
    for text, name, value in ((mix, "kWaves", bm.K_WAVES), (mix, "kMaxPerWave", bm.K_MAX_PER_WAVE),
                              (bowl, "kL", bm.K_L), (bowl, "kShortSlices", bm.SHORT_SLICES),
                              (bowl, "kChainSpw", bm.CHAIN_SPW), (bowl, "kChainThreads", bm.CHAIN_THREADS),
                              (bowl, "kPre", bm.CHAIN_PRE)):
        m = re.search(r"constexpr int %s = (\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    assert re.search(r"constexpr long kShortMax = %d;" % bm.SHORT_MAX, bowl)
    assert "constexpr int tile_len(int kL) { return 64 * kL; }" in mix
    # bowl_launch's three plan lines and the short reduce's two passes, as restated in bowl_plan
    for line in ("std::min(kMaxPerWave, std::max(1, (M + kWaves * 32 - 1) / (kWaves * 32)))",
                 "(long)M * ntiles / ((long)kWaves * 2 * h->target_groups)",
                 "std::max(1, (M + kWaves * per_wave - 1) / (kWaves * per_wave))",
                 "for (; g + 7 * kShortSlices < G; g += 8 * kShortSlices)",
                 "for (; g < G; g += kShortSlices)",
                 "const int first = (blockIdx.x * kWaves + wave) * a.per_wave;",
                 "for (int m0 = tid; m0 < a.M; m0 += kPre * kChainThreads)"):
        assert line in bowl, line
    literals = {float(x) for x in re.findall(r"-?\d+\.\d{10,}", bowl)}
    assert set(bm._POLY) <= literals


def test_plan_literals():
    for (M, g), plans in bc.FILL_PLANS.items():
        for n, want in plans.items():
            p = bm.bowl_plan(M, n, g)
            assert (p["per_wave"], p["G"], p["nseg"], p["reduce"]) == want, (M, g, n)
        for n in bc.FILL_CALLS:   # every call's plan is one of the three
            p, q = bm.bowl_plan(M, n, g), bm.bowl_plan(M, min(bc.PLAN_CALLS, key=lambda c: (c < n, c)), g)
            assert (p["per_wave"], p["G"]) == (q["per_wave"], q["G"]), (M, g, n)
    assert sorted(bc.FILL_PLANS) == sorted((M, g) for M in bc.FILL_M for g in bc.FILL_GROUPS)
    per_wave = {p[3589][0] for p in bc.FILL_PLANS.values()} | {p[1021][0] for p in bc.FILL_PLANS.values()}
    assert {1, bm.K_MAX_PER_WAVE} < per_wave and len(per_wave) > 3      # 1, intermediate values, 64
    assert any(p[17000][2] > 1 for p in bc.FILL_PLANS.values())         # slab reduce, several segments
    # mix_plan against hz_mixplan.h's own properties: no empty segment, n_pad covers n
    for groups in (1, 3, 32, 129):
        for n in (1, 1024, 1025, 3589, 17000, 2 ** 20):
            for tg in (1, 8, 256):
                p = bm.mix_plan(groups, n, bm.TILE, tg)
                assert p["n_pad"] >= n and (p["nseg"] - 1) * p["seg_tiles"] < p["ntiles"] <= p["nseg"] * p["seg_tiles"]


def test_hot_modes_are_the_plans_edges():
    seen = set()
    for (M, g) in bc.FILL_PLANS:
        for n in bc.PLAN_CALLS:
            p = bm.bowl_plan(M, n, g)
            pw, G = p["per_wave"], p["G"]
            hot = set(bm.hot_modes(M, n, g))
            assert hot <= set(bc.fill_hot(M, g)) and {0, M - 1} <= hot
            where = {i: bm.wave_of(p, i) for i in hot}
            # first and last mode of a wave, of a workgroup
            assert where[0] == (0, 0, 0)
            if M >= pw:
                assert where[pw - 1] == (0, 0, pw - 1)
            if M > bm.K_WAVES * pw:
                assert where[bm.K_WAVES * pw - 1] == (0, bm.K_WAVES - 1, pw - 1)
                assert where[bm.K_WAVES * pw] == (1, 0, 0)
            # the last wave: its first mode and the bank's last; count < per_wave when it is ragged
            lw = ((M - 1) // pw) * pw
            assert lw in hot and where[M - 1][:2] == where[lw][:2] and where[M - 1][0] == G - 1
            if M % pw:
                assert where[M - 1][2] == M % pw - 1 < pw - 1
                seen.add("ragged wave")
            if p["reduce"] == "short":
                unrolled, tail = bm.short_reduce_passes(G)
                assert sorted(unrolled + tail) == list(range(G))
                assert bool(unrolled) == (7 * bm.SHORT_SLICES < G)
                for name, groups in (("unrolled", unrolled), ("tail", tail)):
                    for gi in groups[:1] + groups[-1:]:
                        assert gi * bm.K_WAVES * pw in hot and min(M, (gi + 1) * bm.K_WAVES * pw) - 1 in hot
                        seen.add(name)
                if unrolled and tail:
                    seen.add("both passes")
            seen.add("per_wave %d" % min(pw, 2) if pw < bm.K_MAX_PER_WAVE else "per_wave 64")
    assert seen >= {"ragged wave", "unrolled", "tail", "both passes", "per_wave 1", "per_wave 2", "per_wave 64"}
    # the chain kernel: the four table entries of a thread, and the second pass of the mode loop
    slots = {i: bm.chain_slot(i) for i in bc.chain_hot(4100)}
    assert slots == {0: (0, 0, 0), 511: (0, 0, 511), 512: (0, 1, 0), 2047: (0, 3, 511), 2048: (1, 0, 0),
                     4099: (2, 0, 3)}
    assert {bm.chain_slot(M - 1)[:2] for M in bc.CHAIN_M} == {(0, 0), (0, 1), (0, 3), (1, 0), (2, 0)}


# ---- 5. mutants -------------------------------------------------------------------------------------

_bank = {}


def _c5():
    """the C5 bank from trigger(), 3589 samples: restatement mixdown, the model's float64 mode
    sum, and the weak modes the mutants touch"""
    if not _bank:
        M, n = 2048, 3589
        f, a, d = bc.c5_shape_model(M)
        o = OracleBowl(M, f, a, d, np.float32)
        o.trigger()
        total = np.zeros(n)
        for m0 in range(0, M, 256):
            total += bm.model_terms(f[m0:m0 + 256], a[m0:m0 + 256], d[m0:m0 + 256], 0, n, bm.K_L).sum(axis=0)
        weak = np.argsort(a)[:8]
        _bank.update(M=M, n=n, f=f, a=a, d=d, ref=o.fill(n), total=total, weak=weak)
        assert rel_err(total.astype(np.float32), _bank["ref"]) < NORTH_STAR
    return _bank


def _term(b, k, fk=None, **kw):
    return bm.model_terms([b["f"][k] if fk is None else fk], [b["a"][k]], [b["d"][k]], 0, b["n"], bm.K_L, **kw)[0]


def _old_and_new(b, k, mutated_term):
    """a wrong engine as the old and the new check see it: the C5 mixdown against the restatement
    (relative to the mix's peak), and mode k's one-hot bank against its single-mode restatement
    (relative to a_k)"""
    mix = (b["total"] - _term(b, k) + mutated_term).astype(np.float32)
    old = rel_err(mix, b["ref"])
    ref_k = ref_single((b["f"][k], b["a"][k], b["d"][k]), 0, [b["n"]])
    new = bm.per_mode_error(mutated_term.astype(np.float32), ref_k, b["a"][k])
    true = bm.per_mode_error(_term(b, k).astype(np.float32), ref_k, b["a"][k])
    assert true <= bm.PER_MODE
    return old, new


@pytest.mark.parametrize("kind", ["dropped", "swapped", "next_seed", "unrounded_product"])
def test_mutant_passes_mixdown_fails_per_mode(kind):
    b = _c5()
    k, k2 = int(b["weak"][0]), int(b["weak"][1])
    if kind == "dropped":            # the engine leaves mode k out
        old, new = _old_and_new(b, k, np.zeros(b["n"]))
    elif kind == "swapped":          # modes k and k2 read each other's frequency
        mix = b["total"] - _term(b, k) - _term(b, k2) + _term(b, k, fk=b["f"][k2]) + _term(b, k2, fk=b["f"][k])
        old = rel_err(mix.astype(np.float32), b["ref"])
        _, new = _old_and_new(b, k, _term(b, k, fk=b["f"][k2]))
    elif kind == "next_seed":        # mode k's decay seeded from the chunk after its own
        old, new = _old_and_new(b, k, _term(b, k, seed_shift=1))
    else:                            # mode k's phase from the exact product f n, rounded once
        k = int(max(b["weak"], key=lambda i: b["f"][i]))
        old, new = _old_and_new(b, k, _term(b, k, exact_product=True))
    print("mutant %s (mode %d, a = %.2e): mixdown %.3e (passes 1e-5), per mode %.3e a_i (bound 3e-7)"
          % (kind, k, b["a"][k], old, new))
    assert old < NORTH_STAR
    assert new > 10 * bm.PER_MODE
