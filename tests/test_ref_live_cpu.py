"""The C oracle against the live reference binary (CPU): seeded random cases.

Where oracle/_ref/hz_ref_dump exists (`make -C oracle` builds it wherever the reference's sources
are), twenty random cases per class, drawn in the ranges of the pinned table
(tests/golden/make_golden_ref.py), go through the reference's own classes in a child process and
through the oracle's bindings.  Same rule as tests/test_ref_pinned_cpu.py: bit equality, which
holds for every class.  Skips only when the binary is absent (a machine without the reference).
"""
import numpy as np
import pytest

import ref_driver as R

pytestmark = pytest.mark.skipif(not R.available(), reason="oracle/_ref/hz_ref_dump not built (no reference sources)")

CLASSES = ("oscillator", "synth", "sinusoids", "additive", "delay", "bowl", "granulator")
CASES = 20


@pytest.mark.parametrize("cls", CLASSES)
def test_random_cases(cls):
    worst = 0.0
    for seed in range(CASES):
        case = R.random_case(cls, np.random.default_rng([CLASSES.index(cls), seed]))
        ref, got = R.reference(case), R.oracle_outputs(case)
        assert ref.keys() == got.keys()
        for key in ref:
            assert ref[key].size
            worst = max(worst, R.max_abs_diff(got[key], ref[key]))
            assert R.bit_equal(got[key], ref[key]), (cls, seed, key, R.max_abs_diff(got[key], ref[key]))
    print(f"{cls}: {CASES} cases, max |oracle - reference| = {worst:.3e}")


def test_random_scalars_and_waves():
    rng = np.random.default_rng(99)
    case = dict(cls="scalars", relaxation_x=np.append(10.0 ** rng.uniform(-6, 1, 19), 0.0),
                mtof_x=rng.uniform(-20, 140, 20), ftom_x=10.0 ** rng.uniform(0, 4.3, 20), dbtoa_x=rng.uniform(-120, 24, 20))
    ref, got = R.reference(case), R.oracle_outputs(case)
    for key in ref:
        assert R.bit_equal(got[key], ref[key]), key
    case = dict(cls="wave", phase=np.concatenate([rng.uniform(-3, 3, 40), rng.uniform(-100, 100, 20), [0.5, 0.0, 1.0]]))
    assert R.bit_equal(R.oracle_outputs(case)["y"], R.reference(case)["y"])
