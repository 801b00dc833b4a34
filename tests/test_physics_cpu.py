"""CPU: the Minimizer::physics() restatement (tests/oracle_phys.py) against what the reference
itself computed (tests/golden/physics_ref.npz, made by make_golden_physics.py), and the parts of
the physics ABI that need no device."""
import os
import subprocess

import numpy as np
import pytest

from oracle_phys import GRAV_FABS, GRAV_TRUNC, SCENARIOS, PhysAdditive, run_scenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "physics_ref.npz")


@pytest.fixture(scope="module")
def runs():
    """Every scenario under both laws, computed once: name -> {law: (audio, track)}"""
    return {name: {law: run_scenario(sc, law)[:2] for law in (GRAV_TRUNC, GRAV_FABS)} for name, sc in SCENARIOS.items()}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trunc_restatement_equals_reference_bit_for_bit(name, runs):
    g = np.load(GOLD)
    assert str(g["made_by"]) == "reference"
    audio, track = runs[name][GRAV_TRUNC]
    ref = g[name + "_track"]
    assert track.shape == ref.shape
    assert np.array_equal(track.view(np.uint64), ref.view(np.uint64))
    assert np.array_equal(audio, g[name + "_audio"])


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_particles_move_and_laws_differ(name, runs):
    sc = SCENARIOS[name]
    start = PhysAdditive(sc["V"], sc["O"], sc["decay"], sc["harm"], sc["k"], law=GRAV_TRUNC)
    for t, kind, a, b in sc["events"]:
        if t == 0:
            start.makenote(a, b)
    _, trunc = runs[name][GRAV_TRUNC]
    _, fabs = runs[name][GRAV_FABS]
    # frozen positions cannot pass: within 40 steps (before any later note) the partials travel > 0.05 semitone
    assert np.abs(trunc[:40] - start.positions()).max() > 0.05
    assert not np.array_equal(trunc, fabs)
    assert np.abs(trunc - fabs).max() > 1e-3


def test_schedule_rule():
    """T >= p && T % p == 0: period 2 steps at samples 2, 4, ...; period 3 at 3, 6, ...; period 1 at 1, 2, ..."""
    for p, n, want in ((2, 512, 255), (3, 128, 42), (1, 16, 15)):
        assert sum(1 for T in range(n) if T >= p and T % p == 0) == want
    assert np.load(GOLD)["v3o4_track"].shape[0] == 255
    assert np.load(GOLD)["p3_track"].shape[0] == 42


def test_law_is_required():
    with pytest.raises(TypeError):
        PhysAdditive(2, 3, 0.75)
    with pytest.raises(ValueError):
        PhysAdditive(2, 3, 0.75, law=0)


@pytest.fixture(scope="module")
def lib():
    so = os.path.join(ROOT, "huygens_amd", "lib", "libhuygens_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-j8", "-C", ROOT, "lib"], check=True)
    from huygens_amd import load
    return load()


def test_physics_abi_rejects_without_device(lib):
    from huygens_amd._lib import HZ_E_INVALID, HZ_GRAV_FABS, HZ_GRAV_TRUNC
    assert (HZ_GRAV_TRUNC, HZ_GRAV_FABS) == (GRAV_TRUNC, GRAV_FABS)
    assert lib.hz_add_physics_every(None, 2, 0) == HZ_E_INVALID      # no default law
    assert lib.hz_add_physics_every(None, 2, 7) == HZ_E_INVALID
    assert lib.hz_add_physics_every(None, 2, HZ_GRAV_TRUNC) == HZ_E_INVALID   # null handle
    assert lib.hz_add_physics(None, 0) == HZ_E_INVALID
    assert lib.hz_add_tune_physics(None, 0, 0) == HZ_E_INVALID


def test_python_exports():
    import huygens_amd
    assert huygens_amd.GRAV_TRUNC == 1 and huygens_amd.GRAV_FABS == 2
    assert "GRAV_TRUNC" in huygens_amd.__all__ and "GRAV_FABS" in huygens_amd.__all__
    for m in ("physics_every", "physics", "peek", "positions", "tune_physics"):
        assert callable(getattr(huygens_amd.Additive, m))


SNIPPET = r"""
#include "soundmath/additive.h"
using namespace soundmath;
double port(Additive<double>& addi, int n) {
    addi.enable_physics(HZ_GRAV_TRUNC);
    double s = 0;
    for (int t = 0; t < n; t++) {
        s += addi();
        if (t >= 2 && t % 2 == 0) addi.physics();
        addi.tick();
    }
    addi.physics_every(2, HZ_GRAV_FABS);
    return s;
}
int main() { return 0; }
"""


def test_additive_header_compiles_with_physics(tmp_path):
    src = tmp_path / "phys.cpp"
    src.write_text(SNIPPET)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning" not in r.stderr, r.stderr[-2000:]
    hdr = open(os.path.join(ROOT, "include", "soundmath", "additive.h")).read()
    assert "std::logic_error" in hdr and "enable_physics(law) first" in hdr
