"""CPU: the Freezer restatement (oracle/hz_oracle_frz.c) against closed forms and an
independent numpy restatement of src/fourier.h:236-562 (FFrame, IFrame, DFrame, Freezer).

Parity status: the reference holds no fixtures for Freezer; these checks pin the
restatement (the dry Delay path exactly, the frozen path against a second model to 1e-12)."""
import numpy as np
import pytest

from freezer_model import PyFreezer
from huygens_amd._lib import header_symbols
from oracle_frz import OracleFreezer, libc_srand


def test_dry_path_is_an_n_sample_delay():
    o = OracleFreezer(64, 4, 1.0)
    x = np.random.default_rng(0).standard_normal(500)
    assert np.array_equal(o.process(x), np.r_[np.zeros(64), x[:-64]])


def test_dry_path_after_a_freeze_reads_the_stale_ring():
    """While frozen the Delay's input ring is not written (fourier.h:528-533), only ticked."""
    N = 16
    o = OracleFreezer(N, 2, 1.0)
    x = np.arange(1, 301, dtype=float)
    libc_srand(3)
    y = o.process(x, [(100, 1), (130, 0)])
    unfrozen = np.ones(300, bool)
    unfrozen[100:130] = False
    for t in range(130, 180):   # closed form of the ring read (t + 1) mod (N + 1)
        tau = t - N
        while tau >= 0 and not unfrozen[tau]:
            tau -= N + 1
        assert y[t] == (x[tau] if tau >= 0 else 0.0)


@pytest.mark.parametrize("N,laps,width,seed", [(8, 2, 1.0, 1), (16, 4, 1.0, 2), (32, 3, 2.5, 3), (16, 2, 3.0, 4)])
def test_restatement_vs_numpy(N, laps, width, seed):
    rng = np.random.default_rng(seed)
    n = 900
    x = rng.standard_normal(n)
    events = [(37, 1), (150, 1), (211, 0), (212, 0), (400, 1), (777, 0), (778, 1)]
    o, p = OracleFreezer(N, laps, width), PyFreezer(N, laps, width)
    libc_srand(seed)
    yo = o.process(x, events)
    libc_srand(seed)
    yp = p.process(x, events)
    assert np.max(np.abs(yo - yp)) <= 1e-12 * max(1.0, np.max(np.abs(yp)))


def test_abi_declares_freezer():
    syms = header_symbols()
    for s in ("hz_frz_create", "hz_frz_process", "hz_frz_process_device", "hz_frz_freeze", "hz_frz_unfreeze"):
        assert s in syms
