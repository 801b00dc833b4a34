"""CPU: the arithmetic of hz_dly_process_tv (tests/delay_tv_model.py) against the per-sample oracle
-- modulate_forward/back on every tap, then one sample -- bit for bit in both dtypes, and the new
entry points in the C ABI."""
import os
import subprocess

import numpy as np
import pytest

from delay_tv_model import (CALLS, LINES, SPARSITY, TIME, DelayTvModel, make_streams, max_time, oracle_tv, rem,
                            scenario, scenario_reference, slot_age)
from oracle_delay import OracleDelaybank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float64, np.float32]


def test_reciprocal_remainder_is_exact():
    """tv_rem(w, size) == w % size: every w near a multiple of size, the ends of the 32-bit range and
    random w, for ring sizes 1, 2, the tests' and the largest (2^31 - 1)."""
    rng = np.random.default_rng(1)
    for size in (1, 2, 3, 97, 3001, 5001, 48001, 96001, 2 ** 24 + 1, 2 ** 31 - 2, 2 ** 31 - 1):
        q = rng.integers(0, 2 ** 32 // size + 1, 2000)
        near = (q[:, None] * size + np.arange(-2, 3)[None, :]).reshape(-1)
        w = np.concatenate([near[(near >= 0) & (near < 2 ** 32)], rng.integers(0, 2 ** 32, 5000),
                            [0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]]).astype(np.uint64)
        assert np.array_equal(rem(w, size), (w % np.uint64(size)).astype(np.int64)), size


@pytest.mark.parametrize("dtype", DTYPES)
def test_slot_index_wraps_as_uint32(dtype):
    """A time beyond the ring wraps mod 2^32 before `% size`: not (o - c) mod size."""
    idx, age = slot_age(np.array([250], dtype=np.uint32), np.array([10]), 100, dtype)
    assert idx[0] == (10 - 250 + 100 + 2 ** 32) % 100 and age[0] == 54   # test_delay_cpu.py's case
    t = max_time(dtype)
    idx, age = slot_age(np.array([t], dtype=np.uint32), np.array([3]), 97, dtype)
    assert idx[0] == ((3 - t + 97) % 2 ** 32) % 97


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_equals_per_sample_oracle(dtype):
    """N = 3, S = 2, ring 97; calls of 1, 127, 1, 171, 300, mono and per-line input in turn; times
    beyond the ring, the largest legal time, zero-time and age-0 feedback.  Outputs and origin equal
    the oracle's; Lc is 5 on the long calls; the model asserts no read inside its own sub-block."""
    name = np.dtype(dtype).name
    want, origins = scenario_reference(name)
    m = DelayTvModel(LINES, SPARSITY, TIME, dtype)
    for k, c in enumerate(scenario(name)):
        y = m.process_tv(*c)
        assert np.all(np.isfinite(want[k])) and np.max(np.abs(want[k])) < 5
        assert np.array_equal(y, want[k]), (k, CALLS[k])
        assert m.origin() == origins[k]
        if CALLS[k] > 100:
            assert m.last_Lc == 5
    bt = np.concatenate([c[3] for c in scenario(name)], axis=-1)
    assert (bt == 0).any() and (bt == TIME + 1).any()   # zero-time and age-0 feedback were in it


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_pieces_null_back_and_handover(dtype):
    """One call equals the same stream in pieces; null back streams keep the staged feedback taps;
    the staged taps after a call are its last row (a zero-time back tap staged as {0, 0})."""
    rng = np.random.default_rng(5)
    n = 300
    x = rng.uniform(-0.5, 0.5, n).astype(dtype)
    ft, fg, bt, bg = make_streams(rng, n, dtype)
    bt[:, :, -1] = [[0, 9], [17, 0], [6, 98]]
    one, cut = DelayTvModel(LINES, SPARSITY, TIME, dtype), DelayTvModel(LINES, SPARSITY, TIME, dtype)
    o = OracleDelaybank(LINES, SPARSITY, TIME, dtype)
    y = one.process_tv(x, ft, fg, bt, bg)
    assert np.array_equal(y, oracle_tv(o, x, ft, fg, bt, bg))
    parts, a = [], 0
    for p in (1, 127, 1, 171):
        parts.append(cut.process_tv(x[a:a + p], ft[..., a:a + p], fg[..., a:a + p], bt[..., a:a + p], bg[..., a:a + p]))
        a += p
    assert np.array_equal(np.concatenate(parts, axis=-1), y)
    assert np.array_equal(cut.rx, one.rx) and np.array_equal(cut.ry, one.ry) and cut.origin() == one.origin()
    # forward-only call: the oracle keeps the feedback taps of the last row
    x2 = rng.uniform(-0.5, 0.5, (LINES, 150)).astype(dtype)
    ft2, fg2, _, _ = make_streams(rng, 150, dtype)
    assert np.array_equal(one.process_tv(x2, ft2, fg2), oracle_tv(o, x2, ft2, fg2))
    assert np.array_equal(one.bt, bt[:, :, -1]) and np.all(one.bg[one.bt == 0] == 0)


def test_abi_has_the_stream_entries():
    from huygens_amd import header_symbols, load
    from huygens_amd._lib import _SIGS
    names = ["hz_dly_process_tv", "hz_dly_process_tv_device"]
    assert not [s for s in names if s not in header_symbols()]
    assert not [s for s in names if s not in _SIGS]
    so = os.path.join(ROOT, "huygens_amd", "lib", "libhuygens_hip.so")
    if not os.path.exists(so):
        subprocess.run(["make", "-s", "-j8", "-C", ROOT, "lib"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", load()._name], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [s for s in names if s not in exported]
