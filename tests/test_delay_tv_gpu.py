"""GPU: Delaybank.process_tv (hz_dly_process_tv: a {time, gain} for every tap at every sample)
against the per-sample oracle -- modulate_forward/back on every tap, then one sample -- BIT-EXACT
(np.array_equal), in both dtypes and both launch modes."""
import numpy as np
import pytest

from delay_tv_model import (CALLS, LINES, SPARSITY, TIME, make_streams, oracle_tv, scenario, scenario_reference)
from oracle_delay import OracleDelaybank

pytestmark = pytest.mark.gpu
DTYPES = [np.float64, np.float32]


def _bank(dtype, split=0, lines=LINES, S=SPARSITY, time=TIME):
    from huygens_amd import Delaybank
    b = Delaybank(lines, S, time, dtype)
    b.set_split(split)
    return b


def _cut(arrays, a, b):
    return [None if v is None else v[..., a:b] for v in arrays]


@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_oracle_parity(gpu_lib, dtype, split):
    """The CPU test's scenario: ring 97, calls of 1, 127, 1, 171, 300, times beyond the ring, the
    largest legal time, zero-time and age-0 feedback; serial sub-blocks of 5 on the long calls."""
    name = np.dtype(dtype).name
    want, origins = scenario_reference(name)
    g = _bank(dtype, split)
    for k, c in enumerate(scenario(name)):
        assert np.array_equal(g.process_tv(*c), want[k]), (k, CALLS[k])
        assert g.origin() == origins[k]


@pytest.mark.parametrize("dtype", DTYPES)
def test_pieces_equal_one_call(gpu_lib, dtype):
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.5, 0.5, (LINES, 300)).astype(dtype)
    s = make_streams(rng, 300, dtype)
    one, cut = _bank(dtype), _bank(dtype)
    y = one.process_tv(x, *s)
    parts, a = [], 0
    for p in (1, 127, 1, 171):
        parts.append(cut.process_tv(x[:, a:a + p], *_cut(s, a, a + p)))
        a += p
    assert np.array_equal(np.concatenate(parts, axis=-1), y)
    assert cut.origin() == one.origin()
    x2 = rng.uniform(-0.5, 0.5, 200).astype(dtype)   # the rings and the staged taps are equal too
    assert np.array_equal(cut.process(x2), one.process(x2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_stream_equals_process(gpu_lib, dtype):
    """A stream that repeats the static taps (test_streamed_mix_calls' bank: N = 70, S = 3, time 3000,
    one age-0 feedback tap, mixed output) equals process() on a twin bank."""
    rng = np.random.default_rng(11)
    N, S, time = 70, 3, 3000
    g, twin = _bank(dtype, 0, N, S, time), _bank(dtype, 0, N, S, time)
    ft, bt = np.zeros((N, S), dtype=np.uint32), np.zeros((N, S), dtype=np.uint32)
    fg, bg = np.zeros((N, S), dtype=dtype), np.zeros((N, S), dtype=dtype)
    for k in range(N):
        fwd = [(int(rng.integers(0, 1800)), float(rng.uniform(-1, 1))) for _ in range(S)]
        back = [(int(rng.integers(1100, 1900)), float(rng.uniform(-0.3, 0.3))) for _ in range(S - 1)]
        if k == 5:
            back[1] = (time + 1, 0.25)   # age 0: reads the sample's own partial sum
        twin.coefficients(k, fwd, back)
        ft[k], fg[k] = [t for t, _ in fwd], [v for _, v in fwd]
        bt[k, :S - 1], bg[k, :S - 1] = [t for t, _ in back], [v for _, v in back]
    for i, n in enumerate([1024, 1000, 1, 2500]):
        x = rng.standard_normal((N, n) if i % 3 == 2 else n).astype(dtype)
        rep = [np.repeat(a[:, :, None], n, axis=2) for a in (ft, fg, bt, bg)]
        assert np.array_equal(g.process_tv(x, *rep, mix=True), twin.process(x, mix=True)), (i, n)
    assert g.origin() == twin.origin()


@pytest.mark.parametrize("device_entry", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_handover_to_process_and_sample(gpu_lib, dtype, device_entry):
    """After process_tv the staged taps are the stream's last row: process() and sample() continue
    as the oracle does after the loop's last modulate_* (host entry and device entry)."""
    import torch
    rng = np.random.default_rng(33)
    n = 200
    x = rng.uniform(-0.5, 0.5, (LINES, n)).astype(dtype)
    ft, fg, bt, bg = make_streams(rng, n, dtype)
    bt[:, :, -1] = [[0, 9], [17, 0], [6, TIME + 1]]   # zero-time ({0, 0}) and age-0 taps staged
    g, o = _bank(dtype), OracleDelaybank(LINES, SPARSITY, TIME, dtype)
    want = oracle_tv(o, x, ft, fg, bt, bg)
    if device_entry:
        d = [torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else a.dtype)).cuda()
             for a in (x, ft, fg, bt, bg)]
        yt = torch.empty_like(d[0])
        g.process_tv_device(d[0].data_ptr(), yt.data_ptr(), n, *[a.data_ptr() for a in d[1:]], per_line=True)
        g.synchronize()
        y = yt.cpu().numpy()
    else:
        y = g.process_tv(x, ft, fg, bt, bg)
    assert np.array_equal(y, want)
    x2 = rng.uniform(-0.5, 0.5, 150).astype(dtype)
    assert np.array_equal(g.process(x2), o.process(x2))
    for v in rng.uniform(-0.5, 0.5, 3).astype(dtype):
        assert np.array_equal(g.sample(v), o.process(np.array([v], dtype=dtype))[:, 0])
    ft3, fg3, bt3, bg3 = make_streams(rng, 60, dtype)   # and a stream call after them
    x3 = rng.uniform(-0.5, 0.5, 60).astype(dtype)
    assert np.array_equal(g.process_tv(x3, ft3, fg3, bt3, bg3), oracle_tv(o, x3, ft3, fg3, bt3, bg3))
    assert g.origin() == o.origin()


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_null_back_streams_keep_static_feedback(gpu_lib, dtype, split):
    rng = np.random.default_rng(44)
    g, o = _bank(dtype, split), OracleDelaybank(LINES, SPARSITY, TIME, dtype)
    for k in range(LINES):
        for b in (g, o):
            b.coefficients(k, [(0, 1.0)], [(7 + k, 0.3), (TIME + 1 if k == 1 else 30, -0.2)])
    for n in (140, 1, 90):
        x = rng.uniform(-0.5, 0.5, n).astype(dtype)
        ft, fg, _, _ = make_streams(rng, n, dtype)
        assert np.array_equal(g.process_tv(x, ft, fg), oracle_tv(o, x, ft, fg))
    x = rng.uniform(-0.5, 0.5, 120).astype(dtype)   # the feedback taps are still staged
    assert np.array_equal(g.process(x), o.process(x))
    assert g.origin() == o.origin()


@pytest.mark.parametrize("split", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_batched_instance(gpu_lib, dtype, split):
    """Forward only, N = 2, S = 1, time 5000, n = 9001 in one call: no live feedback, so one sub-block
    of 9001 -- with one workgroup per line (split 1) the widest samples-per-thread instance and its
    ragged tail; split 2 cuts it over several workgroups.  No recurrence: each output is one product."""
    rng = np.random.default_rng(55)
    N, time, n = 2, 5000, 9001
    g = _bank(dtype, split, N, 1, time)
    x = rng.uniform(-1, 1, (N, n)).astype(dtype)
    ft = rng.integers(0, 3 * (time + 1), (N, 1, n)).astype(np.uint32)
    fg = rng.uniform(-1, 1, (N, 1, n)).astype(dtype)
    o = OracleDelaybank(N, 1, time, dtype)
    assert np.array_equal(g.process_tv(x, ft, fg), oracle_tv(o, x, ft, fg))
    assert g.origin() == o.origin()


def test_errors_change_nothing(gpu_lib):
    from huygens_amd import HZError
    rng = np.random.default_rng(66)
    g, o = _bank(np.float64), OracleDelaybank(LINES, SPARSITY, TIME, np.float64)
    for k in range(LINES):
        for b in (g, o):
            b.coefficients(k, [(3, 1.0), (50, 0.5)], [(20 + k, 0.3)])
    x = rng.uniform(-0.5, 0.5, 100)
    assert np.array_equal(g.process(x), o.process(x))
    ft, fg, bt, bg = make_streams(rng, 100, np.float64)
    bad = ft.copy()
    bad[1, 1, 57] = 2 ** 31
    with pytest.raises(HZError):
        g.process_tv(x, bad, fg, bt, bg)
    with pytest.raises(HZError):   # one back stream without the other
        g.process_tv(x, ft, fg, bt, None)
    with pytest.raises(HZError):
        g.process_tv(x, ft, fg, None, bg)
    with pytest.raises(ValueError):
        g.process_tv(x, ft[:, :, :99], fg, bt, bg)
    with pytest.raises(ValueError):
        g.process_tv(x, ft, fg[:, :1], bt, bg)
    with pytest.raises(ValueError):
        g.process_tv(x, ft, fg, bt[:2], bg)
    assert g.origin() == o.origin()
    x = rng.uniform(-0.5, 0.5, 250)   # nothing was committed: rings, origin and taps as before
    assert np.array_equal(g.process(x), o.process(x))
    assert g.process_tv(np.zeros(0), ft[:, :, :0], fg[:, :, :0]).shape == (LINES, 0)   # n == 0
    assert np.array_equal(g.process(x), o.process(x))


def test_float_time_limit(gpu_lib):
    """float: the stream's limit is set_tap's, 2147483520 = 2^31 - 128, the largest float below 2^31."""
    from huygens_amd import HZError
    rng = np.random.default_rng(77)
    g, o = _bank(np.float32), OracleDelaybank(LINES, SPARSITY, TIME, np.float32)
    x = rng.uniform(-0.5, 0.5, 64).astype(np.float32)
    ft, fg, bt, bg = make_streams(rng, 64, np.float32)
    bad = ft.copy()
    bad[0, 0, 63] = 2147483521
    with pytest.raises(HZError):
        g.process_tv(x, bad, fg, bt, bg)
    ft[0, 0, 63] = 2147483520
    assert np.array_equal(g.process_tv(x, ft, fg, bt, bg), oracle_tv(o, x, ft, fg, bt, bg))
