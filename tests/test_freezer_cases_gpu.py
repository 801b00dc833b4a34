"""GPU: the Freezer HIP engine at the cases of tests/freezer_cases.py (every accepted frame size
from 4 to 8192, size < N, M = 3 and M = 42, events on every edge), against the restatement
(oracle/hz_oracle_frz.c) and against itself under every way of splitting a schedule into calls
and launches.  tests/test_freezer_cases_cpu.py shows that the cases are well-conditioned and reach
the branches they are named for.

Parity: dry samples bit for bit over the whole schedule; every frozen period within 1e-9 of that
period's own oracle peak (the project's Freezer bound, per period: a quiet period is not hidden by
a loud dry stretch); an all-zero oracle period is all zero on the device.  Splits: bit for bit.
Both sides draw the process's rand(): each run is seeded, and the runs never interleave.
"""
import functools

import numpy as np
import pytest

import freezer_cases as fc
from freezer_cases import F
from freezer_model import split_schedule
from oracle_frz import OracleFreezer, libc_srand

pytestmark = pytest.mark.gpu
TOL = 1e-9
BY_NAME = {c.name: c for c in fc.CASES + fc.CHUNK_CASES}
CHUNK_IDS = [c.name for c in fc.CHUNK_CASES]


@functools.lru_cache(maxsize=None)
def oracle_out(name):
    c = BY_NAME[name]
    libc_srand(c.seed)
    y = OracleFreezer(c.geom.N, c.geom.laps, c.geom.width).process(fc.noise(c), c.events)
    y.setflags(write=False)
    return y


def engine(c, blocks, api=False):
    """the case through a fresh engine, as the calls of `blocks`; api: events that open a call go
    through freeze() / unfreeze() before it"""
    from huygens_amd import Freezer
    g = Freezer(c.geom.N, c.geom.laps, c.geom.width)
    x, ys, pos = fc.noise(c), [], 0
    libc_srand(c.seed)
    for n, ev in blocks:
        if api:
            for t, k in ev:
                assert t == 0
                g.freeze() if k == F else g.unfreeze()
            ev = []
        ys.append(g.process(x[pos:pos + n], ev))
        pos += n
    g.close()
    return np.concatenate(ys)


@functools.lru_cache(maxsize=None)
def single_call(name):
    c = BY_NAME[name]
    y = engine(c, [(c.n, c.events)])
    y.setflags(write=False)
    return y


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def first_diff(a, b):
    d = np.flatnonzero(a.view(np.int64) != b.view(np.int64))
    return (int(d[0]), int(d.size)) if d.size else None


def check_parity(c, gy):
    """asserts the parity of one engine output; returns the largest per-period relative error"""
    oy = oracle_out(c.name)
    dry, periods = split_schedule(c.n, c.events)
    assert np.count_nonzero(oy[dry]) > 0
    assert np.array_equal(gy[dry], oy[dry]), ("dry path", c.name, first_diff(gy[dry], oy[dry]))
    worst = 0.0
    for a, b in periods:
        peak = np.max(np.abs(oy[a:b]))
        err = np.max(np.abs(gy[a:b] - oy[a:b]))
        if peak == 0.0:
            assert not np.any(gy[a:b]), ("zero period", c.name, a, b, err)
            continue
        worst = max(worst, err / peak)
        assert err <= TOL * peak, (c.name, a, b, err / peak)
    return worst


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_parity_per_period(gpu_lib, name):
    """the case as its own calls (events on its cuts arrive as at == n of the earlier call; the
    oracle's loop ends at n - 1, so it takes them as at == 0 of the later call: one schedule)"""
    c = BY_NAME[name]
    gy = engine(c, fc.blocks(c.n, c.events, c.cuts, c.at_n))
    worst = check_parity(c, gy)
    print(f"\nfreezer parity {name}: n {c.n}, largest per-period error {worst:.3e} of the period's peak")
    assert same_bits(gy, single_call(name)), first_diff(gy, single_call(name))


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_split_invariance(gpu_lib, name):
    """The engine is deterministic and a split changes neither a frame nor a summation order."""
    c = BY_NAME[name]
    ref = single_call(name)
    cuts = fc.event_cuts(c.n, c.events)
    # a. calls cut at every event and one sample either side (1-sample calls), events as at == 0
    y = engine(c, fc.blocks(c.n, c.events, cuts))
    assert same_bits(y, ref), ("cut at events", first_diff(y, ref))
    # b. the same calls, every event that sits on a cut as at == n of the earlier call
    y = engine(c, fc.blocks(c.n, c.events, cuts, cuts))
    assert same_bits(y, ref), ("at == n", first_diff(y, ref))
    # c. calls cut at the events, which go through freeze() / unfreeze() between them
    y = engine(c, fc.blocks(c.n, c.events, [t for t, _ in c.events]), api=True)
    assert same_bits(y, ref), ("freeze() / unfreeze()", first_diff(y, ref))


@pytest.mark.parametrize("name", CHUNK_IDS)
def test_chunk_split_invariance(gpu_lib, monkeypatch, name):
    """d. launches of 4096 samples (HZ_FRZ_CHUNK, read at create) against one launch, with chunk
    boundaries on a populate sample, on and beside events and inside a period opened two chunks
    earlier (freezer_cases.chunk_schedule); at N = 8192 the chunk is shorter than a frame"""
    c = BY_NAME[name]
    ref = single_call(name)
    worst = check_parity(c, ref)
    print(f"\nfreezer parity {name}: n {c.n}, largest per-period error {worst:.3e} of the period's peak")
    monkeypatch.setenv("HZ_FRZ_CHUNK", str(fc.CHUNK))
    y = engine(c, [(c.n, c.events)])
    assert same_bits(y, ref), ("chunks of 4096", first_diff(y, ref))
    # and the chunked engine over calls that are no multiple of the chunk
    y = engine(c, fc.blocks(c.n, c.events, [fc.CHUNK + 1, 3 * fc.CHUNK - 1, 6 * fc.CHUNK]))
    assert same_bits(y, ref), ("chunks of 4096 within calls", first_diff(y, ref))


def test_device_pointers_chunked(gpu_lib, monkeypatch):
    import torch
    from huygens_amd import Freezer
    c = BY_NAME["chunk-2048-8"]
    ref = single_call(c.name)
    monkeypatch.setenv("HZ_FRZ_CHUNK", str(fc.CHUNK))
    g = Freezer(c.geom.N, c.geom.laps, c.geom.width)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        xt = torch.from_numpy(fc.noise(c)).cuda()
        yt = torch.empty_like(xt)
        g.set_stream(stream.cuda_stream)
        libc_srand(c.seed)
        g.process_device(xt.data_ptr(), yt.data_ptr(), c.n, c.events)
    stream.synchronize()
    y = yt.cpu().numpy()
    g.close()
    assert same_bits(y, ref), first_diff(y, ref)


@pytest.mark.parametrize("N,laps,width", [
    (2, 2, 1.0),          # below the smallest frame
    (16384, 8, 1.0),      # above kMaxN
    (100, 4, 1.0),        # no power of two
    (64, 65, 1.0),        # laps > N: stride 0
    (8192, 4096, 1.5),    # M = 6145 > 4096
])
def test_creation_errors(gpu_lib, N, laps, width):
    from huygens_amd import Freezer, HZError
    with pytest.raises(HZError):
        Freezer(N, laps, width)


@pytest.mark.parametrize("geo", fc.GEOMETRIES + fc.CHUNK_GEOMETRIES)
def test_info_is_the_oracles_geometry(gpu_lib, geo):
    from huygens_amd import Freezer
    g, o = Freezer(*geo), OracleFreezer(*geo)
    assert g.info() == (o.stride, o.M, False)
    g.freeze()
    assert g.info() == (o.stride, o.M, True)
    g.close()
