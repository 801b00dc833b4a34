"""What every handle does with its stream, its profile timers and its memory over its life --
the part of the C ABI that the parity tests do not touch.  For each Python engine class, at the
smallest shapes its own GPU tests use:

(a) rebinding the stream (default -> a fresh torch stream -> set_stream(0)) between blocks
    changes no bit of the output against one uninterrupted handle;
(b) Filterbank: set_stream(0) leaves a private (non-null) stream, set_stream(s) binds s;
(c) profile(True), two identical calls, profile_read() twice, profile(False), one call,
    profile_read(): the launch (and sample) counts of the three reads are the literals in
    PROFILE_COUNTS.  They were recorded from this file run against the library as it was before
    hz_stream.h existed (every engine managing its stream and timing events by hand), so they pin
    each engine's behaviour as it was, including which profile_read resets its counters
    (gran, het, stft, dly: second read 0) and which does not;
(d) 20 create / rebind / destroy cycles return HZ_OK throughout and leave the device's free
    memory (hipMemGetInfo, through torch.cuda.mem_get_info: the library allocates through HIP
    itself, torch's allocator is not involved) where it was, within 2 x GRANULE.

No case provokes an error on the device."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
B = 256   # samples per block


def _x(i, shape=(B,)):
    return np.random.default_rng(100 + i).standard_normal(shape)


class Engine:
    """make() -> a configured handle; step(h, i) -> block i's output; destroy: the C symbol."""

    def __init__(self, make, step, destroy, counts=None):
        self.make, self.step, self.destroy, self.counts = make, step, destroy, counts


def _fb():
    from huygens_amd import Filterbank
    fb = Filterbank(2, 4)
    for n in range(4):
        fb.coefficients(n, [1.0, 0.0, -1.0], [0.2 + 0.05 * n, -0.1])
    fb.boost(np.ones(4))
    fb.open()
    return fb


def _osc():
    from huygens_amd import Oscbank
    b = Oscbank(8)
    for i in range(8):
        b.freqmod(i, 110.0 * (i + 1))
    b.activate(np.arange(8))
    return b


def _add(physics=False):
    from huygens_amd import GRAV_TRUNC, Additive
    a = Additive(2, 3, 0.75)
    if physics:
        a.physics_every(64, GRAV_TRUNC)
    a.makenote(60, 1.0)
    a.makenote(64, 0.5)
    return a


def _sin():
    from huygens_amd import Sinusoids
    return Sinusoids(220.0, 4, 0.75)


def _sub():
    from huygens_amd import Subtractive
    s = Subtractive(2, 3, 0.75)
    s.makenote(60, 1.0)
    s.makenote(67, 0.5)
    return s


def _bowl():
    from huygens_amd import Bowl
    b = Bowl(3, [440.0, 660.0, 1234.5], [0.3, 0.2, 0.1], [1.0, 3.0, 0.5])
    b.trigger()
    return b


def _dly():
    from huygens_amd import Delaybank
    b = Delaybank(2, 2, 64)
    for k in range(2):
        b.coefficients(k, [(0, 1.0)], [(5 + k, 0.5), (20, 0.25)])
    return b


def _stft():
    from huygens_amd import Fourier
    return Fourier(0, 64, 2)


def _dct():
    from huygens_amd import Cosine
    return Cosine(64)


def _gran():
    from huygens_amd import Granulator
    return Granulator(100, 2)


def _frz():
    from huygens_amd import Freezer
    return Freezer(64, 4)


def _het():
    from huygens_amd import Heterodyne
    radii = np.zeros(8)
    radii[0::2] = [0.95, 0.96, 0.97, 0.98]
    g = Heterodyne(4, 2, radii)
    g.freqmod(0, np.arange(4), [100.0, 200.0, 300.0, 400.0])
    g.freqmod(1, np.arange(4), [-200.0, -400.0, -600.0, -800.0])
    g.open(0)
    g.open(1)
    return g


def _dct_step(c, i):
    c.inp[:] = _x(i, (64,))
    c.forward()
    return np.array(c.out)


# PROFILE_COUNTS: per engine, profile_read()[k:] (everything after the times) of the three reads
ENGINES = {
    "filterbank": Engine(_fb, lambda h, i: h.process(_x(i)), "hz_fb_destroy", (3, [(2,), (2,), (0,)])),
    "oscbank": Engine(_osc, lambda h, i: h.fill(B), "hz_osc_destroy", (1, [(2,), (2,), (0,)])),
    "additive": Engine(_add, lambda h, i: h.fill(B), "hz_add_destroy", (1, [(2,), (2,), (0,)])),
    # (the physics path has its own timers, hz_add_physics_profile_read, and counts no launches)
    "additive_physics": Engine(lambda: _add(True), lambda h, i: h.fill(B), "hz_add_destroy", (1, [(0,), (0,), (0,)])),
    "sinusoids": Engine(_sin, lambda h, i: h.fill(B), "hz_sin_destroy"),
    "subtractive": Engine(_sub, lambda h, i: h.process(0.1 * _x(i, (2, B))), "hz_sub_destroy", (4, [(), (), ()])),
    "bowl": Engine(_bowl, lambda h, i: h.fill(B), "hz_bowl_destroy", (1, [(2,), (2,), (0,)])),
    "delaybank": Engine(_dly, lambda h, i: h.process(_x(i)), "hz_dly_destroy", (1, [(2,), (0,), (0,)])),
    "fourier": Engine(_stft, lambda h, i: np.concatenate(h.process_block(_x(i), _x(i + 50))), "hz_stft_destroy",
                      (2, [(2,), (0,), (0,)])),
    "cosine": Engine(_dct, _dct_step, "hz_dct_destroy"),
    "granulator": Engine(_gran, lambda h, i: h.process(_x(i), [(10, 0.0005, 0.001, 1.0, 0.5, 0.0)])[0],
                         "hz_gran_destroy", (1, [(2, 96), (0, 0), (0, 0)])),
    "freezer": Engine(_frz, lambda h, i: h.process(_x(i)), "hz_frz_destroy", (1, [(2,), (2,), (0,)])),
    "heterodyne": Engine(_het, lambda h, i: h.process(0.2 * _x(i)), "hz_het_destroy",
                         (1, [(2, 2 * B * 4), (0, 0), (0, 0)])),
}
REBINDABLE = [k for k in ENGINES if k not in ("sinusoids", "cosine")]
PROFILED = [k for k, e in ENGINES.items() if e.counts is not None]

# The HIP runtime's device heap moves in granules of 2 MiB: on the library as it was before
# hz_stream.h, a first create / destroy cycle of an engine above changed the free device memory by
# 0 or 2097152 bytes (what the runtime keeps for itself after first use), and 20 further cycles by 0.
# The test allows 2 granules: the runtime caches freed granules.
GRANULE = 2 << 20


@pytest.fixture(scope="module")
def uninterrupted():
    """name -> the three blocks of one handle left alone (computed once per engine)"""
    cache = {}

    def get(name):
        if name not in cache:
            e = ENGINES[name]
            h = e.make()
            cache[name] = np.concatenate([np.ravel(e.step(h, i)) for i in range(3)])
            h.close()
        return cache[name]
    return get


@pytest.mark.parametrize("name", REBINDABLE)
def test_rebind_keeps_every_bit(gpu_lib, uninterrupted, name):
    import torch
    e = ENGINES[name]
    h = e.make()
    s = torch.cuda.Stream()
    blocks = [np.ravel(e.step(h, 0))]
    torch.cuda.synchronize()
    h.set_stream(s.cuda_stream)
    blocks.append(np.ravel(e.step(h, 1)))
    torch.cuda.synchronize()
    h.set_stream(0)
    blocks.append(np.ravel(e.step(h, 2)))
    torch.cuda.synchronize()
    got, ref = np.concatenate(blocks), uninterrupted(name)
    h.close()
    assert np.abs(ref).max() > 0
    assert np.array_equal(got, ref), np.flatnonzero(got != ref)[:8]


def test_filterbank_stream_after_rebind(gpu_lib):
    import torch
    fb = _fb()
    assert fb.stream() != 0   # created with a private stream
    s = torch.cuda.Stream()
    fb.set_stream(s.cuda_stream)
    assert fb.stream() == s.cuda_stream
    fb.set_stream(0)
    assert fb.stream() != 0 and fb.stream() != s.cuda_stream   # null: back to a private stream
    fb.close()


@pytest.mark.parametrize("name", PROFILED)
def test_profile_counts(gpu_lib, name):
    e = ENGINES[name]
    ntimes, expected = e.counts
    h = e.make()
    h.profile(True)
    e.step(h, 0)
    e.step(h, 0)
    read = h.profile_read
    if name == "additive_physics":
        def read():
            return h.profile_read() + h.physics_profile_read()
    reads = [read(), read()]
    h.profile(False)
    e.step(h, 0)
    reads.append(read())
    h.close()
    print(name, "profile reads:", reads)
    for r, want in zip(reads, expected):
        times, counts = r[:ntimes], tuple(r[ntimes:ntimes + len(want)])
        assert counts == want, (reads, expected)
        assert all(math.isfinite(t) and t >= 0 for t in times), reads
        if counts and counts[0] > 0:
            assert all(t > 0 for t in times), reads
    if name == "subtractive":   # no launch count: the times themselves.  Not reset by a read, zero when off
        assert min(reads[0]) > 0 and reads[1] == reads[0] and reads[2] == (0.0, 0.0, 0.0, 0.0), reads
    if name == "additive_physics":   # likewise: (ms 0, launches 0, physics ms, audio ms)
        assert min(reads[0][2:]) > 0 and reads[1] == reads[0] and reads[2] == (0.0, 0, 0.0, 0.0), reads


@pytest.mark.parametrize("name", list(ENGINES))
def test_memory_returns(gpu_lib, name):
    import torch
    from huygens_amd._lib import HZ_OK
    e = ENGINES[name]
    destroy = getattr(gpu_lib, e.destroy)
    s = torch.cuda.Stream()

    def cycle():
        h = e.make()   # every call in it goes through check(): HZ_OK or an exception
        if name in REBINDABLE:
            h.set_stream(s.cuda_stream)
            h.set_stream(0)
        handle, h._h = h._h, None
        assert destroy(handle) == HZ_OK

    cold = torch.cuda.mem_get_info()[0]
    cycle()   # code objects and the runtime's own pools are in place after the first
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    print(name, "first cycle took", cold - free0, "bytes")
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    print(name, "free bytes before", free0, "after", free1, "difference", free0 - free1)
    assert abs(free0 - free1) <= 2 * GRANULE, (free0, free1)
