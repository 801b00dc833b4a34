"""The stationary engine's forward windows by where their samples lie (hz_fb_resp.hip, WindowLoad).

512 bands of the resonant recipe at R = 0.99: horizon K = 8192 (0.99^K < 2^-53 from K = 3656 on,
rounded up to 8192), Q = 4 partitions.  A stationary call of n >= 16384 samples then has windows
wholly inside the history (0, 1, 2), the window that straddles the history's end (3) and windows
in the call alone, and the lengths below add an odd length, a last pair that straddles the call's
end and a short last block.  Every call runs with its input and output 16-byte aligned and with
the same data 8 bytes further on: the two load the same values into the same arithmetic, so they
are equal bitwise, outputs and states; each is within test_filterbank_resp_gpu.py's tolerances of
the restatement (output, x history, band states, smoothers: 1e-9).  The restatement runs once
for all of them."""
import numpy as np
import pytest

from golden.spec_numpy import resonant_coefficients
from oracle import OracleFilterbank, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9   # tests/test_filterbank_resp_gpu.py: TOL and states_close's default
N, ORDER, K = 512, 2, 8192
PRIME = [4000, 16384, 16384]   # smoothers converge, then the history fills
CALLS = [16384, 16385, 16386, 18431, 20480 + 767]
SHARD_CALLS = 2   # the time-shard pair runs the first two of CALLS after the priming
GUARD = 7.0


def lib():
    from huygens_amd import _lib
    return _lib


def states_close(a, b, tol=TOL):
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def setup(fb, fwd, back):
    for n in range(N):
        fb.coefficients(n, fwd[n], back[n])
    fb.boost(np.ones(N))
    fb.open()


@pytest.fixture(scope="module")
def ref():
    """Inputs, the restatement's outputs and its state after every call (priming included)."""
    fwd, back = resonant_coefficients(N, 0.99, 0.5)
    o = OracleFilterbank(ORDER, N, 0.001, 0.001)
    setup(o, fwd, back)
    rng = np.random.default_rng(2024)
    seq = []
    for n in PRIME + CALLS:
        x = rng.uniform(-1, 1, n)
        seq.append((x, o.process(x), o.get_state()))
    return fwd, back, seq


def bank(fwd, back, mode):
    from huygens_amd import Filterbank
    g = Filterbank(ORDER, N, 0.001, 0.001)
    g.set_response(mode)
    g.tune_response(16384, 1)   # 16,384-sample calls admitted, cost model off
    setup(g, fwd, back)
    return g


def run(g, x, mis):
    """One call on device buffers whose pointers are 16-byte aligned (mis = 0) or 8 bytes past
    that (mis = 1); one guard element on either side of the output must stay untouched."""
    import torch
    n = len(x)
    xd = torch.zeros(n + 4, dtype=torch.float64, device="cuda")
    yd = torch.full((n + 4,), GUARD, dtype=torch.float64, device="cuda")
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    xs, ys = xd[2 + mis:2 + mis + n], yd[2 + mis:2 + mis + n]
    assert xs.data_ptr() % 16 == 8 * mis and ys.data_ptr() % 16 == 8 * mis
    xs.copy_(torch.from_numpy(x))
    g.process_device(xs.data_ptr(), ys.data_ptr(), n)
    g.synchronize()
    y = yd.cpu().numpy()
    assert np.all(y[:2 + mis] == GUARD) and np.all(y[2 + mis + n:] == GUARD), "store outside the output"
    return y[2 + mis:2 + mis + n].copy()


@pytest.mark.parametrize("lazy", [False, True])
def test_history_straddling_and_call_windows(gpu_lib, ref, lazy):
    L = lib()
    fwd, back, seq = ref
    banks = [bank(fwd, back, L.HZ_FB_RESP_LAZY if lazy else L.HZ_FB_RESP_EAGER) for _ in range(2)]
    for i, (x, yo, so) in enumerate(seq):
        ys = [run(g, x, mis) for mis, g in enumerate(banks)]
        st = [g.get_state() for g in banks]
        if i >= len(PRIME):   # primed: every call below is the stationary engine's
            for g in banks:
                assert g.last_path() == L.HZ_FB_PATH_RESPONSE, (i, len(x), g.last_path(), g.response_info())
                assert g.response_info()[0] == K
        errs = [rel_err(y, yo) for y in ys]
        print(f"n = {len(x)}: output rel err aligned {errs[0]:.3e}, misaligned {errs[1]:.3e}; state err "
              f"{np.max(np.abs(st[0] - so)) / max(1.0, np.max(np.abs(so))):.3e}")
        assert np.array_equal(bits(ys[0]), bits(ys[1])), (i, len(x))
        assert np.array_equal(bits(st[0]), bits(st[1])), (i, len(x))
        for y, s in zip(ys, st):
            assert rel_err(y, yo) < TOL, (i, len(x), rel_err(y, yo))
            assert states_close(s, so), (i, len(x))
    assert banks[0].response_info()[3] >= len(CALLS)


@pytest.mark.parametrize("fill", [True, False])
def test_time_shard_pair(gpu_lib, ref, fill):
    """set_time_shard(r, 2) on two handles that each hold the whole bank (its own response is the
    bank response): the shares sum to (fill) or tile (no fill) the unsharded mix, for both
    pointer alignments, bitwise the same for both."""
    L = lib()
    fwd, back, seq = ref
    # [alignment][rank]
    banks = [[bank(fwd, back, L.HZ_FB_RESP_EAGER) for _ in range(2)] for _ in range(2)]
    for pair in banks:
        for r, g in enumerate(pair):
            g.response(8192)
            assert g.response_info()[0] == K
            g.set_bank_response(g.response(K))
            g.set_time_shard(r, 2)
            g.set_time_shard_fill(fill)
    sharded = 0
    for i, (x, yo, so) in enumerate(seq[:len(PRIME) + SHARD_CALLS]):
        n = len(x)
        got = []
        for mis, pair in enumerate(banks):
            ready = all(g.stationary_ready(n) for g in pair)
            for g in pair:
                g.arm_time_shard(ready)
            outs = [run(g, x, mis) for g in pair]
            if ready:
                assert all(g.last_path() == L.HZ_FB_PATH_RESPONSE for g in pair)
                share = [g.time_shard_info(n) for g in pair]
                assert all(a for a, _, _ in share)
                assert share[0][1] == 0 and share[0][2] == share[1][1] and share[1][1] + share[1][2] == n
                assert share[0][2] % 2048 == 0
                if fill:
                    for (_, f, c), y in zip(share, outs):
                        assert not np.any(y[:f]) and not np.any(y[f + c:])
                    mix = outs[0] + outs[1]
                else:
                    mix = np.zeros(n)
                    for (_, f, c), y in zip(share, outs):
                        assert np.all(y[:f] == GUARD) and np.all(y[f + c:] == GUARD)   # outside: untouched
                        mix[f:f + c] = y[f:f + c]
            else:
                assert i < len(PRIME), (i, n)
                assert np.array_equal(bits(outs[0]), bits(outs[1]))
                mix = outs[0]
            got.append((mix, outs, [g.get_state() for g in pair]))
        sharded += ready
        for a, b in zip(got[0][1] + got[0][2], got[1][1] + got[1][2]):
            assert np.array_equal(bits(a), bits(b)), (i, n)
        for mix, _, sts in got:
            assert rel_err(mix, yo) < TOL, (i, n, rel_err(mix, yo))
            assert all(states_close(s, so) for s in sts), (i, n)
    assert sharded >= SHARD_CALLS
