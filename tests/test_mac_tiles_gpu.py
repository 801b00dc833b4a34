"""GPU parity of the stationary engine over the call lengths that change the work split of its
three launches (hz_fb_resp.hip): B output blocks of 2048 samples, the LDS-staged MAC
(resp_mac_kernel_lds<QP>) in groups of 32 blocks x 64 bins, the transforms on the thread-order
twiddle tables (hz_fft2k.h).

B = 8 is part of one block group, 33 and 129 leave one block in the last group, 235 is the C2 call,
257 needs a ninth group; n = 2048 B + r with r = 768 leaves the last block ragged.  Every stationary
call is compared with the CPU restatement per 1024-sample block, each block against its own peak, at
the bound of tests/test_filterbank_resp_gpu.py (1e-9).  The time shares of one call (29 or 30
blocks each, their windows at other workgroup indices, other history offsets) equal the long call's
samples bit for bit: a block's arithmetic does not depend on where in a launch it runs.
"""
import numpy as np
import pytest

from golden.spec_numpy import resonant_coefficients, white_noise_f32
from oracle import OracleFilterbank

pytestmark = pytest.mark.gpu

TOL = 1e-9
P = 2048


def q_padded(K):
    """hz_fb_resp.hip: partitions of the horizon, padded as the MAC kernels are instantiated"""
    Q = K // P
    return (Q + 23) // 24 * 24 if Q > 24 else (Q + 7) // 8 * 8


def make(N, R, oracle=True):
    from huygens_amd import Filterbank
    fwd, back = resonant_coefficients(N, R, 0.5)
    objs = [Filterbank(2, N, 0.001, 0.001)]
    objs[0].tune_response(0, 1)   # stationary whenever it is legal (cost model off)
    if oracle:
        objs.append(OracleFilterbank(2, N, 0.001, 0.001))
    for fb in objs:
        for n in range(N):
            fb.coefficients(n, fwd[n], back[n])
        fb.boost(np.ones(N))
        fb.open()
    return objs if oracle else objs[0]


def block_err(got, ref):
    """largest error of a 1024-sample block relative to that block's own peak"""
    worst = 0.0
    for s in range(0, len(ref), 1024):
        g, r = got[s:s + 1024], ref[s:s + 1024]
        worst = max(worst, float(np.max(np.abs(g - r)) / np.max(np.abs(r))))
    return worst


def run_case(N, R, Qp, B):
    from huygens_amd._lib import HZ_FB_PATH_RESPONSE
    g, o = make(N, R)
    for i, n in enumerate([2000, 60000, 20000]):   # smoothers converge, the history fills
        x = white_noise_f32(n, seed=40 + i)
        g.process(x), o.process(x)
    for i, r in enumerate([0, 768]):
        n = P * B + r
        x = white_noise_f32(n, seed=50 + B + i)
        yg, yo = g.process(x), o.process(x)
        assert g.last_path() == HZ_FB_PATH_RESPONSE, (B, r)
        assert q_padded(g.response_info()[0]) == Qp, g.response_info()
        e = block_err(yg, yo)
        print(f"Qp {Qp} B {B} r {r}: worst block error {e:.3e}")
        assert e <= TOL, (B, r, e)


@pytest.mark.parametrize("B", [8, 33, 129, 235, 257])
def test_tiles_qp8(gpu_lib, B):
    """512 bands, R = 0.99: K = 8192, Q = 4 partitions padded to 8"""
    run_case(512, 0.99, 8, B)


@pytest.mark.parametrize("B", [8, 33, 129, 235, 257])
def test_tiles_qp16(gpu_lib, B):
    """512 bands, R = 0.9983: a horizon of 9 to 16 partitions"""
    run_case(512, 0.9983, 16, B)


def test_c2_blocks_qp24(gpu_lib):
    """64 bands (one wave of the response kernel), R = 0.9989 (0.99875 still has K = 32768, 16
    partitions): the shortest horizon padded to 24 partitions, at the C2 call's 235 blocks"""
    run_case(64, 0.9989, 24, 235)


def test_time_shares_equal_long_call_bitwise(gpu_lib):
    """One input as a long call (B = 235) and as eight time shares on handles that hold the whole
    bank (B = 29 or 30 each): every share's samples are the long call's, bit for bit."""
    from huygens_amd._lib import HZ_FB_PATH_RESPONSE
    from huygens_amd.shard import set_time_shards
    N, W = 256, 8
    whole = make(N, 0.99, oracle=False)
    ranks = [make(N, 0.99, oracle=False) for _ in range(W)]
    for r, s in enumerate(ranks):   # the all-reduces of one band shard: its own response and horizon
        assert set_time_shards(s, r, W, lambda h: h, lambda k: k)
    n = P * 235
    lengths = [2000, 60000, 20000, n]
    for i, m in enumerate(lengths):
        x = white_noise_f32(m, seed=70 + i)
        ready = all(s.stationary_ready(m) for s in ranks)
        for s in ranks:
            s.arm_time_shard(ready)
        y = whole.process(x)
        outs = [s.process(x) for s in ranks]
    assert ready and whole.last_path() == HZ_FB_PATH_RESPONSE
    assert all(s.last_path() == HZ_FB_PATH_RESPONSE for s in ranks)
    covered = 0
    for s, ys in zip(ranks, outs):
        on, f, c = s.time_shard_info(n)
        assert on and c <= 32 * P
        assert np.array_equal(ys[f:f + c].view(np.uint64), y[f:f + c].view(np.uint64)), (f, c)
        covered += c
    assert covered == n
