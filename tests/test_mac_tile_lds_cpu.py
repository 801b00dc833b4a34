"""Bank model of the LDS-staged MAC's tile (hz_fb_resp.hip, resp_mac_kernel_lds<QP>) and the index
algebra of the thread-order twiddle tables (hz_fft2k.h, FwdTw::at / InvTw::at).

The LDS has 64 banks of 4 bytes, and a ds_read_b128 / ds_write_b128 is served 16 lanes at a time
(tests/test_modal_lds_layout_cpu.py has the same model): the 16 lanes are conflict-free when their
distinct 16-byte elements fall into 16 different bank groups (element mod 16).  The tile is 64 bins x
4 slices (waves) of 8 output blocks, rows of 64 bins: 16 lanes read or write 256 contiguous bytes.
"""
import numpy as np
import pytest

THREADS = 256
BINS = 64          # kMacBins
BPW = 8            # kMacBpw
LDS_LIMIT = 160 * 1024   # gfx950: LDS bytes a workgroup may use
QPS = [8, 16, 24]


def lds_bytes(qp):
    """mac_lds_bytes<QP>"""
    return 16 * BINS * (qp + 4 * BPW + qp - 1)


def accesses(qp):
    """every LDS instruction of a workgroup as (name, elements[256], active[256]): the staging stores
    of the H and Z rows, the ring's first BPW reads, and the H and Z read of every step"""
    t = np.arange(THREADS)
    lq, sl = t & (BINS - 1), t >> 6
    kzr = 4 * BPW + qp - 1
    zs = qp * BINS
    always = np.ones(THREADS, bool)
    out = []
    for k in range(qp // 4):
        out.append(("store H", (sl + 4 * k) * BINS + lq, always))
    for k in range((kzr + 3) // 4):
        out.append(("store Z", zs + (sl + 4 * k) * BINS + lq, sl + 4 * k < kzr))
    for r in range(BPW):
        out.append(("ring", zs + (BPW * sl + r + qp - 1) * BINS + lq, always))
    for p in range(qp):
        out.append(("H", p * BINS + lq, always))
        if p + 1 < qp:
            out.append(("Z", zs + (BPW * sl + qp - 2 - p) * BINS + lq, always))
    return out


@pytest.mark.parametrize("qp", QPS)
def test_tile_is_conflict_free_and_fits(qp):
    size = lds_bytes(qp) // 16
    assert lds_bytes(qp) <= LDS_LIMIT
    staged = set()
    for name, el, on in accesses(qp):
        assert el[on].min() >= 0 and el[on].max() < size, name
        for g in range(0, THREADS, 16):
            e = np.unique(el[g:g + 16][on[g:g + 16]])
            if len(e):
                assert np.bincount(e & 15).max() == 1, (name, g)
        if name.startswith("store"):
            assert not staged & set(el[on].tolist())
            staged |= set(el[on].tolist())
        else:   # every element the loop reads was staged
            assert set(el[on].tolist()) <= staged, name
    assert len(staged) == size


# ---- thread-order twiddle tables (hz_fft2k.h) ---------------------------------------------------
# The transforms used to gather a thread's stage twiddles from the W_4096 table tw (tw[k] =
# e^{-2 pi i k / 4096}, k < 2048) at tw[2 (p << s)]: Dif<R, LH>::load_tw with p = b mod 2^(LH - R + 1),
# s = 10 - LH + k, and Dit<R, LH>::load_tw with p = b mod 2^LH, s = 10 - LH - k (b the thread's
# group, k < R), FwdTw / InvTw in the order of their members; the split and merge read tw[t + 256 i].
# The tables hold the same entries as table[slot][t].

K_LG, K_T, TW_SLOTS = 11, 256, 10


def dif_gather(R, LH, b):
    """the addresses Dif<R, LH>::load_tw read for group b"""
    p = b & ((1 << (LH - (R - 1))) - 1)
    return [2 * (p << (K_LG - 1 - LH + k)) for k in range(R)]


def dit_gather(R, LH, b):
    """the addresses Dit<R, LH>::load_tw read for group b"""
    p = b & ((1 << LH) - 1)
    return [2 * (p << (K_LG - 1 - LH - k)) for k in range(R)]


def fwd_at(s, t):
    """hz2k::FwdTw::at"""
    def tw_at(R, LH, b, k):
        return 2 * ((b & ((1 << (LH - (R - 1))) - 1)) << (K_LG - 1 - LH + k))
    if s < 2:
        return tw_at(2, 10, t, s)
    if s < 4:
        return tw_at(2, 10, t + K_T, s - 2)
    if s < 7:
        return tw_at(3, 8, t, s - 4)
    return tw_at(3, 5, t, s - 7)


def inv_at(s, t):
    """hz2k::InvTw::at"""
    def tw_at(R, LH, b, k):
        return 2 * ((b & ((1 << LH) - 1)) << (K_LG - 1 - LH - k))
    if s < 3:
        return tw_at(3, 3, t, s)
    if s < 6:
        return tw_at(3, 6, t, s - 3)
    if s < 8:
        return tw_at(2, 9, t, s - 6)
    return tw_at(2, 9, t + K_T, s - 8)


def test_thread_order_twiddle_tables_hold_the_gathered_entries():
    k = np.arange(2048)
    tw = np.exp(-2j * np.pi * k / 4096)
    fwd = np.array([[fwd_at(s, t) for t in range(K_T)] for s in range(TW_SLOTS)])
    inv = np.array([[inv_at(s, t) for t in range(K_T)] for s in range(TW_SLOTS)])
    assert fwd.min() >= 0 and fwd.max() < 2048 and inv.min() >= 0 and inv.max() < 2048
    for t in range(K_T):
        # FwdTw: p1[0] (group t), p1[1] (group t + 256), p2, p3;  InvTw: p2, p3, p4[0], p4[1]
        old_f = dif_gather(2, 10, t) + dif_gather(2, 10, t + K_T) + dif_gather(3, 8, t) + dif_gather(3, 5, t)
        old_i = dit_gather(3, 3, t) + dit_gather(3, 6, t) + dit_gather(2, 9, t) + dit_gather(2, 9, t + K_T)
        assert len(old_f) == len(old_i) == TW_SLOTS
        assert list(fwd[:, t]) == old_f and list(inv[:, t]) == old_i, t
        assert np.array_equal(tw[fwd[:, t]], tw[old_f]) and np.array_equal(tw[inv[:, t]], tw[old_i])
    # no slot of these passes is identically 1 (those passes, LD == 0 / LH == 0, load nothing), and
    # the stage twiddle of pass (R, LH) is W_2048^(p << ...) as the butterflies expect
    assert all(len(np.unique(fwd[s])) > 1 and len(np.unique(inv[s])) > 1 for s in range(TW_SLOTS))
    t = np.arange(K_T)
    assert np.allclose(tw[fwd[4]], np.exp(-2j * np.pi * ((t & 63) << 2) / 2048))
    assert np.allclose(tw[inv[0]], np.exp(-2j * np.pi * ((t & 7) << 7) / 2048))
    # the gathers this replaces touched many 128-byte lines per wave; a table row is 8 per wave
    lines = sum(len(np.unique(fwd[s, w * 64:(w + 1) * 64] // 8)) for s in range(TW_SLOTS) for w in range(1))
    assert lines == 16 + 32 + 16 + 32 + 3 * 64 + 3 * 8
