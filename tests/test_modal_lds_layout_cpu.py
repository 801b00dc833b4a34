"""Bank model of the modal phase 2's LDS operand reads (hz_fb_modal.h, phase2's MAC loop).

The LDS has 64 banks of 4 bytes: a 16-byte element e of a table that starts on a 256-byte boundary
lies in bank group e mod 16 (four banks) of row e // 16.  Lanes that read different rows of one bank
group are served one after the other; lanes that read the same element share one access.  In the
loop lane t = 8 o + qq (output o, r1 eighth qq) reads a[j][16 qq + i] and w128[((16 qq + i) k2) & 127]
in iteration i: unpadded, both indices mod 16 are the same for all eight qq, so the eight lanes of
an output sit in one bank group on up to eight rows.  hz_modal::px puts element e at e + (e >> 4)
(rows of 17): this pins that with it no bank group sees more than two rows from the eight lanes of
an output, for every wave, iteration, part and k2 -- the layout claim, not the hardware's timing.

Phase 1's DFT loop reads w64[((32 h + i) k1) & 63] in lane t (k1 = (t >> 1) & 63, h = t & 1): the
two lanes of an odd k1 read elements 32 apart, one bank group two rows apart.  hz_modal::px1 puts
element e at e + (e >> 5); the same count over the same eight-lane groups.
"""
import numpy as np

K_R1 = 128                   # hz_modal::kR1
K_PAD = K_R1 + K_R1 // 16    # hz_modal::kPad
THREADS = 256


def px(e):
    """hz_modal::px"""
    return e + (e >> 4)


def lane_elements(part, i, index, row_len):
    """16-byte element offsets (from the start of Lds2) of every lane's a and w128 reads in
    iteration i of a workgroup of bin range `part`; Lds2 = a[2][row_len], g[2][128], w128[row_len]"""
    t = np.arange(THREADS)
    o, qq = t >> 3, t & 7
    j, k2 = o >> 4, 16 * part + (o & 15)
    r1 = 16 * qq + i
    a_at = j * row_len + index(r1)
    w_at = 2 * row_len + 2 * K_R1 + index((r1 * k2) & 127)
    return a_at, w_at


def worst_rows(index, row_len):
    """the largest number of distinct rows in one bank group among the eight lanes of an output"""
    worst = 0
    for part in range(4):
        for i in range(16):
            for at in lane_elements(part, i, index, row_len):
                for grp in at.reshape(-1, 8):          # the eight qq lanes of one output (inside a wave)
                    for bank in np.unique(grp & 15):
                        worst = max(worst, len(np.unique(grp[(grp & 15) == bank] >> 4)))
    return worst


def test_tables_start_on_a_row():
    # the model's bank group = element mod 16 needs a, a[1]'s shift aside, and w128 at whole rows
    assert (2 * K_PAD + 2 * K_R1) % 16 == 0


def test_unpadded_layout_conflicts_eight_ways():
    assert worst_rows(lambda e: e, K_R1) == 8


def test_padded_layout_at_most_two_rows_per_bank_group():
    assert worst_rows(px, K_PAD) <= 2


def test_padded_index_is_injective_and_in_range():
    p = px(np.arange(K_R1))
    assert len(np.unique(p)) == K_R1 and p.max() < K_PAD


# ---- phase 1: w64 (Lds1 = red[4][64][2], F[2][64] -- 5120 bytes, whole rows -- then w64) ----------

K_R2 = 64                    # hz_modal::kR2
K_PAD1 = K_R2 + K_R2 // 32   # hz_modal::kPad1


def px1(e):
    """hz_modal::px1"""
    return e + (e >> 5)


def worst_and_total_rows_phase1(index):
    """(largest, summed over iterations and groups) number of distinct rows in one bank group among
    eight consecutive lanes"""
    t = np.arange(THREADS)
    k1, h = (t >> 1) & 63, t & 1
    worst = total = 0
    for i in range(32):
        at = index(((32 * h + i) * k1) & 63)
        for grp in at.reshape(-1, 8):
            m = max(len(np.unique(grp[(grp & 15) == bank] >> 4)) for bank in np.unique(grp & 15))
            worst, total = max(worst, m), total + m
    return worst, total


def test_phase1_table_starts_on_a_row():
    assert (4 * 64 * 2 * 8 + 2 * 64 * 8) % 256 == 0


def test_phase1_padded_layout_at_most_two_rows_per_bank_group():
    w0, t0 = worst_and_total_rows_phase1(lambda e: e)
    w1, t1 = worst_and_total_rows_phase1(px1)
    assert w0 == 4 and w1 <= 2
    # serialised reads over the ideal one per group and iteration (32 x 32 groups): under a quarter
    assert t1 - 1024 < (t0 - 1024) / 4, (t0, t1)
    p = px1(np.arange(K_R2))
    assert len(np.unique(p)) == K_R2 and p.max() < K_PAD1
