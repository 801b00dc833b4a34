"""Index model of the staged MAC (huygens_amd/csrc/hz_fb_mac.h, resp_mac_kernel_lds<QP, S>): the
operands go to LDS in QP / S stages of S partition steps, each stage behind one barrier, so that the
first stage's MACs run while the later rows are still in flight.  The library builds one stage (S =
QP); the splits are the HZ_MAC_STAGE builds that DESIGN.md 3.6 measures against it.

The model restates the kernel's index expressions (row = wave + 4 k; mac_zlo / mac_zhi; the ring's
reads) and checks, for every QP and stage length the kernel can be built with:
  * every (H row, Z row) a step reads was stored by a stage whose barrier precedes that step;
  * every row of the tile is stored exactly once, by exactly one thread row (wave);
  * a thread issues its loads stage by stage, so "the loads of stages <= s have landed" is one
    vmcnt threshold, and within a stage H ascends and Z descends (the order of use);
  * the ring hands accumulator (block lb) the pairs (H_p, Z_{lb + QP - 1 - p}) for p = 0 .. QP - 1 in
    that order: the register kernel's sum, term by term.
"""
import pytest

WAVES = 4          # 256 threads: wave = t >> 6 owns tile rows wave + 4 k
BPW = 8            # kMacBpw: output blocks per wave
BLK = WAVES * BPW  # output blocks per workgroup
SPLITS = [(qp, s) for qp in (8, 16, 24) for s in range(4, qp + 1, 4) if qp % s == 0]
BUILT = [(8, 8), (16, 16), (24, 24)]   # mac_stage<QP>(): one stage; HZ_MAC_STAGE = 8 / 12 build the splits measured


def zlo(qp, s, L):
    """mac_zlo"""
    return (qp - (s + 1) * L) // 4


def zhi(qp, kzl, s, L):
    """mac_zhi"""
    return kzl if s == 0 else (qp - s * L) // 4


def stage_rows(qp, S, s, wave):
    """the (kind, row) a thread of `wave` stores in stage s, in the kernel's order"""
    kzr = BLK + qp - 1
    kzl = (kzr + 3) // 4
    out = [("H", wave + 4 * k) for k in range(s * S // 4, (s + 1) * S // 4)]
    out += [("Z", wave + 4 * k) for k in range(zhi(qp, kzl, s, S) - 1, zlo(qp, s, S) - 1, -1) if wave + 4 * k < kzr]
    return out


def load_order(qp, S, wave):
    """the thread's global loads in issue order: stages of OS steps (8 at a time in a single stage)"""
    OS = S if S < qp else (8 if qp > 8 else qp)
    return [(s, row) for s in range(qp // OS) for row in stage_rows(qp, OS, s, wave)], OS


def step_reads(qp, p, wave):
    """the LDS rows wave `wave` reads at step p: H row p; the ring's first rows (step 0) or its one new row"""
    z = [BPW * wave + r + qp - 1 for r in range(BPW)] if p == 0 else [BPW * wave + qp - 1 - p]
    return [("H", p)] + [("Z", r) for r in z]


def test_the_built_splits_are_modelled():
    assert set(BUILT) <= set(SPLITS)
    assert {(16, 8), (24, 8), (24, 12)} <= set(SPLITS)   # the splits measured against it


@pytest.mark.parametrize("qp,S", SPLITS)
def test_rows_are_stored_once_and_before_use(qp, S):
    kzr = BLK + qp - 1
    stored = {}   # (kind, row) -> stage
    for s in range(qp // S):
        for wave in range(WAVES):
            for key in stage_rows(qp, S, s, wave):
                assert key not in stored, (key, s)
                stored[key] = s
    assert set(stored) == {("H", r) for r in range(qp)} | {("Z", r) for r in range(kzr)}
    for p in range(qp):
        for wave in range(WAVES):
            for key in step_reads(qp, p, wave):
                # the barrier that ends stage stored[key]'s stores precedes every step of that stage
                assert stored[key] <= p // S, (key, p)
    # a later stage overwrites nothing: with rows stored once, no barrier is needed after a stage's steps
    assert len(stored) == qp + kzr


@pytest.mark.parametrize("qp,S", SPLITS)
def test_loads_are_issued_in_order_of_use(qp, S):
    for wave in range(WAVES):
        order, OS = load_order(qp, S, wave)
        stages = [s for s, _ in order]
        assert stages == sorted(stages)
        assert sorted(row for _, row in order) == sorted(
            [("H", wave + 4 * k) for k in range(qp // 4)] + [("Z", r) for r in range(wave, BLK + qp - 1, 4)])
        first_use = {("H", r): r for r in range(qp)}
        first_use.update({("Z", r): max(0, qp - 1 - r) for r in range(BLK + qp - 1)})   # step of the first read
        for s in range(qp // OS):
            rows = [row for st, row in order if st == s]
            assert all(first_use[row] // OS == s for row in rows), (s, rows)
            h = [r for kind, r in rows if kind == "H"]
            z = [r for kind, r in rows if kind == "Z"]
            assert h == sorted(h) and z == sorted(z, reverse=True)
            assert rows[:len(h)] == [("H", r) for r in h]
        if S < qp:   # a stage's stores read what its own loads and earlier ones brought, nothing later
            for s in range(qp // S):
                issued = {row for st, row in order if st <= s}
                assert set(stage_rows(qp, S, s, wave)) <= issued


@pytest.mark.parametrize("qp,S", SPLITS)
def test_the_ring_feeds_every_block_the_register_kernels_terms(qp, S):
    for wave in range(WAVES):
        ring = None
        terms = [[] for _ in range(BPW)]
        for p in range(qp):
            reads = [r for kind, r in step_reads(qp, p, wave) if kind == "Z"]
            ring = reads if p == 0 else [reads[0]] + ring[:-1]   # one block down, one new row
            for r in range(BPW):
                terms[r].append((p, ring[r]))
        for r in range(BPW):
            lb = BPW * wave + r
            assert terms[r] == [(p, lb + qp - 1 - p) for p in range(qp)]
