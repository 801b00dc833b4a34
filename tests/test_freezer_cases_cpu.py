"""CPU: the Freezer cases of tests/freezer_cases.py are well-conditioned and reach their branches.

For every case the two CPU restatements (oracle/hz_oracle_frz.c, long double DFT; the numpy model
of tests/freezer_model.py) agree: bit for bit on dry samples, within 1e-12 of each frozen period's
own peak -- so a GPU mismatch at such a case is the engine's, not the reference's.  And every case
is shown, from the model's trace and from the schedule, to reach the branches it is named for:
conditions on the inputs, mended in freezer_cases.py if a seed or a schedule misses one.
"""
import functools

import numpy as np
import pytest

import freezer_cases as fc
from freezer_cases import F, U
from freezer_model import PyFreezer, split_schedule
from oracle_frz import OracleFreezer, libc_srand

BY_NAME = {c.name: c for c in fc.CASES + fc.CHUNK_CASES}


@functools.lru_cache(maxsize=None)
def run(name):
    """(oracle output, model output, model trace, dry mask, periods) of a case: computed once"""
    c = BY_NAME[name]
    g = c.geom
    x = fc.noise(c)
    libc_srand(c.seed)
    yo = OracleFreezer(g.N, g.laps, g.width).process(x, c.events)
    m = PyFreezer(g.N, g.laps, g.width, trace=True)
    libc_srand(c.seed)
    ym = m.process(x, c.events)
    dry, periods = split_schedule(c.n, c.events)
    for a in (yo, ym, dry):
        a.setflags(write=False)
    return yo, ym, m.trace, dry, periods


def walk(events):
    """the schedule's transitions: (dry gaps between periods, unfreezes while dry)"""
    frozen, last_u, gaps, dry_u = False, None, [], 0
    for t, k in events:
        if k == F:
            if not frozen and last_u is not None:
                gaps.append(t - last_u)
            frozen = True
        else:
            if frozen:
                last_u = t
            else:
                dry_u += 1
            frozen = False
    return gaps, dry_u


def transitions(tr):
    return [f for f in tr.freezes if f[1]]


def refreezes(tr):
    return [f for f in tr.freezes if not f[1]]


def zero_periods(yo, periods):
    return [(a, b) for a, b in periods if not np.any(yo[a:b])]


def on_one_sample(events, kinds):
    k = len(kinds)
    return any(len({t for t, _ in events[i:i + k]}) == 1 and [q for _, q in events[i:i + k]] == kinds
               for i in range(len(events) - k + 1))


# name -> predicate(case, geometry, trace, oracle output, periods)
BRANCHES = {
    "freeze_at_0": lambda c, g, tr, yo, pe: any(f[0] == 0 for f in transitions(tr)),
    "freeze_before_first_process": lambda c, g, tr, yo, pe: any(f[0] < g.s for f in transitions(tr)),
    "zero_period": lambda c, g, tr, yo, pe: len(zero_periods(yo, pe)) > 0,
    "phase_s": lambda c, g, tr, yo, pe: any(f[0] % g.S == g.s for f in transitions(tr)),
    "phase_S-1": lambda c, g, tr, yo, pe: any(f[0] % g.S == g.S - 1 for f in transitions(tr)),
    "phase_0": lambda c, g, tr, yo, pe: any(f[0] % g.S == 0 for f in transitions(tr)),
    "multiple_of_S": lambda c, g, tr, yo, pe: any(f[0] > 0 and f[0] % g.S == 0 for f in transitions(tr)),
    "refreeze_on_populate": lambda c, g, tr, yo, pe: any(
        f[3] % g.s == 0 and any(p["t"] == f[0] and p["slot"] == 0 for p in tr.populates) for f in refreezes(tr)),
    "refreeze_mid_stride": lambda c, g, tr, yo, pe: any(f[3] % g.s != 0 for f in refreezes(tr)),
    "period_len_s": lambda c, g, tr, yo, pe: any(b - a == g.s for a, b in pe),
    "period_lt_s": lambda c, g, tr, yo, pe: any(b - a < g.s and sum(a <= p["t"] < b for p in tr.populates) == 1
                                                for a, b in pe),
    "period_gt_3S": lambda c, g, tr, yo, pe: any(b - a > 3 * g.S for a, b in pe),
    "dry_gap_0": lambda c, g, tr, yo, pe: 0 in walk(c.events)[0],
    "dry_gap_1": lambda c, g, tr, yo, pe: 1 in walk(c.events)[0],
    "dry_gap_N": lambda c, g, tr, yo, pe: g.N in walk(c.events)[0],
    "dry_gap_N+1": lambda c, g, tr, yo, pe: g.N + 1 in walk(c.events)[0],
    "dry_gap_N+2": lambda c, g, tr, yo, pe: g.N + 2 in walk(c.events)[0],
    "dry_gap_2N+3": lambda c, g, tr, yo, pe: 2 * g.N + 3 in walk(c.events)[0],
    "midread": lambda c, g, tr, yo, pe: any(p["midread"] for p in tr.populates),
    "reread": lambda c, g, tr, yo, pe: any(p["reread"] for p in tr.populates),
    "unfreeze_while_dry": lambda c, g, tr, yo, pe: walk(c.events)[1] > 0,
    "freeze_unfreeze_freeze": lambda c, g, tr, yo, pe: on_one_sample(c.events, [F, U, F]),
    # a draw of DFrame excluded - 1 after an earlier freeze wrote it: an audible stale frame
    "stale_after_second_freeze": lambda c, g, tr, yo, pe: any(not p["refreshed"] and p["period"] >= 1
                                                              for p in tr.populates),
    "freeze_at_n": lambda c, g, tr, yo, pe: any(t in c.at_n and t in c.cuts and k == F for t, k in c.events),
    "unfreeze_at_n": lambda c, g, tr, yo, pe: any(t in c.at_n and t in c.cuts and k == U for t, k in c.events),
    "m3_sequence": lambda c, g, tr, yo, pe: [f[2] for f in transitions(tr)] == [0, 2, 1, 0],
}


def test_geometries_are_the_constructors():
    for geo in fc.GEOMETRIES:
        g, o = fc.geometry(*geo), OracleFreezer(*geo)
        assert (g.s, g.M, g.S) == (o.stride, o.M, o.size) == fc.GEOMETRY_FACTS[geo]
    assert fc.geometry(16, 9, 1.0).S < 16


@pytest.mark.parametrize("name", fc.CASE_IDS + [c.name for c in fc.CHUNK_CASES])
def test_schedule_is_sound(name):
    c = BY_NAME[name]
    ts = [t for t, _ in c.events]
    assert ts == sorted(ts) and ts[0] >= 0 and ts[-1] < c.n <= fc.MAX_LEN
    _, _, tr, dry, periods = run(name)
    # the helper's view of the schedule is the model's
    assert np.array_equal(dry, ~tr.frozen)
    for i, (a, b) in enumerate(periods):
        assert np.all(tr.period[a:b] == tr.period[a]) and tr.period[a] >= i
        assert a == 0 or tr.period[a - 1] != tr.period[a]
        # a frozen length that is a multiple of N + 1 leaves the Delay ring where it was
        assert (b - a) % (c.geom.N + 1) != 0
    assert sum(b - a for a, b in periods) == np.count_nonzero(~dry)


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_restatements_agree(name):
    """the conditioning check: a case that fails it gets another input, not a wider bound"""
    yo, ym, _, dry, periods = run(name)
    assert np.array_equal(yo[dry], ym[dry])
    assert np.count_nonzero(yo[dry]) > 0
    for a, b in periods:
        peak = np.max(np.abs(yo[a:b]))
        assert np.max(np.abs(yo[a:b] - ym[a:b])) <= 1e-12 * peak, (name, a, b, peak)


@pytest.mark.parametrize("name", fc.CASE_IDS)
def test_case_reaches_its_branches(name):
    c = BY_NAME[name]
    yo, _, tr, _, periods = run(name)
    assert c.branches
    missed = [b for b in c.branches if not BRANCHES[b](c, c.geom, tr, yo, periods)]
    assert not missed, (name, missed)


def test_every_branch_is_asked_of_some_case():
    asked = {b for c in fc.CASES for b in c.branches}
    assert asked == set(BRANCHES)
    for geo in fc.GEOMETRIES:   # every geometry runs both templates
        names = [c.name for c in fc.CASES if (c.geom.N, c.geom.laps, c.geom.width) == geo]
        assert len(names) >= 2


def test_m3_sequence_plays_zero_fresh_stale_stale():
    """M = 3 at (16, 2, 1): excluded 0 and 1 draw DFrame excluded - 1, which freeze() does not write;
    excluded 2 draws a fresh one."""
    c = BY_NAME["m3-16-2-1"]
    yo, _, tr, _, periods = run(c.name)
    assert len(periods) == 4 and walk(c.events)[0] and min(walk(c.events)[0]) > c.geom.S
    fresh = [[p["refreshed"] for p in tr.populates if a <= p["t"] < b] for a, b in periods]
    assert all(len(f) >= 3 for f in fresh)
    assert not any(fresh[0]) and all(fresh[1]) and not any(fresh[2]) and not any(fresh[3])
    assert not np.any(yo[periods[0][0]:periods[0][1]])
    for a, b in periods[1:]:
        assert np.max(np.abs(yo[a:b])) > 1e-3
    # the stale frame of period 2 is DFrame 0 as period 1 wrote it (excluded 2 refreshes DFrame 0
    # alone), that of period 3 is DFrame 2 as period 2 wrote it
    assert [sorted({p["next"] for p in tr.populates if a <= p["t"] < b}) for a, b in periods] == [[2], [0], [0], [2]]


@pytest.mark.parametrize("name", [c.name for c in fc.CASES if c.geom.N <= 256])
def test_model_stretches_are_its_samples(name):
    """PyFreezer.process by slices gives the bits of sample() called per sample"""
    c = BY_NAME[name]
    g = c.geom
    x = fc.noise(c)
    libc_srand(c.seed)
    y = PyFreezer(g.N, g.laps, g.width).process(x, c.events, per_sample=True)
    assert np.array_equal(y, run(name)[1])


def test_blocks_keep_the_schedule():
    """fc.blocks: every event once, at its absolute time, at == n only where asked"""
    for c in fc.CASES:
        for cuts, at_n in ((c.cuts, c.at_n), (fc.event_cuts(c.n, c.events),) * 2, (fc.event_cuts(c.n, c.events), [])):
            pos, seen = 0, []
            for n, ev in fc.blocks(c.n, c.events, cuts, at_n):
                assert n > 0 and all(0 <= t <= n for t, _ in ev)
                assert all(t < n or pos + t in at_n for t, _ in ev)
                seen += [(pos + t, k) for t, k in ev]
                pos += n
            assert pos == c.n and seen == list(c.events)
    assert min(n for c in fc.CASES for n, _ in fc.blocks(c.n, c.events, fc.event_cuts(c.n, c.events))) == 1


@pytest.mark.parametrize("name", [c.name for c in fc.CHUNK_CASES])
def test_chunk_schedule_meets_the_boundaries(name):
    c, C = BY_NAME[name], fc.CHUNK
    _, _, tr, _, periods = run(name)
    assert c.n > 4 * C
    pop = {p["t"] for p in tr.populates}
    ev = dict()
    for t, k in c.events:
        ev.setdefault(k, set()).add(t)
    assert any(t % C == 0 and t - 1 not in ev[F] and t not in ev[F] for t in pop)        # a populate sample
    for k in (F, U):                                                                    # on, before, after
        assert {0, 1, C - 1} <= {t % C for t in ev[k]}
    assert any(a // C + 2 <= (b - 1) // C for a, b in periods)                           # opened two chunks earlier
    # a chunk that starts frozen and holds an unfreeze, then a freeze
    assert any(tr.frozen[q * C] and any(q * C < u < f < (q + 1) * C for u in ev[U] for f in ev[F])
               for q in range(1, c.n // C))
