"""The cases of tests/test_freezer_cases_gpu.py, shared with their CPU proofs
(tests/test_freezer_cases_cpu.py).  TEST INFRASTRUCTURE; numpy only.

A case is a geometry (N, laps, width), a seed (input and srand), a length and an event schedule.
Schedules are written in the stride s, the frame ring's size S = M s and N, so that their events
land on the intended phases of the write head (t mod S), of the read head (time since the freeze)
and of the Delay ring (mod N + 1) at every geometry.  Each case lists the branches it exists for:
the CPU test proves from the model's trace (and from the schedule) that they are reached, the GPU
test then knows what a pass covered.  Input is white noise: a tone leaves most bins at rounding
level, where their phases are noise and the restatement itself is ill-conditioned.
"""
from collections import namedtuple

import numpy as np

F, U = 1, 0

Geometry = namedtuple("Geometry", "N laps width s M S")
Case = namedtuple("Case", "name geom seed n events cuts at_n branches")


def geometry(N, laps, width):
    """Freezer's constructor arithmetic (fourier.h:397-402)"""
    width, laps = max(width, 1.0), max(laps, 2)
    s, M = N // laps, int(width * laps) + 1
    return Geometry(N, laps, width, s, M, M * s)


GEOMETRIES = [
    (4, 2, 1.0),       # smallest N, M = 3; fewer points than threads
    (8, 8, 1.0),       # stride 1: every sample populates
    (16, 9, 1.0),      # size 10 < N: the `s < size` guard of the frame gather
    (16, 2, 1.0),      # M = 3: every draw is decided by `excluded`
    (64, 2, 20.5),     # M = 42
    (256, 3, 2.5),     # laps does not divide N: stride 85, size 680
    (2048, 8, 1.0),    # the reference's own size
    (4096, 8, 1.0),    # 64 KB dynamic LDS, even-log2 FFT (12 stages)
    (8192, 4, 1.0),    # 128 KB dynamic LDS, odd-log2 FFT (13 stages)
]
# what the constructor makes of them: stride, M, size
GEOMETRY_FACTS = {
    (4, 2, 1.0): (2, 3, 6), (8, 8, 1.0): (1, 9, 9), (16, 9, 1.0): (1, 10, 10), (16, 2, 1.0): (8, 3, 24),
    (64, 2, 20.5): (32, 42, 1344), (256, 3, 2.5): (85, 8, 680), (2048, 8, 1.0): (256, 9, 2304),
    (4096, 8, 1.0): (512, 9, 4608), (8192, 4, 1.0): (2048, 5, 10240),
}
MAX_LEN = 110_000


def edges(g):
    """Freezes at t = 0, on the phases s, S - 1 and 0 and on a multiple of S; re-freezes on a
    populate sample and mid-stride; frozen lengths s, > 3 S and < s; dry gaps 0, 1, N, N + 1, N + 2
    and 2 N + 3.  The first two periods play frames that were never processed: exact zeros."""
    N, s, S = g.N, g.s, g.S
    short = (s + 1) // 2
    ev = [
        (0, F), (s, U),                                   # t = 0; exactly s long
        (s, F), (S - 2, U),                               # dry gap 0; phase s, no frame processed yet
        (S - 1, F),                                       # dry gap 1; phase S - 1
        (S - 1 + 2 * s, F),                               # re-freeze on a populate sample
        (S - 1 + 3 * s + s // 2, F),                      # re-freeze mid-stride (s > 1)
        (6 * S - N, U),                                   # > 3 S long
        (6 * S, F), (6 * S + short, U),                   # dry gap N; a multiple of S; shorter than s
    ]
    t = 6 * S + short + N + 1
    ev += [(t, F), (t + s + 2, U)]                        # dry gap N + 1
    t += s + 2 + N + 2
    ev += [(t, F), (t + 2 * s + 3, U)]                    # dry gap N + 2
    t += 2 * s + 3 + 2 * N + 3
    ev += [(t, F)]                                        # dry gap 2 N + 3; frozen to the end
    n = t + 2 * s + 3
    branches = ["freeze_at_0", "freeze_before_first_process", "zero_period", "phase_s", "phase_S-1", "phase_0",
                "multiple_of_S", "refreeze_on_populate", "period_len_s", "period_gt_3S", "dry_gap_0", "dry_gap_1",
                "dry_gap_N", "dry_gap_N+1", "dry_gap_N+2", "dry_gap_2N+3"]
    if s > 1:
        branches += ["refreeze_mid_stride", "period_lt_s"]
    if g.M == g.laps + 1:   # width 1: every slot is in mid-read, whatever iindex is
        branches += ["midread"]
    return n, ev, [], [], branches


def stale(g):
    """A freeze at t < s, an unfreeze while dry, freeze / unfreeze / freeze on one sample, then
    periods whose draws reach the stale DFrame excluded - 1; one freeze and one unfreeze arrive as
    `at == n` of a call."""
    N, s, S = g.N, g.s, g.S
    t1, t2 = 2 * S + s, 4 * S + 2 * s
    # k strides more of the period at t2 bring the draws before t4 to M - 2 (mod M): the first draw
    # at t4 then hands its frame to the slot one stride into its read, at any width
    draws = -(-(S + 3) // s) - (-(S + s // 2 + 1) // s) - (-(2 * S + 1) // s)
    k = (g.M - 2 - draws) % g.M
    while (2 * S + 1 + k * s) % (N + 1) == 0:             # (a length that leaves the Delay ring in step)
        k += g.M
    t3 = t2 + 2 * S + 1 + k * s
    t4 = t3 + N + S
    ev = [
        (s - 1, F), (S + s + 2, U),                       # t < s (t = 0 where s = 1): a zero period
        (S + s + 3, U),                                   # unfreeze while dry
        (t1, F), (t1, U), (t1, F),                        # one sample: an empty period, then a new one; phase s
        (t1 + S + s // 2 + 1, U),
        (t2, F),                                          # phase 2 s; delivered as at == n
        (t3, U),                                          # delivered as at == n
        (t4, F), (t4 + S + 3, U),
    ]
    n = t4 + S + 3 + N + 2
    branches = ["freeze_before_first_process", "zero_period", "unfreeze_while_dry", "freeze_unfreeze_freeze",
                "stale_after_second_freeze", "freeze_at_n", "unfreeze_at_n", "midread"]
    if g.M <= 10:   # (at M = 42 two slots of 42 are live: a draw of a live slot's frame is left to chance)
        branches += ["reread"]
    return n, ev, [t2, t3], [t2, t3], branches


def m3_sequence(g):
    """M = 3: `excluded` decides every draw.  Freezes with excluded 0, 2, 1, 0, every dry gap longer
    than S: the periods play zeros (stale, never written), a fresh frame, and twice the frame of
    the freeze before (stale)."""
    s, S = g.s, g.S
    ev = [
        (2 * S + 3, F), (4 * S + 8, U),                   # excluded 0
        (6 * S - 3, F), (7 * S + 13, U),                  # excluded 2
        (9 * S + s + 2, F), (11 * S + 12, U),             # excluded 1
        (13 * S + 1, F), (14 * S + 22, U),                # excluded 0
    ]
    return 15 * S + 20, ev, [], [], ["m3_sequence", "zero_period", "stale_after_second_freeze"]


TEMPLATES = {"edges": edges, "stale": stale, "m3": m3_sequence}
# seeds: input noise and srand.  A seed that misses a branch of its case is changed here.
SEEDS = {
    ("edges", 4): 11, ("edges", 8): 12, ("edges", 16, 9): 13, ("edges", 16, 2): 14, ("edges", 64): 15,
    ("edges", 256): 16, ("edges", 2048): 17, ("edges", 4096): 18, ("edges", 8192): 19,
    ("stale", 4): 21, ("stale", 8): 22, ("stale", 16, 9): 23, ("stale", 16, 2): 24, ("stale", 64): 25,
    ("stale", 256): 26, ("stale", 2048): 27, ("stale", 4096): 28, ("stale", 8192): 29,
    ("m3", 16, 2): 31,
}


def _case(template, geo):
    g = geometry(*geo)
    n, ev, cuts, at_n, branches = TEMPLATES[template](g)
    key = (template, g.N) if (template, g.N) in SEEDS else (template, g.N, g.laps)
    return Case(f"{template}-{g.N}-{g.laps}-{g.width:g}", g, SEEDS[key], n, ev, cuts, at_n, branches)


CASES = [_case(t, geo) for t in ("edges", "stale") for geo in GEOMETRIES] + [_case("m3", (16, 2, 1.0))]
CASE_IDS = [c.name for c in CASES]


def noise(case):
    return np.random.default_rng(case.seed).standard_normal(case.n)


# ---- call structures ------------------------------------------------------------------------------
def blocks(n, events, cuts, at_n=()):
    """the schedule as calls cut at `cuts`: [(length, events relative to the call)].  Events on a
    cut listed in at_n go to the earlier call as at == n, the others to the later one as at == 0."""
    edges_ = [0] + sorted(c for c in set(cuts) if 0 < c < n) + [n]
    out = []
    for a, b in zip(edges_[:-1], edges_[1:]):
        ev = [(t - a, k) for t, k in events if (a < t < b) or (t == a and (a == 0 or a not in at_n))
              or (t == b and b in at_n and b < n)]
        out.append((b - a, ev))
    return out


def event_cuts(n, events):
    """cuts at every event and one sample either side of it (1-sample calls around each event)"""
    return sorted({c for t, _ in events for c in (t - 1, t, t + 1) if 0 < c < n})


# ---- chunk splits (HZ_FRZ_CHUNK = 4096) -----------------------------------------------------------
CHUNK = 4096
CHUNK_GEOMETRIES = [(256, 4, 1.0), (2048, 8, 1.0), (8192, 4, 1.0)]   # at 8192 the chunk is shorter than N


def chunk_schedule(g):
    """Ten chunks.  Chunk boundaries fall on a populate sample (2 C, s after the freeze), inside a
    period opened two chunks earlier (3 C), on an unfreeze (4 C) and a freeze (5 C), one sample
    after an unfreeze and before a freeze (6 C), before an unfreeze and after a freeze (7 C .. 8 C),
    and in front of an unfreeze followed by a freeze in one chunk while a period is open (8 C)."""
    s, C = g.s, CHUNK
    ev = [
        (2 * C - s, F), (4 * C, U),
        (5 * C, F), (6 * C - 1, U),
        (6 * C + 1, F), (7 * C + 1, U),
        (8 * C - 1, F), (8 * C + s // 2 + 3, U), (8 * C + s + 7, F),
        (10 * C - 5, U),
    ]
    return 10 * C + 77, ev


def chunk_case(geo):
    g = geometry(*geo)
    n, ev = chunk_schedule(g)
    return Case(f"chunk-{g.N}-{g.laps}", g, 40 + g.laps + g.N % 7, n, ev, [], [], [])


CHUNK_CASES = [chunk_case(geo) for geo in CHUNK_GEOMETRIES]
