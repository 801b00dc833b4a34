"""numpy model of the Bowl<float> kernels' arithmetic (huygens_amd/csrc/hz_bowl.hip), element for
element, and a restatement of bowl_launch's plan.  TEST INFRASTRUCTURE; numpy only.

What is modelled, per mode i and sample t of one call that starts at counter n0:
  counter   ph = float32(min(n0 + t, 2^24))                                   (phase_f)
  phase     p  = float32(f_i * ph) / float32(48000): numpy's float32 divide is the correctly
               rounded quotient that div_sr produces
  wave      float32(sin2pi_ref(p)): the kernel's folding and polynomial with its constants, in
               float64 (numpy has no fma: the Horner steps and y = kE p + u round once more than
               the kernel's, a few 1e-17)
  decay     a_i * exp(float64(x0)) stepped j times by rstep_i, x0 = float32(-d_i * ph0) / 48000 at
               the first sample ph0 of the sample's chunk, j its place in the chunk;
               rstep_i = exp(-float32(d_i) / 48000) from long double (build_brec)
  stuck     a sample whose counter is 2^24 takes a_i * exp(float64(x(2^24))) * wave(2^24) with no
               seed and no stepping (stuck_sum, worked out on the host at creation and stored over
               the kernels' samples); stuck=False is the kernels' arithmetic alone: the stepped
               decay goes on falling inside a chunk and jumps back at the next seed
  sum       the modes' terms in float64, rounded to float32 once

chunk = 16: bowl_mix_kernel (fill, fill_device).  mix_plan's segments are whole 1024-sample
tiles, so every chunk starts a multiple of 16 from the call's first sample.
chunk = 4: bowl_dly_chain_kernel (fill_delaybank).  A workgroup's first sample is 4 blockIdx.x
from the block's first.

The only library call that differs between device and host is exp (last bits of a double), so a
kernel sample is the model's or a float32 neighbour of it (the stuck value is the host's exp).
"""
import numpy as np

SR = 48000
STUCK = 2 ** 24
K_E = 6.58338396844303045e-14   # sin2pi_ref's kE: PI / pi - 1 for the double PI = 3.14159265359, from 50 digits
_POLY = (-14.337175761608114, 42.000013938078347, -76.703669216302146, 81.605209465741268,
         -41.341701930121658, 6.2831853064884768)
_SRF = np.float32(SR)

# ---- bowl_launch's plan ---------------------------------------------------------------------------
K_WAVES = 8            # hz_mix.h
K_MAX_PER_WAVE = 64    # hz_mix.h
K_L = 16               # hz_bowl.hip
TILE = 64 * K_L
SHORT_SLICES = 16      # bowl_reduce_short_kernel
SHORT_MAX = 16384
CHAIN_SPW = 4          # bowl_dly_chain_kernel
CHAIN_THREADS = 512
CHAIN_PRE = 4


def mix_plan(groups, n, tile, target_groups):
    """hz::mix_plan (hz_mixplan.h) -> dict(ntiles, nseg, seg_tiles, n_pad, seg_len)"""
    ntiles = (n + tile - 1) // tile
    nseg = max(1, min(ntiles, (target_groups + groups - 1) // groups))
    seg_tiles = (ntiles + nseg - 1) // nseg
    nseg = (ntiles + seg_tiles - 1) // seg_tiles
    return dict(ntiles=ntiles, nseg=nseg, seg_tiles=seg_tiles, n_pad=ntiles * tile, seg_len=seg_tiles * tile)


def bowl_plan(M, n, target_groups):
    """bowl_launch: modes per wave, workgroups of modes, time segments and which reduce runs"""
    ntiles = (n + TILE - 1) // TILE
    per_wave = min(K_MAX_PER_WAVE, max(1, (M + K_WAVES * 32 - 1) // (K_WAVES * 32)))
    par = M * ntiles // (K_WAVES * 2 * target_groups)
    if par < per_wave:
        per_wave = max(1, par)
    G = max(1, (M + K_WAVES * per_wave - 1) // (K_WAVES * per_wave))
    p = mix_plan(G, n, TILE, target_groups)
    p.update(per_wave=per_wave, G=G, reduce="short" if n <= SHORT_MAX else "slab")
    return p


def wave_of(plan, i):
    """mode i -> (workgroup, wave, place in the wave)"""
    w, q = divmod(i, plan["per_wave"])
    return w // K_WAVES, w % K_WAVES, q


def short_reduce_passes(G):
    """bowl_reduce_short_kernel: (workgroups summed by the 8-wide unrolled pass, by the tail pass),
    each a sorted list.  Slice ty takes g = ty, ty + 16, ...; the unrolled pass runs while
    g + 7 * 16 < G and takes g, g + 16, ..., g + 112."""
    unrolled, tail = [], []
    for ty in range(SHORT_SLICES):
        g = ty
        while g + 7 * SHORT_SLICES < G:
            unrolled += [g + u * SHORT_SLICES for u in range(8)]
            g += 8 * SHORT_SLICES
        tail += list(range(g, G, SHORT_SLICES))
    return sorted(unrolled), sorted(tail)


def hot_modes(M, n, target_groups):
    """The modes whose place in the plan of a call of n samples is an edge: first / last mode of
    the first wave, of a workgroup, of the bank; the last, partly filled wave; the first and last
    workgroup of either pass of the short reduce.  -> sorted list of distinct indices"""
    p = bowl_plan(M, n, target_groups)
    pw, G = p["per_wave"], p["G"]
    per_group = K_WAVES * pw
    hot = {0, pw - 1, pw, per_group - 1, per_group, M - 1}           # wave 0 | 1, workgroup 0 | 1
    hot |= {((M - 1) // pw) * pw, (G - 1) * per_group}               # last wave's, last workgroup's first
    if p["reduce"] == "short":
        for groups in short_reduce_passes(G):
            for g in groups[:1] + groups[-1:]:
                hot |= {g * per_group, min(M, (g + 1) * per_group) - 1}
    return sorted(i for i in hot if 0 <= i < M)


def chain_slot(i):
    """bowl_dly_chain_kernel: mode i -> (pass of the mode loop, table entry u, thread)"""
    ps, r = divmod(i, CHAIN_PRE * CHAIN_THREADS)
    return ps, r // CHAIN_THREADS, r % CHAIN_THREADS


# ---- the arithmetic -------------------------------------------------------------------------------

def counter(n0, n):
    """the float phase counter of n samples from n0 (phase_f): sticks at 2^24"""
    return np.minimum(float(n0) + np.arange(n, dtype=np.float64), float(STUCK)).astype(np.float32)


def advance(n0, n):
    return min(n0 + n, STUCK)


def sin2pi_ref(p):
    """sin2pi_ref of hz_bowl.hip for float32 p >= 0 -> float64"""
    p = np.asarray(p, dtype=np.float32)
    u = p - np.floor(p)                                        # [0, 1), exact
    u = np.where(u >= np.float32(0.5), u - np.float32(1), u)   # [-1/2, 1/2), exact
    refl = np.abs(u) > np.float32(0.25)
    u = np.where(refl, np.copysign(np.float32(0.5), u) - u, u).astype(np.float32)
    y = np.where(refl, -K_E, K_E) * p.astype(np.float64) + u.astype(np.float64)
    z = y * y
    s = np.full_like(z, _POLY[0])
    for c in _POLY[1:]:
        s = s * z + c
    return y * s


def rstep(d):
    """build_brec's per-sample decay factor for a float Bowl (BRec::R)"""
    d32 = np.asarray(d, dtype=np.float64).astype(np.float32)
    return np.exp(-d32.astype(np.longdouble) / np.longdouble(SR)).astype(np.float64)


def wave_f(f32, ph, exact_product=False):
    """float32 wave values [M][n] of float32 frequencies at the counters ph.  exact_product: p from
    the unrounded product f ph (a mutant)"""
    if exact_product:
        p = (f32.astype(np.float64)[:, None] * ph.astype(np.float64)[None, :] / SR).astype(np.float32)
    else:
        p = (f32[:, None] * ph[None, :]) / _SRF
    return sin2pi_ref(p).astype(np.float32)


def _decay(a32, d32, rs, ph, chunk, seed_shift=0):
    """[M][n] float64: a exp(float64(x0)) at each chunk's first sample, times rstep once per place
    in the chunk, multiplied up one step at a time as the kernels do.  seed_shift: take the seed of
    the chunk `seed_shift` further on (a mutant)"""
    n = len(ph)
    nch = (n + chunk - 1) // chunk
    # seeds of padded chunks repeat the last sample's counter; they are cut off again below
    first = np.minimum((np.arange(nch) + seed_shift) * chunk, n - 1)
    x0 = (-d32[:, None] * ph[first][None, :]) / _SRF
    cur = a32.astype(np.float64)[:, None] * np.exp(x0.astype(np.float64))
    out = np.empty((len(a32), nch, chunk))
    for j in range(chunk):
        out[:, :, j] = cur
        cur = cur * rs[:, None]
    return out.reshape(len(a32), nch * chunk)[:, :n]


def model_terms(f, a, d, n0, n, chunk, stuck=True, seed_shift=0, exact_product=False):
    """one call of n samples from counter n0 -> the modes' terms, float64 [M][n]"""
    f32, a32, d32 = (np.asarray(v, dtype=np.float64).astype(np.float32) for v in (f, a, d))
    ph = counter(n0, n)
    wv = wave_f(f32, ph, exact_product)
    terms = _decay(a32, d32, rstep(d32), ph, chunk, seed_shift) * wv.astype(np.float64)
    if stuck and ph[-1] == np.float32(STUCK):
        at = ph == np.float32(STUCK)
        xs = (-d32 * np.float32(STUCK)) / _SRF
        s = a32.astype(np.float64) * np.exp(xs.astype(np.float64)) * wv[:, -1].astype(np.float64)
        terms[:, at] = s[:, None]
    return terms


def model_fill(f, a, d, calls, chunk, n0=0, modes=256, **kw):
    """consecutive calls of the given lengths from counter n0 -> float32 samples, concatenated.
    The mode sum is kept in float64 (in blocks of `modes` modes, which bounds the memory) and
    rounded once."""
    f, a, d = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (f, a, d))
    out = []
    for n in calls:
        acc = np.zeros(n)
        for m0 in range(0, len(f), modes):
            sl = slice(m0, m0 + modes)
            acc += model_terms(f[sl], a[sl], d[sl], n0, n, chunk, **kw).sum(axis=0)
        out.append(acc.astype(np.float32))
        n0 = advance(n0, n)
    return np.concatenate(out)


# ---- the two comparisons of the GPU cases ---------------------------------------------------------
PER_MODE = 3e-7   # |y - reference| <= PER_MODE * a_i, derived in tests/test_bowl_float_model_cpu.py


def per_mode_error(y, ref, a_i):
    """(a): max |y - ref| / a_i, with a_i the hot mode's float amplitude"""
    a32 = float(np.float32(a_i))
    return float(np.max(np.abs(np.asarray(y, dtype=np.float64) - np.asarray(ref, dtype=np.float64)))) / a32


def spacing_error(y, model, slack=0.0):
    """(b): max of |y - model| / (np.spacing(|model|) + slack), and the share of bit-identical
    samples.  <= 1 means: never further than one float32 spacing (plus slack) from the model"""
    y, model = np.asarray(y, dtype=np.float32), np.asarray(model, dtype=np.float32)
    dlt = np.abs(y.astype(np.float64) - model.astype(np.float64))
    room = np.spacing(np.abs(model)).astype(np.float64) + slack
    return float(np.max(dlt / room)), float(np.mean(y == model))
