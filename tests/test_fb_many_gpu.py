"""GPU tests of hz_fb_process_many / hz_fb_process_many_device: block calls over several Filterbanks
in one launch sequence.  Per member the call gives what its own hz_fb_process_device call gives, so
every case is checked against the CPU restatement per channel (TOL of test_filterbank_gpu.py), or,
where both routes plan the same time segments (hz_fb_set_target_groups(h, 1)), bit for bit against
the per-handle loop on twin handles.  hz_fb_many_info tells which members a call batched."""
import ctypes as C

import numpy as np
import pytest

from golden.spec_numpy import resonant_coefficients, white_noise_f32
from oracle import OracleFilterbank, rel_err
from test_filterbank_gpu import TOL

pytestmark = pytest.mark.gpu

NONE, SOFTCLIP, SATURATE, LIMITER = 0, 1, 2, 3   # HZ_DIST_*
HZ_E_INVALID = -1


def coefficients(order, N, seed):
    """order 2: the resonant recipe with a per-seed radius and centre; else random stable banks
    (test_filterbank_rt_gpu.pair)"""
    if order == 2:
        return resonant_coefficients(N, 0.999 - 0.002 * (seed % 5), 0.5 - 0.05 * (seed % 3))
    rng = np.random.default_rng(seed)
    fwd = rng.uniform(-1, 1, (N, order + 1))
    back = (np.array([np.poly(rng.uniform(-0.9, 0.9, order))[1:] for _ in range(N)]).reshape(N, order)
            if order else np.zeros((N, 0)))
    return fwd, back


def bank(order, N, seed, dist=NONE, param=None, oracle=False, waves=0, groups=None, kg=0.3):
    """one channel: its own coefficients, targets and k_p -> the handle, or (handle, restatement)"""
    from huygens_amd import Filterbank
    fwd, back = coefficients(order, N, seed)
    rng = np.random.default_rng(1000 + seed)
    kp = 0.02 + 0.01 * (seed % 7)
    fbs = [Filterbank(order, N, kp, kg)] + ([OracleFilterbank(order, N, kp, kg)] if oracle else [])
    pin, gin = rng.uniform(0.5, 1.5, N), rng.uniform(0.2, 1.0, N)
    for fb in fbs:
        for n in range(N):
            fb.coefficients(n, fwd[n], back[n])
        fb.boost(pin)
        fb.mix(gin)
        fb.distortion(dist, param)
    if waves:
        fbs[0].tune(waves, 1)
    if groups:
        fbs[0].set_target_groups(groups)
    return tuple(fbs) if oracle else fbs[0]


def many_device(gs, X, in_pad=0, out_pad=0, sentinel=None):
    """process_many_device on device copies of the rows of X -> (C, n) outputs (and the padded
    output buffer when a sentinel is given)"""
    import torch
    from huygens_amd import process_many_device
    c, n = X.shape
    xt = torch.zeros((c, n + in_pad), dtype=torch.float64, device="cuda")
    xt[:, :n] = torch.from_numpy(np.ascontiguousarray(X))
    yt = torch.full((c, n + out_pad), 0.0 if sentinel is None else sentinel, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    process_many_device(gs, xt.data_ptr(), n + in_pad, yt.data_ptr(), n + out_pad, n)
    for g in gs:
        g.synchronize()
    torch.cuda.synchronize()
    full = yt.cpu().numpy()
    return full[:, :n].copy() if sentinel is None else (full[:, :n].copy(), full)


def loop_device(gs, X):
    """the per-handle loop on device buffers"""
    import torch
    c, n = X.shape
    xt = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    yt = torch.zeros_like(xt)
    torch.cuda.synchronize()
    for j, g in enumerate(gs):
        g.process_device(xt[j].data_ptr(), yt[j].data_ptr(), n)
    for g in gs:
        g.synchronize()
    return yt.cpu().numpy()


def noise(c, n, seed):
    return np.stack([white_noise_f32(n, seed=seed + j).astype(np.float64) for j in range(c)])


# ---- 1. parity per channel ------------------------------------------------------------------

@pytest.mark.parametrize("dist", [NONE, SOFTCLIP])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1023, 1024, 1025, 2500])
def test_parity_per_channel(gpu_lib, n, dist):
    """C = 3, order 2, N = 37 / 5 / 130 (no multiple of the wave count), distinct coefficients,
    targets, k_p and starting points (a warm-up call of another length per channel).  At the default
    geometry the 5-band channel runs 4-wave workgroups and the other two 16-wave ones: those two
    are the batch and the small one runs by itself."""
    Ns = (37, 5, 130)
    pairs = [bank(2, N, seed=j, dist=dist, param=0.125 if dist else None, oracle=True) for j, N in enumerate(Ns)]
    for j, (g, o) in enumerate(pairs):
        w = white_noise_f32(50 + 13 * j, seed=90 + j)
        assert rel_err(g.process(w), o.process(w)) <= TOL
    X = noise(3, n, seed=5)
    Y = many_device([g for g, _ in pairs], X)
    for j, (g, o) in enumerate(pairs):
        err = rel_err(Y[j], o.process(X[j]))
        print(f"n={n} dist={dist} channel {j} (N={Ns[j]}): rel err {err:.3e}")
        assert err <= TOL, (j, err)
        assert g.many_info() == ((0, 1) if j == 1 else (1, 0)), (j, g.many_info())


# ---- 2. same bits as the loop -----------------------------------------------------------------

@pytest.mark.parametrize("waves", [4, 8, 16])
@pytest.mark.parametrize("dist", [NONE, SOFTCLIP, SATURATE, LIMITER])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_same_bits_as_the_loop(gpu_lib, order, dist, waves):
    """one segment on both routes (target groups 1): outputs and states bit for bit; every member
    batched.  The functor's parameter differs per channel."""
    def build():
        return [bank(order, 37, seed=10 * order + j, dist=dist, param=0.125 * (j + 1), waves=waves, groups=1)
                for j in range(3)]
    gs, tw = build(), build()
    X = noise(3, 1500, seed=20 + order)
    Y, Yl = many_device(gs, X), loop_device(tw, X)
    assert np.array_equal(Y, Yl)
    for g, t in zip(gs, tw):
        assert np.array_equal(g.get_state(), t.get_state())
        assert g.many_info() == (1, 0)
        assert t.many_info() == (0, 0)


# ---- 3. segments ------------------------------------------------------------------------------

def test_segments(gpu_lib):
    """C = 2, N = 7, n = 9000 with 4096 groups wanted: the batch cuts time into segments and runs
    its pre-pass and carry once for both members"""
    def build(oracle):
        return [bank(2, 7, seed=40 + j, dist=SOFTCLIP, param=0.125, oracle=oracle, groups=4096) for j in range(2)]
    pairs, tw = build(True), build(False)
    gs = [g for g, _ in pairs]
    gs[0].profile(True)
    X = noise(2, 9000, seed=41)
    Y, Yl = many_device(gs, X), loop_device(tw, X)
    seg_ms, mix_ms, red_ms, launches = gs[0].profile_read()
    print(f"segments: pre-pass {seg_ms:.4f} ms, mix {mix_ms:.4f} ms, reduce {red_ms:.4f} ms, launches {launches}")
    assert launches == 1 and seg_ms > 0.0
    for j, (g, o) in enumerate(pairs):
        err, err_loop = rel_err(Y[j], o.process(X[j])), rel_err(Y[j], Yl[j])
        print(f"segments channel {j}: rel err {err:.3e} (restatement), {err_loop:.3e} (loop)")
        assert err <= TOL and err_loop <= TOL
        assert g.many_info() == (1, 0)


# ---- 4. members that run by themselves ---------------------------------------------------------

def odd_member(kind):
    from huygens_amd import Filterbank
    if kind == "order":
        return bank(3, 37, seed=77, dist=SOFTCLIP, param=0.125, groups=1)
    if kind == "dist":
        return bank(2, 37, seed=77, dist=SATURATE, groups=1)
    if kind == "bands_per_wave":
        g = bank(2, 37, seed=77, dist=SOFTCLIP, param=0.125, groups=1)
        g.tune(4, 2)
        return g
    if kind == "converged":   # no functor, the smoothers at their targets: the LTI or streaming engine
        fwd, back = resonant_coefficients(37, 0.99, 0.5)
        g = Filterbank(2, 37, 0.001, 0.001)   # (k in seconds: 2^-60 of the targets after ~60 samples)
        for n in range(37):
            g.coefficients(n, fwd[n], back[n])
        g.boost(np.ones(37))
        g.open()
        g.set_target_groups(1)
        g.process(white_noise_f32(4096, seed=78))
        return g
    g = bank(2, 37, seed=77, dist=SOFTCLIP, param=0.125, groups=1)   # "cached": operator() without tick()
    g(0.25)
    return g


@pytest.mark.parametrize("kind", ["order", "dist", "bands_per_wave", "converged", "cached"])
def test_members_that_run_by_themselves(gpu_lib, kind):
    from huygens_amd import _lib as L
    def build():
        gs = [bank(2, 37, seed=60 + j, dist=SOFTCLIP, param=0.125, groups=1) for j in range(3)]
        gs.insert(1, odd_member(kind))
        return gs
    gs, tw = build(), build()
    X = noise(4, 1500, seed=61)
    Y, Yl = many_device(gs, X), loop_device(tw, X)
    assert np.array_equal(Y, Yl)
    if kind == "converged":
        assert gs[1].last_path() in (L.HZ_FB_PATH_LTI, L.HZ_FB_PATH_STREAM), gs[1].last_path()
        assert tw[1].last_path() == gs[1].last_path()
    for j, (g, t) in enumerate(zip(gs, tw)):
        assert np.array_equal(g.get_state(), t.get_state()), j
        assert g.many_info() == ((0, 1) if j == 1 else (1, 0)), (j, g.many_info())


# ---- 5. continuity ----------------------------------------------------------------------------

def test_continuity(gpu_lib):
    """five process_many calls of 256 samples with boost / mix on one channel between them, then
    per-handle process, then operator() / tick() on each: the whole run against the restatement"""
    from huygens_amd import process_many
    Ns = (37, 5, 130)
    pairs = [bank(2, N, seed=30 + j, dist=SOFTCLIP, param=0.125, oracle=True, waves=8) for j, N in enumerate(Ns)]
    gs = [g for g, _ in pairs]
    got, ref = [[] for _ in pairs], [[] for _ in pairs]
    for call in range(5):
        X = noise(3, 256, seed=300 + 3 * call)
        Y = process_many(gs, X)
        for j, (g, o) in enumerate(pairs):
            got[j].append(Y[j])
            ref[j].append(o.process(X[j]))
        for fb in pairs[1]:
            fb.boost(call % 5, 0.3 + 0.2 * call)
            fb.mix((call + 2) % 5, 1.0 - 0.15 * call)
    for j, (g, o) in enumerate(pairs):
        x = white_noise_f32(300, seed=400 + j)
        got[j].append(g.process(x))
        ref[j].append(o.process(x))
        x = white_noise_f32(20, seed=410 + j)
        for fb, dst in ((g, got[j]), (o, ref[j])):
            ys = []
            for v in x:
                ys.append(fb(float(v)))
                fb.tick()
            dst.append(np.array(ys))
        err = rel_err(np.concatenate(got[j]), np.concatenate(ref[j]))
        print(f"continuity channel {j}: rel err {err:.3e}")
        assert err <= TOL, (j, err)
        assert g.many_info() == (5, 0)


# ---- 6. streams -------------------------------------------------------------------------------

def test_streams(gpu_lib):
    """every handle on a torch stream of its own; process_many_device and per-handle process_device
    alternate for 6 rounds of 512 samples with no host synchronisation until the end, and give the
    bits of the same calls synchronised one by one"""
    import torch
    from huygens_amd import process_many_device
    C_, n, rounds = 3, 512, 6
    X = noise(C_, n * rounds, seed=50)

    def run(sync):
        gs = [bank(2, (37, 5, 130)[j], seed=50 + j, dist=SOFTCLIP, param=0.125, waves=8, groups=1) for j in range(C_)]
        streams = [torch.cuda.Stream() for _ in gs]
        for g, s in zip(gs, streams):
            g.set_stream(s.cuda_stream)
        xt = torch.from_numpy(X).cuda()
        yt = torch.zeros_like(xt)
        torch.cuda.synchronize()
        w = 8 * X.shape[1]   # bytes per row
        for r in range(rounds):
            off = 8 * n * r
            if r % 2 == 0:
                process_many_device(gs, xt.data_ptr() + off, X.shape[1], yt.data_ptr() + off, X.shape[1], n)
            else:
                for j, g in enumerate(gs):
                    g.process_device(xt.data_ptr() + j * w + off, yt.data_ptr() + j * w + off, n)
            if sync:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        out, states = yt.cpu().numpy(), [g.get_state() for g in gs]
        infos = [g.many_info() for g in gs]
        for g in gs:
            g.close()
        return out, states, infos

    free, free_states, infos = run(False)
    ref, ref_states, _ = run(True)
    assert infos == [(rounds // 2, 0)] * C_, infos
    assert np.array_equal(free, ref)
    for a, b in zip(free_states, ref_states):
        assert np.array_equal(a, b)


# ---- 7. the program's shape --------------------------------------------------------------------

def test_program_shape(gpu_lib):
    """tests/filterbanks.cpp: 8 channels x 864 bands, order 2, &softclip, the banks built as
    test_rt_server_gpu.py::test_sample_many_multichannel builds them; four 1024-sample callbacks with
    a note on and a note off (9 bands x boost + mix on every channel) between them.  That test
    bounds a block call on this recipe by 1e-8 of the output's peak (the recipe's last band sits on
    Nyquist: test_filterbank_gpu.py TOL_STIFF's note); the same bound here.  One launch per call on
    handles[0]'s profile; the per-handle loop on twins records one per handle per call."""
    from huygens_amd import Filterbank
    H, N, n = 8, 864, 1024
    fwd, back = resonant_coefficients(N, 0.999, 1.0)

    def build(oracle):
        out = []
        for k in range(H):
            fbs = [Filterbank(2, N)] + ([OracleFilterbank(2, N)] if oracle else [])
            for fb in fbs:
                for b in range(N):
                    fb.coefficients(b, fwd[b], back[b])
                fb.boost(np.full(N, 1.0 + 0.1 * k))
                fb.open()
                fb.distortion(SOFTCLIP, None)
            out.append(tuple(fbs) if oracle else fbs[0])
        return out

    pairs, tw = build(True), build(False)
    gs = [g for g, _ in pairs]
    gs[0].profile(True)
    for t in tw:
        t.profile(True)
    note = range(9 * 31, 9 * 32)
    for call in range(4):
        X = noise(H, n, seed=700 + 8 * call)
        Y, Yl = many_device(gs, X), loop_device(tw, X)
        for k, (g, o) in enumerate(pairs):
            yo = o.process(X[k])
            peak = np.max(np.abs(yo))
            assert np.max(np.abs(Y[k] - yo)) <= 1e-8 * peak, (call, k)
            assert np.max(np.abs(Y[k] - Yl[k])) <= 1e-8 * peak, (call, k)
        if call in (0, 2):   # note on after the first callback, note off after the third
            on = call == 0
            for k in range(H):
                for fb in (*pairs[k], tw[k]):
                    for b in note:
                        fb.boost(b, 1.0 if on else 0.0)
                        fb.mix(b, 2.0 if on else 0.0)
    assert gs[0].profile_read()[3] == 4
    for g, t in zip(gs, tw):
        assert g.many_info() == (4, 0)
        assert t.profile_read()[3] == 4


# ---- 8. host buffers ---------------------------------------------------------------------------

def test_host_buffer_call(gpu_lib):
    """hz_fb_process_many equals the device call bit for bit; with strides larger than n both leave
    the gaps between the rows untouched (sentinel)"""
    from huygens_amd._lib import PD, check
    def build():
        return [bank(2, (37, 5, 130)[j], seed=80 + j, dist=SOFTCLIP, param=0.125, groups=1) for j in range(3)]
    gs, tw = build(), build()
    n, ip, op, sent = 700, 7, 5, -12345.5
    X = noise(3, n, seed=81)
    Yd, full = many_device(tw, X, in_pad=ip, out_pad=op, sentinel=sent)
    assert np.all(full[:, n:] == sent)
    xin = np.full((3, n + ip), 9.0)
    xin[:, :n] = X
    out = np.full((3, n + op), sent)
    hs = (C.c_void_p * 3)(*[g._h for g in gs])
    check(gpu_lib.hz_fb_process_many(hs, 3, xin.ctypes.data_as(PD), n + ip, out.ctypes.data_as(PD), n + op, n))
    assert np.all(out[:, n:] == sent)
    assert np.array_equal(out[:, :n], Yd)
    for g, t in zip(gs, tw):
        assert np.array_equal(g.get_state(), t.get_state())


# ---- 9. errors ----------------------------------------------------------------------------------

def test_errors(gpu_lib):
    import torch
    gs = [bank(2, 37, seed=95 + j) for j in range(3)]
    for g in gs:
        g.process(white_noise_f32(64, seed=96))
    before = [g.get_state() for g in gs]
    n = 256
    xt = torch.zeros((3, n), dtype=torch.float64, device="cuda")
    yt = torch.zeros_like(xt)
    torch.cuda.synchronize()
    x, y = C.c_void_p(xt.data_ptr()), C.c_void_p(yt.data_ptr())
    call = gpu_lib.hz_fb_process_many_device
    hs = (C.c_void_p * 3)(*[g._h for g in gs])
    null = (C.c_void_p * 3)(gs[0]._h, None, gs[2]._h)
    twice = (C.c_void_p * 3)(gs[0]._h, gs[1]._h, gs[0]._h)
    assert call(null, 3, x, n, y, n, n) == HZ_E_INVALID
    assert b"null" in gpu_lib.hz_last_error()
    assert call(twice, 3, x, n, y, n, n) == HZ_E_INVALID
    assert b"twice" in gpu_lib.hz_last_error()
    assert call(hs, 3, x, n - 1, y, n, n) == HZ_E_INVALID
    assert b"stride" in gpu_lib.hz_last_error()
    assert call(hs, 3, x, n, y, n - 1, n) == HZ_E_INVALID
    assert b"overlap" in gpu_lib.hz_last_error()
    assert call(hs, 3, None, n, y, n, n) == HZ_E_INVALID
    assert call(hs, 257, x, n, y, n, n) == HZ_E_INVALID
    assert call(hs, 0, x, n, y, n, n) == 0
    assert call(hs, 3, x, n, y, n, 0) == 0
    xh, yh = np.zeros((3, n)), np.zeros((3, n))
    host = gpu_lib.hz_fb_process_many
    from huygens_amd._lib import PD
    assert host(twice, 3, xh.ctypes.data_as(PD), n, yh.ctypes.data_as(PD), n, n) == HZ_E_INVALID
    assert host(hs, 0, xh.ctypes.data_as(PD), n, yh.ctypes.data_as(PD), n, n) == 0
    for g, b in zip(gs, before):
        assert np.array_equal(g.get_state(), b)
        assert g.many_info() == (0, 0)
