"""GPU parity of hz_fb_process_events: boost / mix setters at sample positions inside ONE block
call (the general engine's event form, hz_filterbank.hip fb_mix_kernel<.., EV>) against the oracle
driven through the same events as setter calls between process() pieces
(fb_events_model.run_events_split).  The bound is the project's own: TOL = 1e-9 norm-wise
(oracle.rel_err), TOL_STIFF = 1e-7 only for the Nyquist-pole fixture, as in test_filterbank_gpu.py
-- the event form keeps the same closed form per segment, so nothing looser is justified."""
import numpy as np
import pytest

from fb_events_model import EV_BOOST, EV_MIX, positions_events, run_events_split
from golden.spec_numpy import resonant_coefficients, white_noise_f32
from oracle import OracleFilterbank, golden_names, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-9
TOL_STIFF = 1e-7
STIFF = {"fb_o2_n16_r0999"}


def make_pair(order, N, fwd, back, kp=0.1, kg=1.0, boost=True, opened=True, shard=None):
    from huygens_amd import Filterbank
    g = Filterbank(order, N, kp, kg, shard=shard)
    o = OracleFilterbank(order, N, kp, kg)
    for fb in (g, o):
        for n in range(N):
            fb.coefficients(n, fwd[n], back[n])
        if boost:
            fb.boost(np.ones(N))
        if opened:
            fb.open()
    return g, o


def random_poles(rng, order, N, radius=0.97):
    """the test_orders_random recipe: conjugate pole pairs (+ one real pole for odd orders)"""
    fwd = rng.uniform(-1, 1, (N, order + 1))
    back = np.zeros((N, max(order, 1)))
    for n in range(N):
        roots = []
        for _ in range(order // 2):
            p = radius * np.exp(1j * rng.uniform(0, np.pi))
            roots += [p, np.conj(p)]
        if order % 2 == 1:
            roots.append(radius * rng.uniform(-1, 1))
        if order:
            back[n, :order] = np.real(np.poly(roots))[1:]
    return fwd, back[:, :order]


def random_events(rng, count, N, n, extra_at=()):
    at = np.sort(np.concatenate([rng.integers(0, n + 1, count), np.asarray(extra_at, dtype=np.int64)]))
    return [(int(t), int(rng.integers(-1, N)), int(rng.integers(0, 2)), float(rng.uniform(0.0, 2.0))) for t in at]


def check_call(g, o, x, events, tol=TOL):
    y = g.process_events(x, events)
    ref = run_events_split(o, x, events)
    err = rel_err(y, ref)
    assert err < tol, err
    return y


def check_state(g, o):
    sg, so = g.get_state(), o.get_state()
    assert rel_err(sg, so) < TOL, rel_err(sg, so)
    N, O = o.N, o.order
    assert rel_err(sg[-2 * N:], so[-2 * N:]) < TOL   # pre, gain on their own scale
    if O:
        assert rel_err(sg[:O], so[:O]) < TOL


def golden_events(g):
    ev = []
    for t, idx in sorted(zip(g["sched_t"].tolist(), range(len(g["sched_t"])))):
        kind = str(g["sched_kind"][idx])
        if kind == "boost_all":
            ev.append((t, -1, EV_BOOST, 1.0))
        elif kind in ("mix_all", "open"):
            ev.append((t, -1, EV_MIX, 1.0))
        elif kind == "boost":
            ev.append((t, int(g["sched_band"][idx]), EV_BOOST, float(g["sched_val"][idx])))
        elif kind == "mix":
            ev.append((t, int(g["sched_band"][idx]), EV_MIX, float(g["sched_val"][idx])))
        else:
            raise AssertionError(kind)
    return ev


@pytest.mark.parametrize("name", golden_names("fb_"))
def test_golden_as_one_call(gpu_lib, name):
    """each fb_* golden's setter schedule as the events of one call"""
    from huygens_amd import Filterbank
    g = load_golden(name)
    N = int(g["N"])
    fb = Filterbank(int(g["order"]), N, float(g["kp"]), float(g["kg"]))
    fb.distortion(int(g["dist"]), float(g["dist_param"]))
    for n in range(N):
        fb.coefficients(n, g["fwd"][n], g["back"][n])
    y = fb.process_events(g["x"], golden_events(g))
    err = rel_err(y, g["y"])
    assert err < (TOL_STIFF if name in STIFF else TOL), err


def test_positions(gpu_lib):
    """events at 0, 1, 15, 16, 17, 1023, 1024, 1025, n - 1 and n; two in one 16-sample chunk; equal
    `at` on one band and kind (the last wins); BOOST and MIX at one `at`; band 36, the last of a
    ragged group; then a plain process() call continues, and the state matches after each call"""
    from huygens_amd._lib import HZ_FB_PATH_GENERAL
    rng = np.random.default_rng(102)
    N, n = 37, 3000
    fwd, back = random_poles(rng, 2, N)
    g, o = make_pair(2, N, fwd, back, kp=0.05, kg=0.3)
    x = rng.uniform(-1, 1, n + 2100)
    check_call(g, o, x[:n], positions_events(N, n))
    assert g.last_path() == HZ_FB_PATH_GENERAL
    check_state(g, o)
    assert rel_err(g.process(x[n:]), o.process(x[n:])) < TOL
    check_state(g, o)


@pytest.mark.parametrize("order", [0, 1, 3, 4])
def test_orders(gpu_lib, order):
    rng = np.random.default_rng(100 + order)
    N, n = 37, 2500
    fwd, back = random_poles(rng, order, N)
    g, o = make_pair(order, N, fwd, back, kp=0.05, kg=0.3)
    check_call(g, o, rng.uniform(-1, 1, n), random_events(rng, 40, N, n))
    check_state(g, o)


def test_dense(gpu_lib):
    """one band of nine takes 300 events in 2500 samples (several rows per chunk, over a hundred per
    tile), band -1 events interleaved"""
    rng = np.random.default_rng(7)
    N, n = 9, 2500
    fwd, back = random_poles(rng, 2, N)
    g, o = make_pair(2, N, fwd, back, kp=0.05, kg=0.3)
    at = np.sort(rng.integers(0, n, 300))
    ev = []
    for i, t in enumerate(at):
        ev.append((int(t), 4, i % 2, float(rng.uniform(0, 2))))
        if i % 40 == 7:
            ev.append((int(t), -1, (i // 40) % 2, float(rng.uniform(0.5, 1.5))))
    check_call(g, o, rng.uniform(-1, 1, n), ev)
    check_state(g, o)


def test_instant_preamp(gpu_lib):
    """kp = 0 (pre == pin from the event's own sample on), kg = 0.01: the shape of
    test_setters_between_calls as one call"""
    N = 16
    fwd, back = resonant_coefficients(N, 0.99, 0.5)
    g, o = make_pair(2, N, fwd, back, kp=0.0, kg=0.01)
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, 6 * 700)
    ev = []
    for step in range(6):
        n = int(rng.integers(0, N))
        ev += [(700 * (step + 1), n, EV_BOOST, float(step) * 0.3), (700 * (step + 1), n, EV_MIX, -1.0 + step)]
    check_call(g, o, x, ev)
    check_state(g, o)
    x2 = rng.uniform(-1, 1, 700)   # the targets staged at the call's end act on the next call
    assert rel_err(g.process(x2), o.process(x2)) < TOL


@pytest.mark.parametrize("dist_id,param", [(1, 0.125), (2, 0.0), (3, 0.0)])
def test_distortions(gpu_lib, dist_id, param):
    N, n = 24, 4000
    fwd, back = resonant_coefficients(N, 0.995, 0.5)
    g, o = make_pair(2, N, fwd, back)
    g.distortion(dist_id, param)
    o.distortion(dist_id, param)
    rng = np.random.default_rng(60 + dist_id)
    x = 0.5 * white_noise_f32(n, seed=6)
    check_call(g, o, x, random_events(rng, 30, N, n, extra_at=(1024, 2048)))


def test_tiny_calls(gpu_lib):
    rng = np.random.default_rng(11)
    N = 12
    fwd, back = random_poles(rng, 2, N)
    g, o = make_pair(2, N, fwd, back, kp=0.05, kg=0.3)
    check_call(g, o, rng.uniform(-1, 1, 1), [(0, 3, EV_BOOST, 2.0), (0, -1, EV_MIX, 0.5), (1, 3, EV_MIX, 1.5)])
    check_state(g, o)
    check_call(g, o, rng.uniform(-1, 1, 5), [(0, 1, EV_MIX, 0.2), (2, 1, EV_BOOST, 0.7), (4, -1, EV_BOOST, 1.2),
                                             (5, 2, EV_MIX, 0.0)])
    check_state(g, o)
    assert g.process_events(np.zeros(0), []).shape == (0,)
    # no samples, events at 0 == n: the targets are staged for the next call
    assert g.process_events(np.zeros(0), [(0, 5, EV_BOOST, 3.0)]).shape == (0,)
    o.boost(5, 3.0)
    x = rng.uniform(-1, 1, 300)
    assert rel_err(g.process(x), o.process(x)) < TOL
    check_state(g, o)


@pytest.mark.parametrize("N,n,groups", [(7, 50000, 4096), (64, 9000, 1024)])
def test_time_segments(gpu_lib, N, n, groups):
    """small banks are cut into time segments whose zero-state end states depend on pre[t] too:
    events at multiples of 1024 (where segment boundaries fall), one sample around them, and about
    50 random ones; two calls"""
    fwd, back = resonant_coefficients(N, 0.9995, 0.5)
    g, o = make_pair(2, N, fwd, back, kp=0.002, kg=0.01)
    g.set_target_groups(groups)
    rng = np.random.default_rng(N)
    x = white_noise_f32(n, seed=10)
    cut = n // 3
    for lo, hi in ((0, cut), (cut, n)):
        m = hi - lo
        edges = [t + d for t in range(1024, m, 1024 * max(1, m // 8192)) for d in (-1, 0, 1)]
        check_call(g, o, x[lo:hi], random_events(rng, 50, N, m, extra_at=edges))
    check_state(g, o)


@pytest.mark.parametrize("waves,nb", [(4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (16, 1)])
def test_geometries(gpu_lib, waves, nb):
    """every workgroup geometry of test_geometries at N = 37; the event form is built for one band
    per wave, so nb > 1 must give the right answer through its fallback"""
    rng = np.random.default_rng(2037)
    order, N = 2, 37
    fwd = rng.uniform(-0.05, 0.05, (N, order + 1))
    back = np.array([np.poly(rng.uniform(0.5, 0.99, order))[1:] for _ in range(N)])
    g, o = make_pair(order, N, fwd, back, boost=False)
    g.tune(waves, nb)
    boost = rng.uniform(0.5, 1.5, N)
    for fb in (g, o):
        fb.boost(boost)
    check_call(g, o, white_noise_f32(3000, seed=3), random_events(rng, 30, N, 3000, extra_at=(1024,)))
    x2 = white_noise_f32(2100, seed=4)
    assert rel_err(g.process(x2), o.process(x2)) < TOL   # the handle's own geometry again
    check_call(g, o, x2, random_events(rng, 10, N, 2100))


def test_shards(gpu_lib):
    """global band indices on shards (out-of-shard events ignored, -1 = every band of the handle):
    the shards' sum equals the full handle and the oracle"""
    from huygens_amd import Filterbank
    N, n = 300, 2500
    fwd, back = resonant_coefficients(N, 0.999, 0.5)
    full, o = make_pair(2, N, fwd, back)
    shards = []
    for b0, cnt in [(0, 128), (128, 100), (228, 72)]:
        s = Filterbank(2, N, shard=(b0, cnt))
        for b in range(N):
            s.coefficients(b, fwd[b], back[b])
        s.boost(np.ones(N))
        s.open()
        shards.append(s)
    rng = np.random.default_rng(70)
    ev = random_events(rng, 40, N, n) + [(n, -1, EV_MIX, 0.5)]
    ev[5] = (ev[5][0], -1, EV_BOOST, 1.5)
    ev[20] = (ev[20][0], 127, EV_MIX, 0.1)
    ev[21] = (ev[21][0], 128, EV_MIX, 1.9)
    x = white_noise_f32(n, seed=7)
    ref = run_events_split(o, x, ev)
    assert rel_err(full.process_events(x, ev), ref) < TOL
    assert rel_err(sum(s.process_events(x, ev) for s in shards), ref) < TOL
    x2 = white_noise_f32(600, seed=8)
    assert rel_err(sum(s.process(x2) for s in shards), o.process(x2)) < TOL


def test_engine_hand_over(gpu_lib):
    """a converged bank on the LTI engine; an events call whose first event sits mid-call (the
    samples before it through the ordinary dispatch) runs GENERAL with parity across the seam;
    later plain calls re-arm the LTI engine; per-sample calls before and after an events call"""
    from huygens_amd._lib import HZ_FB_PATH_AUTO, HZ_FB_PATH_GENERAL, HZ_FB_PATH_LTI, HZ_FB_RESP_OFF
    N = 64
    fwd, back = resonant_coefficients(N, 0.999, 0.5)
    g, o = make_pair(2, N, fwd, back, kp=0.001, kg=0.001)
    g.set_response(HZ_FB_RESP_OFF)
    g.set_path(HZ_FB_PATH_AUTO)
    rng = np.random.default_rng(12)
    for n in (300, 4096):   # the smoothers converge within the first call
        x = rng.uniform(-1, 1, n)
        assert rel_err(g.process(x), o.process(x)) < TOL
    assert g.last_path() == HZ_FB_PATH_LTI
    x = rng.uniform(-1, 1, 6000)
    check_call(g, o, x, [(3000, 9, EV_BOOST, 2.0), (3000, 9, EV_MIX, 0.3), (4100, -1, EV_MIX, 0.9)])
    assert g.last_path() == HZ_FB_PATH_GENERAL
    check_state(g, o)
    paths = []
    for _ in range(3):   # the smoothers converge again (kp = kg = 0.001: 2^-60 after ~42 samples)
        x = rng.uniform(-1, 1, 2048)
        assert rel_err(g.process(x), o.process(x)) < TOL
        paths.append(g.last_path())
    assert paths[-1] == HZ_FB_PATH_LTI, paths
    # per-sample mode before and after an events call
    ys, yo = [], []
    for v in rng.uniform(-1, 1, 20):
        ys.append(g(v)), yo.append(o(v))
        g.tick(), o.tick()
    assert rel_err(np.array(ys), np.array(yo)) < TOL
    x = rng.uniform(-1, 1, 1500)
    check_call(g, o, x, [(0, 3, EV_MIX, 0.2), (700, 3, EV_BOOST, 1.4), (1500, 3, EV_MIX, 1.0)])
    assert g.last_path() == HZ_FB_PATH_GENERAL
    ys, yo = [], []
    for v in rng.uniform(-1, 1, 20):
        ys.append(g(v)), yo.append(o(v))
        g.tick(), o.tick()
    assert rel_err(np.array(ys), np.array(yo)) < TOL
    check_state(g, o)


def test_errors_change_nothing(gpu_lib):
    """a descending at, at = n + 1, kind = 2, band = N and band = -2: the stated code, and the
    handle then equals an untouched twin's bit for bit"""
    from huygens_amd._lib import HZ_E_INVALID, HZ_E_RANGE, HZError
    rng = np.random.default_rng(13)
    N, n = 20, 500
    fwd, back = random_poles(rng, 2, N)
    g, _ = make_pair(2, N, fwd, back, kp=0.05, kg=0.3)
    twin, _ = make_pair(2, N, fwd, back, kp=0.05, kg=0.3)
    x = rng.uniform(-1, 1, n)
    ok = (10, 2, EV_BOOST, 3.0)
    for bad, code in (([ok, (9, 1, EV_MIX, 1.0)], HZ_E_INVALID), ([ok, (n + 1, 1, EV_MIX, 1.0)], HZ_E_INVALID),
                      ([ok, (20, 1, 2, 1.0)], HZ_E_INVALID), ([ok, (20, N, EV_MIX, 1.0)], HZ_E_RANGE),
                      ([ok, (20, -2, EV_MIX, 1.0)], HZ_E_RANGE)):
        with pytest.raises(HZError) as ei:
            g.process_events(x, bad)
        assert ei.value.code == code, (bad, ei.value)
    assert np.array_equal(g.process(x), twin.process(x))
    assert np.array_equal(g.get_state(), twin.get_state())


def test_no_events_is_process(gpu_lib):
    rng = np.random.default_rng(14)
    N = 50
    fwd, back = resonant_coefficients(N, 0.999, 0.5)
    g, _ = make_pair(2, N, fwd, back)
    twin, _ = make_pair(2, N, fwd, back)
    for n in (1234, 1024, 3000):
        x = rng.uniform(-1, 1, n)
        assert np.array_equal(g.process_events(x, []), twin.process(x))
        assert g.last_path() == twin.last_path()
    assert np.array_equal(g.get_state(), twin.get_state())


def test_device_pointers(gpu_lib):
    torch = pytest.importorskip("torch")
    N = 512
    fwd, back = resonant_coefficients(N, 0.999, 0.5)
    g, o = make_pair(2, N, fwd, back)
    rng = np.random.default_rng(15)
    n = 4096 + 100
    x = white_noise_f32(n, seed=9)
    ev = random_events(rng, 60, N, n, extra_at=(0, n))
    at, band, kind, value = (np.array(c) for c in zip(*ev))   # four parallel arrays
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty_like(xd)
    torch.cuda.synchronize()
    g.process_events_device(xd.data_ptr(), yd.data_ptr(), n, (at, band, kind, value))
    g.synchronize()
    assert rel_err(yd.cpu().numpy(), run_events_split(o, x, ev)) < TOL
    check_state(g, o)
