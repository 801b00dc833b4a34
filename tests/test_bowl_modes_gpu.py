"""GPU parity, mode by mode: Bowl<float>'s two kernels (bowl_mix_kernel behind fill(), and
bowl_dly_chain_kernel behind fill_delaybank) against the float restatement and against the numpy
model of their arithmetic.

The mixdown tests (test_bowl_gpu.py, test_chain_gpu.py, test_fullsize_gpu.py) bound a sum of
thousands of modes by 1e-5 of its peak: a dropped mode, a mode on the wrong thread or a decay
seeded from the wrong sample passes them (tests/test_bowl_float_model_cpu.py shows it with
mutants).  Here every case makes two comparisons:

  (a) kernel against restatement, one mode sounding:  |y - ref| <= 3e-7 a_i.  A one-hot bank's
      restatement is OracleBowl(1, ...) of that mode, bit for bit; bound, visibility and the place
      of every hot mode in the launch plan are proved on the CPU (test_bowl_float_model_cpu.py);
  (b) kernel against the numpy model (bowl_float_model.py): at most one float32 spacing apart --
      device and host exp differ in the last bits of a double.  The share of bit-identical
      samples is printed, not asserted.

Multi-mode banks are compared with the model's float64 sum rounded to float32, within one spacing
plus 1e-12 x sum a_i (summation order, exp): about 3e-7 of the peak where the restatement, which
rounds its running sum after every mode, allows 1e-5.

At 2^24 the float counter stops (phase++ no longer moves it) and the reference repeats one value
for ever; the kernels must too, exactly, in the call the counter sticks in and in later calls.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import bowl_float_model as bm
import bowl_mode_cases as bc
from oracle import rel_err
from oracle_bowl import OracleBowl

pytestmark = pytest.mark.gpu
SR = 48000
NORTH_STAR = 1e-5


@functools.lru_cache(maxsize=None)
def ref_single(fad, start, n):
    o = OracleBowl(1, [fad[0]], [fad[1]], [fad[2]], np.float32)
    o.seek(start)
    out = o.fill(n)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_single(fad, start, calls, chunk):
    out = bm.model_fill([fad[0]], [fad[1]], [fad[2]], list(calls), chunk, n0=start)
    out.setflags(write=False)
    return out


class Worst:
    """the largest figures of a test, printed before anything is asserted"""

    def __init__(self, what):
        self.what, self.a, self.b, self.same, self.n = what, 0.0, 0.0, 1.0, 0

    def one_hot(self, y, fad, start, calls, chunk):
        ea = bm.per_mode_error(y, ref_single(fad, start, int(sum(calls))), fad[1])
        eb, same = bm.spacing_error(y, model_single(fad, start, tuple(calls), chunk))
        self.a, self.b, self.same, self.n = max(self.a, ea), max(self.b, eb), min(self.same, same), self.n + 1
        return ea, eb

    def report(self):
        print("%s: %d runs, (a) kernel - restatement <= %.3e a_i (bound 3e-7), (b) kernel - model <= %.2f "
              "float32 spacings (bound 1), bit-identical share >= %.4f" % (self.what, self.n, self.a, self.b, self.same))
        assert self.a <= bm.PER_MODE and self.b <= 1.0


def advance(torch, bowl, start):
    """fill_device into a scratch buffer until the counter is `start`"""
    if start:
        scratch = torch.empty(bc.LATE_STEP, dtype=torch.float32, device="cuda")
        for n in bc.advance_calls(start):
            bowl.fill_device(scratch.data_ptr(), n)
        torch.cuda.synchronize()
    assert bowl.phase() == start


def assert_stuck(y, k):
    """every sample from the first one at 2^24 (index k) equals it, and it is not silence"""
    assert y[k] != 0 and np.all(y[k:] == y[k]), (
        "the output moves after the counter has stuck: %d distinct values, spread %.3e"
        % (len(np.unique(y[k:])), float(np.ptp(y[k:].astype(np.float64)))))


# ---- fill(): one mode sounding, at the edges of the launch plan ------------------------------------

@pytest.mark.parametrize("groups", bc.FILL_GROUPS)
@pytest.mark.parametrize("M", bc.FILL_M)
def test_fill_one_hot(gpu_lib, M, groups):
    from huygens_amd import Bowl
    w = Worst("fill one-hot M = %d, groups = %d" % (M, groups))
    for i in bc.fill_hot(M, groups):
        fad = bc.mode_of(M, i)
        b = Bowl(M, *bc.one_hot(M, i, fad), np.float32)
        b.set_target_groups(groups)
        b.trigger()
        y = np.concatenate([b.fill(n) for n in bc.FILL_CALLS])
        assert b.phase() == sum(bc.FILL_CALLS)
        b.close()
        w.one_hot(y, fad, 0, bc.FILL_CALLS, bm.K_L)
    w.report()


# ---- whole banks against the model -------------------------------------------------------------------

@pytest.mark.parametrize("kind,M,n,groups", bc.MULTI)
def test_multi_mode_against_model(gpu_lib, kind, M, n, groups):
    from huygens_amd import Bowl
    if kind == "bench":
        import bench_rows
        f, a, d = bench_rows.c5_model(M)
    else:
        f, a, d = bc.c5_shape_model(M)
    b = Bowl(M, f, a, d, np.float32)
    b.set_target_groups(groups)
    calls = bc.multi_calls(n)
    y = np.concatenate([b.fill(L) for L in calls])
    b.trigger()
    y = np.concatenate([y, b.fill(1000)])
    b.close()
    model = np.concatenate([bm.model_fill(f, a, d, calls, bm.K_L), bm.model_fill(f, a, d, [1000], bm.K_L)])
    slack = bc.SUM_SLACK * float(np.sum(a))
    e, same = bm.spacing_error(y, model, slack)
    print("multi-mode %s M = %d: kernel - model <= %.2f x (spacing + %.1e), %.3e of the peak, bit-identical "
          "share %.4f" % (kind, M, e, slack, rel_err(y, model), same))
    assert e <= 1.0


# ---- late counters and the saturation ----------------------------------------------------------------

@pytest.mark.parametrize("M", bc.LATE_M)
@pytest.mark.parametrize("start", bc.LATE_STARTS)
def test_late_counters(gpu_lib, start, M):
    torch = pytest.importorskip("torch")
    from huygens_amd import Bowl
    calls = [bc.LATE_WINDOW, 1000]        # the second call starts stuck when the first one sticks
    k = bc.STUCK - start if start + bc.LATE_WINDOW > bc.STUCK else None
    w = Worst("late counter %d, M = %d one-hot" % (start, M))
    stuck_fail = []
    for i in bc.LATE_HOT[M]:
        for fad in bc.late_modes(start):
            b = Bowl(M, *bc.one_hot(M, i, fad), np.float32)
            b.trigger()
            advance(torch, b, start)
            y = np.concatenate([b.fill(n) for n in calls])
            assert b.phase() == min(start + sum(calls), bc.STUCK)
            b.close()
            w.one_hot(y, fad, start, calls, bm.K_L)
            if k is not None and not np.all(y[k:] == y[k]):
                stuck_fail.append((i, fad, float(np.ptp(y[k:].astype(np.float64))) / fad[1]))
    print("modes whose output moves after 2^24 (mode, (f, a, d), spread / a):", stuck_fail)
    w.report()
    assert not stuck_fail
    # every mode sounding
    f, a, d = bc.late_bank(M)
    b = Bowl(M, f, a, d, np.float32)
    b.trigger()
    advance(torch, b, start)
    y = np.concatenate([b.fill(n) for n in calls])
    phase = b.phase()
    b.close()
    o = OracleBowl(M, f, a, d, np.float32)
    o.seek(start)
    slack = bc.SUM_SLACK * float(np.sum(a))
    e, same = bm.spacing_error(y, bm.model_fill(f, a, d, calls, bm.K_L, n0=start), slack)
    er = rel_err(y, o.fill(sum(calls)))
    print("late counter %d, M = %d all-hot: kernel - model <= %.2f x (spacing + %.1e), bit-identical share "
          "%.4f; kernel - restatement %.3e of the peak" % (start, M, e, slack, same, er))
    assert e <= 1.0 and er < NORTH_STAR
    if k is not None:
        assert phase == bc.STUCK
        assert_stuck(y, k)


# ---- the fused Bowl -> Delaybank block ---------------------------------------------------------------

def _chain_run(torch, M, i, fad, start, blocks):
    """-> (fill buffer, bank outputs, reference bank's outputs, the bank's own launches)"""
    from huygens_amd import Bowl, Delaybank
    bowl = Bowl(M, *bc.one_hot(M, i, fad), np.float32)
    banks = [Delaybank(bc.CHAIN_LINES, 3, 2 * SR, np.float32) for _ in range(2)]
    for bank in banks:
        for k in range(bc.CHAIN_LINES):
            bank.coefficients(k, *bc.chain_taps(k))
    bank, ref_bank = banks
    s = torch.cuda.Stream()
    bowl.set_stream(s.cuda_stream)
    bank.set_stream(s.cuda_stream)
    bowl.trigger()
    advance(torch, bowl, start)
    total = sum(blocks)
    buf = torch.zeros(total, dtype=torch.float32, device="cuda")
    out = torch.zeros(total, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bank.profile(True)
    at = 0
    for n in blocks:
        bowl.fill_delaybank(bank, buf.data_ptr() + 4 * at, out.data_ptr() + 4 * at, n, True)
        at += n
    torch.cuda.synchronize()
    launches = bank.profile_read()[1]
    bank.profile(False)
    assert bowl.phase() == min(start + total, bc.STUCK)
    bf, of = buf.cpu().numpy(), out.cpu().numpy()
    edges = np.cumsum([0] + list(blocks))
    ref = np.concatenate([ref_bank.process(bf[lo:hi], mix=True) for lo, hi in zip(edges[:-1], edges[1:])])
    for obj in (bowl, bank, ref_bank):
        obj.close()
    return bf, of, ref, launches


@pytest.mark.parametrize("M", bc.CHAIN_M)
def test_chain_one_hot(gpu_lib, M):
    torch = pytest.importorskip("torch")
    runs = [(0, bc.CHAIN_BLOCKS, False)]
    if M in bc.CHAIN_LATE_M:
        runs += [(bc.CHAIN_LATE, bc.CHAIN_BLOCKS, True), (bc.CHAIN_STUCK_START, bc.CHAIN_STUCK_BLOCKS, True)]
    for start, blocks, late in runs:
        w = Worst("chain one-hot M = %d from %d" % (M, start))
        stuck_fail = []
        for i in bc.chain_hot(M):
            fad = bc.chain_mode(M, i, late)
            bf, of, ref, launches = _chain_run(torch, M, i, fad, start, blocks)
            assert launches == 0                     # the fused path ran: nothing launched on the bank
            assert np.array_equal(of, ref)           # the bank's part, bit for bit, on the fused fill buffer
            w.one_hot(bf, fad, start, blocks, bm.CHAIN_SPW)
            if start + sum(blocks) > bc.STUCK:
                k = bc.STUCK - start
                assert bf[k] != 0
                if not np.all(bf[k:] == bf[k]):
                    stuck_fail.append((i, fad, float(np.ptp(bf[k:].astype(np.float64))) / fad[1]))
        print("modes whose fill buffer moves after 2^24:", stuck_fail)
        w.report()
        assert not stuck_fail


# ---- hz_bowl_render_device ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", bc.RENDER_DEVICE_N)
def test_render_device_equals_render(gpu_lib, n):
    """Bowl<double> samples straight into device memory: render()'s, bit for bit"""
    torch = pytest.importorskip("torch")
    from huygens_amd import Bowl
    from huygens_amd._lib import check
    f, a, d = bc.c5_shape_model(303)
    host, dev = Bowl(303, f, a, d), Bowl(303, f, a, d)
    want = host.render(n)
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                         # the bowl writes from a stream of its own
    check(gpu_lib.hz_bowl_render_device(dev._h, C.c_void_p(out.data_ptr()), n))
    assert dev.phase() == n == host.phase()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.max(np.abs(want)) > 0 or n == 1        # sample 0 of a bowl is sin(0)
    assert np.array_equal(got, want)
    # and a second call, the counter carried
    want2 = host.render(max(n, 64))
    out2 = torch.zeros(max(n, 64), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    check(gpu_lib.hz_bowl_render_device(dev._h, C.c_void_p(out2.data_ptr()), max(n, 64)))
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy(), want2) and np.max(np.abs(want2)) > 0
    host.close()
    dev.close()
