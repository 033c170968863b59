"""zmi_resample on the GPU: against the fp64 evaluation of the same table (tests/resample_cases.py) and against
speaker.resample() at the lengths where the frame / tap / tile arithmetic changes, chunk and lane invariance of the
streamed form (bit for bit), an analytic sine, DACAutoencoder.preprocess, and the argument errors. Parity with
torchaudio itself is unpinned (torchaudio is absent)."""
import math

import pytest
import torch

from tests import resample_cases as rc
from zonos_vibes_amd import _lib, speaker
from zonos_vibes_amd import resampling as rs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -12345.0
PAIRS = [(44100, r) for r in (48000, 24000, 16000, 8000, 22050)] + [(r, 44100) for r in (48000, 24000, 16000, 22050)]
STREAM_PAIRS = [(44100, r) for r in rc.OUT_RATES] + [(r, 44100) for r in rc.IN_RATES]
KINDS = ("uniform", "impulse0", "impulse_last", "ones")
LENGTHS = {"head": (2000, 1600, 700), "ones": (1100, 500, 37)}


def lengths_of(plan) -> list:
    o, n, W, T = plan
    return [0, 1, W, W + 1, o - 1, o, o + 1, T, T + 1, 3 * o + 5, 4099]


def signal(kind: str, N: int, seed: int) -> torch.Tensor:
    if kind == "uniform":
        return torch.rand(N, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    x = torch.ones(N) if kind == "ones" else torch.zeros(N)
    if N and kind == "impulse0":
        x[0] = 1.0
    if N and kind == "impulse_last":
        x[-1] = 1.0
    return x


_tables = {}


def kern_t(plan):
    if plan not in _tables:
        _tables[plan] = rs.table(plan).t().contiguous().to(DEV)
    return _tables[plan]


def launch(plan, xs: list, gap: int = 5):
    """The whole of every xs[i] (device, 1-D) as one segment each, all in ONE zmi_resample launch into a guard-filled
    buffer, segment i at dst = gap + the lengths before it (no room between segments: a write past a segment's end
    lands in its neighbour). Returns (status, the buffer on the CPU, [(dst, L)])."""
    o, n, W, T = plan
    rows, spans, dst = [], [], gap
    for x in xs:
        L = rs.out_len(x.numel(), plan)
        # carry, n_carry, src, n_src, i0, n_total, j0, n_out, dst, carry_out, n_keep
        rows.append((0, 0, x.data_ptr() if x.numel() else 0, x.numel(), 0, x.numel(), 0, L, dst, 0, 0))
        spans.append((dst, L))
        dst += L
    total = dst
    out = torch.full((total + gap,), GUARD, dtype=torch.float32, device=DEV)
    host = torch.tensor(rows, dtype=torch.int64)
    dev = host.to(DEV)
    rc_ = _lib.lib().zmi_resample(dev.data_ptr(), host.data_ptr(), len(rows), total, kern_t(plan).data_ptr(), o, n, W,
                                  out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc_, out.cpu(), spans


# ------------------------------------------------------------------ 1. the kernel against fp64
@pytest.mark.parametrize("orig,new", PAIRS)
def test_kernel_against_fp64(orig, new):
    plan = rs.resample_plan(orig, new)
    o, n, W, T = plan
    lens = lengths_of(plan)
    triples = [[lens[(3 * k + i) % len(lens)] for i in range(3)] for k in range(4)]  # every length, three a launch
    assert {m for t in triples for m in t} == set(lens)
    worst = 0.0
    for kind in KINDS:
        for k, triple in enumerate(triples):
            xs = [signal(kind, N, 100 * k + i) for i, N in enumerate(triple)]
            status, buf, spans = launch(plan, [x.to(DEV) for x in xs])
            assert status == 0
            written = torch.zeros(buf.numel(), dtype=torch.bool)
            for x, (dst, L) in zip(xs, spans):
                assert L == math.ceil(n * x.numel() / o)
                got = buf[dst: dst + L].double()
                written[dst: dst + L] = True
                ref, bound = rc.ref64(x, orig, new)
                err = (got - ref).abs()
                assert bool((err <= bound).all()), (kind, x.numel(), float((err / bound).max()))
                worst = max(worst, float((err / bound).max()) if L else 0.0)
                spk = speaker.resample(x[None], orig, new)[0].double()
                assert spk.shape == got.shape and bool(((got - spk).abs() <= 2 * bound).all()), (kind, x.numel())
            assert bool((buf[~written] == GUARD).all()), (kind, triple)
    print(f"{orig} -> {new}: worst |got - ref64| / bound = {worst:.3f}")


def test_kernel_long_span_reads_memory():
    """44100 -> 100 Hz: o = 441, n = 1, W = 2673, T = 5787. A tile part of 16 or more outputs spans more input than the
    kernel stages in LDS and is read from memory; one of fewer is staged. Both against fp64, and the streamed form
    (few outputs a push: staged) equals the one-shot (whole tiles: from memory) bit for bit."""
    orig, new = 44100, 100
    plan = rs.resample_plan(orig, new)
    assert plan == (441, 1, 2673, 5787)
    xs = {0: signal("uniform", 30000, 1), 1: signal("uniform", 4410, 2), 2: signal("uniform", 9000, 3)}
    status, buf, spans = launch(plan, [x.to(DEV) for x in xs.values()])
    assert status == 0 and [L for _, L in spans] == [69, 10, 21]
    for x, (dst, L) in zip(xs.values(), spans):
        ref, bound = rc.ref64(x, orig, new)
        assert bool(((buf[dst: dst + L].double() - ref).abs() <= bound).all())
    sr = rs.StreamResampler(3, orig, new, device=DEV)
    got = rc.run_streamed(sr, {k: x.to(DEV) for k, x in xs.items()}, "head")
    for (lane, x), (dst, L) in zip(xs.items(), spans):
        assert torch.equal(got[lane].cpu(), buf[dst: dst + L]), lane


# ------------------------------------------------------------------ 2. chunk and lane invariance
@pytest.mark.parametrize("which", ["head", "ones"])
@pytest.mark.parametrize("orig,new", STREAM_PAIRS)
def test_streamed_equals_one_shot(orig, new, which):
    plan = rs.resample_plan(orig, new)
    g = torch.Generator().manual_seed(7)
    xs = {lane: (torch.rand(m, generator=g) * 2 - 1).to(DEV) for lane, m in enumerate(LENGTHS[which])}
    one = rs.GpuResampler(DEV, orig, new)
    want = {lane: one(x) for lane, x in xs.items()}

    def check(lane, recv, emitted, final):
        assert emitted == (rs.out_len(recv, plan) if final else rs.emitted(recv, plan))

    got = rc.run_streamed(rs.StreamResampler(3, orig, new, device=DEV), xs, which, check)
    for lane in xs:
        assert got[lane].shape == want[lane].shape and torch.equal(got[lane], want[lane]), lane
    # a lane alone (segment 0 of its launches) gives what it gives as lane 2 among three
    alone = rc.run_streamed(rs.StreamResampler(1, orig, new, device=DEV), {0: xs[2]}, which)
    assert torch.equal(alone[0], want[2])


def test_one_shot_rows_are_segments_of_one_launch():
    one = rs.GpuResampler(DEV, 44100, 24000)
    x = (torch.rand(2, 3, 3000, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    y = one(x)
    assert y.shape == (2, 3, rs.out_len(3000, one.plan))
    for a in range(2):
        for b in range(3):
            assert torch.equal(y[a, b], one(x[a, b]))
    assert one(x[..., :0]).shape == (2, 3, 0)
    same = rs.GpuResampler(DEV, 48000, 48000)
    assert same(x) is x
    with pytest.raises(ValueError):
        one(x.cpu())


def test_reset_and_reuse_on_the_gpu():
    orig, new = 44100, 16000
    g = torch.Generator().manual_seed(11)
    a, b = [(torch.rand(m, generator=g) * 2 - 1).to(DEV) for m in (1500, 2100)]
    sr = rs.StreamResampler(2, orig, new, device=DEV)
    sr.push({0: a[:1000], 1: b[:600]})
    sr.reset(0)                                     # lane 0's utterance is dropped; b starts over in it
    parts = [sr.push({0: b[:900], 1: b[600:1300]})[0], sr.push({0: b[900:]}, final=[0])[0]]
    assert torch.equal(torch.cat([p.view(-1) for p in parts]), rs.GpuResampler(DEV, orig, new)(b))


def test_chunks_on_another_device_are_refused_before_any_launch():
    """A CPU chunk's pointer must never reach the segment table: ValueError, and the push changes nothing."""
    sr = rs.StreamResampler(2, 44100, 24000, device=DEV)
    x = (torch.rand(1000, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)
    first = sr.push({0: x[:600], 1: x[:300]})
    state = [(sr.received(k), sr.emitted(k)) for k in range(2)]
    with pytest.raises(ValueError, match="cpu"):
        sr.push({0: x[600:], 1: x[300:].cpu()})          # lane 0's chunk is fine, lane 1's is on the host
    with pytest.raises(ValueError):
        sr.push({1: x[300:].cpu()}, final=[1])
    assert [(sr.received(k), sr.emitted(k)) for k in range(2)] == state
    rest = sr.push({0: x[600:], 1: x[300:]}, final=[0, 1])  # and the lanes go on as if nothing had happened
    want = rs.GpuResampler(DEV, 44100, 24000)(x)
    for k in range(2):
        assert torch.equal(torch.cat([first[k].view(-1), rest[k].view(-1)]), want)
    kernel = rs.HipResampleKernel(DEV, sr.plan)              # the kernel adapter refuses such a piece too
    none = x.new_empty(0)
    with pytest.raises(ValueError):
        kernel([rs.Piece(none, x.cpu(), 0, 1000, 0, 8, 0, none)], torch.empty(8, device=DEV))


# ------------------------------------------------------------------ 3. a sine
@pytest.mark.parametrize("orig,new", [(48000, 44100), (44100, 16000)])
def test_sine_on_the_gpu(orig, new):
    """2e-3 is about 3x the fp64 reference's own worst error against the analytic sine (6.9e-4,
    test_resample_cpu.py): it flags a wrong rate or phase, not rounding."""
    one = rs.GpuResampler(DEV, orig, new)
    err = rc.sine_error(lambda x: one(x.float().to(DEV)), orig, new)
    print(f"{orig} -> {new}: {err:.2e}")
    assert err < 2e-3


# ------------------------------------------------------------------ 4. preprocess
@pytest.fixture(scope="module")
def dac():
    from zonos_vibes_amd.autoencoder import DACAutoencoder
    return DACAutoencoder(DEV)


def test_preprocess_resamples_on_the_gpu(dac):
    x = (torch.rand(1, 1, 4800, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    y = dac.resample(x, 48000, 44100)
    L = math.ceil(4800 * 44100 / 48000)
    assert y.shape == (1, 1, L) and torch.equal(y, rs.GpuResampler(DEV, 48000, 44100)(x))
    ref, bound = rc.ref64(x.cpu().view(-1), 48000, 44100)
    assert bool(((y.cpu().view(-1).double() - ref).abs() <= bound).all())
    p = dac.preprocess(x, 48000)
    padded = 512 * math.ceil(L / 512)
    assert p.shape == (1, 1, padded) and torch.equal(p[..., :L], y) and not bool(p[..., L:].any())
    codes = dac.encode(p)
    assert codes.shape == (1, 9, math.ceil(L / 512)) and codes.dtype == torch.int64
    with pytest.raises(NotImplementedError):
        dac.preprocess(x.cpu(), 24000)
    with pytest.raises(NotImplementedError):
        dac.resample(x.cpu(), 24000, 44100)
    z = (torch.rand(1, 1, 1000, generator=torch.Generator().manual_seed(6)) * 2 - 1).to(DEV)
    q = dac.preprocess(z, 44100)                    # the 44.1 kHz path: the pad alone, as before
    assert torch.equal(q, torch.nn.functional.pad(z, (0, 24))) and dac.resample(z, 44100, 44100) is z
    with pytest.raises(ValueError):
        dac.resample(x, 44101, 44100)
    with pytest.raises(ValueError, match="fp32"):     # no silent cast: the 44.1 kHz path keeps the input's dtype
        dac.preprocess(x.half(), 48000)
    assert dac.preprocess(z.half(), 44100).dtype == torch.float16


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_write_nothing():
    lib = _lib.lib()
    plan = rs.resample_plan(44100, 48000)
    o, n, W, T = plan
    x = signal("uniform", 1000, 0).to(DEV)
    L = rs.out_len(1000, plan)
    out = torch.full((L + 8,), GUARD, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    # carry, n_carry, src, n_src, i0, n_total, j0, n_out, dst, carry_out, n_keep
    good = [0, 0, x.data_ptr(), 1000, 0, 1000, 0, L, 0, 0, 0]

    def call(row, n_segs=1, total=L, kt=kern_t(plan), dst=out, o_=o, n_=n, W_=W, host_ok=True, dev_ok=True):
        host = torch.tensor([row], dtype=torch.int64)
        dev = host.to(DEV)
        return lib.zmi_resample(dev.data_ptr() if dev_ok else None, host.data_ptr() if host_ok else None, n_segs, total,
                                kt.data_ptr() if kt is not None else None, o_, n_, W_,
                                dst.data_ptr() if dst is not None else None, stream)

    def bad(**kw):
        row = list(good)
        for k, v in kw.items():
            row[int(k[1:])] = v
        return row

    assert call(good, n_segs=0) == 0 and call(good, total=0, n_segs=0) == 0   # nothing to do: nothing launched
    torch.cuda.synchronize()
    assert bool((out == GUARD).all())
    cases = [
        call(good, dev_ok=False), call(good, host_ok=False), call(good, kt=None), call(good, dst=None),
        call(good, n_segs=-1), call(good, total=-1), call(good, o_=0), call(good, n_=0), call(good, W_=0),
        call(good, n_=1 << 20, o_=1 << 20),       # a table over 2^22 floats
        call(bad(_2=0)),                          # NULL src with n_src > 0
        call(bad(_3=-1)), call(bad(_7=-1)),       # negative counts
        call(bad(_7=L + 1), total=L + 1),         # more outputs than ceil(n N / o)
        call(bad(_5=-1)),                         # not final, yet frames whose taps have not arrived
        call(bad(_5=999)),                        # final, but n_total is not where the samples end
        call(bad(_8=4), total=L),                 # dst + n_out past total_out
        call(bad(_4=500, _5=1500)),               # outputs whose taps lie before what the segment holds
        call(bad(_2=x.data_ptr() + 2)),           # misaligned
        call(bad(_10=5)),                         # n_keep without carry_out
    ]
    torch.cuda.synchronize()
    assert all(c != 0 for c in cases), cases
    assert b"resample" in lib.zmi_last_error()
    assert bool((out == GUARD).all())
    assert call(good) == 0                        # and the good table does run
    torch.cuda.synchronize()
    assert bool((out[:L] != GUARD).all()) and bool((out[L:] == GUARD).all())
    # the carry entry checks the same table
    host = torch.tensor([bad(_10=5)], dtype=torch.int64)
    assert lib.zmi_resample_carry(host.to(DEV).data_ptr(), host.data_ptr(), 1, o, n, W, stream) != 0
    assert lib.zmi_resample_carry(None, None, 0, o, n, W, stream) == 0
