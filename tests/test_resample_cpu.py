"""CPU checks of the resampling contract (zonos_vibes_amd/resampling.py): the plan and E(I) rule, StreamResampler's
bookkeeping over a torch restatement of the kernel (chunked == whole, bit for bit), the fp64 reference against an
analytic sine, and the argument errors. The HIP kernel itself is tested in test_gpu_resample.py."""
import math

import pytest
import torch

from tests import resample_cases as rc
from zonos_vibes_amd import resampling as rs
from zonos_vibes_amd import speaker

PAIRS = [(44100, r) for r in rc.OUT_RATES] + [(r, 44100) for r in rc.IN_RATES]
LENGTHS = {"head": (2000, 1600, 700), "ones": (1100, 500, 37)}


def utterances(which: str, seed: int = 0) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {lane: torch.rand(m, generator=g) * 2 - 1 for lane, m in enumerate(LENGTHS[which])}


def test_plan_matches_the_speaker_table():
    for orig, new in PAIRS + [(22050, 44100), (44100, 22050)]:
        o, n, W, T = rs.resample_plan(orig, new)
        g = math.gcd(orig, new)
        kern, width = speaker.resample_kernel(orig // g, new // g)
        assert (o, n, W) == (orig // g, new // g, width) and tuple(kern.shape) == (n, T) and T == 2 * W + o
    assert rs.resample_plan(44100, 48000)[:3] == (147, 160, 7)


def test_emitted_rule_and_latency():
    for orig, new in PAIRS:
        plan = rs.resample_plan(orig, new)
        o, n, W, T = plan
        for received in (0, 1, W - 1, W, W + o - 1, W + o, W + o + 1, W + 5 * o + 3):
            want = n * max(0, (received - W) // o)
            assert rs.emitted(received, plan) == want
            # a frame is counted exactly when its last tap (f o - W + T - 1 = f o + W + o - 1) has arrived
            assert all((f * o + W + o - 1 < received) == (f < want // n) for f in range(8))
    o, n, W, T = rs.resample_plan(44100, 48000)
    assert (W + o) / 44100 < 3.6e-3
    o, n, W, T = rs.resample_plan(44100, 8000)
    assert (W + o) / 44100 < 11.5e-3


def test_torch_restatement_matches_fp64_and_speaker_resample():
    x = utterances("head")[2]
    for orig, new in PAIRS:
        y = rc.whole(x, orig, new)
        ref, bound = rc.ref64(x, orig, new)
        assert y.numel() == math.ceil(new * x.numel() / orig)
        assert bool(((y.double() - ref).abs() <= bound).all())
        spk = speaker.resample(x[None], orig, new)[0]
        assert spk.shape == y.shape and bool(((spk.double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("orig,new", [(44100, 48000), (44100, 8000), (22050, 44100), (44100, 22050)])
def test_edge_lengths_against_fp64(orig, new):
    """The lengths the GPU test uses, through the torch restatement: the reference and its bound hold at N = 0, 1 and
    around W, o and T."""
    o, n, W, T = rs.resample_plan(orig, new)
    for N in (0, 1, W, W + 1, o - 1, o, o + 1, T, T + 1, 3 * o + 5):
        for x in (torch.ones(N), torch.rand(N, generator=torch.Generator().manual_seed(N)) * 2 - 1):
            y = rc.whole(x, orig, new)
            ref, bound = rc.ref64(x, orig, new)
            assert y.shape == ref.shape == (math.ceil(n * N / o),)
            assert bool(((y.double() - ref).abs() <= bound).all()), N
            assert bool(((speaker.resample(x[None], orig, new)[0].double() - ref).abs() <= bound).all()), N


@pytest.mark.parametrize("which", ["head", "ones"])
@pytest.mark.parametrize("orig,new", PAIRS)
def test_stream_resampler_chunked_equals_whole(orig, new, which):
    plan = rs.resample_plan(orig, new)
    kernel = rc.torch_kernel(plan)
    xs = utterances(which)
    sr = rs.StreamResampler(3, orig, new, kernel=kernel)

    def check(lane, recv, emitted, final):
        assert emitted == (rs.out_len(recv, plan) if final else rs.emitted(recv, plan))

    got = rc.run_streamed(sr, xs, which, check)
    for lane, x in xs.items():
        want = rc.whole(x, orig, new, kernel)
        assert got[lane].numel() == math.ceil(plan[1] * x.numel() / plan[0])
        assert torch.equal(got[lane], want)
        assert sr.received(lane) == 0 and sr.emitted(lane) == 0  # a lane that ended is ready for the next utterance


def test_reset_then_reuse_of_a_lane():
    orig, new = 44100, 16000
    plan = rs.resample_plan(orig, new)
    kernel = rc.torch_kernel(plan)
    sr = rs.StreamResampler(2, orig, new, kernel=kernel)
    xs = utterances("head", seed=1)
    sr.push({0: xs[0][:900], 1: xs[1][:1300]})          # lane 0 is abandoned mid-utterance
    sr.reset(0)
    assert sr.received(0) == 0 and sr.emitted(0) == 0 and sr.received(1) == 1300
    a = sr.push({0: xs[2][:600], 1: xs[1][1300:]}, final=[1])
    b = sr.push({0: xs[2][600:]}, final=[0])
    assert torch.equal(torch.cat([a[0].view(-1), b[0].view(-1)]), rc.whole(xs[2], orig, new, kernel))
    c = sr.flush([0])                                   # an utterance of no samples
    assert c[0].shape == (1, 1, 0)


def test_empty_pushes_and_flush_only():
    orig, new = 48000, 44100
    plan = rs.resample_plan(orig, new)
    kernel = rc.torch_kernel(plan)
    sr = rs.StreamResampler(1, orig, new, kernel=kernel)
    x = utterances("head", seed=2)[2]
    parts = [sr.push({0: x[:0]})[0], sr.push({0: x[:400]})[0], sr.push({}), sr.push({0: x[400:]})[0], sr.flush([0])[0]]
    got = torch.cat([p.view(-1) for p in parts if not isinstance(p, dict)])
    assert torch.equal(got, rc.whole(x, orig, new, kernel))


def test_identity_rates_pass_through():
    sr = rs.StreamResampler(2, 44100, 44100)
    x = torch.arange(10, dtype=torch.float32)
    out = sr.push({1: x}, final=[1])
    assert out[1].shape == (1, 1, 10) and torch.equal(out[1].view(-1), x) and out[1].data_ptr() == x.data_ptr()


@pytest.mark.parametrize("orig,new", [(44100, 16000), (48000, 44100)])
def test_mutants_are_rejected(orig, new, monkeypatch):
    """A carry read without its first sample, and frames emitted early: while their last min(o // 2, W - 1) taps have
    not arrived (they read 0). That many keeps the early count below ceil(n I / o) and the carry consistent, so the
    mutant runs to the end like the real thing and is rejected by its samples alone."""
    plan = rs.resample_plan(orig, new)
    xs = utterances("head")
    want = {lane: rc.whole(x, orig, new) for lane, x in xs.items()}
    mutant = rs.StreamResampler(3, orig, new, kernel=rc.torch_kernel(plan, drop_carry_head=True))
    got = rc.run_streamed(mutant, xs, "head")
    assert not any(torch.equal(got[lane], want[lane]) for lane in xs)
    o, n, W, T = plan
    early = min(o // 2, W - 1)
    monkeypatch.setattr(rs, "emitted", lambda received, plan: n * max(0, (received - W + early) // o))
    xs = utterances("ones")  # every sample alone: each frame is emitted `early` samples before its last tap
    got = rc.run_streamed(rs.StreamResampler(3, orig, new, kernel=rc.torch_kernel(plan)), xs, "ones")
    for lane, x in list(xs.items())[:2]:  # (the third is shorter than one frame: everything comes from its final push)
        ok = rc.whole(x, orig, new)
        assert got[lane].shape == ok.shape and not torch.equal(got[lane], ok), lane


@pytest.mark.parametrize("orig,new", PAIRS + [(24000, 44100), (8000, 44100)])
def test_fp64_reference_resamples_a_sine(orig, new):
    """The fp64 reference's own error against the analytic 1 kHz sine, measured: 48000 -> 44100 4.5e-4,
    24000 -> 44100 1.0e-4, 16000 -> 44100 6.9e-4, 8000 -> 44100 1.7e-4, 44100 -> 48000 5.7e-4, -> 24000 3.6e-5,
    -> 16000 4.0e-4, -> 8000 1.4e-4. Under 1e-3 each: a swapped orig / new in this file's plumbing reads ~1."""
    err = rc.sine_error(lambda x: rc.ref64(x, orig, new)[0], orig, new)
    print(f"{orig} -> {new}: {err:.2e}")
    assert err < 1e-3


def test_argument_errors():
    for bad in (0, -1, 44100.0, 2.5, True, "44100"):
        with pytest.raises(ValueError):
            rs.resample_plan(bad, 44100)
        with pytest.raises(ValueError):
            rs.resample_plan(44100, bad)
        with pytest.raises(ValueError):
            rs.StreamResampler(1, 44100, bad, kernel=lambda pieces, out: None)
    calls = []
    orig_table = speaker.resample_kernel
    try:
        speaker.resample_kernel = lambda *a, **k: calls.append(a) or orig_table(*a, **k)
        with pytest.raises(ValueError, match="table"):
            rs.StreamResampler(1, 44101, 44100, kernel=lambda pieces, out: None)
        with pytest.raises(ValueError, match="table"):
            rs.resample_plan(44101, 44100)
    finally:
        speaker.resample_kernel = orig_table
    assert calls == []  # refused before the 7.8 GB table is built
    with pytest.raises(ValueError):
        rs.StreamResampler(0, 44100, 48000, kernel=lambda pieces, out: None)
    sr = rs.StreamResampler(2, 44100, 48000, kernel=lambda pieces, out: None)
    with pytest.raises(ValueError):
        sr.push({2: torch.zeros(4)})
    with pytest.raises(ValueError):
        sr.push({0: torch.zeros(4, dtype=torch.float64)})
    assert sr.received(0) == 0  # a refused push changes nothing
