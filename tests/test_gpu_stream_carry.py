"""The carried-state streaming DAC decoder on the GPU: the range transposed conv and the state-move kernel, then
stream_decoder(carry=True), stream_decoder_batch(carry=True) and Zonos.stream / stream_batch / serve with
decoder="carry", each bit for bit (torch.equal) against decode() or against the default window decoder."""
import ctypes

import pytest
import torch

from tests import dac_cases as dc
from tests.stream_cases import PATTERNS, lengths, pushes, random_codes, run_stream
from tests.test_gpu_dac_kernels import forms
from tests.test_gpu_serve import Req, alone, check as serve_check, drain
from tests.test_gpu_stream import _check, _cond
from tests.test_gpu_stream_batch import _build, _check as batch_check
from zonos_vibes_amd.autoencoder import pack_conv_transpose
from zonos_vibes_amd.config import tiny_hybrid, tiny_transformer

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNKS = (1, 4, 16)
NAN16 = 0x7E51  # an fp16 NaN of known payload


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------ zmi_dac_conv_t_range_lanes
CONV_T = ((8, 4, 32), (2, 1, 32), (8, 4, 64))  # stride, pad, c_out (64: the staged and loader-wave kernels' class)
T_IN, C_IN, C_OUT, LANES = 5, 64, 32, 2


def _conv_t_case(stride, pad, c_out=C_OUT):
    cs = [dc.conv_t_inputs(C_IN, c_out, stride, T_IN, pad, 700 + lane) for lane in range(LANES)]
    w = pack_conv_transpose(cs[0]["w"], stride, pad).to(DEV)
    bias, alpha = cs[0]["bias"].float().to(DEV), cs[0]["alpha"].float().to(DEV)
    x = torch.stack([c["x"].half() for c in cs]).to(DEV)
    return x, w, bias, alpha


def _filled(*shape):
    return torch.full(shape, NAN16, dtype=torch.int16, device=DEV)


@pytest.mark.parametrize("shape", CONV_T, ids=str)
def test_conv_t_range_equals_slices_of_conv_t(gpu_lib, shape):
    """Rows [n0, n0 + n) of zmi_dac_conv_t_lanes, under every tile form: the first row, the last row the streaming
    frontier s t - p allows, a range that starts and ends inside phase groups, and the whole; every byte outside
    the range keeps its NaN payload."""
    s, p, C_OUT = shape
    x, w, bias, alpha = _conv_t_case(s, p, C_OUT)
    to = s * T_IN
    want = {k: _filled(LANES, to, C_OUT) for k in ("raw", "snake")}
    rc = gpu_lib.zmi_dac_conv_t_lanes(x.data_ptr(), T_IN, C_IN, w.data_ptr(), bias.data_ptr(), C_OUT, s, p,
                                      want["raw"].data_ptr(), want["snake"].data_ptr(), alpha.data_ptr(), LANES,
                                      T_IN * C_IN, to * C_OUT, to * C_OUT, _stream())
    assert rc == 0, gpu_lib.zmi_last_error()
    assert not (want["raw"] == NAN16).all(-1).any()
    ranges = [(0, 1), (s * T_IN - p - 1, 1), (s - 1 if s > 2 else 1, s + 3), (0, to)]
    with forms(gpu_lib) as f:
        for n0, n in ranges:
            got = {}

            def launch():
                got.update({k: _filled(LANES, to, C_OUT) for k in ("raw", "snake")})
                rc = gpu_lib.zmi_dac_conv_t_range_lanes(
                    x.data_ptr(), 0, T_IN, C_IN, w.data_ptr(), bias.data_ptr(), C_OUT, s, p, n0, n,
                    got["raw"][0, n0].data_ptr(), got["snake"][0, n0].data_ptr(), alpha.data_ptr(), LANES, T_IN * C_IN,
                    to * C_OUT, to * C_OUT, _stream())
                assert rc == 0, gpu_lib.zmi_last_error()
                torch.cuda.synchronize()
                for k in got:
                    assert torch.equal(got[k][:, n0: n0 + n], want[k][:, n0: n0 + n]), (k, n0, n)
                    assert (got[k][:, :n0] == NAN16).all() and (got[k][:, n0 + n:] == NAN16).all(), (k, n0, n)
                return {}
            f.run(launch)


def test_conv_t_range_with_an_input_window(gpu_lib):
    """x0 > 0: the input given starts at row x0 of the utterance (the carried history row and the new rows)."""
    s, p = 8, 4
    x, w, bias, alpha = _conv_t_case(s, p)
    to = s * T_IN
    want = _filled(LANES, to, C_OUT)
    assert gpu_lib.zmi_dac_conv_t_lanes(x.data_ptr(), T_IN, C_IN, w.data_ptr(), bias.data_ptr(), C_OUT, s, p,
                                        want.data_ptr(), None, alpha.data_ptr(), LANES, T_IN * C_IN, to * C_OUT, 0,
                                        _stream()) == 0
    x0, n0, n = 2, 3 * s - p, s + 5  # row n0 reads input rows 2 and 3
    got = _filled(LANES, to, C_OUT)
    rc = gpu_lib.zmi_dac_conv_t_range_lanes(x[0, x0].data_ptr(), x0, T_IN - x0, C_IN, w.data_ptr(), bias.data_ptr(),
                                            C_OUT, s, p, n0, n, got[0, n0].data_ptr(), None, alpha.data_ptr(), LANES,
                                            T_IN * C_IN, to * C_OUT, 0, _stream())
    assert rc == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(got[:, n0: n0 + n], want[:, n0: n0 + n])
    assert (got[:, :n0] == NAN16).all() and (got[:, n0 + n:] == NAN16).all()


def test_conv_t_range_empty_and_bad_bounds(gpu_lib):
    s, p = 8, 4
    x, w, bias, alpha = _conv_t_case(s, p)
    to = s * T_IN
    out = _filled(LANES, to, C_OUT)

    def call(x0, t_in, n0, n, lanes=LANES, ls=to * C_OUT):
        return gpu_lib.zmi_dac_conv_t_range_lanes(x.data_ptr(), x0, t_in, C_IN, w.data_ptr(), bias.data_ptr(), C_OUT,
                                                  s, p, n0, n, out.data_ptr(), None, alpha.data_ptr(), lanes,
                                                  T_IN * C_IN, ls, 0, _stream())

    assert call(0, T_IN, 7, 0) == 0            # n = 0 launches nothing
    assert call(0, T_IN, -1, 4) != 0           # before the first row
    assert call(0, T_IN, 0, -1) != 0
    assert call(0, T_IN, to - 3, 4) != 0       # past the last row, stride (x0 + t_in)
    assert call(2, T_IN - 2, s - p, 4) != 0    # reads input row 0 < x0
    assert call(0, T_IN, 0, 8, lanes=0) != 0
    assert call(0, T_IN, 0, 8, ls=8 * C_OUT - 1) != 0  # a lane's stride below its extent
    assert b"dac_conv" in gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert (out == NAN16).all()  # nothing ran


# ------------------------------------------------------------------------------------------------ zmi_dac_state_move
def _segs(*segs):
    flat = [v for g in segs for v in g]
    return (ctypes.c_uint32 * len(flat))(*flat), len(segs)


def test_state_move_round_trip(gpu_lib):
    """Lanes (2, 0) of a 3-lane pool, segments of 1 row x 32 and 54 rows x 96 halfs: gather, then scatter into a second
    pool, moves exactly the segments; lane 1 and every byte outside them keep their NaN payload; the zero mode
    writes zeros to the scratch segments and reads nothing."""
    a, b = 1 * 32 // 8, 54 * 96 // 8                     # segment sizes in 16-byte units
    lane_units, gap = a + b + 6, 3                       # pool lane: [2 slack | a | 2 slack | b | 2 slack]
    pa, pb = 2, 2 + a + 2
    sls_a, sls_b = a + 1, b + gap                        # scratch lane strides: not dense
    sa, sb = 5, 5 + 2 * sls_a + 7
    scratch_units = sb + 2 * sls_b + 4
    g = torch.Generator().manual_seed(4)
    pool = torch.randint(-30000, 30000, (3, lane_units * 8), generator=g, dtype=torch.int16).to(DEV)
    scratch = _filled(scratch_units * 8)
    ids = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    segs, n = _segs((pa, sa, a, sls_a), (pb, sb, b, sls_b))

    def move(p, mode, lanes=2, ids_=ids, segs_=segs, n_=n, scratch_units_=scratch_units):
        return gpu_lib.zmi_dac_state_move(p.data_ptr(), lane_units, 3, scratch.data_ptr(), scratch_units_,
                                          ids_.data_ptr(), lanes, segs_, n_, mode, _stream())

    assert move(pool, 0) == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    want = _filled(scratch_units * 8)
    for l, lane in enumerate((2, 0)):
        want[(sa + l * sls_a) * 8: (sa + l * sls_a + a) * 8] = pool[lane, pa * 8: (pa + a) * 8]
        want[(sb + l * sls_b) * 8: (sb + l * sls_b + b) * 8] = pool[lane, pb * 8: (pb + b) * 8]
    assert torch.equal(scratch, want)
    back = _filled(3, lane_units * 8)
    assert move(back, 1) == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    inside = torch.zeros(lane_units * 8, dtype=torch.bool, device=DEV)
    inside[pa * 8: (pa + a) * 8] = True
    inside[pb * 8: (pb + b) * 8] = True
    for lane in (0, 2):
        assert torch.equal(back[lane][inside], pool[lane][inside])
        assert (back[lane][~inside] == NAN16).all()
    assert (back[1] == NAN16).all()
    # zero mode: the same scratch bytes, zeros; the pool is not touched
    assert move(back, 2) == 0, gpu_lib.zmi_last_error()
    torch.cuda.synchronize()
    assert torch.equal(scratch == 0, want != NAN16) and torch.equal(scratch == NAN16, want == NAN16)
    # nothing to do, and refused calls
    before = scratch.clone()
    assert move(pool, 0, lanes=0) == 0 and move(pool, 0, n_=0) == 0
    assert move(pool, 3) != 0                                                 # mode
    assert move(pool, 0, segs_=_segs((pa, sa, a + b + 5, sls_b))[0], n_=1) != 0    # leaves the lane's state
    assert move(pool, 0, scratch_units_=sb + sls_b + b - 1) != 0              # leaves the scratch
    assert move(pool, 0, segs_=_segs((pa, sa, a, a - 1))[0], n_=1) != 0        # lane stride below the count
    assert b"dac_state_move" in gpu_lib.zmi_last_error()
    bad = torch.tensor([3, -1], dtype=torch.int32, device=DEV)                # ids outside the pool move nothing
    assert move(pool, 0, ids_=bad) == 0
    torch.cuda.synchronize()
    assert torch.equal(scratch, before)


# --------------------------------------------------------------------------------------- stream_decoder(carry=True)
@pytest.fixture(scope="module")
def dac():
    from zonos_vibes_amd.autoencoder import DACAutoencoder
    return DACAutoencoder(DEV)


@pytest.fixture(scope="module")
def offline(dac):
    """decode() of each test utterance, computed once."""
    out = {}
    for T in sorted({T for c in CHUNKS for T in lengths(c)}):
        codes = random_codes(T, seed=T).to(DEV)
        out[T] = (codes, dac.decode(codes))
    return out


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_carry_stream_decoder_equals_decode(dac, offline, chunk, capture):
    """Every split of the codes into pushes gives decode()'s bits, with and without the captured steady-state step;
    the same object serves every utterance, so no state is left over."""
    dec = dac.stream_decoder(chunk, capture=capture, carry=True)
    step = dec.decode_step
    pushed = 0
    for T in lengths(chunk):
        codes, want = offline[T]
        for pattern in PATTERNS:
            got = run_stream(dec, codes, pushes(pattern, T))
            pushed += T
            assert got.shape == want.shape and got.dtype == torch.float32 and got.device == want.device
            assert torch.equal(got, want), (T, pattern, float((got - want).abs().max()))
    # whole chunks past the utterance's start take the steady-state step
    assert (step.graph_replays > 0) == capture
    assert step.frames_computed == pushed  # a push costs its own frames
    codes, want = offline[75]
    assert torch.equal(run_stream(dec, codes, pushes("ragged", 75)), want)


def test_carry_rollback(dac, offline):
    """stream()'s rollback: a push past the utterance's end is undone by _restore, two pushes back too."""
    dec = dac.stream_decoder(4, carry=True)
    codes, want = offline[75]
    c = codes[0]
    parts = [dec.push(c[:, :30])]
    saved = dec._state()
    dec.push(c[:, 30:34] + 1 - 2 * (c[:, 30:34] % 2))  # other codes, then more of them
    dec.push(c[:, 34:38])
    dec._restore(saved)
    parts += [dec.push(c[:, 30:]), dec.flush()]
    assert torch.equal(torch.cat(parts, dim=-1), want)
    saved = dec._state()  # at an utterance's start
    dec.push(c[:, :20])
    dec._restore(saved)
    assert torch.equal(run_stream(dec, codes, pushes("ragged", 75)), want)


# ---------------------------------------------------------------------------------- stream_decoder_batch(carry=True)
def test_carry_batch_staggered_lanes(dac):
    """Three lanes, staggered: lane 1 starts while lane 0 is mid-stream, lane 2 starts as lane 0 flushes; lane 0 is
    then reset() in the middle of a second utterance, the state pool poisoned with NaN, and the lane used again.
    Every lane's chunks are its own decode(). Mid-stream lanes that push equal n are one launch sequence whatever
    their positions, and the frames computed at the code rate are the frames pushed (the window decoder computes
    36 for 16 in the steady state)."""
    chunk = 4
    T = (41, 37, 23)
    codes = [random_codes(t, seed=500 + t).to(DEV) for t in T]
    want = [dac.decode(c) for c in codes]
    dec = dac.stream_decoder_batch(3, chunk, carry=True)
    steps = dec.decode_steps
    got = {0: [], 1: [], 2: []}
    pushed = 0

    def push(d):
        nonlocal pushed
        pushed += sum(c.shape[-1] for c in d.values())
        for lane, w in dec.push(d).items():
            got[lane].append(w)

    def flush(lanes):
        for lane, w in dec.flush(lanes).items():
            got[lane].append(w)

    c0, c1, c2 = (c[0] for c in codes)
    push({0: c0[:, :13]})                                   # lane 0 alone: 13 frames in
    push({0: c0[:, 13:17], 1: c1[:, :12]})                  # lane 1 starts while lane 0 is mid-stream
    before = steps.lane_launches
    push({1: c1[:, 12:16], 0: c0[:, 17:21]})                # both mid-stream, equal n, different positions
    assert steps.lane_launches == before + 1 and steps.launch_log[-1] == ((1, 0), 4)
    push({0: c0[:, 21:], 1: c1[:, 16:30], 2: c2[:, :5]})    # lane 2 starts as lane 0 ends
    flush([0])
    push({1: c1[:, 30:], 2: c2[:, 5:]})
    flush([2, 1])
    for lane in range(3):
        wav = torch.cat(got[lane], dim=-1)
        assert wav.shape == want[lane].shape
        assert torch.equal(wav, want[lane]), (lane, float((wav - want[lane]).abs().max()))
    assert steps.frames_computed == pushed == sum(T)
    # a partial utterance on lane 0, dropped; every lane's state poisoned; lane 0 and lane 2 used again
    got = {0: [], 1: [], 2: []}
    push({0: c1[:, :19]})
    dec.reset(0)
    assert dec.frames_received(0) == 0
    steps.state.pool.view(torch.int16).fill_(NAN16)
    got = {0: [], 1: [], 2: []}
    push({0: c0[:, :20], 2: c2[:, :20]})
    push({0: c0[:, 20:], 2: c2[:, 20:]})
    flush([0, 2])
    for lane in (0, 2):
        assert torch.equal(torch.cat(got[lane], dim=-1), want[lane]), lane
    # one steady round of two lanes at chunk 16: the window decoder computes 2 R + 16 = 36 frames per lane, the carried
    # one the 16 pushed
    long = [random_codes(80, seed=9 + i).to(DEV)[0] for i in range(2)]
    counts = {}
    for carry in (False, True):
        d = dac.stream_decoder_batch(2, 16, carry=carry)
        counter = d.decode_steps if carry else d.decode_windows
        for a in range(0, 48, 16):
            d.push({i: long[i][:, a: a + 16] for i in range(2)})
        before = counter.frames_computed
        d.push({i: long[i][:, 48: 64] for i in range(2)})
        counts[carry] = counter.frames_computed - before
    assert counts == {False: 2 * 36, True: 2 * 16}


# ------------------------------------------------------------------------------ Zonos.stream / stream_batch / serve
@pytest.fixture(scope="module")
def model_no_eos():
    return _build(tiny_transformer(), zero_eos=True)


@pytest.fixture(scope="module")
def model_eos():
    return _build(tiny_transformer(), eos_row_scale=6.0)


@pytest.mark.parametrize("chunk_frames", [4, 16])
def test_stream_carry_equals_generate_then_decode(model_no_eos, chunk_frames):
    prefix = random_codes(12, seed=5).to(DEV)
    codes, want, chunks = _both(model_no_eos, 7, _cond(12, 9), chunk_frames, audio_prefix_codes=prefix,
                                max_new_tokens=40, sampling_params=dict(min_p=0.1))
    assert codes.shape[-1] == 52
    _check(codes, want, chunks)
    # the same chunk boundaries as the default decoder
    torch.manual_seed(7)
    default = list(model_no_eos.stream(_cond(12, 9), chunk_frames=chunk_frames, audio_prefix_codes=prefix,
                                       max_new_tokens=40, sampling_params=dict(min_p=0.1)))
    assert len(default) == len(chunks) and all(torch.equal(a, b) for a, b in zip(default, chunks))


def test_stream_carry_ended_by_eos(model_eos):
    """The EOS countdown ends the utterance inside a round already decoded: the carried state is rolled back."""
    codes, want, chunks = _both(model_eos, 1, _cond(23, 10), 4, max_new_tokens=40,
                                sampling_params=dict(temperature=0.0))
    assert 0 < codes.shape[-1] <= 20, codes.shape
    _check(codes, want, chunks)


def test_stream_carry_hybrid():
    model = _build(tiny_hybrid(), zero_eos=True)
    codes, want, chunks = _both(model, 3, _cond(14, 10), 8, max_new_tokens=30, sampling_params=dict(min_p=0.1))
    assert codes.shape[-1] == 30
    _check(codes, want, chunks)


def _both(model, seed, cond, chunk_frames, **kw):
    """(codes, decode(generate()), the chunks of stream(decoder="carry")) under the same torch.manual_seed."""
    torch.manual_seed(seed)
    codes = model.generate(cond, progress_bar=False, **kw)
    want = model.autoencoder.decode(codes)
    torch.manual_seed(seed)
    chunks = list(model.stream(cond, chunk_frames=chunk_frames, decoder="carry", **kw))
    return codes, want, chunks


MNT3 = (40, 24, 33)


def _three():
    conds = [_cond(30 + i, 9 + i) for i in range(3)]
    prefixes = [None, random_codes(12, seed=5).to(DEV), None]
    return conds, prefixes


@pytest.mark.parametrize("sample_rate", [None, 24000])
def test_stream_batch_carry_equals_the_default_decoder(model_no_eos, sample_rate):
    """3 utterances over 2 slots, one with an audio prefix: per utterance the items are the default decoder's, item
    for item (the chunk boundaries do not move, so the resampler sees the same pieces)."""
    conds, prefixes = _three()
    kw = dict(max_new_tokens=list(MNT3), chunk_frames=4, sampling_params=dict(min_p=0.1), seeds=[50, 51, 52],
              max_slots=2, sample_rate=sample_rate)
    window = list(model_no_eos.stream_batch(conds, prefixes, **kw))
    carry = list(model_no_eos.stream_batch(conds, prefixes, decoder="carry", **kw))
    assert len(window) == len(carry) > 3
    for (i, w, last), (j, v, last2) in zip(window, carry):
        assert (i, last) == (j, last2) and torch.equal(w, v), (i, w.shape, v.shape)
    if sample_rate is None:
        codes = model_no_eos.generate_batch(conds, prefixes, max_new_tokens=list(MNT3), sampling_params=dict(min_p=0.1),
                                            seeds=[50, 51, 52], max_slots=2)
        batch_check([model_no_eos.autoencoder.decode(c) for c in codes], carry)


@pytest.mark.parametrize("sample_rate", [None, 24000])
def test_serve_carry_equals_the_default_decoder(model_no_eos, sample_rate):
    conds, prefixes = _three()
    reqs = [Req(conds[i], prefixes[i], MNT3[i], dict(min_p=0.1), 2.0, 50 + i) for i in range(3)]
    runs = {}
    for decoder in ("window", "carry"):
        with model_no_eos.serve(2, max_seqlen=128, max_prefill=64, chunk_frames=4, sample_rate=sample_rate,
                                decoder=decoder) as session:
            tickets = {r.submit(session): r for r in reqs[:2]}
            items = session.run_round() + session.run_round()
            tickets[reqs[2].submit(session)] = reqs[2]  # admitted mid-stream, when a slot frees
            runs[decoder] = (tickets, drain(session, items))
    (_, window), (tickets, carry) = runs["window"], runs["carry"]
    assert len(window) == len(carry) > 3
    for (t, w, last), (u, v, last2) in zip(window, carry):
        assert (t, last) == (u, last2) and torch.equal(w, v), (t, w.shape, v.shape)
    if sample_rate is None:
        serve_check({t: alone(model_no_eos, r) for t, r in tickets.items()}, carry)


def test_unknown_decoder_is_refused(model_no_eos):
    cond = _cond(11, 12)
    with pytest.raises(ValueError):
        next(model_no_eos.stream(cond, max_new_tokens=4, decoder="nope"))
    with pytest.raises(ValueError):
        next(model_no_eos.stream_batch([cond], max_new_tokens=4, decoder="nope"))
    with pytest.raises(ValueError):
        model_no_eos.serve(2, max_seqlen=128, max_prefill=64, decoder="nope")
    gen = model_no_eos.stream(cond, max_new_tokens=12, decoder="window")
    assert next(gen).shape[-1] > 0
    gen.close()
