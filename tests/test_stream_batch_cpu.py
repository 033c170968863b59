"""CPU checks of DACBatchStreamDecoder: every lane behaves as a DACStreamDecoder of its own, all windows of a call
go to one decode_windows call, and reset(lane) leaves the other lanes alone. decode_windows is the oracle's decode
on the thinned weights of test_stream_cpu (same layer list, so the same lookahead)."""
import pytest
import torch
from tests.helpers import dac_weights
from tests.stream_cases import PATTERNS, pushes, random_codes
from tests.test_stream_cpu import thin_weights

from oracle.dac_cpu import OracleDAC
from zonos_vibes_amd.streaming import DAC_LOOKAHEAD_FRAMES, DACBatchStreamDecoder, DACStreamDecoder

LENGTHS = (5, 23, 41)
CHUNK = 4
STAGGER = 2  # lane l makes its first push in round STAGGER * l: the lanes are at different phases


@pytest.fixture(scope="module")
def oracle():
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    return OracleDAC(thin_weights(dac_weights(0)))


def _window(oracle, codes, f0, f1):
    return oracle.decode(codes[None])[..., 512 * f0: 512 * f1]


def _schedule(pattern):
    """Per round, {lane: (start, size)} of the pushes made in it; a lane whose pushes are used up is flushed."""
    plan = {lane: pushes(pattern, T) for lane, T in enumerate(LENGTHS)}
    rounds = max(STAGGER * lane + len(p) for lane, p in plan.items())
    out = []
    for r in range(rounds + 1):
        step, flush = {}, []
        for lane, p in plan.items():
            k = r - STAGGER * lane
            if 0 <= k < len(p):
                step[lane] = (sum(p[:k]), p[k])
            elif k == len(p):
                flush.append(lane)
        out.append((step, flush))
    return out


@pytest.mark.parametrize("pattern", PATTERNS)
def test_each_lane_equals_its_own_stream_decoder(oracle, pattern):
    calls = []

    def decode_windows(windows):
        calls.append([(c.shape[1], f0, f1) for c, f0, f1 in windows])
        return [_window(oracle, c, f0, f1) for c, f0, f1 in windows]

    codes = [random_codes(T, seed=100 + T) for T in LENGTHS]
    dec = DACBatchStreamDecoder(decode_windows, len(LENGTHS), chunk_frames=CHUNK)
    single_calls = {lane: [] for lane in range(len(LENGTHS))}
    singles = []
    for lane in range(len(LENGTHS)):
        def decode_window(c, f0, f1, lane=lane):
            single_calls[lane].append((c.shape[1], f0, f1))
            return _window(oracle, c, f0, f1)
        singles.append(DACStreamDecoder(decode_window, chunk_frames=CHUNK))
    got = {lane: [] for lane in range(len(LENGTHS))}
    for step, flush in _schedule(pattern):
        for sc in single_calls.values():
            sc.clear()
        if step:
            before = len(calls)
            # both accepted shapes: [1, 9, n] and [9, n]
            res = dec.push({lane: codes[lane][..., t: t + n] if lane % 2 else codes[lane][0, :, t: t + n]
                            for lane, (t, n) in step.items()})
            assert sorted(res) == sorted(step)
            want = {lane: singles[lane].push(codes[lane][..., t: t + n]) for lane, (t, n) in step.items()}
            # one decode_windows call holds every lane's windows of this push, each lane's in its own order
            due = [w for lane in step for w in single_calls[lane]]
            assert len(calls) - before == (1 if due else 0), (pattern, step)
            if due:
                assert calls[-1] == due
            for lane in step:
                assert res[lane].shape[:2] == (1, 1) and torch.equal(res[lane], want[lane]), (pattern, lane)
                got[lane].append(res[lane])
                assert dec.frames_received(lane) == singles[lane].frames_received
                assert dec.frames_emitted(lane) == singles[lane].frames_emitted
        if flush:
            for sc in single_calls.values():
                sc.clear()
            before = len(calls)
            res = dec.flush(flush)
            want = {lane: singles[lane].flush() for lane in flush}
            assert len(calls) - before == (1 if any(single_calls[lane] for lane in flush) else 0)
            for lane in flush:
                assert torch.equal(res[lane], want[lane]), (pattern, lane)
                got[lane].append(res[lane])
                assert dec.frames_received(lane) == 0
    for lane, T in enumerate(LENGTHS):
        wav = torch.cat(got[lane], dim=-1)
        assert wav.shape == (1, 1, 512 * T)
        # and the stream equals the offline decode to the bound of test_stream_cpu's thin sweep
        assert float((wav - oracle.decode(codes[lane])).abs().max()) <= 1e-6
    assert all(w <= 2 * DAC_LOOKAHEAD_FRAMES + CHUNK and f1 - f0 <= CHUNK for call in calls for w, f0, f1 in call)


def test_reset_leaves_the_other_lanes_untouched(oracle):
    def decode_windows(windows):
        return [_window(oracle, c, f0, f1) for c, f0, f1 in windows]

    codes = [random_codes(T, seed=200 + T) for T in LENGTHS]
    dec = DACBatchStreamDecoder(decode_windows, 3, chunk_frames=CHUNK)
    ref = DACBatchStreamDecoder(decode_windows, 3, chunk_frames=CHUNK)
    first = {lane: codes[lane][0, :, :4] for lane in range(3)}
    a, b = dec.push(first), ref.push({0: first[0], 2: first[2]})
    dec.reset(1)
    assert dec.frames_received(1) == dec.frames_emitted(1) == 0
    rest = {lane: codes[lane][0, :, 4:] for lane in (0, 2)}
    a2, b2 = dec.push(rest), ref.push(rest)
    a3, b3 = dec.flush([0, 2]), ref.flush([0, 2])
    for lane in (0, 2):
        for x, y in ((a, b), (a2, b2), (a3, b3)):
            assert torch.equal(x[lane], y[lane])
    # the reset lane starts a new utterance from frame 0
    w = dec.push({1: codes[0][0]})[1]
    w = torch.cat([w, dec.flush([1])[1]], dim=-1)
    one = DACStreamDecoder(lambda c, f0, f1: _window(oracle, c, f0, f1), chunk_frames=CHUNK)
    want = torch.cat([one.push(codes[0]), one.flush()], dim=-1)
    assert torch.equal(w, want)


def test_arguments():
    dec = DACBatchStreamDecoder(lambda ws: [torch.zeros(1, 1, 512 * (f1 - f0)) for _, f0, f1 in ws], 2, chunk_frames=4)
    assert dec.push({}) == {} and dec.flush([]) == {}
    assert dec.push({0: torch.zeros(9, 3, dtype=torch.int64)})[0].shape == (1, 1, 0)
    with pytest.raises(ValueError):
        dec.push({2: torch.zeros(9, 3, dtype=torch.int64)})
    with pytest.raises(ValueError):
        dec.push({1: torch.zeros(2, 9, 3, dtype=torch.int64)})
    assert dec.frames_received(0) == 3 and dec.frames_received(1) == 0
    with pytest.raises(ValueError):
        DACBatchStreamDecoder(lambda ws: [], 0)
    bad = DACBatchStreamDecoder(lambda ws: [], 1, chunk_frames=4)
    with pytest.raises(RuntimeError):
        bad.push({0: torch.zeros(9, 30, dtype=torch.int64)})
