"""zmi_pcm16_pack against the reference server's conversion (server.py:142-146) as torch evaluates it on the CPU:
(t.clamp(-1, 1) * 32767.0).to(torch.int16), bit for bit, over segment lengths around the kernel's head / middle / tail
and piece edges, source and destination alignments, and the special values."""
import numpy as np
import pytest
import torch

from zonos_vibes_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -12345
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 511, 512, 513, 8193)


def _specials() -> torch.Tensor:
    f = np.float32
    v = [1.0, -1.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-40, 0.99999994]
    for k in (1, 2, 16383, 32766, 32767):
        for sgn in (1.0, -1.0):
            x = f(sgn * k) / f(32767)
            v += [x, np.nextafter(x, f(np.inf), dtype=f), np.nextafter(x, f(-np.inf), dtype=f)]
    with np.errstate(over="ignore"):
        return torch.from_numpy(np.array(v, dtype=np.float32))


def _values(n: int, seed: int) -> torch.Tensor:
    """n inputs: the special values (cycled through, so short segments see them too) among seeded uniform ones."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, generator=g) * 2.4 - 1.2
    sp = _specials()
    idx = torch.arange(0, n, 3)
    x[idx] = sp[(idx // 3 + seed) % len(sp)]
    return x


def reference(x: torch.Tensor) -> torch.Tensor:
    return (x.clamp(-1, 1) * 32767.0).to(torch.int16)


def test_reference_is_the_issue_s_arithmetic():
    """The CPU expression truncates fp32 products toward zero and sends NaN to 0, as the kernel spells out."""
    x = torch.tensor([0.99999994, 3.06e-5, -3.06e-5, float("nan"), float("inf"), -float("inf"), -0.0, 1e-40, -1.5])
    assert reference(x).tolist() == [32766, 1, -1, 0, 32767, -32767, 0, 0, -32767]
    with np.errstate(invalid="ignore"):  # numpy warns about the NaN's cast (and gives 0)
        assert torch.equal(reference(x), torch.from_numpy((np.clip(x.numpy(), -1, 1) * 32767).astype(np.int16)))


def pack(lengths, src_offset: int, base: int, seed: int = 0):
    """Segments of `lengths` samples, each a slice of ONE fp32 device tensor starting `src_offset` elements past a
    256-byte boundary (then back to back, so later segments start wherever the lengths put them), packed from int16
    index `base` of a guard-filled buffer. Returns (out on the CPU, expected)."""
    lib = _lib.lib()
    total_in = sum(lengths)
    x = _values(total_in + 8, seed)
    xd = x.to(DEV)
    assert xd.data_ptr() % 256 == 0
    rows, want, pos, dst = [], [], src_offset, base
    for n in lengths:
        rows.append((xd.data_ptr() + 4 * pos, n, dst))
        want.append(reference(x[pos: pos + n]))
        pos, dst = pos + n, dst + n
    total = dst
    out = torch.full((total + 64,), GUARD, dtype=torch.int16, device=DEV)
    segs = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3).to(DEV)
    s = torch.cuda.current_stream()
    _lib.check(lib.zmi_pcm16_pack(segs.data_ptr(), len(rows), total, out.data_ptr(), s.cuda_stream), "pcm16_pack")
    s.synchronize()
    exp = torch.full((total + 64,), GUARD, dtype=torch.int16)
    if want:
        exp[base: total] = torch.cat(want)
    return out.cpu(), exp


@pytest.mark.parametrize("base", [0, 1, 6, 2047], ids=lambda b: f"dst{b}")
@pytest.mark.parametrize("src_offset", [0, 1, 2, 3], ids=lambda o: f"src{o}")
@pytest.mark.parametrize("n", LENGTHS)
def test_one_segment(n, src_offset, base):
    got, want = pack([n], src_offset, base, seed=n + src_offset)
    assert torch.equal(got, want), (got != want).nonzero()[:8].flatten().tolist()


@pytest.mark.parametrize("base", [0, 1], ids=lambda b: f"dst{b}")
@pytest.mark.parametrize("src_offset", [0, 1, 2, 3], ids=lambda o: f"src{o}")
def test_five_segments_together(src_offset, base):
    got, want = pack([3, 512, 1, 0, 1025], src_offset, base, seed=17)
    assert torch.equal(got, want), (got != want).nonzero()[:8].flatten().tolist()
    assert (got[:base] == GUARD).all() and (got[base + 1541:] == GUARD).all()  # nothing outside [first dst, total)


def test_a_round_s_shape():
    """What the session launches: many 512-multiples back to back, more than one piece per segment."""
    got, want = pack([512 * f for f in (4, 16, 0, 23, 16, 1)], 0, 0, seed=3)
    assert torch.equal(got, want)


def test_every_special_value_elementwise():
    """The special values in every position of the head / 4-sample unit / tail split (shifted through 8 offsets)."""
    sp = _specials()
    lib = _lib.lib()
    s = torch.cuda.current_stream()
    for shift in range(8):
        x = torch.cat([torch.zeros(shift), sp])
        xd = x.to(DEV)
        out = torch.full((x.numel() + 8,), GUARD, dtype=torch.int16, device=DEV)
        segs = torch.tensor([[xd.data_ptr(), x.numel(), 3]], dtype=torch.int64).to(DEV)
        _lib.check(lib.zmi_pcm16_pack(segs.data_ptr(), 1, 3 + x.numel(), out.data_ptr(), s.cuda_stream), "pcm16_pack")
        s.synchronize()
        assert torch.equal(out.cpu()[3: 3 + x.numel()], reference(x)), shift
        assert (out.cpu()[:3] == GUARD).all() and (out.cpu()[3 + x.numel():] == GUARD).all()


def test_no_segments_launch_nothing():
    lib = _lib.lib()
    out = torch.full((16,), GUARD, dtype=torch.int16, device=DEV)
    s = torch.cuda.current_stream()
    assert lib.zmi_pcm16_pack(None, 0, 0, out.data_ptr(), s.cuda_stream) == 0
    assert lib.zmi_pcm16_pack(None, 0, 16, out.data_ptr(), s.cuda_stream) == 0
    s.synchronize()
    assert (out.cpu() == GUARD).all()
    assert lib.zmi_pcm16_pack(None, -1, 0, out.data_ptr(), s.cuda_stream) != 0  # an error, not a launch
