"""Plain-torch CPU restatement of the speaker encoder (reference zonos/speaker_cloning.py), its log-mel filterbank
and its resampler (torchaudio's documented defaults), for the speaker tests.

`operand_dtype=torch.float16` rounds exactly where the HIP kernels round: the conv inputs (every stored activation,
the features included), the conv weights, and every stored activation (conv + BatchNorm (+ ReLU) outputs, block
outputs). Accumulation, the BatchNorm scale / shift, the SimAM statistics and the tail stay fp32 in both modes.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-5


def block_plan(in_planes, num_blocks):
    out, c = [], in_planes
    for li, n in enumerate(num_blocks):
        planes = in_planes << li
        for b in range(n):
            out.append((f"front.layer{li + 1}.{b}.", c, planes, (1 if li == 0 else 2) if b == 0 else 1))
            c = planes
    return out


class SpeakerCPU:
    def __init__(self, sd: dict, lda: dict, in_planes: int, num_blocks, operand_dtype=torch.float32):
        self.sd = {k: v.float() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        self.lda = {k: v.float() for k, v in lda.items()}
        self.in_planes, self.num_blocks, self.dt = in_planes, tuple(num_blocks), operand_dtype

    def q(self, t):  # a stored activation / a conv operand
        return t.to(self.dt).float()

    def conv_bn(self, x, conv, bn, stride, relu):
        w = self.sd[conv + ".weight"]
        y = F.conv2d(x, self.q(w), None, stride, w.shape[-1] // 2)
        # eval BatchNorm with the reference's own op (the kernels apply it as fp32 scale / shift: an fp32-ulp
        # difference before the fp16 rounding, of the same kind as their summation order)
        y = F.batch_norm(y, self.sd[bn + ".running_mean"], self.sd[bn + ".running_var"], self.sd[bn + ".weight"],
                         self.sd[bn + ".bias"], False, 0.0, BN_EPS)
        return self.q(torch.relu(y) if relu else y)

    def simam_tail(self, x, res):
        """speaker_cloning.py:83-96 after bn2: SimAM, + residual, ReLU; stored once."""
        n = x.shape[2] * x.shape[3] - 1
        d = (x - x.mean(dim=[2, 3], keepdim=True)).pow(2)
        v = d.sum(dim=[2, 3], keepdim=True) / n
        return self.q(torch.relu(x * torch.sigmoid(d / (4 * (v + 1e-4)) + 0.5) + res))

    def front(self, feat, record=None):
        """feat [H, W] fp32 -> [1, C, H / 8, W / 8]"""
        x = self.conv_bn(self.q(feat)[None, None], "front.conv1", "front.bn1", 1, True)
        if record is not None:
            record["stem"] = x
        for p, ci, co, s in block_plan(self.in_planes, self.num_blocks):
            out = self.conv_bn(x, p + "conv1", p + "bn1", s, True)
            out = self.conv_bn(out, p + "conv2", p + "bn2", 1, False)
            res = self.conv_bn(x, p + "downsample.0", p + "downsample.1", s, False) if (s != 1 or ci != co) else x
            x = self.simam_tail(out, res)
            if record is not None:
                record[p[len("front."):-1]] = x
        return x

    def pool(self, fr):
        sd, a = self.sd, "pooling.attention."
        x = fr.reshape(1, -1, fr.shape[-1])
        h = torch.relu(F.conv1d(x, sd[a + "0.weight"], sd[a + "0.bias"]))
        h = F.batch_norm(h, sd[a + "2.running_mean"], sd[a + "2.running_var"], sd[a + "2.weight"], sd[a + "2.bias"],
                         False, 0.0, BN_EPS)
        w = torch.softmax(F.conv1d(h, sd[a + "3.weight"], sd[a + "3.bias"]), dim=2)
        mu = torch.sum(x * w, dim=2)
        sg = torch.sqrt((torch.sum((x ** 2) * w, dim=2) - mu ** 2).clamp(min=1e-5))
        return torch.cat((mu, sg), 1)

    @torch.inference_mode()
    def __call__(self, feat, record=None):
        fr = self.front(feat, record)
        pooled = self.pool(fr)
        emb = F.linear(pooled, self.sd["bottleneck.weight"], self.sd["bottleneck.bias"])
        lda = F.linear(emb, self.lda["weight"], self.lda["bias"])
        if record is not None:
            record.update(front=fr, pooled=pooled, emb=emb, lda=lda)
        return emb, lda


# ------------------------------------------------------------------------------------- front end
def resample(wav, orig, new, dtype=torch.float32, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio.functional.resample's default (sinc_interp_hann): wav [C, N] -> [C, ceil(new N / orig)]."""
    g = math.gcd(orig, new)
    orig, new = orig // g, new // g
    if orig == new:
        return wav
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = (torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)).to(dtype)
    n = wav.shape[-1]
    x = F.pad(wav.to(dtype), (width, width + orig))
    out = F.conv1d(x[:, None], kern, stride=orig)                    # [C, new, n_out]
    return out.transpose(1, 2).reshape(wav.shape[0], -1)[..., : math.ceil(new * n / orig)]


def mel_filterbank(n_freqs=257, n_mels=80, sample_rate=16000):
    """torchaudio.functional.melscale_fbanks(n_freqs, 0, sr / 2, n_mels, sr, norm=None, mel_scale='htk')."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_max = 2595.0 * math.log10(1.0 + (sample_rate / 2) / 700.0)
    f_pts = 700.0 * (10 ** (torch.linspace(0.0, m_max, n_mels + 2) / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down, up)), f_pts


def mel_power(wav, n_mels=80, n_fft=512, win_length=400, hop=160):
    """torchaudio MelSpectrogram defaults with the DFT written out: wav [1, N] at 16 kHz -> [n_mels, 1 + N // hop]."""
    win = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)
    ang = 2 * math.pi * torch.arange(n_fft, dtype=torch.float64)[:, None] * k[None] / n_fft
    x = F.pad(wav[None].float(), (n_fft // 2, n_fft // 2), mode="reflect")[0, 0]
    frames = x.unfold(0, n_fft, hop)
    re = frames @ (win[:, None] * torch.cos(ang)).float()
    im = frames @ (win[:, None] * torch.sin(ang)).float()
    return ((re ** 2 + im ** 2) @ mel_filterbank(n_fft // 2 + 1, n_mels)[0]).t()


def log_fbank(wav, n_mels=80):
    """logFbankCal (speaker_cloning.py:13-35): log(mel + 1e-6) minus each bin's mean over time."""
    out = torch.log(mel_power(wav, n_mels) + 1e-6)
    return out - out.mean(dim=1, keepdim=True)
