"""Speaker encoder with the reference's SpeakerEmbeddingLDA surface (zonos/speaker_cloning.py:356-412), on HIP.

    enc = SpeakerEmbeddingLDA("cuda")                       # synthetic weights, or state_dict= / from_files(...)
    emb, lda = enc(wav, sample_rate)                        # [1, 256] fp32, [1, 128] fp32
    embs, ldas = enc.embed_batch([(wav, sample_rate), ..])  # [B, 256], [B, 128]: row i has the bits of enc(clip i)

The ResNet293 trunk (stem, 97 SimAM blocks: 3x3 / 1x1 convs with eval BatchNorm, SimAM, residual) runs on the
kernels of csrc/zmi_spk.hip: fp16 channels-last activations, fp16 channel-blocked weights, fp32 accumulation and
fp32 BatchNorm scale / shift. The front end (mono mean, resampling to 16 kHz, log-mel filterbank) and the tail
(attentive statistics pooling, bottleneck, LDA; < 0.1 % of the work) are fp32 torch ops on the device. A batch of clips
runs the trunk as ragged lanes (one launch sequence for a group of clips, each with its own frame count: `plan_lanes`,
`front_lanes`); the front end and the tail stay per clip, so every clip keeps the bits of its single call.

torchaudio is absent in this build: the resampler and the filterbank restate its documented defaults
(`Resample`: Hann-windowed sinc, lowpass_filter_width 6, rolloff 0.99; `MelSpectrogram`: n_fft 512, periodic Hann
of 400, hop 160, centred with reflect padding, power 2, 80 HTK triangles over 0-8 kHz, norm None). Their parity
with torchaudio is unpinned.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from . import _lib
from . import synthetic as syn
from .autoencoder import _blocked

SPK_SAMPLE_RATE = 16_000
BN_EPS = 1e-5


@dataclass(frozen=True)
class SpeakerEncoderConfig:
    in_planes: int = 64
    num_blocks: tuple = (10, 20, 64, 3)
    acoustic_dim: int = 80
    embd_dim: int = 256
    lda_dim: int = 128


# ------------------------------------------------------------------------------------- state dict
def expected_shapes(config: SpeakerEncoderConfig) -> dict[str, tuple]:
    """Every key of `ResNet293_based.state_dict()` with its shape (the loader table). BatchNorm's integer
    `num_batches_tracked` counters are part of a published checkpoint; they are accepted and unused."""
    out = {}
    for sp in syn.speaker_specs(config):
        if sp.name.startswith("lda."):
            continue
        out[sp.name] = sp.shape
        if sp.name.endswith(".running_var"):
            out[sp.name[: -len("running_var")] + "num_batches_tracked"] = ()
    return out


def lda_shapes(config: SpeakerEncoderConfig) -> dict[str, tuple]:
    return {"weight": (config.lda_dim, config.embd_dim), "bias": (config.lda_dim,)}


def check_state_dict(sd: dict, table: dict[str, tuple], what: str) -> None:
    """Unknown keys, missing keys and wrong shapes are errors (num_batches_tracked may be absent)."""
    unknown = sorted(k for k in sd if k not in table)
    missing = sorted(k for k in table if k not in sd and not k.endswith("num_batches_tracked"))
    if unknown or missing:
        raise KeyError(f"{what}: unknown keys {unknown[:4]}{'...' if len(unknown) > 4 else ''}, "
                       f"missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}")
    for k, v in sd.items():
        if tuple(v.shape) != tuple(table[k]):
            raise ValueError(f"{what}: {k} has shape {tuple(v.shape)}, expected {tuple(table[k])}")


def load_weights_file(path: str) -> dict:
    """A local .safetensors or .pt state dict (torch.load with weights_only=True and nothing looser)."""
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    return torch.load(path, weights_only=True, map_location="cpu")


# ------------------------------------------------------------------------------------- front end
def resample_kernel(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """torchaudio's default `sinc_interp_hann` polyphase kernel [new][width 2 + orig] (fp32) and its half width,
    for rates already reduced by their gcd."""
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window * (base / orig)
    return kern.float(), width


def resample(wav: torch.Tensor, orig: int, new: int = SPK_SAMPLE_RATE) -> torch.Tensor:
    """[C, N] fp32 -> [C, ceil(new N / orig)]: a strided conv1d against the polyphase kernel."""
    g = math.gcd(int(orig), int(new))
    orig, new = int(orig) // g, int(new) // g
    if orig == new:
        return wav
    kern, width = resample_kernel(orig, new)
    n = wav.shape[-1]
    x = torch.nn.functional.pad(wav, (width, width + orig))
    frames = x.unfold(-1, kern.shape[1], orig)                      # [C, n_out, taps]
    out = frames @ kern.to(wav.device).t()                          # [C, n_out, new]
    return out.reshape(wav.shape[0], -1)[..., : math.ceil(new * n / orig)]


def mel_points(n_mels: int = 80, sample_rate: int = SPK_SAMPLE_RATE) -> torch.Tensor:
    """The n_mels + 2 corner frequencies (Hz) of the HTK-scale triangles over 0 .. sample_rate / 2: triangle m rises
    from point m to its peak at point m + 1 and falls to point m + 2."""
    m_max = 2595.0 * math.log10(1.0 + (sample_rate / 2) / 700.0)
    return 700.0 * (10 ** (torch.linspace(0.0, m_max, n_mels + 2) / 2595.0) - 1.0)


def mel_filterbank(n_freqs: int = 257, n_mels: int = 80, sample_rate: int = SPK_SAMPLE_RATE) -> torch.Tensor:
    """[n_freqs, n_mels] HTK-scale triangles over 0 .. sample_rate / 2, norm None (torchaudio melscale_fbanks)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    f_pts = mel_points(n_mels, sample_rate)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


def dft_basis(n_fft: int = 512, win_length: int = 400) -> torch.Tensor:
    """[n_fft, 2 (n_fft / 2 + 1)] fp32: periodic Hann of win_length centred in the frame, times cos | sin."""
    win = torch.zeros(n_fft, dtype=torch.float64)
    left = (n_fft - win_length) // 2
    win[left:left + win_length] = torch.hann_window(win_length, periodic=True, dtype=torch.float64)
    ang = 2 * math.pi * torch.arange(n_fft, dtype=torch.float64)[:, None] * \
        torch.arange(n_fft // 2 + 1, dtype=torch.float64)[None] / n_fft
    return (win[:, None] * torch.cat([torch.cos(ang), torch.sin(ang)], dim=1)).float()


def mel_power(wav: torch.Tensor, basis: torch.Tensor, fb: torch.Tensor, n_fft: int = 512, hop: int = 160) -> torch.Tensor:
    """MelSpectrogram (speaker_cloning.py:23-29) with the DFT as a matmul: [1, N] fp32 at 16 kHz -> [n_mels, 1 + N // hop]."""
    x = torch.nn.functional.pad(wav[None], (n_fft // 2, n_fft // 2), mode="reflect")[0]
    frames = x.unfold(-1, n_fft, hop)[0]                            # [T, n_fft]
    spec = frames @ basis                                           # [T, 2 F]
    f = basis.shape[1] // 2
    power = spec[:, :f] ** 2 + spec[:, f:] ** 2
    return (power @ fb).t()                                         # [n_mels, T]


def log_fbank(wav: torch.Tensor, basis: torch.Tensor, fb: torch.Tensor) -> torch.Tensor:
    """logFbankCal.forward (speaker_cloning.py:31-35): log(mel + 1e-6) minus each bin's mean over time."""
    out = torch.log(mel_power(wav, basis, fb) + 1e-6)
    return out - out.mean(dim=1, keepdim=True)


# ------------------------------------------------------------------------------------- lanes
def plan_lanes(frames: list, max_lanes: int = _lib.SPK_MAX_LANES, max_lane_frames: int = 32768) -> list:
    """Groups of clip indices, each one ragged launch sequence of the trunk: longest clips first (ties by index), at
    most `max_lanes` clips per group and len(group) x the group's longest clip <= `max_lane_frames`; a clip longer
    than that is a group of its own. The workspace holds len(group) lanes of the longest clip, and its three
    activation buffers take 3 x acoustic_dim x in_planes x 2 B = 30,720 B per lane-frame at full size, so the default
    bounds them at 32768 x 30,720 B = 1.0 GB."""
    if not 1 <= max_lanes <= _lib.SPK_MAX_LANES or max_lane_frames < 1:
        raise ValueError(f"max_lanes must be 1 .. {_lib.SPK_MAX_LANES} and max_lane_frames >= 1")
    groups = []
    for i in sorted(range(len(frames)), key=lambda i: (-frames[i], i)):
        g = groups[-1] if groups else None  # the group's first clip is its longest
        if g is None or len(g) == max_lanes or (len(g) + 1) * frames[g[0]] > max_lane_frames:
            groups.append([i])
        else:
            g.append(i)
    return groups


# ------------------------------------------------------------------------------------- the encoder
class SpeakerEmbeddingLDA:
    def __init__(self, device="cuda", state_dict: dict | None = None, lda_state_dict: dict | None = None, seed: int = 0,
                 config: SpeakerEncoderConfig = SpeakerEncoderConfig()):
        if config.in_planes % 32 or len(config.num_blocks) != 4 or config.acoustic_dim % 8:
            raise ValueError("in_planes must be a multiple of 32, acoustic_dim of 8, with four stages of blocks")
        if (state_dict is None) != (lda_state_dict is None):
            raise ValueError("give both state_dict and lda_state_dict, or neither (synthetic weights)")
        self.config = config
        self.dev = torch.device(device)
        self.lib = _lib.lib()
        if state_dict is None:
            state_dict, lda_state_dict = {}, {}
            sptr = torch.cuda.current_stream(self.dev).cuda_stream
            for sp in syn.speaker_specs(config):
                t = torch.empty(sp.shape, dtype=torch.float32, device=self.dev)
                _lib.check(self.lib.zmi_fill_uniform(t.data_ptr(), sp.numel, syn.tensor_key(seed, sp.name), sp.scale,
                                                     sp.offset, 1, sptr), "fill")
                if sp.name.startswith("lda."):
                    lda_state_dict[sp.name[4:]] = t
                else:
                    state_dict[sp.name] = t
        check_state_dict(state_dict, expected_shapes(config), "speaker encoder")
        check_state_dict(lda_state_dict, lda_shapes(config), "speaker LDA")
        self._prepare(state_dict, lda_state_dict)
        self._basis = dft_basis().to(self.dev)
        self._fb = mel_filterbank(n_mels=config.acoustic_dim).to(self.dev)
        self._lane_sizes = {}                                  # widest W -> one lane's elements per workspace buffer
        self._cap = dict(act=0, x16=0, psum=0, ws=0)           # elements allocated

    @classmethod
    def from_files(cls, ckpt_path: str, lda_path: str, device="cuda",
                   config: SpeakerEncoderConfig = SpeakerEncoderConfig()) -> "SpeakerEmbeddingLDA":
        """The published pair (ResNet293_SimAM_ASP_base.pt, ..._LDA-128.pt) from local files; no hub download."""
        return cls(device, load_weights_file(ckpt_path), load_weights_file(lda_path), config=config)

    # --------------------------------------------------------------- weight layout
    def _prepare(self, sd: dict, lda: dict):
        f32 = lambda t: t.to(self.dev, torch.float32).contiguous()  # noqa: E731

        def bn(p):  # eval BatchNorm as fp32 scale / shift, applied to the fp32 accumulator (never folded into weights)
            scale = f32(sd[p + ".weight"]) / torch.sqrt(f32(sd[p + ".running_var"]) + BN_EPS)
            return scale.contiguous(), (f32(sd[p + ".bias"]) - f32(sd[p + ".running_mean"]) * scale).contiguous()

        def conv(name):  # [co][ci][k][k] -> [tap][ci / 32][co][32] fp16
            w = f32(sd[name + ".weight"])
            co, ci, k, _ = w.shape
            return dict(w=_blocked(w.permute(2, 3, 0, 1).reshape(k * k, co, ci)), k=k, ci=ci, co=co)

        w1 = f32(sd["front.conv1.weight"])                                    # [P][1][3][3] -> [9][P]
        self.stem_w = w1.reshape(w1.shape[0], 9).t().contiguous().half()
        self.stem_bn = bn("front.bn1")
        self.blocks = []
        for p, ci, co, stride in syn.speaker_block_plan(self.config):
            blk = dict(name=p[len("front."):-1], stride=stride, c1=conv(p + "conv1"), bn1=bn(p + "bn1"),
                       c2=conv(p + "conv2"), bn2=bn(p + "bn2"), ds=None)
            if stride != 1 or ci != co:
                blk["ds"], blk["dsbn"] = conv(p + "downsample.0"), bn(p + "downsample.1")
            self.blocks.append(blk)
        a = "pooling.attention."
        self.att_w0, self.att_b0 = f32(sd[a + "0.weight"])[:, :, 0].contiguous(), f32(sd[a + "0.bias"])
        self.att_bn = [f32(sd[a + "2." + k]) for k in ("weight", "bias", "running_mean", "running_var")]
        self.att_w3, self.att_b3 = f32(sd[a + "3.weight"])[:, :, 0].contiguous(), f32(sd[a + "3.bias"])
        self.bott_w, self.bott_b = f32(sd["bottleneck.weight"]), f32(sd["bottleneck.bias"])
        self.lda_w, self.lda_b = f32(lda["weight"]), f32(lda["bias"])

    def _workspace(self, W: int, lanes: int = 1):
        """Three fp16 activation buffers (two ping-pong plus the residual) and the SimAM sums, sized from the frame
        count and grown on demand. The largest activation is the stem's [acoustic_dim][W][in_planes]. With lanes,
        W is the widest lane and every buffer holds `lanes` of them, lane l at l * `self._ls[buffer]` elements (the
        same stride at every stage: later stages are smaller)."""
        cfg = self.config
        if W not in self._lane_sizes:
            psum = ws = 0  # the largest stage's per-tile sums and SimAM workspace
            for li in range(4):
                h, w, c = (cfg.acoustic_dim - 1) // (1 << li) + 1, (W - 1) // (1 << li) + 1, cfg.in_planes << li
                psum = max(psum, self.lib.zmi_spk_conv2d_tiles(h, w, 3, 1) * c)
                ws = max(ws, self.lib.zmi_spk_simam_ws_floats(h, w, c))
            self._lane_sizes[W] = dict(act=cfg.acoustic_dim * W * cfg.in_planes, x16=cfg.acoustic_dim * W, psum=psum,
                                       ws=ws)
        self._ls = self._lane_sizes[W]
        if any(lanes * n > self._cap[k] for k, n in self._ls.items()):
            self._cap = {k: max(lanes * n, self._cap[k]) for k, n in self._ls.items()}
            self._acts = [torch.empty(self._cap["act"], dtype=torch.float16, device=self.dev) for _ in range(3)]
            self._x16 = torch.empty(self._cap["x16"], dtype=torch.float16, device=self.dev)
            self._psum = torch.empty(self._cap["psum"], dtype=torch.float32, device=self.dev)
            self._ws = torch.empty(self._cap["ws"], dtype=torch.float32, device=self.dev)
        return self._acts

    # --------------------------------------------------------------- trunk
    def _conv(self, x, H, W, c, bnp, stride, relu, y, psum=None):
        p = _lib.ptr
        _lib.check(self.lib.zmi_spk_conv2d(p(x), H, W, c["ci"], p(c["w"]), p(bnp[0]), p(bnp[1]), c["co"], c["k"], stride,
                                           int(relu), p(y), p(psum), self._sptr), "spk_conv2d")

    @torch.inference_mode()
    def front(self, feat: torch.Tensor, record: dict | None = None) -> torch.Tensor:
        """ResNet.forward (speaker_cloning.py:186-192): feat [acoustic_dim, W] fp32 -> [H / 8, W / 8, 8 in_planes]
        fp16 channels-last. `record` (a dict) receives the stem's and every block's output as [1, C, H, W] fp32."""
        cfg = self.config
        H, W = feat.shape
        if H != cfg.acoustic_dim or W < 2:
            raise ValueError(f"features must be [{cfg.acoustic_dim}, frames >= 2], got {tuple(feat.shape)}")
        self._sptr = torch.cuda.current_stream(self.dev).cuda_stream
        b0, b1, b2 = self._workspace(W)
        self._x16.view(-1)[: H * W].copy_(feat.reshape(-1))
        c = cfg.in_planes
        _lib.check(self.lib.zmi_spk_stem(self._x16.data_ptr(), H, W, self.stem_w.data_ptr(), self.stem_bn[0].data_ptr(),
                                         self.stem_bn[1].data_ptr(), c, b0.data_ptr(), self._sptr), "spk_stem")

        def rec(name, buf, h, w, ch):
            if record is not None:
                record[name] = buf[: h * w * ch].view(h, w, ch).permute(2, 0, 1)[None].float()

        rec("stem", b0, H, W, c)
        for blk in self.blocks:
            s, co = blk["stride"], blk["c1"]["co"]
            ho, wo = (H - 1) // s + 1, (W - 1) // s + 1
            tiles = self.lib.zmi_spk_conv2d_tiles(ho, wo, 3, 1)
            self._conv(b0, H, W, blk["c1"], blk["bn1"], s, True, b1)
            if blk["ds"] is None:
                self._conv(b1, ho, wo, blk["c2"], blk["bn2"], 1, False, b2, self._psum)
                x, res, out = b2, b0, b1
            else:
                self._conv(b0, H, W, blk["ds"], blk["dsbn"], s, False, b2)
                self._conv(b1, ho, wo, blk["c2"], blk["bn2"], 1, False, b0, self._psum)
                x, res, out = b0, b2, b1
            _lib.check(self.lib.zmi_spk_simam(x.data_ptr(), res.data_ptr(), ho, wo, co, self._psum.data_ptr(), tiles,
                                              self._ws.data_ptr(), out.data_ptr(), self._sptr), "spk_simam")
            b0, b1, b2 = out, x, res
            H, W, c = ho, wo, co
            rec(blk["name"], b0, H, W, c)
        return b0[: H * W * c].view(H, W, c)

    @torch.inference_mode()
    def front_lanes(self, feats: list) -> list:
        """`front` for up to 32 clips as ragged lanes of one launch sequence: feats [acoustic_dim, W_l] fp32 each ->
        views [H / 8, W_l / 8, 8 in_planes] fp16 of the workspace, each with the bits `front` gives that clip alone.
        The launches are those of one clip; every lane keeps its own width down the stages."""
        cfg, p, lib = self.config, _lib.ptr, self.lib
        H = cfg.acoustic_dim
        if any(f.ndim != 2 or f.shape[0] != H or f.shape[1] < 2 for f in feats):
            raise ValueError(f"features must be [{H}, frames >= 2], got {[tuple(f.shape) for f in feats]}")
        ws = [int(f.shape[1]) for f in feats]
        sptr = torch.cuda.current_stream(self.dev).cuda_stream
        b0, b1, b2 = self._workspace(max(ws), len(ws))
        ls = self._ls
        for l, f in enumerate(feats):
            self._x16[l * ls["x16"]: l * ls["x16"] + H * ws[l]].copy_(f.reshape(-1))
        c, L = cfg.in_planes, _lib.SpkLanes.of(ws)
        _lib.check(lib.zmi_spk_stem_lanes(p(self._x16), H, L, p(self.stem_w), p(self.stem_bn[0]), p(self.stem_bn[1]), c,
                                          p(b0), ls["x16"], ls["act"], sptr), "spk_stem_lanes")

        def conv(x, h, lanes, cv, bnp, stride, relu, y, psum=None):
            _lib.check(lib.zmi_spk_conv2d_lanes(p(x), h, lanes, cv["ci"], p(cv["w"]), p(bnp[0]), p(bnp[1]), cv["co"],
                                                cv["k"], stride, int(relu), p(y), p(psum), ls["act"], ls["act"],
                                                ls["psum"], sptr), "spk_conv2d_lanes")

        tiles = None
        for blk in self.blocks:
            s, co = blk["stride"], blk["c1"]["co"]
            Lo, ho = L, H
            if s != 1 or tiles is None:  # the widths change: this stage's lanes and their conv2 tile counts
                ho, ws = (H - 1) // s + 1, [(w - 1) // s + 1 for w in ws]
                Lo = _lib.SpkLanes.of(ws)
                tiles = (_lib.c_int * len(ws))(*[lib.zmi_spk_conv2d_tiles(ho, w, 3, 1) for w in ws])
            conv(b0, H, L, blk["c1"], blk["bn1"], s, True, b1)
            if blk["ds"] is None:
                conv(b1, ho, Lo, blk["c2"], blk["bn2"], 1, False, b2, self._psum)
                x, res, out = b2, b0, b1
            else:
                conv(b0, H, L, blk["ds"], blk["dsbn"], s, False, b2)
                conv(b1, ho, Lo, blk["c2"], blk["bn2"], 1, False, b0, self._psum)
                x, res, out = b0, b2, b1
            _lib.check(lib.zmi_spk_simam_lanes(p(x), p(res), ho, Lo, co, p(self._psum), tiles, p(self._ws), p(out),
                                               ls["act"], ls["act"], ls["psum"], ls["ws"], ls["act"], sptr),
                       "spk_simam_lanes")
            b0, b1, b2 = out, x, res
            H, L, c = ho, Lo, co
        return [b0[l * ls["act"]: l * ls["act"] + H * w * c].view(H, w, c) for l, w in enumerate(ws)]

    # --------------------------------------------------------------- tail (fp32 torch ops on the device)
    def pool(self, front: torch.Tensor) -> torch.Tensor:
        """ASP (speaker_cloning.py:38-61) on the trunk's [H, W, C] output -> [1, 2 C H] fp32."""
        H, W, C = front.shape
        x = front.permute(2, 0, 1).reshape(C * H, W).float()              # the reference's reshape: row c H + h
        h = torch.relu(self.att_w0 @ x + self.att_b0[:, None])
        g, b, m, v = self.att_bn
        h = (h - m[:, None]) / torch.sqrt(v[:, None] + BN_EPS) * g[:, None] + b[:, None]
        w = torch.softmax(self.att_w3 @ h + self.att_b3[:, None], dim=1)
        mu = (x * w).sum(1)
        sg = torch.sqrt(((x ** 2 * w).sum(1) - mu ** 2).clamp(min=1e-5))
        return torch.cat([mu, sg])[None]

    @torch.inference_mode()
    def embed_features(self, feat: torch.Tensor, record: dict | None = None):
        """ResNet293_based.forward after featCal (speaker_cloning.py:217-224) + the LDA: ([1, embd], [1, lda]) fp32."""
        feat = feat.to(self.dev, torch.float32)
        fr = self.front(feat, record)
        pooled = self.pool(fr)
        emb = pooled @ self.bott_w.t() + self.bott_b
        lda = emb @ self.lda_w.t() + self.lda_b
        if record is not None:
            record["front"] = fr.permute(2, 0, 1)[None].float()
            record["pooled"] = pooled
        return emb, lda

    @torch.inference_mode()
    def embed_features_batch(self, feats: list, max_lanes: int = _lib.SPK_MAX_LANES, max_lane_frames: int = 32768):
        """`embed_features` for many clips: feats [acoustic_dim, W_i] each -> (emb [B, embd], lda [B, lda]) fp32 in the
        caller's order, row i with the bits embed_features(feats[i]) gives. The trunk runs once per group of
        `plan_lanes` (one clip's launches for the whole group); the tail stays per clip, on the clip's own slice, so
        rocBLAS sees the single form's shapes."""
        feats = [f.to(self.dev, torch.float32) for f in feats]
        emb = torch.empty(len(feats), self.config.embd_dim, dtype=torch.float32, device=self.dev)
        lda = torch.empty(len(feats), self.config.lda_dim, dtype=torch.float32, device=self.dev)
        for group in plan_lanes([int(f.shape[-1]) for f in feats], max_lanes, max_lane_frames):
            for i, fr in zip(group, self.front_lanes([feats[i] for i in group])):
                e = self.pool(fr) @ self.bott_w.t() + self.bott_b
                emb[i], lda[i] = e[0], (e @ self.lda_w.t() + self.lda_b)[0]
        return emb, lda

    def embed_batch(self, clips: list, max_lanes: int = _lib.SPK_MAX_LANES, max_lane_frames: int = 32768):
        """`__call__` for many clips [(wav, sample_rate), ..]: the front end per clip, then embed_features_batch."""
        return self.embed_features_batch([self.features(w, sr) for w, sr in clips], max_lanes, max_lane_frames)

    @torch.inference_mode()
    def features(self, wav: torch.Tensor, sample_rate: int) -> torch.Tensor:
        """prepare_input + logFbankCal (speaker_cloning.py:376-381, 31-35): [acoustic_dim, frames] fp32."""
        assert wav.ndim < 3
        wav = wav.to(self.dev, torch.float32)
        wav = wav.mean(0, keepdim=True) if wav.ndim == 2 else wav[None]
        return log_fbank(resample(wav, sample_rate), self._basis, self._fb)

    def __call__(self, wav: torch.Tensor, sample_rate: int):
        return self.embed_features(self.features(wav, sample_rate))
