"""Zonos with the reference's generate() surface (zonos/model.py:218-315), on the HIP engine.

    model = Zonos.synthetic(zonos_v01_transformer(), device="cuda")      # or Zonos.from_local(...)
    codes = model.generate(prefix_conditioning)                          # [1, 9, T] int64
    wav = model.autoencoder.decode(codes)                                # [1, 1, 512 T] fp32
    for wav in model.stream(prefix_conditioning): ...                    # the same samples, in chunks, as they are ready
    for i, wav, last in model.stream_batch(conds): ...                   # many utterances' chunks, each as decode(generate_batch)
    with model.serve(64, 2048, 512, pcm16=True) as session: ...          # requests admitted mid-stream (serving.py)
    codes = model.generate(prefix_conditioning[:1], cfg_scale=1)         # guidance-free: one row per utterance

`generate` keeps the reference's arguments and batch_size=1 semantics; `generate_batch`
runs many independent utterances through the slots of one engine (continuous batching at
chunk granularity), each with exactly the per-utterance result of `generate`.

cfg_scale == 1 is the reference's guidance-free branch (zonos/model.py:112, 134-136, 193): no unconditional row is
run at all. Such a call runs the engine's single layout (one activation / KV row per utterance, engine.set_layout);
any other cfg_scale runs the paired layout. The layout is chosen per call, so one model serves both.
"""
from __future__ import annotations

import json
from typing import Callable, Sequence

import torch

from . import _lib  # noqa: F401  (fail loudly at import if the HIP library is missing)
from .autoencoder import DACAutoencoder
from .conditioning import PrefixConditioner
from .config import N_CODEBOOKS, ZonosConfig
from .engine import ST_FIELDS, SamplingParams, codes_count, make_engine
from .prefill_plan import check_chunk
from .serving import BatchRounds, ServeSession


def _draw_seed() -> int:
    # the reference draws its noise from torch's global RNG (sampling.py:20); derive our
    # counter-based stream from the same generator so torch.manual_seed() controls it
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class Zonos:
    def __init__(self, config: ZonosConfig, device="cuda", max_slots: int = 1, max_seqlen: int = 2048,
                 max_prefill: int = 512, autoencoder: DACAutoencoder | None = None, weights: str = "bf16",
                 mixer_weights: str = "bf16"):
        """weights: "bf16", or "fp8" for weight-only E4M3 MLP projections (transformer backbones; quant.py): the
        decode step then streams 0.6 of the bytes and computes exactly the bf16 model on the dequantised weights.
        mixer_weights: "bf16", or "fp8" for the same format on the Mamba2 mixers' in_proj / out_proj (hybrid
        backbones): half the bytes of those projections per decode step and per replica, again exactly the bf16
        model on the dequantised weights."""
        self.config = config
        self.eos_token_id = config.eos_token_id
        self.masked_token_id = config.masked_token_id
        self._device = torch.device(device)
        self.weights = weights
        self.mixer_weights = mixer_weights
        self.engine = make_engine(config, device, max_slots, max_seqlen, max_prefill, weights, mixer_weights)
        self.autoencoder = autoencoder if autoencoder is not None else DACAutoencoder(device)
        pcc = config.prefix_conditioner
        self.prefix_conditioner = (PrefixConditioner(pcc.conditioners, config.backbone.d_model, device, pcc.projection)
                                   if pcc.conditioners else None)
        self.spk_clone_model = None      # created lazily (model.py:90-93) by make_speaker_embedding
        self._spk_synthetic_seed = None  # Zonos.synthetic: the seed of the synthetic speaker encoder
        self._stream_decoders: dict = {}  # stream(): one DACStreamDecoder per chunk_frames
        self._stream_resamplers: dict = {}  # stream() / stream_batch(sample_rate=): one StreamResampler per rate
        self._stream_batch_decoders: dict = {}  # stream_batch(): one DACBatchStreamDecoder per chunk_frames
        # stream(): True lets the DAC windows run beside the next decode steps. Measured: the decode
        # step's codes are then not reproducible (a few utterances in ten diverge from generate() at some frame), so
        # the windows run between the rounds of steps instead and stream() is exact. tools/bench_stream.py sets it to
        # time the overlapped form.
        self._stream_overlap = False
        self._stream_glue = None
        self._serving = None  # the open serve() session, if any: it owns the slots

    @property
    def device(self) -> torch.device:
        return self._device

    # ------------------------------------------------------------------ construction
    @classmethod
    def synthetic(cls, config: ZonosConfig, device="cuda", seed: int = 0, zero_eos: bool = False,
                  eos_row_scale: float | None = None, dac_seed: int = 0, **kw) -> "Zonos":
        m = cls(config, device, autoencoder=DACAutoencoder(device, seed=dac_seed), **kw)
        m.engine.init_synthetic(seed, zero_eos=zero_eos, eos_row_scale=eos_row_scale)
        m._spk_synthetic_seed = seed
        if m.prefix_conditioner is not None:
            from . import synthetic as syn
            pcc = config.prefix_conditioner
            sd = dict(syn.iter_torch_cpu(syn.prefix_conditioner_specs(pcc.conditioners, config.backbone.d_model), seed))
            m.prefix_conditioner.load_state_dict(sd, prefix="prefix_conditioner.")
        return m

    @classmethod
    def from_local(cls, config_path: str, model_path: str, device="cuda", backbone: str | None = None,
                   dac_path: str | None = None, **kw) -> "Zonos":
        """model.py:65-88 with local files only (safetensors, no pickle)."""
        from safetensors.torch import load_file
        if backbone not in (None, "hip"):
            raise ValueError(f"backbone {backbone!r}: the HIP build registers BACKBONES['hip'] only "
                             "(transformer and hybrid)")
        config = ZonosConfig.from_dict(json.load(open(config_path)))
        dac = DACAutoencoder(device, state_dict=load_file(dac_path) if dac_path else None)
        m = cls(config, device, autoencoder=dac, **kw)
        sd = load_file(model_path)
        m.engine.load_state_dict(sd)
        if m.prefix_conditioner is not None:
            m.prefix_conditioner.load_state_dict(sd, prefix="prefix_conditioner.")
        return m

    @classmethod
    def from_pretrained(cls, repo_id: str, revision: str | None = None, device="cuda", **kw) -> "Zonos":
        """model.py:57-63: resolves files through the local HF cache (no network in this build)."""
        from huggingface_hub import hf_hub_download
        cfg = hf_hub_download(repo_id=repo_id, filename="config.json", revision=revision)
        mdl = hf_hub_download(repo_id=repo_id, filename="model.safetensors", revision=revision)
        return cls.from_local(cfg, mdl, device, **kw)

    def _ensure_capacity(self, slots: int, seqlen: int, prefill: int):
        e = self.engine
        if slots > e.S or seqlen > e.smax or prefill > e.max_prefill:
            w = e.w
            self.engine = make_engine(self.config, self._device, max(slots, e.S), max(seqlen, e.smax),
                                      max(prefill, e.max_prefill), self.weights, self.mixer_weights)
            self.engine.w = w
            self.engine._build_plan()

    def _prefill_rows(self, need_pre: int, prefill_chunk) -> int:
        """The prefill rows a call asks of the engine: with prefill_chunk = C a prompt runs C rows at a time, so a long
        prompt asks for C rows, not its length (and no longer rebuilds the engine)."""
        chunk = check_chunk(prefill_chunk)
        return need_pre if chunk is None else min(need_pre, chunk)

    def _engine_chunk(self, prefill_chunk):
        """prefill_chunk as the engine takes it (<= its max_prefill). After _ensure_capacity(_prefill_rows(...)) a
        larger value means that every prompt of the call fits one chunk, so the boundaries do not change."""
        return None if prefill_chunk is None else min(int(prefill_chunk), self.engine.max_prefill)

    def _select_layout(self, cfg_scale: float) -> int:
        """The engine's row layout for a call (after _ensure_capacity, which may have rebuilt the engine): single
        (one row per utterance) for cfg_scale == 1, the reference's guidance-free branch, else paired."""
        rps = 1 if cfg_scale == 1 else 2
        self.engine.set_layout(rps)
        return rps

    @staticmethod
    def _cond_rows_ok(cond: torch.Tensor, cfg_scale: float) -> bool:
        """[2, Lc, d] (cond, uncond); with cfg_scale == 1 also [1, Lc, d] (of [2, Lc, d] row 0 alone is used)."""
        return cond.shape[0] == 2 or (cfg_scale == 1 and cond.shape[0] == 1)

    # ------------------------------------------------------------------ speaker embedding
    def load_speaker_model(self, ckpt_path: str, lda_path: str) -> None:
        """The published speaker encoder and its LDA (speaker_cloning.py:391-406) from local .pt / .safetensors
        files: there is no hub download in this build."""
        from .speaker import SpeakerEmbeddingLDA
        self.spk_clone_model = SpeakerEmbeddingLDA.from_files(ckpt_path, lda_path, self._device)

    def _speaker_model(self):
        """The loaded speaker encoder, or (Zonos.synthetic) the synthetic one, created on first use."""
        if self.spk_clone_model is None:
            if self._spk_synthetic_seed is None:
                raise RuntimeError("no speaker encoder weights: call load_speaker_model(ckpt_path, lda_path) first "
                                   "(this build does not download them)")
            from .speaker import SpeakerEmbeddingLDA
            self.spk_clone_model = SpeakerEmbeddingLDA(self._device, seed=self._spk_synthetic_seed)
        return self.spk_clone_model

    def make_speaker_embedding(self, wav: torch.Tensor, sr: int) -> torch.Tensor:
        """model.py:90-95: [channels, N] (or [N]) waveform at `sr` -> [1, 1, 128] bf16 for make_cond_dict(speaker=)."""
        _, spk_embedding = self._speaker_model()(wav.to(self._device), sr)
        return spk_embedding.unsqueeze(0).bfloat16()

    def make_speaker_embeddings(self, wavs, srs) -> list:
        """make_speaker_embedding for many clips (srs: one rate per clip, or one int for all): the ResNet trunk runs
        over the clips as ragged lanes of one launch sequence per group (speaker.plan_lanes). Element i is bit-equal
        to make_speaker_embedding(wavs[i], srs[i])."""
        srs = [srs] * len(wavs) if isinstance(srs, int) else list(srs)
        if len(srs) != len(wavs):
            raise ValueError(f"{len(wavs)} clips but {len(srs)} sample rates")
        _, lda = self._speaker_model().embed_batch([(w.to(self._device), sr) for w, sr in zip(wavs, srs)])
        return [lda[i:i + 1].unsqueeze(0).bfloat16() for i in range(len(wavs))]

    # ------------------------------------------------------------------ conditioning
    def prepare_conditioning(self, cond_dict: dict, uncond_dict: dict | None = None) -> torch.Tensor:
        """model.py:204-212: [2, Lc, d] bf16 (conditional rows, then unconditional), one HIP launch."""
        if self.prefix_conditioner is None:
            raise ValueError("this config has no prefix conditioners")
        return self.prefix_conditioner.prepare_conditioning(cond_dict, uncond_dict)

    # ------------------------------------------------------------------ generation
    @torch.inference_mode()
    def generate(self, prefix_conditioning: torch.Tensor, audio_prefix_codes: torch.Tensor | None = None,
                 max_new_tokens: int = 86 * 30, cfg_scale: float = 2.0, batch_size: int = 1,
                 sampling_params: dict = dict(min_p=0.1), progress_bar: bool = True,
                 disable_torch_compile: bool = False,
                 callback: Callable[[torch.Tensor, int, int], bool] | None = None,
                 chunk: int = 64, prefill_chunk: int | None = None) -> torch.Tensor:
        """Reference model.py:218-315 (batch_size=1). `disable_torch_compile` is accepted and ignored:
        the decode step is a hipGraph of hand-written kernels in every mode. cfg_scale == 1: the guidance-free
        branch (model.py:112), one row through the backbone; prefix_conditioning [1, Lc, d], or [2, Lc, d] of which
        row 0 is used. prefill_chunk = C: the prompt (Lc + P + 1 rows) goes through the layers C rows at a time
        (HipEngine.prefill_many), so a long audio prefix needs C prefill rows, not its length; None: one pass."""
        self._check_not_serving("generate")
        if batch_size != 1 or not self._cond_rows_ok(prefix_conditioning, cfg_scale):
            raise ValueError("the reference generate() supports batch_size=1 only (SURVEY.md §0.3); "
                             "use generate_batch() for many utterances")
        lc = prefix_conditioning.shape[1]
        p = 0 if audio_prefix_codes is None else audio_prefix_codes.shape[2]
        self._ensure_capacity(1, lc + p + max_new_tokens + 9, self._prefill_rows(lc + p + 1, prefill_chunk))
        self._select_layout(cfg_scale)
        e = self.engine
        params = SamplingParams.from_dict(dict(sampling_params), cfg_scale, _draw_seed())
        slot = 0
        e.prefill(slot, prefix_conditioning, audio_prefix_codes, max_new_tokens, params,
                  prefill_chunk=self._engine_chunk(prefill_chunk))
        max_steps = max_new_tokens + 8
        bar = None
        if progress_bar:
            from tqdm import tqdm
            bar = tqdm(total=max_steps, desc="Generating")
        step = 0
        if callback is None:
            while step < max_steps:
                n = min(chunk, max_steps - step)
                e.step(n, slots=1)
                step += n
                if bar is not None:
                    bar.update(n)
                if not e.slot_state(slot)["active"]:
                    break
        else:
            # exact reference semantics: the callback sees every frame and may stop the loop
            while step < max_steps:
                e.step(1, slots=1)
                step += 1
                if bar is not None:
                    bar.update(1)
                stt = e.slot_state(slot)
                o = stt["offset"]
                frame = e.delayed[slot, :, o:o + 1].to(torch.int64).unsqueeze(0)
                if not callback(frame, step, max_steps) or not stt["active"]:
                    break
        if bar is not None:
            bar.close()
        e.check_errors()  # a hand-off that gave up (or a position past a form's reach) must not pass silently
        out = e.read_codes(slot)
        e.release(slot)
        return out

    @torch.inference_mode()
    def stream(self, prefix_conditioning: torch.Tensor, audio_prefix_codes: torch.Tensor | None = None,
               max_new_tokens: int = 86 * 30, cfg_scale: float = 2.0, sampling_params: dict = dict(min_p=0.1),
               chunk_frames: int = 16, sample_rate: int | None = None, decoder: str = "window",
               prefill_chunk: int | None = None):
        """generate() + autoencoder.decode() as a generator of waveform chunks [1, 1, 512 n] fp32 (device): audio
        is yielded while the utterance is still being generated. With the same torch.manual_seed, the chunks
        concatenated are bit for bit decode(generate(...)) (batch 1, generate()'s arguments).

        A frame is final once the delayed buffer's column frame + 9 is written; it is decoded once the DAC decoder's
        lookahead (DAC_LOOKAHEAD_FRAMES) beyond it is final too. A round is `chunk_frames` decode steps on the engine's
        stream, the read of the frames they make final, and those frames' DAC windows on the autoencoder's stream,
        all enqueued one round ahead of the host and ordered by events; the host waits only for a round's one small
        state copy before it yields the round's audio.

        sample_rate (None or 44100: exactly the path above): the chunks leave at that rate, [1, 1, any n > 0], and
        concatenated are bit for bit autoencoder.resample(decode(generate(...)), 44100, sample_rate). A round's
        waveform goes through a streaming resampler (resampling.StreamResampler, zmi_resample) once the round's state
        copy has shown how much of it counts, so the resampler is never rolled back.

        decoder: "window" (the default) or "carry", the carried-state DAC decoder (autoencoder.stream_decoder(carry=
        True)): the same chunks, each decoded at the cost of its own frames; a round's rollback point then holds a
        copy of the decoder's state.

        cfg_scale == 1: guidance-free, as generate(cfg_scale=1). prefill_chunk: as generate(prefill_chunk=)."""
        self._check_not_serving("stream")
        carry = self._decoder_mode(decoder)
        rate = self._output_rate(sample_rate)
        if not self._cond_rows_ok(prefix_conditioning, cfg_scale):
            raise ValueError("stream() has generate()'s batch_size=1 semantics: prefix_conditioning [2, Lc, d] "
                             "([1, Lc, d] too with cfg_scale=1)")
        if chunk_frames < 1:
            raise ValueError("chunk_frames >= 1")
        lc = prefix_conditioning.shape[1]
        p = 0 if audio_prefix_codes is None else audio_prefix_codes.shape[2]
        self._ensure_capacity(1, lc + p + max_new_tokens + 9, self._prefill_rows(lc + p + 1, prefill_chunk))
        self._select_layout(cfg_scale)
        e = self.engine
        params = SamplingParams.from_dict(dict(sampling_params), cfg_scale, _draw_seed())
        slot = 0
        key = (id(self.autoencoder), int(chunk_frames), carry)
        if key not in self._stream_decoders:  # kept: its window graph and stage buffers serve every later call
            self._stream_decoders[key] = self.autoencoder.stream_decoder(chunk_frames, carry=carry)
        dec = self._stream_decoders[key]
        dec._reset()  # (an earlier stream closed before its end)
        rs = None if rate is None else self._stream_resampler(rate, 1)
        n_audio, max_steps = p + max_new_tokens, max_new_tokens + 8
        host = [torch.empty(e.SNAPSHOT_INTS, dtype=torch.int32).pin_memory() for _ in range(2)]
        cur = torch.cuda.current_stream(self._device)
        if self._stream_glue is None:
            self._stream_glue = torch.cuda.Stream(self._device)
        # the rounds' decoder calls are enqueued ahead of the host on a stream of their own: the caller's stream waits
        # only for the chunk it is handed, not for the round already in flight behind it
        glue = self._stream_glue
        steps = read_to = rounds = 0

        def launch(n: int):
            """Enqueue n more decode steps, the read of the frames they make final, the slot's state copy, and the
            DAC windows of those frames. After `steps` steps a running slot's offset is p + 1 + steps, so the frames
            are known on the host before the steps have run; if the state copy later shows that the slot stopped
            within these steps (EOS countdown), fewer frames count and the decoder is rolled back to `saved`."""
            nonlocal steps, read_to, rounds
            if n:
                if not self._stream_overlap:
                    e.stream.wait_stream(ae.stream)  # the previous round's windows first (see _stream_overlap)
                e.step(n, slots=1)
                steps += n
            t0, t1 = read_to, max(min(p + 1 + steps - 9, n_audio), read_to)
            codes = e.read_final_codes(slot, t0, t1)
            h = host[rounds & 1]
            rounds += 1
            read_to = t1
            ev = e.snapshot(slot, h)
            saved = dec._state()
            with torch.cuda.stream(glue):
                glue.wait_event(ev)
                if t1 > t0:
                    codes.record_stream(glue)
                wav = dec.push(codes)
                ready = torch.cuda.Event()
                ready.record(glue)
            return codes, t0, t1, h, ev, saved, wav, ready

        ae = self.autoencoder
        try:
            e.prefill(slot, prefix_conditioning, audio_prefix_codes, max_new_tokens, params,
                      prefill_chunk=self._engine_chunk(prefill_chunk))
            queue = [launch(0)]  # audio-prefix frames are final before any decode step
            while queue:
                if steps < max_steps:  # keep the engine one round ahead of the host
                    queue.append(launch(min(chunk_frames, max_steps - steps)))
                codes, t0, t1, h, ev, saved, wav, ready = queue.pop(0)
                ev.synchronize()
                vals = h.tolist()
                if any(vals[len(ST_FIELDS):]):  # the words check_errors() reads, copied with the state
                    e.check_errors()
                stt = dict(zip(ST_FIELDS, vals))
                if stt["active"]:
                    if t1 > t0 and stt["offset"] - 9 < t1:
                        raise RuntimeError("stream: the slot's offset is behind the steps enqueued")
                else:  # ended (EOS countdown or max_new_tokens): read_codes' count, then the decoder's tail
                    good = min(codes_count(stt), t1)
                    with torch.cuda.stream(glue):
                        if good < t1 or queue:  # the rounds decoded past the end are dropped
                            dec._restore(saved)
                            wav = dec.push(codes[..., :max(good - t0, 0)])
                        queue.clear()
                        tail = dec.flush()
                        wav = tail if wav.shape[-1] == 0 else torch.cat([wav, tail], dim=-1)
                        ready = torch.cuda.Event()
                        ready.record(glue)
                if rs is not None and (wav.shape[-1] or not stt["active"]):  # fed only what is known to count
                    with torch.cuda.stream(glue):
                        wav = rs.push({0: wav}, final=() if stt["active"] else (0,))[0]
                        ready = torch.cuda.Event()
                        ready.record(glue)
                if wav.shape[-1]:
                    cur.wait_event(ready)
                    wav.record_stream(cur)
                    yield wav
        finally:
            dec._reset()
            if rs is not None:
                rs.reset(0)
            e.release(slot)

    @torch.inference_mode()
    def generate_batch(self, conds: Sequence[torch.Tensor], prefixes: Sequence[torch.Tensor | None] | None = None,
                       max_new_tokens: Sequence[int] | int = 86 * 30, cfg_scale: float = 2.0,
                       sampling_params: dict = dict(min_p=0.1), seeds: Sequence[int] | None = None,
                       max_slots: int | None = None, chunk: int = 32,
                       prefill_chunk: int | None = None) -> list[torch.Tensor]:
        """Many independent utterances through the engine's slots; result i equals generate() on utterance i.
        cfg_scale == 1: guidance-free (one row per utterance, so a step of k busy slots runs k rows, not 2 k).
        prefill_chunk = C: every prompt runs C rows at a time (result i equals generate(prefill_chunk=C) on utterance
        i: a prompt's chunk boundaries do not depend on its batch mates)."""
        self._check_not_serving("generate_batch")
        n = len(conds)
        prefixes = list(prefixes) if prefixes is not None else [None] * n
        mnt = [max_new_tokens] * n if isinstance(max_new_tokens, int) else list(max_new_tokens)
        seeds = list(seeds) if seeds is not None else [_draw_seed() for _ in range(n)]
        need_seq = max(c.shape[1] + (0 if p is None else p.shape[2]) + m + 9 for c, p, m in zip(conds, prefixes, mnt))
        need_pre = max(c.shape[1] + (0 if p is None else p.shape[2]) + 1 for c, p in zip(conds, prefixes))
        slots = min(max_slots or n, n)
        self._ensure_capacity(slots, need_seq, self._prefill_rows(need_pre, prefill_chunk))
        self._select_layout(cfg_scale)
        e = self.engine
        pchunk = self._engine_chunk(prefill_chunk)
        # longest-processing-time first, so the tail is short
        order = sorted(range(n), key=lambda i: -mnt[i])
        queue = list(order)
        owner = [-1] * slots
        results: list[torch.Tensor | None] = [None] * n
        remaining = [0] * slots

        def fill():
            items = []
            for s in range(slots):
                if owner[s] < 0 and queue:
                    i = queue.pop(0)
                    params = SamplingParams.from_dict(dict(sampling_params), cfg_scale, seeds[i])
                    items.append((s, conds[i], prefixes[i], mnt[i], params))
                    owner[s] = i
                    remaining[s] = mnt[i] + 8
            e.prefill_many(items, pchunk)  # the free slots' prefills in as few passes through the layers as fit

        # a step runs slots 0 .. the highest busy one (rounded up to a few sizes, one decode graph each): LPT
        # fills the low slots with the longest utterances, so the tail of a job steps a handful of rows instead
        # of every slot's (every kernel is row-invariant: the codes do not depend on the row count)
        sizes = sorted({slots} | {b for b in (1, 2, 4, 8, 16, 24, 32, 40, 48, 56) if b < slots})

        fill()
        while any(o >= 0 for o in owner):
            k = min(chunk, max(r for s, r in enumerate(remaining) if owner[s] >= 0))
            hi = max(s for s in range(slots) if owner[s] >= 0) + 1 if e.batch_shrink else slots
            e.step(k, slots=next(b for b in sizes if b >= hi))
            e.stream.synchronize()
            e.check_errors()
            act = e.st["active"].cpu()
            for s in range(slots):
                if owner[s] >= 0:
                    remaining[s] -= k
                    if not act[s]:
                        results[owner[s]] = e.read_codes(s)
                        owner[s] = -1
                        e.pos_hi[s] = 0  # its rows are inactive (position -1): no bound on the attention form
            fill()
        return results

    @torch.inference_mode()
    def stream_batch(self, conds: Sequence[torch.Tensor], prefixes: Sequence[torch.Tensor | None] | None = None,
                     max_new_tokens: Sequence[int] | int = 86 * 30, cfg_scale: float = 2.0,
                     sampling_params: dict = dict(min_p=0.1), seeds: Sequence[int] | None = None,
                     max_slots: int | None = None, chunk_frames: int = 16, sample_rate: int | None = None,
                     decoder: str = "window", prefill_chunk: int | None = None):
        """generate_batch() + autoencoder.decode() per utterance as a generator of (utterance index, waveform chunk
        [1, 1, 512 n] fp32 (device), last): every utterance's audio is yielded while it and the others are still being
        generated. With the same seeds, utterance i's chunks concatenated are bit for bit
        autoencoder.decode(generate_batch(...)[i]); each utterance yields exactly one item with last = True (its chunk
        may be empty).

        A round is `chunk_frames` decode steps over slots 0 .. the highest busy one (generate_batch's sizes and
        batch_shrink rule), one copy of every slot's state to the host, the read of the frames the round made final
        in every busy slot, and ONE push of all of them to a DACBatchStreamDecoder, which decodes the slots' windows
        of equal shape as lanes of one launch sequence (cfg_scale == 1: guidance-free, one row per slot). Slots that
        ended are flushed and refilled from the queue (longest first). The DAC windows run between the rounds, never beside decode steps (stream()'s ordering rule,
        DESIGN.md §5g): they are ordered behind the round's reads and the next round's steps wait for the
        autoencoder's stream. The state is read before the push, so nothing is decoded past an utterance's end.

        sample_rate (None or 44100: exactly the path above): a round's waveforms go through ONE push of a streaming
        resampler over the slots (zmi_resample, on the engine's stream); utterance i's chunks, [1, 1, any n >= 0],
        concatenated are bit for bit autoencoder.resample(decode(generate_batch(...)[i]), 44100, sample_rate).

        decoder: "window" (the default) or "carry", the carried-state DAC decoder (autoencoder.stream_decoder_batch(
        carry=True)): the same items; the slots that push equal frame counts past their start are one launch sequence
        whatever their positions, and a round decodes the frames it made final, not their windows.

        prefill_chunk: as generate_batch(prefill_chunk=)."""
        self._check_not_serving("stream_batch")
        carry = self._decoder_mode(decoder)
        rate = self._output_rate(sample_rate)
        if chunk_frames < 1:
            raise ValueError("chunk_frames >= 1")
        n = len(conds)
        if n == 0:
            return
        prefixes = list(prefixes) if prefixes is not None else [None] * n
        mnt = [max_new_tokens] * n if isinstance(max_new_tokens, int) else list(max_new_tokens)
        seeds = list(seeds) if seeds is not None else [_draw_seed() for _ in range(n)]
        plen = [0 if p is None else p.shape[2] for p in prefixes]
        need_seq = max(c.shape[1] + p + m + 9 for c, p, m in zip(conds, plen, mnt))
        need_pre = max(c.shape[1] + p + 1 for c, p in zip(conds, plen))
        slots = min(max_slots or n, n)
        self._ensure_capacity(slots, need_seq, self._prefill_rows(need_pre, prefill_chunk))
        self._select_layout(cfg_scale)
        e, ae = self.engine, self.autoencoder
        pchunk = self._engine_chunk(prefill_chunk)
        key = (id(ae), int(chunk_frames), carry)
        dec = self._stream_batch_decoders.get(key)
        if dec is None or dec.lanes < slots:  # kept: its graphs and stage buffers serve every later call
            dec = self._stream_batch_decoders[key] = ae.stream_decoder_batch(slots, chunk_frames, carry=carry)
        for s in range(slots):
            dec.reset(s)  # (an earlier stream_batch closed before its end)
        queue = sorted(range(n), key=lambda i: -mnt[i])  # longest-processing-time first, so the tail is short
        owner = [-1] * slots
        rs = None if rate is None else self._stream_resampler(rate, slots)
        rounds = BatchRounds(e, ae, dec, slots, chunk_frames, rs)  # the round serve() runs too (serving.py)

        def fill():
            items = []
            for s in range(slots):
                if owner[s] < 0 and queue:
                    i = queue.pop(0)
                    params = SamplingParams.from_dict(dict(sampling_params), cfg_scale, seeds[i])
                    items.append((s, conds[i], prefixes[i], mnt[i], params))
                    owner[s] = i
                    rounds.start(s, plen[i], mnt[i])
                    if rs is not None:
                        rs.reset(s)
            e.prefill_many(items, pchunk)

        try:
            fill()
            while any(o >= 0 for o in owner):
                wavs, ended = rounds.round([s for s in range(slots) if owner[s] >= 0])
                out = [(owner[s], w, s in ended) for s, w in wavs.items()]
                for s in ended:
                    owner[s] = -1
                fill()  # before the round's audio is handed out: the consumer's time is not the engine's
                yield from out
        finally:
            for s in range(slots):
                dec.reset(s)
                if rs is not None:
                    rs.reset(s)
                if owner[s] >= 0:
                    e.release(s)

    def serve(self, max_slots: int, max_seqlen: int, max_prefill: int, chunk_frames: int = 16,
              pcm16: bool = False, sample_rate: int | None = None, decoder: str = "window",
              guidance: bool = True, prefill_chunk: int | None = None) -> ServeSession:
        """A serving session (serving.ServeSession, a context manager): submit() requests from any thread while
        others are being spoken, run_round() from one thread hands out every ticket's chunks, each ticket's
        concatenated bit for bit decode(generate_batch()) of the request alone; with pcm16 they leave as int16 CPU
        tensors (zmi_pcm16_pack); with sample_rate they leave at that rate (zmi_resample between the round's waveforms
        and the egress; None or 44100: no resampler, the unchanged path); decoder "window" or "carry" as in
        stream_batch(). Capacity is fixed here; while the session is
        open generate(), stream(), generate_batch(), stream_batch() and another serve() raise RuntimeError.
        guidance=False opens a guidance-free session (the single layout, one row per slot): its submit() takes
        cfg_scale=1 only, and conditioning [1, Lc, d] or [2, Lc, d]. A session is one or the other; guided and
        guidance-free requests do not mix in one session.
        prefill_chunk = C (1 <= C <= max_prefill): a request's prompt runs C rows at a time, at most one pass in front
        of a round while any ticket is decoding, so a prompt longer than max_prefill is admitted (the KV capacity,
        max_seqlen, still bounds it) and the running tickets' audio waits for one chunk, not for the whole prompt. Every
        ticket's chunks are then decode(generate_batch(..., prefill_chunk=C)) of the request alone."""
        self._check_not_serving("serve")
        return ServeSession(self, max_slots, max_seqlen, max_prefill, chunk_frames, pcm16, sample_rate, decoder,
                            guidance, prefill_chunk)

    @staticmethod
    def _decoder_mode(decoder: str) -> bool:
        """True for the carried-state DAC decoder, False for the window decoder."""
        if decoder not in ("window", "carry"):
            raise ValueError(f'decoder must be "window" or "carry", got {decoder!r}')
        return decoder == "carry"

    def _output_rate(self, sample_rate):
        """None for the decoder's own 44.1 kHz (no resampler), else the validated rate."""
        if sample_rate is None:
            return None
        from .config import DAC_SAMPLE_RATE
        from .resampling import resample_plan
        resample_plan(DAC_SAMPLE_RATE, sample_rate)  # ValueError for a bad rate, before anything is built
        return None if sample_rate == DAC_SAMPLE_RATE else int(sample_rate)

    def _stream_resampler(self, rate: int, lanes: int):
        """The streaming resampler of stream() / stream_batch() / serve() to `rate`, every lane reset; kept (its table
        and carry buffers stay on the device)."""
        key = (id(self.autoencoder), rate)
        rs = self._stream_resamplers.get(key)
        if rs is None or rs.lanes < lanes:
            rs = self._stream_resamplers[key] = self.autoencoder.resampler(rate, lanes)
        for lane in range(rs.lanes):
            rs.reset(lane)
        return rs

    def _check_not_serving(self, what: str):
        if self._serving is not None:
            raise RuntimeError(f"{what}(): a serve() session is open on this model (it owns the engine's slots); "
                               "close it first")

    def __repr__(self):
        bb = self.config.backbone
        kind = "hybrid" if bb.is_hybrid else "transformer"
        return (f"Zonos(hip {kind}, d={bb.d_model}, layers={bb.n_layer}, heads={bb.num_heads}/{bb.num_heads_kv}, "
                f"weights={self.weights}" + (f", mixer_weights={self.mixer_weights})" if bb.is_hybrid else ")"))


__all__ = ["Zonos", "DACAutoencoder", "N_CODEBOOKS"]
