"""Zonos.serve(): requests admitted while others are being spoken, each leaving as chunks (the reference's server loop,
server.py, without its HTTP layer).

    with model.serve(max_slots=64, max_seqlen=2048, max_prefill=512, pcm16=True) as session:
        ticket = session.submit(cond)                 # any thread, no GPU work
        for ticket, chunk, last in session.run_round(): ...   # one thread: int16 CPU chunks [1, 1, 512 n]

Three parts:
  SlotScheduler   the slot table, FIFO queue, tickets, capacity check and cancellation: pure Python, no engine (the CPU
                  tests drive it with a fake one);
  BatchRounds     one round of decode steps + state snapshot + reads + ONE batched DAC push + flushes over the busy
                  slots: the body stream_batch() and ServeSession.run_round() both run;
  ServeSession    the two on a model, with the PCM16 egress (zmi_pcm16_pack: one launch, one copy, one event a round).
"""
from __future__ import annotations

import threading
from collections import deque
from dataclasses import dataclass
from typing import Any

SIZE_BUCKETS = (1, 2, 4, 8, 16, 24, 32, 40, 48, 56)  # row counts a round is rounded up to (one decode graph each)


def size_buckets(slots: int) -> list:
    return sorted({slots} | {b for b in SIZE_BUCKETS if b < slots})


# ---------------------------------------------------------------------- the scheduler (no GPU, no engine)
@dataclass
class Request:
    ticket: int
    lc: int               # conditioning rows
    p: int                # audio-prefix frames
    max_new_tokens: int
    payload: Any = None   # whatever the engine side needs (ServeSession: cond, prefix, SamplingParams)


class SlotScheduler:
    """Which request runs in which slot. Tickets count up from 0 in submission order; waiting requests are admitted
    FIFO by ticket into the lowest free slot (so the rows a round steps, 0 .. the highest busy slot, stay few).
    submit() / cancel() / wait_for_work() may be called from any thread; begin_round() / finish() / release_all() from
    the one thread that drives the engine."""

    def __init__(self, max_slots: int, max_seqlen: int, max_prefill: int, d_model: int | None = None,
                 guidance: bool = True, prefill_chunk: int | None = None):
        from .prefill_plan import check_chunk
        if max_slots < 1:
            raise ValueError("max_slots >= 1")
        self.max_slots, self.max_seqlen, self.max_prefill = int(max_slots), int(max_seqlen), int(max_prefill)
        # chunked prefill: a prompt runs prefill_chunk rows at a time, so max_prefill no longer bounds a request
        self.prefill_chunk = check_chunk(prefill_chunk, self.max_prefill)
        self.d_model = d_model
        self.guidance = bool(guidance)  # False: a guidance-free session, conditioning [1, Lc, d] too
        self._cond = threading.Condition()
        self._next = 0
        self._waiting: deque = deque()
        self._slots: list = [None] * self.max_slots   # slot -> Request
        self._cancelled: set = set()                  # running tickets to release at the next round's start
        self._closed = False

    def fit(self, cond_shape, prefix_shape, max_new_tokens: int) -> tuple:
        """(Lc, P) of a request that fits a slot; ValueError for one that never can."""
        cond_shape = tuple(cond_shape)
        rows_ok = len(cond_shape) == 3 and (cond_shape[0] == 2 or (cond_shape[0] == 1 and not self.guidance))
        if not rows_ok or (self.d_model is not None and cond_shape[2] != self.d_model):
            want = "[2 (cond, uncond), Lc, d_model]" if self.guidance else "[1, Lc, d_model] or [2, Lc, d_model]"
            raise ValueError(f"prefix_conditioning must be {want}, got {list(cond_shape)}")
        p = 0
        if prefix_shape is not None:
            prefix_shape = tuple(prefix_shape)
            if len(prefix_shape) != 3 or prefix_shape[0] != 1 or prefix_shape[1] != 9:
                raise ValueError(f"audio_prefix_codes must be [1, 9, P], got {list(prefix_shape)}")
            p = prefix_shape[2]
        lc, n = cond_shape[1], int(max_new_tokens)
        if n < 1:
            raise ValueError("max_new_tokens >= 1")
        if lc + p + n + 9 > self.max_seqlen:
            raise ValueError(f"Lc + P + max_new_tokens + 9 = {lc + p + n + 9} > the session's max_seqlen {self.max_seqlen}")
        if lc + p + 1 > self.max_prefill and self.prefill_chunk is None:
            raise ValueError(f"Lc + P + 1 = {lc + p + 1} > the session's max_prefill {self.max_prefill}")
        return lc, p

    def submit(self, cond_shape, prefix_shape, max_new_tokens: int, payload: Any = None) -> int:
        lc, p = self.fit(cond_shape, prefix_shape, max_new_tokens)
        with self._cond:
            if self._closed:
                raise RuntimeError("the session is closed")
            ticket = self._next
            self._next += 1
            self._waiting.append(Request(ticket, lc, p, int(max_new_tokens), payload))
            self._cond.notify_all()
        return ticket

    def cancel(self, ticket: int) -> bool:
        with self._cond:
            for r in self._waiting:
                if r.ticket == ticket:
                    self._waiting.remove(r)
                    return True
            if ticket in self._cancelled:
                return False
            if any(r is not None and r.ticket == ticket for r in self._slots):
                self._cancelled.add(ticket)
                return True
        return False

    def is_cancelled(self, ticket: int) -> bool:
        with self._cond:
            return ticket in self._cancelled

    def cancelled(self) -> frozenset:
        """The running tickets cancelled since the last begin_round()."""
        with self._cond:
            return frozenset(self._cancelled)

    def begin_round(self) -> tuple:
        """(slots released by cancellation, [(slot, Request)] admitted): cancellations first, then the waiting
        requests FIFO into the free slots, lowest first."""
        with self._cond:
            released = [s for s, r in enumerate(self._slots) if r is not None and r.ticket in self._cancelled]
            for s in released:
                self._slots[s] = None
            self._cancelled.clear()
            admitted = []
            for s in range(self.max_slots):
                if not self._waiting:
                    break
                if self._slots[s] is None:
                    self._slots[s] = self._waiting.popleft()
                    admitted.append((s, self._slots[s]))
        return released, admitted

    def busy(self) -> list:
        """[(slot, Request)] of the running requests, by slot."""
        with self._cond:
            return [(s, r) for s, r in enumerate(self._slots) if r is not None]

    def finish(self, slot: int):
        """The slot's request has ended: (its Request, False if it was cancelled meanwhile); the slot is free."""
        with self._cond:
            r = self._slots[slot]
            self._slots[slot] = None
            live = r.ticket not in self._cancelled
            self._cancelled.discard(r.ticket)
        return r, live

    def release_all(self) -> list:
        """Close: drop the waiting requests and free every slot; returns the slots that were busy."""
        with self._cond:
            self._closed = True
            busy = [s for s, r in enumerate(self._slots) if r is not None]
            self._slots = [None] * self.max_slots
            self._waiting.clear()
            self._cancelled.clear()
            self._cond.notify_all()
        return busy

    @property
    def idle(self) -> bool:
        with self._cond:
            return not self._waiting and all(r is None for r in self._slots)

    def wait_for_work(self, timeout: float | None = None) -> bool:
        """Block until something is waiting or running (a submit() wakes it); False if `timeout` seconds pass first."""
        with self._cond:
            return self._cond.wait_for(
                lambda: self._closed or bool(self._waiting) or any(r is not None for r in self._slots), timeout)


# ---------------------------------------------------------------------- one round on the engine
class BatchRounds:
    """The round stream_batch() and ServeSession.run_round() run over the engine's slots 0 .. slots - 1:
    min(chunk_frames, max remaining) decode steps over slots 0 .. the highest busy one (rounded up to a size bucket),
    one copy of every slot's state to the host, the read of the frames the round made final in every busy slot, ONE
    push of all of them to the DACBatchStreamDecoder and the flush of the slots that ended. The DAC windows run
    between the rounds, never beside decode steps: they are ordered behind the round's reads and the
    next round's steps wait for the autoencoder's stream. The state is read before the push, so nothing is decoded past
    an utterance's end."""

    def __init__(self, engine, autoencoder, decoder, slots: int, chunk_frames: int, resampler=None):
        import torch
        from .engine import ST_FIELDS
        self.rs = resampler  # a StreamResampler over the slots (sample_rate), or None: the waveforms leave as decoded
        self.e, self.ae, self.dec, self.slots, self.chunk = engine, autoencoder, decoder, int(slots), int(chunk_frames)
        self.sizes = size_buckets(self.slots)
        self.plen, self.mnt = [0] * self.slots, [0] * self.slots
        self.remaining, self.steps, self.read_to = [0] * self.slots, [0] * self.slots, [0] * self.slots
        self.fields = ST_FIELDS
        self.host = torch.empty(engine.snapshot_all_ints(), dtype=torch.int32).pin_memory()
        self.cur = torch.cuda.current_stream(engine.dev)

    def start(self, slot: int, plen: int, max_new_tokens: int):
        """A request was prefilled into the slot."""
        self.plen[slot], self.mnt[slot] = plen, max_new_tokens
        self.remaining[slot], self.steps[slot], self.read_to[slot] = max_new_tokens + 8, 0, 0

    def round(self, busy, egress=None) -> tuple:
        """One round over the busy slots -> ({slot: fp32 waveform [1, 1, 512 n] of the round, for the slots with
        audio or that ended}, the slots that ended). With a resampler the waveforms go through ONE push of it first
        (the ended slots as final) and leave at its rate, [1, 1, any n >= 0]. egress(wavs), if given, is called on the
        engine's stream behind the round's windows (the PCM16 pack)."""
        import torch
        from .engine import codes_count
        e, dec, fields = self.e, self.dec, self.fields
        nf, S = len(fields), e.st_all.shape[1]
        remaining, steps, read_to = self.remaining, self.steps, self.read_to
        k = min(self.chunk, max(remaining[s] for s in busy))
        hi = max(busy) + 1 if e.batch_shrink else self.slots
        e.stream.wait_stream(self.ae.stream)  # the previous round's windows first
        e.step(k, slots=next(b for b in self.sizes if b >= hi))
        e.snapshot_all(self.host).synchronize()
        vals = self.host.tolist()
        if any(vals[nf * S:]):  # the words check_errors() reads, copied with the state
            e.check_errors()
        pieces, ended = {}, []
        for s in busy:
            remaining[s] -= k
            steps[s] += k
            stt = {f: vals[j * S + s] for j, f in enumerate(fields)}
            if stt["active"]:
                t1 = min(self.plen[s] + 1 + steps[s] - 9, self.plen[s] + self.mnt[s])
                if t1 > read_to[s] and stt["offset"] - 9 < t1:
                    raise RuntimeError("a slot's offset is behind the steps enqueued")
            else:  # ended (EOS countdown or max_new_tokens): read_codes' count
                t1 = codes_count(stt)
                ended.append(s)
            t1 = max(t1, read_to[s])
            if t1 > read_to[s]:
                pieces[s] = e.read_final_codes(s, read_to[s], t1)
                read_to[s] = t1
        with torch.cuda.stream(e.stream):  # ordered behind the reads; the next round waits for ae.stream
            wavs = dec.push(pieces) if pieces else {}
            tails = dec.flush(ended) if ended else {}
            for s, tail in tails.items():
                w = wavs.get(s)
                wavs[s] = tail if w is None or w.shape[-1] == 0 else \
                    w if tail.shape[-1] == 0 else torch.cat([w, tail], dim=-1)
            wavs = {s: wavs[s] for s in sorted(wavs) if wavs[s].shape[-1] or s in tails}
            if self.rs is not None and wavs:
                wavs = self.rs.push(wavs, final=ended)
            if egress is not None:
                egress(wavs)
        self.cur.wait_stream(e.stream)
        for w in wavs.values():
            w.record_stream(self.cur)
        for s in ended:
            e.pos_hi[s] = 0  # its rows are inactive (position -1): no bound on the attention form
        return wavs, ended


# ---------------------------------------------------------------------- PCM16 egress
class Pcm16Egress:
    """A round's waveforms -> int16 on the host: ONE zmi_pcm16_pack launch converts every lane's samples and packs them
    back to back into one device buffer, ONE asynchronous copy moves it to a pinned staging buffer, and the host waits
    on ONE event. The device buffer, the staging buffer and the segment tables are kept across rounds (sized for
    lanes x (2 chunk_frames + DAC_LOOKAHEAD_FRAMES) frames, grown if a round ever exceeds that)."""

    def __init__(self, device, lanes: int, chunk_frames: int):
        import torch
        from . import _lib
        from .config import DAC_HOP
        from .streaming import DAC_LOOKAHEAD_FRAMES
        self.dev, self.lib = torch.device(device), _lib.lib()
        self.seg_host = torch.empty(int(lanes), 3, dtype=torch.int64).pin_memory()  # ZmiPcmSeg rows: src, n, dst
        self.seg_np = self.seg_host.numpy()
        self.seg_dev = torch.empty(int(lanes), 3, dtype=torch.int64, device=self.dev)
        self._alloc(int(lanes) * (2 * int(chunk_frames) + DAC_LOOKAHEAD_FRAMES) * DAC_HOP)
        self.event = torch.cuda.Event()
        self.layout: list = []  # (key, dst, n) of the round in flight
        self.keep = None

    def _alloc(self, samples: int):
        import torch
        self.cap = samples
        self.pcm_dev = torch.empty(samples, dtype=torch.int16, device=self.dev)
        self.pcm_host = torch.empty(samples, dtype=torch.int16).pin_memory()

    def enqueue(self, wavs: dict, stream):
        """Pack wavs {key: fp32 [.., n]} (in the dict's order) on `stream` and start the copy to the host."""
        import torch
        from . import _lib
        self.layout, rows, total = [], [], 0
        self.keep = [w.contiguous().view(-1) for w in wavs.values()]  # alive until the pack has run
        for key, w in zip(wavs, self.keep):
            n = w.numel()
            self.layout.append((key, total, n))
            if n:
                rows.append((w.data_ptr(), n, total))
                total += n
        if not rows:
            return
        if len(rows) > self.seg_host.shape[0] or total > self.cap:
            raise RuntimeError(f"pcm16 egress: {len(rows)} segments / {total} samples exceed the buffers")
        with torch.cuda.stream(stream):
            self.seg_np[:len(rows)] = rows
            self.seg_dev[:len(rows)].copy_(self.seg_host[:len(rows)], non_blocking=True)
            _lib.check(self.lib.zmi_pcm16_pack(self.seg_dev.data_ptr(), len(rows), total, self.pcm_dev.data_ptr(),
                                               stream.cuda_stream), "pcm16_pack")
            self.pcm_host[:total].copy_(self.pcm_dev[:total], non_blocking=True)
            self.event.record(stream)

    def reserve(self, lanes: int, samples: int):
        """Grow the buffers (between rounds: nothing is in flight)."""
        import torch
        if lanes > self.seg_host.shape[0]:
            self.seg_host = torch.empty(lanes, 3, dtype=torch.int64).pin_memory()
            self.seg_np = self.seg_host.numpy()
            self.seg_dev = torch.empty(lanes, 3, dtype=torch.int64, device=self.dev)
        if samples > self.cap:
            self._alloc(samples)

    def collect(self) -> dict:
        """{key: int16 CPU tensor [1, 1, n]} of the round enqueued; each owns its memory (a copy out of the staging
        buffer), so a consumer may keep it."""
        if any(n for _, _, n in self.layout):
            self.event.synchronize()
        out = {key: self.pcm_host[dst: dst + n].clone().view(1, 1, -1) for key, dst, n in self.layout}
        self.layout, self.keep = [], None
        return out


# ---------------------------------------------------------------------- the session
class ServeSession:
    """Zonos.serve(): see the module docstring. For every ticket the chunks concatenated are, bit for bit,
    autoencoder.decode(generate_batch([cond], [prefix], max_new_tokens=[n], cfg_scale=c, sampling_params=sp,
    seeds=[seed])[0]) (with sample_rate, autoencoder.resample(that, 44100, sample_rate); with pcm16, the waveform's
    clamp(-1, 1) * 32767 truncated to int16, a launch of its own behind the resampler's), whenever the request was
    admitted, whichever slot it got and whatever the other slots were doing: the stepping kernels are row-invariant.
    Every ticket that is not cancelled gets exactly one item with last = True (its chunk may be empty).
    guidance=False: a guidance-free session (the engine's single layout for as long as it is open); submit() then
    takes cfg_scale=1 only. Guided and guidance-free requests do not mix in one session."""

    def __init__(self, model, max_slots: int, max_seqlen: int, max_prefill: int, chunk_frames: int = 16,
                 pcm16: bool = False, sample_rate: int | None = None, decoder: str = "window",
                 guidance: bool = True, prefill_chunk: int | None = None):
        if chunk_frames < 1:
            raise ValueError("chunk_frames >= 1")
        carry = model._decoder_mode(decoder)
        rate = model._output_rate(sample_rate)  # None: 44.1 kHz, the path without a resampler
        if getattr(model, "_serving", None) is not None:
            raise RuntimeError("a serve() session is already open on this model")
        self.model, self.pcm16 = model, bool(pcm16)
        self.guidance = bool(guidance)
        self.sched = SlotScheduler(max_slots, max_seqlen, max_prefill, model.config.backbone.d_model, self.guidance,
                                   prefill_chunk)
        model._ensure_capacity(max_slots, max_seqlen, max_prefill)  # once: a session never rebuilds the engine
        model._select_layout(2.0 if self.guidance else 1)  # the session's layout, for as long as it is open
        e, ae = model.engine, model.autoencoder
        key = (id(ae), int(chunk_frames), carry)
        dec = model._stream_batch_decoders.get(key)
        if dec is None or dec.lanes < max_slots:  # kept: its graphs and stage buffers serve every later call
            dec = model._stream_batch_decoders[key] = ae.stream_decoder_batch(max_slots, chunk_frames, carry=carry)
        for s in range(max_slots):
            dec.reset(s)
        self.dec = dec
        self.rs = None if rate is None else model._stream_resampler(rate, max_slots)  # kept, every lane reset
        self.rounds = BatchRounds(e, ae, dec, max_slots, chunk_frames, self.rs)
        self.egress = Pcm16Egress(e.dev, max_slots, chunk_frames) if self.pcm16 else None
        # chunked prefill: the prompts in flight (prefill_plan.ChunkPlanner) and their slots, occupied but inactive
        self.planner = None if self.sched.prefill_chunk is None else e.chunk_planner(self.sched.prefill_chunk)
        self.mid: dict = {}  # slot -> Request of the slots mid-prompt
        self.passes_run = 0
        self.rounds_run = 0
        self._open = True
        model._serving = self

    # ---- any thread
    def submit(self, cond, audio_prefix_codes=None, max_new_tokens: int = 86 * 30, cfg_scale: float = 2.0,
               sampling_params: dict = dict(min_p=0.1), seed: int | None = None) -> int:
        """Queue a request; returns its ticket. No GPU work. ValueError for a request that can never fit (the session
        is untouched)."""
        from .engine import SamplingParams
        from .model import _draw_seed
        if self.guidance:
            assert cfg_scale != 1, "cfg_scale=1 runs in a serve(guidance=False) session (one layout per session)"
        elif cfg_scale != 1:
            raise ValueError(f"a serve(guidance=False) session takes cfg_scale=1 only, got {cfg_scale!r}")
        self.sched.fit(cond.shape, None if audio_prefix_codes is None else audio_prefix_codes.shape, max_new_tokens)
        params = SamplingParams.from_dict(dict(sampling_params), cfg_scale, _draw_seed() if seed is None else seed)
        return self.sched.submit(cond.shape, None if audio_prefix_codes is None else audio_prefix_codes.shape,
                                 max_new_tokens, (cond, audio_prefix_codes, params))

    def cancel(self, ticket: int) -> bool:
        """A waiting request never runs; a running one is released at the start of the next round. No further item is
        produced for the ticket. False for an unknown or finished ticket."""
        return self.sched.cancel(ticket)

    @property
    def idle(self) -> bool:
        return self.sched.idle

    def wait_for_work(self, timeout: float | None = None) -> bool:
        return self.sched.wait_for_work(timeout)

    # ---- the driving thread
    def run_round(self) -> list:
        """One round: cancellations, admissions (one prefill_many; with prefill_chunk the admitted prompts are queued and
        _prefill_passes runs their chunks, a slot mid-prompt being occupied but inactive: not stepped as busy, no
        items), the steps, and the round's audio as
        [(ticket, chunk, last)]: fp32 device tensors [1, 1, 512 n] as stream_batch() yields them, or with pcm16
        int16 CPU tensors; with sample_rate a chunk has any length >= 0. [] at once when nothing is running or
        waiting."""
        import torch
        if not self._open:
            raise RuntimeError("the session is closed")
        with torch.inference_mode():
            e, rounds = self.model.engine, self.rounds
            released, admitted = self.sched.begin_round()
            for s in released:
                self.dec.reset(s)
                if self.rs is not None:
                    self.rs.reset(s)
                e.release(s)
                if self.mid.pop(s, None) is not None:  # cancelled mid-prompt: its remaining chunks are dropped
                    self.planner.drop(s)
            if admitted and self.planner is None:
                e.prefill_many([(s, *r.payload[:2], r.max_new_tokens, r.payload[2]) for s, r in admitted])
                for s, r in admitted:
                    rounds.start(s, r.p, r.max_new_tokens)
                    if self.rs is not None:
                        self.rs.reset(s)
            elif self.planner is not None:
                self._prefill_passes(admitted)
            busy = [(s, r) for s, r in self.sched.busy() if s not in self.mid]
            if not busy:
                return []
            owner = dict(busy)
            pack = None
            if self.egress is not None:
                def pack(wavs):
                    self.egress.reserve(len(wavs), sum(w.shape[-1] for w in wavs.values()))
                    self.egress.enqueue(wavs, e.stream)
            wavs, ended = rounds.round([s for s, _ in busy], pack)
            self.rounds_run += 1
            chunks = self.egress.collect() if self.egress is not None else wavs
            live = {s: self.sched.finish(s)[1] for s in ended}
            gone = self.sched.cancelled()  # cancelled from another thread while the round ran: no further item
            return [(owner[s].ticket, chunks[s], s in live) for s in chunks
                    if live.get(s, True) and owner[s].ticket not in gone]

    def _prefill_passes(self, admitted):
        """Chunked prefill's share of a round: the admitted requests are staged (occupied, inactive) and queued; while
        any ticket is decoding, at most ONE pass runs in front of the round's steps, so its audio waits for a chunk and
        not for a prompt; when none is decoding, passes run back to back until a slot starts. A slot whose last chunk
        has run starts its round bookkeeping (rounds.start) and decodes from this round on."""
        e = self.model.engine
        for s, r in admitted:
            e.chunked_admit(self.planner, s, *r.payload[:2], r.max_new_tokens, r.payload[2])
            self.mid[s] = r
        decoding = any(s not in self.mid for s, _ in self.sched.busy())
        while self.planner.pending:
            done = e.chunked_pass(self.planner)
            self.passes_run += 1
            for s in done:
                r = self.mid.pop(s)
                self.rounds.start(s, r.p, r.max_new_tokens)
                if self.rs is not None:
                    self.rs.reset(s)
            if decoding or done:
                break

    def close(self):
        """Reset every DAC lane, release every busy slot, and let the model's other entry points run again."""
        if not self._open:
            return
        self._open = False
        try:
            busy = self.sched.release_all()
            for s in range(self.sched.max_slots):
                self.dec.reset(s)
                if self.rs is not None:
                    self.rs.reset(s)
            for s in busy:
                self.model.engine.release(s)
            if self.planner is not None:
                self.planner.clear()
                self.mid.clear()
        finally:
            self.model._serving = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


__all__ = ["SlotScheduler", "Request", "BatchRounds", "Pcm16Egress", "ServeSession", "size_buckets"]
