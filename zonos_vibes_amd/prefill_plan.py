"""Chunked prefill's planner: which rows of which prompt go through the layers in which pass. Pure host code, used by
the engines (HipEngine.prefill_many(prefill_chunk=C), ServeSession) and tested without a GPU.

A prompt of s_len rows runs as chunks [k C, min((k + 1) C, s_len)), k = 0, 1, ...: the boundaries depend on the prompt
and C alone, never on what else is admitted (on the hybrid the Mamba2 state is rounded to bf16 at a boundary, so the
boundaries are part of the result). A pass holds at most `pre_rows` rows and at most one chunk per slot; a slot's
sequences (cond and uncond in the paired layout) sit in the same pass; chunks are taken oldest slot first, and a pass
ends at the first chunk that does not fit, so no younger prompt overtakes an older one.
"""
from __future__ import annotations

from dataclasses import dataclass, field


def check_chunk(prefill_chunk, max_prefill: int | None = None):
    """None, or the chunk length as an int; ValueError unless 1 <= prefill_chunk (<= max_prefill, where one is given:
    an engine's or a session's)."""
    if prefill_chunk is None:
        return None
    if isinstance(prefill_chunk, bool) or int(prefill_chunk) != prefill_chunk:
        raise ValueError(f"prefill_chunk must be None or an integer, got {prefill_chunk!r}")
    c = int(prefill_chunk)
    if c < 1 or (max_prefill is not None and c > int(max_prefill)):
        raise ValueError(f"prefill_chunk {c}: expected at least 1" +
                         ("" if max_prefill is None else f" and at most max_prefill {int(max_prefill)}"))
    return c


def chunk_bounds(s_len: int, chunk: int) -> list:
    """[(begin, end)] of a prompt's chunks."""
    if s_len < 1 or chunk < 1:
        raise ValueError("s_len >= 1 and chunk >= 1")
    return [(a, min(a + chunk, s_len)) for a in range(0, s_len, chunk)]


@dataclass
class PassEntry:
    slot: int
    begin: int   # first prompt row of the chunk (= pos0 of its sequences)
    end: int     # row past its last
    off: int     # first row of the slot's chunk in the pass's buffers (rows_per_slot x (end - begin) rows from there)
    last: bool   # the prompt's last chunk: the slot starts after this pass
    job: object = None  # what add() was given for the prompt (the engine: its conditioning, length, first-sample noise)


@dataclass
class Pass:
    entries: list = field(default_factory=list)
    rows: int = 0

    def seqs(self, rps: int) -> list:
        """ZmiAttnSeq rows (q_row0, len, kv_row, pos0) of the pass: sequence `half` of slot s on KV row rps s + half."""
        return [(e.off + half * (e.end - e.begin), e.end - e.begin, rps * e.slot + half, e.begin)
                for e in self.entries for half in range(rps)]

    @property
    def max_pos(self) -> int:
        return max(e.end for e in self.entries) - 1


class ChunkPlanner:
    """The prompts in flight, oldest first, and the next pass over them."""

    def __init__(self, pre_rows: int, rows_per_slot: int, chunk: int):
        if rows_per_slot not in (1, 2):
            raise ValueError("rows_per_slot must be 1 or 2")
        if chunk < 1 or rows_per_slot * chunk > pre_rows:
            raise ValueError(f"a chunk of {chunk} positions ({rows_per_slot} sequences) does not fit {pre_rows} rows")
        self.pre_rows, self.rps, self.chunk = int(pre_rows), int(rows_per_slot), int(chunk)
        self._jobs: list = []  # [slot, s_len, next row, job], in admission order

    def add(self, slot: int, s_len: int, job=None):
        if any(j[0] == slot for j in self._jobs):
            raise ValueError(f"slot {slot} is already mid-prompt")
        if s_len < 1:
            raise ValueError("s_len >= 1")
        self._jobs.append([int(slot), int(s_len), 0, job])

    def drop(self, slot: int) -> bool:
        """Forget the slot's remaining chunks (a cancelled request); False if it had none."""
        n = len(self._jobs)
        self._jobs = [j for j in self._jobs if j[0] != slot]
        return len(self._jobs) != n

    def clear(self):
        self._jobs = []

    @property
    def pending(self) -> bool:
        return bool(self._jobs)

    def slots(self) -> list:
        return [j[0] for j in self._jobs]

    def next_pass(self):
        """The next pass (None when nothing is pending); the chunks it holds are taken off the prompts."""
        if not self._jobs:
            return None
        out = Pass()
        for j in self._jobs:
            slot, s_len, a, job = j
            b = min(a + self.chunk, s_len)
            if out.rows + self.rps * (b - a) > self.pre_rows:
                break
            out.entries.append(PassEntry(slot, a, b, out.rows, b == s_len, job))
            out.rows += self.rps * (b - a)
            j[2] = b
        self._jobs = [j for j in self._jobs if j[2] < j[1]]
        return out
