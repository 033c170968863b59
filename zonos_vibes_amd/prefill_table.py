"""The tile table of zmi_attention_prefill (include/zonos_hip.h): which QT consecutive positions of which
sequence each workgroup takes, in dispatch order. Pure host code (numpy), used by the engines' prefill and
tested without a GPU."""
from __future__ import annotations

import numpy as np

PREFILL_ATTN = ("tiles", "rows")  # HipEngine.prefill_attn: zmi_attention_prefill / one query per row (zmi_attention_pf)


def prefill_table(seqs, qt: int) -> tuple[np.ndarray, np.ndarray]:
    """seqs: (q_row0, len, kv_row, pos0) per sequence (ZmiAttnSeq); qt: zmi_attention_prefill_queries(hq, hkv).

    Returns (seq table int32 [n_seq][4], tile table int32 [n_tiles][2] of (seq, off)). Sequence s is cut from its
    first position into tiles of qt positions, off = 0, qt, 2 qt, ... (the last one may be short), so every
    (sequence, position) lies in exactly one tile, no tile spans two sequences and n_tiles = sum of
    ceil(len / qt). The tiles are ordered by their key count pos0 + min(off + qt, len) (the keys the tile's last
    row attends), largest first: the later tiles of a causal walk do more work, so they are dispatched first.
    Ties keep (sequence, off) order."""
    if qt <= 0:
        raise ValueError(f"qt must be positive, got {qt}")
    sa = np.asarray(list(seqs), dtype=np.int64).reshape(-1, 4)
    if (sa < 0).any():
        raise ValueError("prefill_table: negative row, length or position")
    if sa.size and int(sa.max()) > np.iinfo(np.int32).max:
        raise ValueError("prefill_table: value beyond int32")
    lens, pos0 = sa[:, 1], sa[:, 3]
    counts = (lens + qt - 1) // qt
    seq = np.repeat(np.arange(len(sa), dtype=np.int64), counts)
    first = np.cumsum(counts) - counts  # index of each sequence's first tile
    off = (np.arange(int(counts.sum()), dtype=np.int64) - first[seq]) * qt
    keys = pos0[seq] + np.minimum(off + qt, lens[seq])
    order = np.argsort(-keys, kind="stable")
    tiles = np.stack([seq[order], off[order]], axis=1) if len(order) else np.zeros((0, 2), dtype=np.int64)
    return np.ascontiguousarray(sa, dtype=np.int32), np.ascontiguousarray(tiles, dtype=np.int32)


def tile_keys(sa: np.ndarray, tiles: np.ndarray, qt: int) -> np.ndarray:
    """Key count of each tile (its last row's position + 1)."""
    s, off = tiles[:, 0], tiles[:, 1].astype(np.int64)
    return sa[s, 3] + np.minimum(off + qt, sa[s, 1])


def prefill_counts(seqs, qt: int, hkv: int, hd: int = 128) -> dict:
    """K/V bytes read and MFMAs issued by one launch per layer, counted from the shapes: the tiled kernel
    (per tile and kv head: its keys once, 2 cache tensors) against one query per row (every row its own keys).
    MFMAs are v_mfma_f32_16x16x32_bf16: per 32 keys hd / 32 x 2 for the scores and hd / 16 for P.V, issued for
    whole 32-key tiles."""
    sa, tiles = prefill_table(seqs, qt)
    per32 = hd // 32 * 2 + hd // 16
    tk = tile_keys(sa, tiles, qt)
    rows_keys = sum(int(l) * int(p0) + int(l) * (int(l) + 1) // 2 for _, l, _, p0 in sa)
    rows_t32 = sum(int(((np.arange(int(l)) + int(p0) + 1 + 31) // 32).sum()) for _, l, _, p0 in sa)
    return {"tiles": {"kv_bytes": int(tk.sum()) * hkv * hd * 2 * 2, "mfma": int(((tk + 31) // 32).sum()) * hkv * per32},
            "rows": {"kv_bytes": rows_keys * hkv * hd * 2 * 2, "mfma": rows_t32 * hkv * per32}}
