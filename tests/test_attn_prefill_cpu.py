"""The tile table of the causal prefill attention (zonos_vibes_amd/prefill_table.py): every (sequence, position) in
exactly one tile, no tile across two sequences, most keys first, n_tiles = sum of ceil(len / QT)."""
import numpy as np
import pytest

from zonos_vibes_amd.prefill_table import prefill_counts, prefill_table, tile_keys


def _edge_sets(qt):
    lens = [0, 1, qt - 1, qt, qt + 1]
    yield [(0, 0, 0, 0)]
    yield []
    for pos0 in (0, 3, 509):  # 3 and 509 are multiples of no QT (16, 8, 4)
        seqs, row = [], 0
        for i, n in enumerate(lens):
            seqs.append((row, n, len(lens) - 1 - i, pos0 + i))
            row += n + 1  # (a gap row between the sequences)
        yield seqs
    rng = np.random.default_rng(7 + qt)
    for _ in range(6):
        n_seq = int(rng.integers(1, 9))
        seqs, row = [], 0
        for s in rng.permutation(n_seq):
            n = int(rng.integers(0, 700))
            seqs.append((row, n, int(s), int(rng.integers(0, 600))))
            row += n
        yield [seqs[i] for i in rng.permutation(n_seq)]  # q rows not in sequence order


@pytest.mark.parametrize("qt", [4, 8, 16])
def test_tiles_partition_every_sequence(qt):
    for seqs in _edge_sets(qt):
        sa, tiles = prefill_table(seqs, qt)
        assert sa.dtype == np.int32 and tiles.dtype == np.int32
        assert sa.shape == (len(seqs), 4) and tiles.shape[1:] == (2,)
        assert sa.tolist() == [list(s) for s in seqs]
        assert len(tiles) == sum((n + qt - 1) // qt for _, n, _, _ in seqs)  # n_tiles
        cover = [np.zeros(n, dtype=np.int64) for _, n, _, _ in seqs]
        for s, off in tiles.tolist():
            assert 0 <= s < len(seqs) and off % qt == 0 and 0 <= off < seqs[s][1]  # inside ONE sequence
            cover[s][off: min(off + qt, seqs[s][1])] += 1
        assert all((c == 1).all() for c in cover)  # every (sequence, position) in exactly one tile
        keys = tile_keys(sa, tiles, qt)
        assert (np.diff(keys) <= 0).all()  # non-increasing key count: the longest walks are dispatched first
        for (s, off), k in zip(tiles.tolist(), keys.tolist()):
            assert k == seqs[s][3] + min(off + qt, seqs[s][1])


def test_table_refuses_bad_sequences():
    with pytest.raises(ValueError):
        prefill_table([(0, -1, 0, 0)], 4)
    with pytest.raises(ValueError):
        prefill_table([(0, 4, 0, -2)], 4)
    with pytest.raises(ValueError):
        prefill_table([(0, 4, 0, 0)], 0)


def test_engine_tables_are_two_sequences_per_slot():
    from zonos_vibes_amd.engine import HipEngine
    assert HipEngine._slot_seqs(3, 10, 161) == [(10, 161, 6, 0), (171, 161, 7, 0)]


def test_counted_traffic_matches_the_shapes():
    """C5 (S 591, production heads): one query per row reads S (S + 1) / 2 keys x 512 B per (sequence, kv head);
    a tile of 4 positions reads its keys once."""
    seqs = [(0, 591, 0, 0), (591, 591, 1, 0)]
    c = prefill_counts(seqs, 4, 4)
    assert c["rows"]["kv_bytes"] == 2 * 4 * (591 * 592 // 2) * 512
    assert c["tiles"]["kv_bytes"] == 2 * 4 * sum(min(o + 4, 591) for o in range(0, 591, 4)) * 512
    assert 3.9 < c["rows"]["kv_bytes"] / c["tiles"]["kv_bytes"] < 4.0
    assert 3.5 < c["rows"]["mfma"] / c["tiles"]["mfma"] <= 4.0
