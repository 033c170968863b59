"""Shared cases of the guidance-free (cfg_scale = 1) tests.

oracle_run() is the loop of oracle.zonos_cpu.OracleZonos.generate() (reference model.py:218-315) restated so that it
also takes the branch the oracle's generate() asserts away: with cfg_scale == 1 the cache has ONE row per utterance,
input ids are not expanded, hidden states are not repeated and compute_logits applies no CFG arithmetic
(model.py:112, 134-136, 193; OracleZonos.prefill / compute_logits already take that branch). In its guided mode it
is OracleZonos.generate() op for op (tests/test_cfg1_cpu.py pins that), which is what validates the loop. It can be
teacher-forced along a fixed delayed trajectory and returns the logits of every decision.
"""
import torch

from oracle.zonos_cpu import (EOS, MASK, N_CB, UNKNOWN, apply_delay_pattern, revert_delay_pattern, sample,
                              sample_params)


@torch.inference_mode()
def oracle_run(om, prefix_conditioning, audio_prefix_codes=None, max_new_tokens=24, cfg_scale=2.0,
               sampling_params=dict(min_p=0.1), teacher=None, max_decisions=None):
    """-> (codes [1, 9, T], [logits [1, 9, 1026] per decision, as compute_logits returns them: before the EOS bias],
    final delayed buffer). teacher: a delayed trajectory [1, 9, >= P + N + 9] whose frames are the inputs whatever is
    sampled. cfg_scale == 1: prefix_conditioning [1, Lc, d] (of [2, Lc, d] row 0), one cache row."""
    guided = cfg_scale != 1
    if not guided:
        prefix_conditioning = prefix_conditioning[:1]
    bsz = 1
    p_len = 0 if audio_prefix_codes is None else audio_prefix_codes.shape[2]
    audio_len = p_len + max_new_tokens
    seq_len = prefix_conditioning.shape[1] + audio_len + 9
    cache = om.new_cache((2 if guided else 1) * bsz, seq_len)
    codes = torch.full((bsz, N_CB, audio_len), UNKNOWN)
    if audio_prefix_codes is not None:
        codes[..., :p_len] = audio_prefix_codes
    delayed = apply_delay_pattern(codes, MASK)
    if teacher is not None:
        delayed = teacher[..., : delayed.shape[2]].clone().long()
    pre = delayed[..., : p_len + 1]
    sp = sample_params(sampling_params)
    trace = []

    logits = om.prefill(prefix_conditioning, pre, cache, cfg_scale)
    trace.append(logits.clone())
    nxt = sample(logits, generated=None, **sp)
    offset = pre.shape[2]
    frame = delayed[..., offset: offset + 1]
    frame.masked_scatter_(frame == UNKNOWN, nxt)
    plen = prefix_conditioning.shape[1] + p_len + 1
    cache["offset"] += plen
    cache["lengths"][:] += plen

    bias = torch.zeros_like(logits)
    bias[:, 1:, EOS] = -torch.inf
    stopping = torch.zeros(bsz, dtype=torch.bool)
    max_steps = delayed.shape[2] - offset
    remaining = torch.full((bsz,), max_steps)
    cfg_t = torch.tensor(cfg_scale)
    while torch.max(remaining) > 0 and (max_decisions is None or len(trace) < max_decisions):
        offset += 1
        ids = delayed[..., offset - 1: offset]
        if guided:
            logits = om.decode_one(ids, cache, cfg_t)
        else:  # model.py:134-136 without the repeat: one row
            logits = om.compute_logits(om.embed_codes(ids), cache, 1.0)
        trace.append(logits.clone())
        logits += bias
        nxt = sample(logits, generated=delayed[..., :offset], **sp)
        eos0 = nxt[:, 0] == EOS
        remaining[eos0[:, 0]] = torch.minimum(remaining[eos0[:, 0]], torch.tensor(9))
        stopping |= eos0[:, 0]
        idx = torch.clamp(9 - remaining, max=8)
        for i in range(nxt.shape[0]):
            if stopping[i]:
                j = idx[i].item()
                nxt[i, :j] = MASK
                nxt[i, j] = EOS
        frame = delayed[..., offset: offset + 1]
        frame.masked_scatter_(frame == UNKNOWN, nxt)
        cache["offset"] += 1
        cache["lengths"][:] += 1
        remaining -= 1
    out = revert_delay_pattern(delayed)
    out.masked_fill_(out >= 1024, 0)
    return out[..., : offset - 9], trace, delayed


def cond_single(lc: int, d: int, seed: int) -> torch.Tensor:
    """One conditioning row block [1, Lc, d] bf16 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, lc, d, generator=g) * 0.5).to(torch.bfloat16)


def random_prefix(p: int, seed: int) -> torch.Tensor:
    """Audio prefix codes [1, 9, p] int64 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 1024, (1, 9, p), generator=g)
