"""Scoring of given token sequences on the GPU: per-token log-probabilities, ranks and argmax,
per-sequence negative log-likelihood, and the multiple-choice prediction of the reference's
HellaSwag evaluation (train_gpt2.py:190-202, 394-426).

Position t of a sequence predicts ids[:, t + 1], weighted by mask[:, t + 1] (the shift of
get_most_likely_row).  The model runs up to its final LayerNorm once; the lm_head GEMM then runs
only on the hidden rows that are scored (HellaSwag's context rows and a caption model's image
rows never reach it), in chunks of at most `chunk_rows` rows through one reused logits buffer,
and gvl_token_logprobs reads each chunk once.  gvl_sequence_score reduces the per-token values
per sequence and per example.  No [N, T, V] logits tensor and no fp32 copy of one exists.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import functional as Fn
from . import kernels as K
from .functional import bf

__all__ = ["Score", "score", "most_likely_row", "evaluate_hellaswag"]


@dataclass
class Score:
    """sum_nll, mean_nll fp32 [N] and count int32 [N] over each sequence's scored positions;
    pred_norm, pred int32 [N / group]: per example the index of the sequence with the lowest
    mean_nll / sum_nll (first minimum; -1 when one of its sequences has no scored position).
    With return_tokens: logp fp32, rank and argmax int32, each [N, T - 1], column t for the
    prediction of ids[:, t + 1]; positions that were not scored hold 0, -1, -1."""
    sum_nll: torch.Tensor
    count: torch.Tensor
    mean_nll: torch.Tensor
    pred_norm: torch.Tensor
    pred: torch.Tensor
    logp: Optional[torch.Tensor] = None
    rank: Optional[torch.Tensor] = None
    argmax: Optional[torch.Tensor] = None


def _text_hidden(model, ids, z):
    """-> (x [N, S, C] final-LayerNorm hidden states, M: text position t is row M + t of a
    sequence, T: text positions kept, lm_head weight)."""
    from . import caption, cross_att, gpt2
    if isinstance(model, caption.GPT_Caption):
        if z is None:
            raise ValueError("gvl.score: a caption model needs its image tokens z")
        x, M, T = model.hidden(z, ids)
        return x, M, T, model.gpt.lm_head.weight
    if isinstance(model, cross_att.GPT):
        return model.hidden(ids, z), 0, ids.shape[1], model.lm_head.weight
    if isinstance(model, gpt2.GPT):
        if z is not None:
            raise ValueError("gvl.score: gvl.gpt2.GPT takes no image tokens")
        return model.hidden(ids), 0, ids.shape[1], model.lm_head.weight
    raise TypeError(f"gvl.score: unsupported model {type(model).__name__} (gvl.gpt2.GPT, "
                    "gvl.caption.GPT_Caption or gvl.cross_att.GPT)")


@torch.no_grad()
def score(model, ids, mask=None, *, z=None, group=1, select="masked", chunk_rows=8192,
          return_tokens=False):
    """Score ids [N, T] under `model` (gvl.gpt2.GPT; gvl.caption.GPT_Caption and subclasses with
    the image tokens z, text after the bridge tokens, cut at block_size as in forward;
    gvl.cross_att.GPT with z or None).  mask [N, T] of 0 / 1 (default: ones) selects the scored
    tokens; `group` consecutive sequences form one multiple-choice example.

    select="masked": the lm_head runs on the rows with a nonzero shifted mask only (one host read
    for their number).  select="all": on every one of the N * (T - 1) shifted rows, so every
    position has per-token results; the mask still selects what the sequence sums count.
    -> Score."""
    if select not in ("masked", "all"):
        raise ValueError(f"gvl.score: select must be 'masked' or 'all' (got {select!r})")
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("gvl.score: chunk_rows must be >= 1")
    if ids.dim() != 2:
        raise ValueError("gvl.score: ids must be [N, T]")
    if mask is not None and tuple(mask.shape) != tuple(ids.shape):
        raise ValueError("gvl.score: mask must have the shape of ids")
    dev = ids.device

    def selection(T):
        """(shifted mask uint8 [N, T - 1] or None, flat indices of its nonzero entries or None)"""
        if mask is None:
            return None, None
        smask = (mask[:, 1:T].to(dev) != 0).to(torch.uint8).contiguous()
        if select != "masked":
            return smask, None
        return smask, smask.view(-1).nonzero().view(-1)  # the host read: how many rows

    # before the model runs: the host read then waits for no kernel, and everything after it is
    # queued behind the forward without a stall
    smask, sel = selection(ids.shape[1])
    was_training = model.training
    if was_training:
        model.eval()
    try:
        x, M, T, w = _text_hidden(model, ids, z)
        N, S, C = x.shape
        if T < ids.shape[1]:  # a caption model cut the text at block_size
            ids = ids[:, :T]
            smask, sel = selection(T)
        Ts = T - 1
        targets = ids[:, 1:].reshape(-1)
        # row of x.view(N * S, C) that predicts shifted position (n, t)
        pos = (torch.arange(N, device=dev)[:, None] * S + M +
               torch.arange(Ts, device=dev)[None, :]).reshape(-1)
        if sel is not None:
            pos, targets = pos[sel], targets[sel]
        R = pos.numel()
        rows = x.reshape(N * S, C).index_select(0, pos)
        targets = targets.contiguous()
        i32 = torch.int32
        logp = torch.empty(R, dtype=torch.float32, device=dev)
        rank = torch.empty(R, dtype=i32, device=dev) if return_tokens else None
        amax = torch.empty(R, dtype=i32, device=dev) if return_tokens else None
        wp, V = Fn.pad_vocab(bf(w))
        if R > 0:
            buf = torch.empty(min(chunk_rows, R), wp.shape[0], dtype=torch.bfloat16, device=dev)
        for i in range(0, R, chunk_rows):
            n = min(chunk_rows, R - i)
            logits = K.linear(rows[i:i + n], wp, out=buf[:n])
            K.token_logprobs(logits, targets[i:i + n], vocab=V, logp=logp[i:i + n], lse=None,
                             argmax=None if amax is None else amax[i:i + n],
                             rank=None if rank is None else rank[i:i + n])
        if sel is not None:  # scatter the scored rows; the others hold 0, -1, -1

            def full(t, fill):
                return torch.full((N * Ts,), fill, dtype=t.dtype, device=dev).index_copy_(0, sel, t)

            logp = full(logp, 0.0)
            if return_tokens:
                rank, amax = full(rank, -1), full(amax, -1)
        logp = logp.view(N, Ts)
        out = K.sequence_score(logp, smask, group)
        res = Score(*out)
        if return_tokens:
            res.logp, res.rank, res.argmax = logp, rank.view(N, Ts), amax.view(N, Ts)
        return res
    finally:
        if was_training:
            model.train()


def most_likely_row(model, tokens, mask, *, z=None) -> int:
    """get_most_likely_row (train_gpt2.py:190-202) without a logits tensor from the caller: the
    index of the row of tokens [E, T] with the lowest masked mean loss, E <= 16."""
    return int(score(model, tokens, mask, z=z, group=tokens.shape[0]).pred_norm[0].item())


def evaluate_hellaswag(model, examples, process_group=None):
    """The HellaSwag loop of train_gpt2.py:394-426.  examples: any iterable of (tokens [4, T],
    mask [4, T], label), what the reference's render_example yields after its first item; example
    i is scored by rank i % world_size (:399) and the counts are summed over the group (:410-416).
    -> (num_correct_norm, num_correct, num_total)."""
    import torch.distributed as dist

    from .dist import all_reduce_sum_
    rank, world = 0, 1
    if dist.is_initialized():
        rank, world = dist.get_rank(process_group), dist.get_world_size(process_group)
    dev = next(model.parameters()).device
    stats = torch.zeros(3, dtype=torch.long, device=dev)  # correct_norm, correct, total
    for i, (tokens, mask, label) in enumerate(examples):
        if i % world != rank:
            continue
        tokens, mask = tokens.to(dev), mask.to(dev)
        s = score(model, tokens, mask, group=tokens.shape[0])
        stats[0] += (s.pred_norm[0] == int(label)).long()
        stats[1] += (s.pred[0] == int(label)).long()
        stats[2] += 1
    all_reduce_sum_(stats, process_group)
    nc_norm, nc, total = (int(v) for v in stats.tolist())
    return nc_norm, nc, total
