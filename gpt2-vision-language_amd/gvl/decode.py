"""KV-cached incremental decoding and sampling.

The reference re-runs the whole sequence through forward() for every new token
(train_gpt2.py:440-449 top-k sampling; gpt2_linear/data.py:111-127 temperature + top-p
caption decoding).  Here a prompt is prefilled once into a per-layer KV cache and every new
token costs one row through each block:

  * cache: one packed bf16 [B, Tmax, 3C] tensor per layer — the c_attn GEMM of a new token
    writes its q|k|v row straight into cache[:, t] (ldc = Tmax*3C), so nothing is copied;
  * attention of the new row: gvl_attn_decode over cache[:, :t+1] (k and v as strided views);
  * caption models prefill [bridge(z) | prompt embeddings] (positions on text only,
    gpt2_linear/model.py:197-200); the cross-att model projects z once and caches every
    layer's kv_proj(z_proj) (gpt2_cross-att/model.py:160-165, :49-57);
  * the next token comes from gvl_sample (temperature / top-k / top-p, inverse CDF of a
    uniform drawn from the caller's torch.Generator) or its greedy form (top_k = 1, u = 0:
    the first maximum, torch.argmax's tie-break);
  * beam search (BeamDecoder, beam_search): B items x K beams share one R = B*K-row cache
    through an int32 indirection table src[r, t] (the row holding position t of hypothesis r),
    so reordering beams rewrites the table (gvl_beam_step) and attention reads through it
    (gvl_attn_decode_beam); the prefix is prefilled once per item and no cache row is copied;
  * repetition penalty, no-repeat n-gram, minimum length and bad-token bans edit each step's
    logits in place before the token choice (gvl_logits_process: one launch, a hypothesis'
    history read through the same src table, only the few logits concerned are touched);
  * prompts of different lengths in one batch (prompt_lens): prompt_ids [B, P] is right-padded
    and the cache stays time-aligned.  The prefill runs over all S = M + P columns as ever
    (causality keeps the pads from the real positions), every row's i-th new token lands in
    column S + i, so the c_attn GEMM still writes one uniform column per step, and row r attends
    [0, M + len_r) and [S, S + i]: gvl_attn_decode_ragged skips its gap [M + len_r, S) without
    loading it.  The first logits are gathered from each row's last real row, the new tokens take
    positions len_r + i (gvl_embedding_fwd_pos), and the beam table, gvl_beam_step and the final
    ids gather are untouched (t0 stays S).  Each row decodes as if it had been called alone, and
    no output bit depends on the pad ids.  Writing row r's tokens at M + len_r + i instead would
    need per-row GEMM output addresses.
  * speculative decoding (KVDecoder.step_multi, speculative_generate): Q = draft_len + 1 tokens
    per row per decoder pass.  Rows accept different numbers of drafted tokens, so here the cache
    is compacted, not time-aligned: row r holds kv_len[r] columns (int32 on the device), the
    c_attn GEMM of a pass writes a contiguous [B, Q, 3C] buffer, and gvl_attn_decode_multi lets
    query j of row r attend the cache below kv_len[r] and the buffer's rows 0..j, copying the
    new k / v into cache[r, kv_len[r] + j] in the same launch (no per-row GEMM address, no
    scatter; what a pass wrote and the accept step did not keep is overwritten by the next).
    Query j has the bits of gvl_attn_decode at Tk = kv_len[r] + j + 1.  The draft is a lookup of
    the row's last n-gram in its own prompt + output (gvl_ngram_draft) or the caller's
    draft_ids; gvl_spec_accept compares it with the tokens gvl_sample chose and advances n,
    kv_len, pos and the output on the device.  After start(..., prompt_lens) row r begins at
    kv_len = M + len_r, pos = len_r: its tokens overwrite its pad columns and the gap arrays go
    unused.  step(), BeamDecoder and the ragged path are as they were.
  * graph-replayed decoding (GraphedGenerate, GraphedBeamSearch; generate / beam_search with
    graph=True): step() issues about nine launches per block from Python, and at one row per
    sequence the GPU finishes them faster than the host issues them.  A session keeps every
    buffer of a token's work at a fixed address, keeps what the host used to pass per token
    (the cache column, Tk, n_hist / ban_eos, the beam step) in device scalars read by
    gvl_attn_decode_step, gvl_logits_process_dev and gvl_beam_step_dev, captures one token for all
    rows as one graph and replays it.  The prefill stays eager.  Results equal the eager call's
    bit for bit; nothing existing launches differently.
  * int8 weight-only decoding (weights="int8" or a gvl.quant.quantize_decoder(model) snapshot on
    every entry point; gvl/quant.py): the block matrices and the lm_head as per-row int8.  The
    decoders reach their linears through KVDecoder._linear: K.linear as ever by default, else
    gvl_linear_w8 for the steps and the dequantised matrix through K.linear for the prefill.  An
    element of gvl_linear_w8's output has the same bits at any row count, so graph replay, Q = 1
    and speculative decoding keep their equalities in this mode too.

  * int8 KV cache (kv_cache="int8" on KVDecoder, BeamDecoder, generate, beam_search and the
    graphed sessions; independent of weights=): a layer's cache is kv8 int8 [rows, Tmax, 2C] (k
    heads, then v heads) with kvs fp32 [rows, Tmax, 2H] (one scale per head vector and position,
    gvl_quantize_rows_i8's format) instead of bf16 [rows, Tmax, 3C]: 2.125C bytes per position
    against 6C (kv_cache_bytes), and the q third is not stored.  The prefill quantises its k / v
    in one launch per layer (gvl_kv_quantize_i8); a step writes c_attn into a [rows, 3C] scratch
    and gvl_attn_decode_q8 quantises the new k / v into column t and attends: the attention of a
    step sees, for every position including the step's own, fp32(q8) * scale, and nothing else
    changes.  step() and step_dev() call the one entry point (the column from the host or from
    the device), so the graphed calls keep the eager call's bits; beams pass src, prompts of
    different lengths the gap.  The cross-att model's projected image tokens stay bf16.  Not for
    speculative decoding (step_multi), whose queries read each other's un-appended keys.

Everything runs on the libgvl kernels; no autograd (inference only).
"""
from __future__ import annotations

import weakref

import torch

from . import functional as Fn
from . import kernels as K
from . import quant
from .functional import bf

BF16 = torch.bfloat16


def check_kv_cache(kv_cache):
    """kv_cache: None (the bf16 [rows, Tmax, 3C] cache) or "int8"."""
    if kv_cache is not None and kv_cache != "int8":
        raise ValueError(f"kv_cache must be None or 'int8' (got {kv_cache!r})")
    return kv_cache


def kv_cache_bytes(config, rows, Tmax, kv_cache=None):
    """Bytes of all layers' self-attention caches of a decoder of `config` (n_layer, n_head,
    n_embd) with `rows` sequences of Tmax columns: 6C per position for the bf16 cache (q | k | v),
    2C int8 + 2H fp32 = 2.125C for kv_cache="int8".  Host arithmetic only."""
    check_kv_cache(kv_cache)
    C, H = int(config.n_embd), int(config.n_head)
    per_pos = 2 * C + 4 * 2 * H if kv_cache == "int8" else 2 * 3 * C
    return int(config.n_layer) * int(rows) * int(Tmax) * per_pos


def _block_params(blk):
    a, m = blk.attn, blk.mlp
    return dict(ln1=(bf(blk.ln_1.weight), bf(blk.ln_1.bias)), attn=(bf(a.c_attn.weight), bf(a.c_attn.bias)),
                aproj=(bf(a.c_proj.weight), bf(a.c_proj.bias)), ln2=(bf(blk.ln_2.weight), bf(blk.ln_2.bias)),
                fc=(bf(m.c_fc.weight), bf(m.c_fc.bias)), mproj=(bf(m.c_proj.weight), bf(m.c_proj.bias)),
                H=a.n_head)


def _cross_params(blk):
    xa = blk.xattn
    return dict(ln=(bf(blk.ln_x.weight), bf(blk.ln_x.bias)), q=(bf(xa.q_proj.weight), bf(xa.q_proj.bias)),
                kv=(bf(xa.kv_proj.weight), bf(xa.kv_proj.bias)), c=(bf(xa.c_proj.weight), bf(xa.c_proj.bias)),
                gate=bf(blk.cross_gate), H=xa.n_head)


def check_prompt_lens(prompt_ids, prompt_lens, n_new, block_size):
    """The real lengths of the rows of a right-padded prompt_ids [B, P] as an int64 CPU tensor
    [B].  prompt_lens: B integers (a list, a CPU or a device tensor: one host read), each in
    1..P, and max(len) + n_new - 1 <= block_size: the positions of the n_new - 1 tokens that are
    fed back must exist (what step() otherwise finds out at the step that runs past them)."""
    B, P = prompt_ids.shape
    lens = torch.as_tensor(prompt_lens)
    if lens.is_floating_point() or lens.is_complex() or lens.dtype == torch.bool:
        raise ValueError(f"prompt_lens must hold integers (got {lens.dtype})")
    lens = lens.detach().to(device="cpu", dtype=torch.int64).reshape(-1)
    if lens.numel() != B:
        raise ValueError(f"prompt_lens has {lens.numel()} entries for {B} prompts")
    if B and (int(lens.min()) < 1 or int(lens.max()) > P):
        raise ValueError(f"prompt_lens must lie in 1..P = {P} (got {int(lens.min())}.."
                         f"{int(lens.max())})")
    if B and int(lens.max()) + int(n_new) - 1 > block_size:
        raise ValueError(f"a prompt of {int(lens.max())} tokens + {int(n_new)} new tokens exceeds "
                         f"block_size {block_size}")
    return lens


def ragged_prompt_for_controls(prompt_ids, lens):
    """The prompt gvl_logits_process sees for right-padded prompt_ids [B, P] with lengths lens
    [B]: int64 [B, P], row r = P - len_r entries of -1, then prompt_ids[r, :len_r], so the real
    tokens end where the generated ones begin.  An id outside [0, V) never indexes logits and a
    real token never equals -1, so the bans and penalties are those of the unpadded prompt."""
    P = prompt_ids.shape[1]
    dev = prompt_ids.device
    shift = (P - lens.to(device=dev, dtype=torch.int64)).view(-1, 1)
    col = torch.arange(P, device=dev).view(1, -1)
    real = prompt_ids.to(torch.int64).gather(1, (col - shift).clamp_(min=0))
    return torch.where(col >= shift, real, real.new_full((), -1)).contiguous()


class KVDecoder:
    """Prefill + one-token steps for gvl.gpt2.GPT, gvl.caption.GPT_Caption (its frozen
    decoder) and gvl.cross_att.GPT.  Batch B; the cache holds the prefix + max_new tokens.
    With prompt_lens (start) the prompts are right-padded rows of different lengths: see the
    module docstring."""

    def __init__(self, model, batch: int, max_new: int, weights=None, kv_cache=None):
        from . import caption, cross_att
        self.model = model
        # kv_cache: None (bf16 [rows, Tmax, 3C] per layer) or "int8" ((kv8, kvs) pairs per layer)
        self.kv8 = check_kv_cache(kv_cache) == "int8"
        self.src = None  # BeamDecoder: the table of the step
        # weights: None (bf16), "int8" or a gvl.quant.quantize_decoder(model) result: the whole
        # call then runs the quantised model (gvl.quant; _linear below)
        self.qdec = quant.resolve_weights(model, weights)
        self._dq = False   # prefill: dequantise each matrix ahead of its K.linear
        self._scr = None   # the bf16 buffer it is dequantised into
        self.kind = ("caption" if isinstance(model, caption.GPT_Caption) else
                     "cross" if isinstance(model, cross_att.GPT) else "gpt")
        dec = model.gpt if self.kind == "caption" else model
        tr = dec.transformer
        self.wte, self.wpe = bf(tr.wte.weight), bf(tr.wpe.weight)
        self.lnf = (bf(tr.ln_f.weight), bf(tr.ln_f.bias))
        self.head = bf(dec.lm_head.weight)
        self.blocks = [_block_params(b) for b in tr.h]
        self.cross = [_cross_params(b) for b in tr.h] if self.kind == "cross" else None
        if self.qdec is not None:
            if len(self.qdec.blocks) != len(self.blocks) or self.qdec.n_embd != self.wte.shape[1] \
                    or (self.cross is not None) != (self.qdec.cross is not None):
                raise ValueError("weights: the quantised decoder was made from another model")
            for P, Q in zip(self.blocks, self.qdec.blocks):
                for k in ("attn", "aproj", "fc", "mproj"):
                    P[k] = (Q[k], P[k][1])
            if self.cross is not None:
                for P, Q in zip(self.cross, self.qdec.cross):
                    for k in ("q", "c"):
                        P[k] = (Q[k], P[k][1])
        self.block_size = dec.config.block_size
        C = self.wte.shape[1]
        self.C, self.B, self.max_new = C, batch, max_new
        self.rows = batch  # sequences per step() (BeamDecoder: batch * beams)
        self.Tmax = 0
        self.cache = None  # allocated by prefill: [B, prefix + max_new, 3C] per layer
        self.kvz = None
        self.t = 0        # positions in the cache
        self.txt0 = 0     # cache position of the first text token (caption prefix length)
        # prompts of different lengths (prefill with lens); None: every row has P tokens
        self.gap_lo = None  # int32 [rows], device: row r skips cache columns [gap_lo[r], gap_hi)
        self.gap_hi = 0     # = the prefix length S
        self.pos = None     # int32 [rows], device: the position of the next token of each row
        self.max_len = 0    # the longest prompt (host)
        self.slack = 0      # extra cache columns past prefix + max_new (step_multi: Q of them)

    # ---------------------------------------------------------------- pieces
    def _linear(self, x2, wb, **kw):
        """The one door to the decoders' linears: wb = (weight, bias or None).  bf16 weights go
        to K.linear as ever; a gvl.quant.QWeight to gvl_linear_w8 (dequantised first in the
        prefill and above the kernel's row cap)."""
        if self.qdec is None:
            return K.linear(x2, wb[0], wb[1], **kw)
        qw = wb[0]
        scr = None
        if self._dq or x2.shape[0] > K.LINEAR_W8_MAX_ROWS:
            need = max(qw.q.numel(), self.qdec.scratch_elems())
            if self._scr is None or self._scr.numel() < need:
                self._scr = torch.empty(need, dtype=BF16, device=qw.q.device)
            scr = self._scr
        return qw.linear(x2, wb[1], scratch=scr, dequant=self._dq, **kw)

    def _ln(self, x2, wb):
        return K.layernorm_fwd(x2, wb[0], wb[1], stats=False)[0]

    def _cross(self, l, x2, S, src=None):
        """x + tanh(g) * c_proj(attn(q_proj(ln_x x), kv_proj(z_proj))) for S new rows.
        src (step_multi): int32 [rows of x2, image tokens], the kvz row of each row of x2; the
        rows then go through the one-query kernel, as the rows of step() do."""
        P = self.cross[l]
        kvz = self.kvz[l]
        q = self._linear(self._ln(x2, P["ln"]), P["q"])
        C = self.C
        if src is not None:
            y = K.attn_decode_beam(q, kvz[:, :, :C], kvz[:, :, C:], P["H"], src)
        elif S == 1:
            y = self._attend(q, kvz[:, :, :C], kvz[:, :, C:], P["H"], True)
        else:
            y = K.attn_fwd(q.view(self.B, S, C), kvz[:, :, :C], kvz[:, :, C:], P["H"], False)[0]
            y = y.view(self.B * S, C)
        return self._linear(y, P["c"], residual=x2, gate=P["gate"])

    def _attend(self, q, k, v, H, cross):
        """One new query per row over cached keys / values (self-attention cache, or the
        cross-att model's projected image tokens: no gap there)."""
        if self.gap_lo is not None and not cross:
            return K.attn_decode_ragged(q, k, v, H, self.gap_lo, self.gap_hi)
        return K.attn_decode(q, k, v, H)

    def _new_cache(self, rows, C, device, fill=None):
        """One cache per layer for `rows` sequences: bf16 [rows, Tmax, 3C], or with
        kv_cache="int8" the pair (kv8 int8 [rows, Tmax, 2C], kvs fp32 [rows, Tmax, 2H]).  fill:
        a value to fill it with (kv8 takes it cast to int8)."""
        out = []
        for P in self.blocks:
            if self.kv8:
                c = (torch.empty(rows, self.Tmax, 2 * C, dtype=torch.int8, device=device),
                     torch.empty(rows, self.Tmax, 2 * P["H"], dtype=torch.float32, device=device))
                if fill is not None:
                    c[0].fill_(int(fill))
                    c[1].fill_(fill)
            else:
                c = torch.empty(rows, self.Tmax, 3 * C, dtype=BF16, device=device)
                if fill is not None:
                    c.fill_(fill)
            out.append(c)
        return out

    def _alloc_cache(self, B, C, device):
        """Per-layer cache tensors the prefill writes (_new_cache)."""
        return self._new_cache(B, C, device)

    def _attend_q8(self, qkv, l, t, H):
        """The new row qkv [rows, 3C] over layer l's int8 cache at column t (an int, or one
        int32 on the device): gvl_attn_decode_q8 appends and attends."""
        kv8, kvs = self.cache[l]
        return K.attn_decode_q8(qkv, kv8, kvs, t, H, src=self.src, gap_lo=self.gap_lo,
                                gap_hi=self.gap_hi)

    def _mlp(self, x2, P):
        h = self._linear(self._ln(x2, P["ln2"]), P["fc"], act=1)
        return self._linear(h, P["mproj"], residual=x2)

    def _logits(self, x2):
        xf = self._ln(x2, self.lnf)
        if self.qdec is not None:  # padded to a multiple of 8 rows when it was quantised
            lg, V = self._linear(xf, (self.qdec.head, None)), self.qdec.head.rows
            return lg if lg.shape[1] == V else lg[:, :V]
        wp, V = Fn.pad_vocab(self.head)
        lg = self._linear(xf, (wp, None))
        return lg if wp is self.head else lg[:, :V]

    # ------------------------------------------------------------------ API
    @torch.no_grad()
    def prefill(self, x_emb, lens=None):
        """x_emb [B, S, C]: the whole prefix (image tokens + prompt embeddings).  Returns the
        logits of the last position [B, V].  lens (int64 CPU [B], from check_prompt_lens): the
        real text length of every right-padded row; the logits are then those of each row's last
        real position, and the steps skip the row's pad columns."""
        B, S, C = x_emb.shape
        self.gap_lo = self.pos = None
        if lens is not None:
            dl = lens.to(x_emb.device)
            self.gap_lo = (dl + self.txt0).to(torch.int32)
            self.gap_hi = S
            self.pos = dl.to(torch.int32)
            self.max_len = int(lens.max())
        self.Tmax = S + self.max_new + self.slack
        self.cache = self._alloc_cache(B, C, x_emb.device)
        x2 = x_emb.to(BF16).reshape(B * S, C).contiguous()
        self._dq = self.qdec is not None
        try:
            for l, P in enumerate(self.blocks):
                if self.cross is not None:
                    x2 = self._cross(l, x2, S)
                qkv = self._linear(self._ln(x2, P["ln1"]), P["attn"])
                q3 = qkv.view(B, S, 3 * C)
                if self.kv8:
                    K.kv_quantize_i8(q3, *self.cache[l], P["H"])
                else:
                    self.cache[l][:, :S].copy_(q3)
                y = K.attn_fwd(q3[:, :, :C], q3[:, :, C:2 * C], q3[:, :, 2 * C:], P["H"], True)[0]
                x2 = self._linear(y.view(B * S, C), P["aproj"], residual=x2)
                x2 = self._mlp(x2, P)
        finally:
            self._dq = False
        self.t = S
        if self.gap_lo is None:
            last = x2.view(B, S, C)[:, S - 1].contiguous()
        else:  # row b's last real row: b*S + gap_lo[b] - 1
            rows = torch.arange(B, device=x2.device) * S + (self.gap_lo.long() - 1)
            last = x2.index_select(0, rows)
        return self._logits(last)

    @torch.no_grad()
    def step(self, ids):
        """Append one token per sequence (ids [B]) and return the next logits [B, V]."""
        B, C, t = self.rows, self.C, self.t
        if t >= self.Tmax:
            raise ValueError("KV cache full")
        ragged = self.gap_lo is not None
        # the furthest position of this step: the longest prompt's when the rows differ
        pos = self.max_len + t - self.gap_hi if ragged else t - self.txt0
        if pos >= self.wpe.shape[0]:
            raise ValueError(f"position {pos} exceeds block_size {self.wpe.shape[0]}")
        Fn.check_index_range(ids, self.wte.shape[0], "token id")
        x = torch.empty(B, 1, C, dtype=BF16, device=ids.device)
        if ragged:
            K.embedding_fwd_pos(ids.view(B), self.pos, self.wte, self.wpe, x)
            self.pos += 1
        else:
            K.embedding_fwd(ids.view(B, 1), self.wte, self.wpe[pos:pos + 1], x, 1, 1, 0)
        x2 = x.view(B, C)
        for l, P in enumerate(self.blocks):
            if self.cross is not None:
                x2 = self._cross(l, x2, 1)
            if self.kv8:
                qkv = self._linear(self._ln(x2, P["ln1"]), P["attn"])
                y = self._attend_q8(qkv, l, t, P["H"])
            else:
                row = self.cache[l][:, t]  # [B, 3C] view, row stride Tmax*3C
                self._linear(self._ln(x2, P["ln1"]), P["attn"], out=row)
                cl = self.cache[l][:, :t + 1]
                y = self._attend(row[:, :C], cl[:, :, C:2 * C], cl[:, :, 2 * C:], P["H"], False)
            x2 = self._linear(y, P["aproj"], residual=x2)
            x2 = self._mlp(x2, P)
        self.t = t + 1
        return self._logits(x2)

    @torch.no_grad()
    def step_multi(self, ids, kv_len, pos):
        """Append Q tokens per sequence at per-sequence cache lengths (ids [B, Q], 1 <= Q <= 8;
        kv_len, pos int32 [B] on the device, owned by the caller) and return the logits of all of
        them [B*Q, V], row b*Q + j following token j of sequence b.  Token j of sequence b goes
        to cache column kv_len[b] + j and takes position min(pos[b] + j, block_size - 1); the
        caller keeps kv_len[b] + Q <= Tmax (KVDecoder.slack = Q before start()) and decides
        afterwards how many of the Q columns count (gvl_spec_accept): the next call overwrites
        the rest.  After start(prompt_ids, z, prompt_lens) sequence r begins at
        kv_len = txt0 + len_r and pos = len_r (its new tokens overwrite its pad columns; gap_lo,
        gap_hi and self.t go unused on this path)."""
        if self.kv8:
            raise ValueError("kv_cache='int8' is not supported by step_multi / speculative "
                             "decoding: its queries read each other's un-appended keys")
        B, C = self.rows, self.C
        Q = ids.shape[1]
        if ids.shape[0] != B or not 1 <= Q <= 8:
            raise ValueError(f"step_multi takes ids [{B}, 1..8] (got {tuple(ids.shape)})")
        if Q > self.Tmax:
            raise ValueError("KV cache full")
        Fn.check_index_range(ids, self.wte.shape[0], "token id")
        at = pos.view(B, 1) + torch.arange(Q, dtype=torch.int32, device=ids.device)
        at = at.clamp_(max=self.block_size - 1).reshape(B * Q)
        x2 = K.embedding_fwd_pos(ids.reshape(B * Q), at, self.wte, self.wpe)
        kv_src = None
        if self.cross is not None:  # row b*Q + j reads the projected image tokens of sequence b
            seq = torch.arange(B * Q, dtype=torch.int32, device=ids.device) // Q
            kv_src = seq.view(-1, 1).expand(B * Q, self.kvz[0].shape[1]).contiguous()
        for l, P in enumerate(self.blocks):
            if self.cross is not None:
                x2 = self._cross(l, x2, Q, kv_src)
            qkv = self._linear(self._ln(x2, P["ln1"]), P["attn"])
            y = K.attn_decode_multi(qkv.view(B, Q, 3 * C), self.cache[l], kv_len, P["H"])
            x2 = self._linear(y, P["aproj"], residual=x2)
            x2 = self._mlp(x2, P)
        return self._logits(x2)

    # ------------------------------------------------------- model-specific prefixes
    @torch.no_grad()
    def start(self, prompt_ids, z=None, prompt_lens=None):
        """Prefill for the model kind: text-only (GPT), [bridge(z) | text] (caption), or text
        with the cached cross-attention keys/values of z (cross-att).  Returns logits [B, V].
        prompt_lens: the real lengths of the right-padded rows of prompt_ids (the pad entries
        must be valid ids; no output depends on them)."""
        m = self.model
        self.kvz = None
        lens = None
        if prompt_lens is not None:
            lens = check_prompt_lens(prompt_ids, prompt_lens, self.max_new, self.block_size)
        if self.kind == "caption":
            pt = z.unsqueeze(1) if z.dim() == 2 else z
            if m.use_cls_only:
                pt = pt[:, 0:1, :]
            img = m.bridge(pt).to(BF16)
            M = img.shape[1]
            emb = Fn.EmbedFn.apply(prompt_ids, self.wte, self.wpe, img)
            self.txt0 = M
            return self.prefill(emb, lens)
        if self.kind == "cross" and z is not None:
            zp = m.transformer.vis_proj(z).to(BF16)
            Sz = zp.shape[1]
            z2 = zp.reshape(-1, self.C).contiguous()
            self.kvz = [K.linear(z2, *P["kv"]).view(self.B, Sz, 2 * self.C) for P in self.cross]
        elif self.kind == "cross":
            self.cross = None  # z=None: the gated cross-attention is skipped (model.py:159-165)
        self.txt0 = 0
        emb = Fn.EmbedFn.apply(prompt_ids, self.wte, self.wpe, None)
        return self.prefill(emb, lens)


class BeamDecoder(KVDecoder):
    """KVDecoder for beam search: B items x K beams = R cache rows, and an int32 table
    src [R, Tmax] naming, per hypothesis and position, the cache row that holds its key / value.

    The prefix is prefilled once per item, at batch B, into cache rows b*K (src[:, :t0] = b*K);
    step(ids, src) appends one token per hypothesis into the hypothesis' own row and attends
    through src (gvl_attn_decode_beam), so reordering beams rewrites the table, never the cache.
    The cross-att model's kv_proj(z_proj) stays at B rows, read through a constant table.
    cache_fill: a value to fill the new cache with (a test hook: rows the prefill must not
    write keep it)."""

    def __init__(self, model, batch: int, beams: int, max_new: int, cache_fill=None,
                 weights=None, kv_cache=None):
        super().__init__(model, batch, max_new, weights=weights, kv_cache=kv_cache)
        if not 1 <= beams <= 8:
            raise ValueError(f"beams={beams}: 1..8 supported")
        self.K = beams
        self.rows = batch * beams
        self.cache_fill = cache_fill
        self.prefill_batch = None
        self.src = None
        self.kv_src = None

    def _alloc_cache(self, B, C, device):
        self._full = self._new_cache(B * self.K, C, device, self.cache_fill)
        rows_bk = lambda c: c.view(B, self.K, self.Tmax, c.shape[2])[:, 0]  # rows b*K
        if self.kv8:
            return [(rows_bk(c8), rows_bk(cs)) for c8, cs in self._full]
        return [rows_bk(c) for c in self._full]

    def _attend(self, q, k, v, H, cross):
        if self.src is None:  # a one-token prefill of the cross-att model: B plain rows
            return super()._attend(q, k, v, H, cross)
        if cross:
            return K.attn_decode_beam(q, k, v, H, self.kv_src)
        if self.gap_lo is not None:
            return K.attn_decode_ragged(q, k, v, H, self.gap_lo, self.gap_hi, src=self.src)
        return K.attn_decode_beam(q, k, v, H, self.src)

    @torch.no_grad()
    def prefill(self, x_emb, lens=None):
        self.prefill_batch = x_emb.shape[0]
        logits = super().prefill(x_emb, lens)
        self.cache, self._full = self._full, None  # step() sees all R rows
        if self.gap_lo is not None:  # per hypothesis: those of its item
            self.gap_lo = self.gap_lo.repeat_interleave(self.K)
            self.pos = self.pos.repeat_interleave(self.K)
        return logits

    @torch.no_grad()
    def start(self, prompt_ids, z=None, prompt_lens=None):
        """Prefill at batch B.  Returns the items' logits [B, V] (those of slot 0 of each)."""
        logits = super().start(prompt_ids, z, prompt_lens)
        if self.kvz is not None:
            Sz = self.kvz[0].shape[1]
            item = torch.arange(self.rows, device=logits.device, dtype=torch.int32) // self.K
            self.kv_src = item.view(-1, 1).expand(self.rows, Sz).contiguous()
        return logits

    def initial_src(self, device):
        """src [R, Tmax] with the prefix columns pointing at the items' prefilled rows b*K."""
        src = torch.zeros(self.rows, self.Tmax, dtype=torch.int32, device=device)
        first = torch.arange(self.rows, device=device, dtype=torch.int32) // self.K * self.K
        src[:, :self.t] = first.view(-1, 1)
        return src

    @torch.no_grad()
    def step(self, ids, src):
        """Append one token per hypothesis (ids [R]) whose cached positions are src[r, :t]
        (src[r, t] = r: the new token lands in its own row).  Returns the next logits [R, V]."""
        self.src = src
        try:
            return super().step(ids)
        finally:
            self.src = None


def sample_next(logits, *, greedy=False, temperature=1.0, top_k=0, top_p=1.0, generator=None,
                out=None):
    """Next token ids [B] from logits [B, V] on the gvl_sample kernel (into `out` if given)."""
    rows = logits.shape[0]
    if greedy:
        u = torch.zeros(rows, dtype=torch.float32, device=logits.device)
        return K.sample(logits, u, 1.0, 1, 1.0, out=out)
    u = torch.rand(rows, generator=generator, device=logits.device, dtype=torch.float32)
    return K.sample(logits, u, temperature, top_k, top_p, out=out)


class _Controls:
    """The logits processors of generate / beam_search (gvl_logits_process): what is on, the
    prompt as part of the penalised sequence (with prompt_lens: each row's real tokens, moved up
    against the generated ones by ragged_prompt_for_controls), the bad-token list uploaded once."""

    def __init__(self, prompt_ids, repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos,
                 bad_tokens, penalize_prompt, prompt_lens=None):
        # prompt_lens: None or the checked lengths (check_prompt_lens)
        self.pen = float(repetition_penalty)
        self.ngram = int(no_repeat_ngram_size)
        self.eos = eos
        self.min_new = int(min_new_tokens) if eos is not None else 0
        self.bad = None
        if bad_tokens is not None and len(bad_tokens) > 0:
            self.bad = torch.as_tensor(bad_tokens).to(device=prompt_ids.device,
                                                      dtype=torch.int32).contiguous()
        self.always = self.pen != 1.0 or self.ngram != 0 or self.bad is not None
        self.prompt = None
        if penalize_prompt and (self.pen != 1.0 or self.ngram != 0):
            if prompt_lens is None:
                self.prompt = prompt_ids.to(torch.int64).contiguous()
            else:
                self.prompt = ragged_prompt_for_controls(prompt_ids, prompt_lens)

    def apply(self, logits, hist, step, **kw):
        ban_eos = step < self.min_new
        if self.always or ban_eos:
            K.logits_process(logits, hist, step, prompt=self.prompt,
                             repetition_penalty=self.pen, no_repeat_ngram_size=self.ngram,
                             eos=self.eos, ban_eos=ban_eos, bad_tokens=self.bad, **kw)


@torch.no_grad()
def generate(model, prompt_ids, n_new, *, z=None, greedy=False, temperature=1.0, top_k=0,
             top_p=1.0, generator=None, return_logits=False, eos=None, return_lengths=False,
             repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, bad_tokens=None,
             penalize_prompt=True, prompt_lens=None, graph=False, weights=None, kv_cache=None):
    """KV-cached decode of n_new tokens after prompt_ids [B, P].  greedy: argmax (first max);
    else temperature / top-k / top-p sampling with `generator` (a CUDA torch.Generator).

    prompt_lens (B integers: a list or a tensor): prompt_ids is right-padded and row r's prompt
    is prompt_ids[r, :prompt_lens[r]], 1 <= prompt_lens[r] <= P.  Row r then decodes as if it had
    been called alone with that prompt, the penalised sequence included; the pad entries must be
    valid ids and no output depends on them.  max(prompt_lens) + n_new - 1 <= block_size.

    Before the token choice (and before temperature / top-k / top-p, Hugging Face's order) each
    step's logits pass gvl_logits_process: repetition_penalty (Hugging Face's rule, once per
    distinct token), no_repeat_ngram_size, bad_tokens (a list or int tensor of banned ids) and,
    for the first min_new_tokens steps, a ban of `eos`.  penalize_prompt: the prompt ids count as
    part of the sequence the penalty and the n-gram rule look at.  With the defaults no such
    kernel runs.  eos: a row that draws it is done, its later tokens are eos, and the loop ends
    once every row is done (one host read per step, only when eos is given).

    Returns the new ids [B, n_new], then if asked the per-step logits [B, steps that ran, V] as
    the decoder gave them (before the processors), then if asked lengths [B] int32: the count of
    tokens up to and including eos, n_new for a row that never ended.

    graph: replay every token after the first as one captured graph (a GraphedGenerate built for
    this call and closed after it: same results; its docstring says what differs for the
    generator).

    weights: None decodes in bf16 as ever; "int8" quantises the model's block matrices and
    lm_head (gvl.quant) for this call and runs every linear of it on them (the steps on
    gvl_linear_w8, the prefill on the dequantised matrices); a gvl.quant.quantize_decoder(model)
    result does the same without quantising again.

    kv_cache: None keeps the bf16 cache; "int8" stores every layer's keys and values as int8 with
    one fp32 scale per head vector and position (0.354 of the bytes), and every step's attention
    then sees fp32(q8) * scale for every position, its own included (the module docstring)."""
    quant.check_weights(weights)
    check_kv_cache(kv_cache)
    if graph:
        with GraphedGenerate(model, prompt_ids.shape[1], n_new, greedy=greedy,
                             temperature=temperature, top_k=top_k, top_p=top_p, eos=eos,
                             repetition_penalty=repetition_penalty,
                             no_repeat_ngram_size=no_repeat_ngram_size,
                             min_new_tokens=min_new_tokens, bad_tokens=bad_tokens,
                             penalize_prompt=penalize_prompt, return_logits=return_logits,
                             weights=weights, kv_cache=kv_cache) as ses:
            return ses(prompt_ids, n_new, z=z, prompt_lens=prompt_lens, generator=generator,
                       return_lengths=return_lengths)
    B = prompt_ids.shape[0]
    dec = KVDecoder(model, B, n_new, weights=weights, kv_cache=kv_cache)
    lens = None
    if prompt_lens is not None:
        lens = check_prompt_lens(prompt_ids, prompt_lens, n_new, dec.block_size)
    logits = dec.start(prompt_ids, z, lens)
    dev = logits.device
    ctl = _Controls(prompt_ids, repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos,
                    bad_tokens, penalize_prompt, lens)
    hist = torch.empty(n_new, B, dtype=torch.int64, device=dev)
    lengths = torch.full((B,), n_new, dtype=torch.int32, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    lg, steps = [], n_new
    for i in range(n_new):
        if return_logits:
            lg.append(logits.to(torch.float32, copy=True))
        ctl.apply(logits, hist, i)
        nxt = sample_next(logits, greedy=greedy, temperature=temperature, top_k=top_k,
                          top_p=top_p, generator=generator, out=hist[i])
        if eos is not None:
            nxt.copy_(torch.where(done, eos, nxt))
            ended = (nxt == eos) & ~done
            lengths = torch.where(ended, i + 1, lengths).to(torch.int32)
            done |= ended
            if bool(done.all()):
                steps = i + 1
                break
        if i + 1 < n_new:
            logits = dec.step(nxt)
    if steps < n_new:
        hist[steps:] = eos
    out = [hist.t().contiguous()]
    if return_logits:
        out.append(torch.stack(lg, dim=1))
    if return_lengths:
        out.append(lengths)
    return out[0] if len(out) == 1 else tuple(out)


@torch.no_grad()
def speculative_generate(model, prompt_ids, n_new, *, z=None, draft_len=4, ngram=3,
                         draft_ids=None, greedy=False, temperature=1.0, top_k=0, top_p=1.0,
                         generator=None, eos=None, prompt_lens=None, return_lengths=False,
                         return_stats=False, weights=None, kv_cache=None):
    """generate() with several tokens per decoder pass: draft draft_len (1..7) tokens per row,
    feed [last token, draft] through KVDecoder.step_multi, choose a token from every one of the
    B * (draft_len + 1) logits rows with gvl_sample and keep, per row, the drafted tokens the
    chosen ones confirm plus the first chosen token that differs (gvl_spec_accept).

    The draft is the continuation of the most recent earlier occurrence of the row's last
    `ngram` (1..4) tokens in its prompt + output, falling back to shorter suffixes
    (gvl_ngram_draft); draft_ids int [B, n_new] overrides it where >= 0: draft_ids[b, i] is the
    guess for new token i of row b.  A guess of -1 is fed as id 0 and never accepted.

    The draft is deterministic, so draw-and-compare is exact: new token i of row b is drawn with
    u[i, b] from the logits that follow the accepted tokens, whatever was drafted.  u is n_new
    successive torch.rand(B, generator=...) made up front, the uniforms generate() consumes: with
    the same seed both aim at the same tokens (they differ only where the bf16 logits of a
    B * (draft_len + 1)-row pass and of a B-row pass round a choice differently).  greedy:
    top_k = 1, u = 0.  eos, prompt_lens, return_lengths: as in generate().  No logits
    processors, return_logits or beams here.

    One host read per round (n.min(), to stop once every row is done).  Returns ids
    [B, n_new], then if asked lengths [B] int32, then if asked stats: dict(steps = rounds of
    token choice: one on the prefill's logits, then one per decoder pass (passes = steps - 1),
    drafted / accepted = int32 [B]: guesses made, and guesses that reached the output).

    weights: as in generate().  kv_cache: None only; "int8" is refused (the queries of a pass
    read each other's un-appended keys, which the int8 cache's attention does not serve)."""
    quant.check_weights(weights)
    if check_kv_cache(kv_cache) is not None:
        raise ValueError("kv_cache='int8' is not supported by speculative_generate")
    if prompt_ids.dim() != 2 or prompt_ids.shape[0] < 1 or prompt_ids.shape[1] < 1:
        raise ValueError("prompt_ids must be [B, P] with B, P >= 1")
    B, P = prompt_ids.shape
    n_new, draft_len, ngram = int(n_new), int(draft_len), int(ngram)
    if n_new < 1:
        raise ValueError(f"n_new={n_new}: at least 1")
    if not 1 <= draft_len <= 7:
        raise ValueError(f"draft_len={draft_len}: 1..7 supported")
    if not 1 <= ngram <= 4:
        raise ValueError(f"ngram={ngram}: 1..4 supported")
    if not greedy and not (temperature > 0 and 0 < top_p <= 1 and top_k >= 0):
        raise ValueError("temperature > 0, 0 < top_p <= 1 and top_k >= 0 required")
    if draft_ids is not None:
        draft_ids = torch.as_tensor(draft_ids)
        if (tuple(draft_ids.shape) != (B, n_new) or draft_ids.is_floating_point() or
                draft_ids.is_complex() or draft_ids.dtype == torch.bool):
            raise ValueError(f"draft_ids must be integers [B, n_new] = [{B}, {n_new}] "
                             f"(got {draft_ids.dtype} {tuple(draft_ids.shape)})")
    Q = draft_len + 1
    dec = KVDecoder(model, B, n_new, weights=weights)
    dec.slack = Q
    if prompt_lens is not None:
        lens = check_prompt_lens(prompt_ids, prompt_lens, n_new, dec.block_size)
    else:
        lens = None
        if P + n_new - 1 > dec.block_size:
            raise ValueError(f"a prompt of {P} tokens + {n_new} new tokens exceeds block_size "
                             f"{dec.block_size}")
    if P + n_new > 4096:
        raise ValueError(f"prompt + new tokens = {P + n_new} exceeds 4096")
    logits = dec.start(prompt_ids, z, lens)
    dev = logits.device
    if dec.t + n_new + Q > 4096:
        raise ValueError(f"prefix {dec.t} + {n_new} new tokens + {Q} exceeds 4096 cache columns")
    i32 = dict(dtype=torch.int32, device=dev)
    if greedy:
        temperature, top_k, top_p = 1.0, 1, 1.0
        u = torch.zeros(B, n_new, dtype=torch.float32, device=dev)
    else:
        u = torch.stack([torch.rand(B, generator=generator, device=dev, dtype=torch.float32)
                         for _ in range(n_new)], dim=1)  # u[b, i]: row b's new token i
    prompt = prompt_ids.to(device=dev, dtype=torch.int64).contiguous()
    given = None if draft_ids is None else draft_ids.to(device=dev, dtype=torch.int64).contiguous()
    plen = torch.full((B,), P, **i32) if lens is None else lens.to(**i32)
    # The first round takes the prefill's logits as a pass of one row: it moves the state by one
    # like any accepted token, so it starts one short of where start() left each row.
    kv_len = plen + (dec.txt0 - 1)
    pos = plen - 1
    n = torch.zeros(B, **i32)
    lengths = torch.full((B,), n_new, **i32)
    drafted, accepted = torch.zeros(B, **i32), torch.zeros(B, **i32)
    last = torch.zeros(B, dtype=torch.int64, device=dev)
    out = torch.zeros(B, n_new, dtype=torch.int64, device=dev)
    x = K.sample(logits, u[:, 0].contiguous(), temperature, top_k, top_p)
    K.spec_accept(x.view(B, 1), None, n, kv_len, pos, lengths, last, out, eos)
    steps = 1
    slot = torch.arange(Q, device=dev)
    while int(n.min()) < n_new:
        draft = K.ngram_draft(prompt, plen, out, n, ngram, draft_len, given=given)
        ids = torch.cat([last.view(B, 1), draft.clamp(min=0)], dim=1)
        logits = dec.step_multi(ids, kv_len, pos)
        uq = u.gather(1, (n.long().view(B, 1) + slot).clamp_(max=n_new - 1))
        x = K.sample(logits, uq.reshape(B * Q), temperature, top_k, top_p)
        K.spec_accept(x.view(B, Q), draft, n, kv_len, pos, lengths, last, out, eos, drafted,
                      accepted)
        steps += 1
    res = [out]
    if return_lengths:
        res.append(lengths)
    if return_stats:
        res.append(dict(steps=steps, passes=steps - 1, drafted=drafted, accepted=accepted))
    return res[0] if len(res) == 1 else tuple(res)


@torch.no_grad()
def beam_search(model, prompt_ids, n_new, *, z=None, num_beams=4, eos=50256, length_penalty=1.0,
                return_all=False, repetition_penalty=1.0, no_repeat_ngram_size=0,
                min_new_tokens=0, bad_tokens=None, penalize_prompt=True, prompt_lens=None,
                graph=False, weights=None, kv_cache=None):
    """KV-cached beam search of up to n_new tokens after prompt_ids [B, P] with num_beams (<= 8)
    hypotheses per item (prompt_lens: right-padded prompts of different lengths, as in
    generate()).  A hypothesis' raw score is the sum of the fp32 log-probabilities of its
    tokens; hypotheses are ranked by raw * n ** -length_penalty (n = its length, end token
    included), ties to the lower parent slot and then the lower token id (gvl_beam_step).  One
    that emits `eos` is finished and competes with its final score; the search ends after n_new
    steps or once every hypothesis is finished (eos=None: never).

    repetition_penalty, no_repeat_ngram_size, min_new_tokens (eos banned for that many steps),
    bad_tokens and penalize_prompt act as in generate(), per hypothesis: gvl_logits_process reads
    each live hypothesis' own history through the beam table before every step, and leaves
    finished ones alone.  The log-probabilities summed into a score are then those of the
    *processed* distribution (the softmax of the edited logits), as in Hugging Face.  With the
    defaults no such kernel runs.

    Returns (ids [B, n_new] of the best hypothesis, padded with eos past its end, lengths [B],
    raw scores [B]); return_all: all of them in rank order, [B, K, n_new], [B, K], [B, K].

    graph: replay every step after the first as one captured graph (a GraphedBeamSearch built
    for this call and closed after it: same results).

    weights, kv_cache: as in generate()."""
    quant.check_weights(weights)
    check_kv_cache(kv_cache)
    if graph:
        with GraphedBeamSearch(model, prompt_ids.shape[1], n_new, num_beams=num_beams, eos=eos,
                               length_penalty=length_penalty,
                               repetition_penalty=repetition_penalty,
                               no_repeat_ngram_size=no_repeat_ngram_size,
                               min_new_tokens=min_new_tokens, bad_tokens=bad_tokens,
                               penalize_prompt=penalize_prompt, weights=weights,
                               kv_cache=kv_cache) as ses:
            return ses(prompt_ids, n_new, z=z, prompt_lens=prompt_lens, return_all=return_all)
    B, Kb = prompt_ids.shape[0], num_beams
    R = B * Kb
    dec = BeamDecoder(model, B, Kb, n_new, weights=weights, kv_cache=kv_cache)
    lens = None
    if prompt_lens is not None:
        lens = check_prompt_lens(prompt_ids, prompt_lens, n_new, dec.block_size)
    first = dec.start(prompt_ids, z, lens)
    dev, V, t0 = first.device, first.shape[1], dec.t
    ctl = _Controls(prompt_ids, repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos,
                    bad_tokens, penalize_prompt, lens)
    logits = torch.empty(R, V, dtype=first.dtype, device=dev)
    logits.view(B, Kb, V)[:, 0] = first  # slots 1.. start empty (score -inf): never read
    len_norm = torch.arange(n_new + 2, dtype=torch.float32).clamp_(min=1.0).pow_(
        -float(length_penalty)).to(dev)
    score = torch.full((B, Kb), float("-inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0
    score = [score.view(R), torch.empty(R, dtype=torch.float32, device=dev)]
    flen = [torch.zeros(R, dtype=torch.int32, device=dev) for _ in range(2)]
    src = [dec.initial_src(dev), torch.zeros(R, dec.Tmax, dtype=torch.int32, device=dev)]
    parent = torch.empty(R, dtype=torch.int32, device=dev)
    nws = K._L().gvl_beam_step_workspace_size(B, Kb)
    ws = torch.empty(max(nws, 8) // 4, dtype=torch.float32, device=dev)
    hist = torch.empty(n_new, R, dtype=torch.int64, device=dev)  # step-major: hist[s] = tok_out
    S, cur = 0, 0
    for s in range(n_new):
        tok = hist[s]
        ctl.apply(logits, hist, s, src=src[cur], t0=t0, rows_per_item=Kb, flen=flen[cur])
        K.beam_step(logits, score[cur], flen[cur], len_norm, src[cur], Kb, s, eos, t0,
                    out=(tok, parent, score[1 - cur], flen[1 - cur], src[1 - cur]), workspace=ws)
        cur = 1 - cur
        S = s + 1
        if s + 1 == n_new:
            break
        # finished hypotheses only carry over, in their order: stopping here or later is the same
        if eos is not None and bool(((flen[cur] > 0) | (score[cur] == float("-inf"))).all()):
            break
        logits = dec.step(tok, src[cur])
    ids = hist[:S].t().gather(0, src[cur][:, t0:t0 + S].long())
    if S < n_new:
        ids = torch.cat([ids, ids.new_full((R, n_new - S), eos)], dim=1)
    live = torch.where(score[cur] == float("-inf"), 0, S).to(torch.int32)
    lengths = torch.where(flen[cur] > 0, flen[cur], live)
    ids, lengths, scores = ids.view(B, Kb, n_new), lengths.view(B, Kb), score[cur].view(B, Kb)
    if return_all:
        return ids, lengths, scores.clone()
    return ids[:, 0], lengths[:, 0], scores[:, 0].clone()


# ------------------------------------------------------------------ graph-replayed decoding
def _release_graphs(graphs, state, dev):
    """Finalizer / close() of a session: drain the device, reset the captured graphs (the
    private memory pool goes with the last reset) and drop the static buffers."""
    try:
        if torch.cuda.is_initialized():
            torch.cuda.synchronize(dev)
    finally:
        for g in graphs:
            g.reset()
        graphs.clear()
        state.clear()


class _Static:
    """KVDecoder / BeamDecoder mixin for a session that replays one token's work as a graph:
    every tensor a step touches keeps its address from call to call, and what step() takes from
    the host each token (the cache column, the positions) is read on the device.

      * the cache is allocated once with Tmax = image tokens + max_prompt + max_new; every
        start() prefills into it (columns past a call's own are never read);
      * what start() makes anew per call (gap_lo, pos, the cross-att model's kvz and kv_src) is
        copied into the first call's tensors, which the captured launches name;
      * lm_head is padded to a multiple of 8 rows once, not per token;
      * step_dev() is step() at the column *t and the positions pos[], both on the device.
    A session always starts with prompt_lens (all P when the caller gave none): an empty gap has
    the bits of the instance without one, and gvl_embedding_fwd_pos those of gvl_embedding_fwd."""

    _static = None

    def _init_static(self, max_prompt, cap_new):
        self.max_prompt, self.cap_new = int(max_prompt), int(cap_new)
        self._pinned = {}
        self.head_p = Fn.pad_vocab(self.head)[0]

    def _alloc_cache(self, B, C, device):
        self.Tmax = self.txt0 + self.max_prompt + self.cap_new
        if self.Tmax > 4096:
            raise ValueError(f"image tokens + max_prompt + max_new = {self.Tmax} exceeds 4096 "
                             "cache columns")
        if self._static is None:
            views = super()._alloc_cache(B, C, device)
            self._static = (views, getattr(self, "_full", None))
        views, self._full = self._static
        return views

    def _logits(self, x2):
        if self.qdec is not None:
            return super()._logits(x2)
        lg = self._linear(self._ln(x2, self.lnf), (self.head_p, None))
        V = self.head.shape[0]
        return lg if self.head_p is self.head else lg[:, :V]

    def _pin(self, name):
        cur = getattr(self, name)
        if cur is None:
            return
        first = self._pinned.setdefault(name, cur)
        if first is not cur:
            for dst, src in zip(*(x if isinstance(x, list) else [x] for x in (first, cur))):
                dst.copy_(src)
            setattr(self, name, first)

    @torch.no_grad()
    def start(self, prompt_ids, z=None, prompt_lens=None):
        self.src = None  # (BeamDecoder: the prefill attends plain rows)
        logits = super().start(prompt_ids, z, prompt_lens)
        for name in ("gap_lo", "pos", "kvz", "kv_src"):
            if hasattr(self, name):
                self._pin(name)
        return logits

    @torch.no_grad()
    def step_dev(self, ids, t):
        """step(ids) with the cache column read from t (one int32 on the device) and the
        positions from self.pos; neither is advanced here.  self.src (BeamDecoder): the table of
        this step.  No host read and no host-side state: safe to capture."""
        x2 = K.embedding_fwd_pos(ids, self.pos, self.wte, self.wpe)
        for l, P in enumerate(self.blocks):
            if self.cross is not None:
                x2 = self._cross(l, x2, 1)
            qkv = self._linear(self._ln(x2, P["ln1"]), P["attn"])
            if self.kv8:
                y = self._attend_q8(qkv, l, t, P["H"])
            else:
                y = K.attn_decode_step(qkv, self.cache[l], t, P["H"], src=self.src,
                                       gap_lo=self.gap_lo, gap_hi=self.gap_hi)
            x2 = self._linear(y, P["aproj"], residual=x2)
            x2 = self._mlp(x2, P)
        return self._logits(x2)


class _StaticKV(_Static, KVDecoder):
    pass


class _StaticBeam(_Static, BeamDecoder):
    pass


class _GraphedSession:
    """What GraphedGenerate and GraphedBeamSearch share: the decoder with static buffers, the
    device counters, capture on first use, the replay loop and teardown.

    Per token the host used to pass the cache column t, Tk = t + 1, n_hist / ban_eos and the
    beam step; here they are three device scalars (t, step, and step as the int64 index torch's
    indexing ops take) that the graph advances itself, next to the rows' positions.  Frozen at
    capture: every address, the batch, the image-token shape, every control and sampling
    setting, and the prefix length S = image tokens + P where a launch takes it from the host
    (the gap end of prompts of different lengths; the beam table's t0): a call whose S needs
    another value captures its own graph over the same buffers (stats["captures"])."""

    def __init__(self, model, max_prompt, max_new, poll_every, weights=None, kv_cache=None):
        quant.check_weights(weights)
        self.kv_cache = check_kv_cache(kv_cache)
        self.max_prompt, self.max_new = int(max_prompt), int(max_new)
        self.poll_every = int(poll_every)
        if self.max_prompt < 1 or self.max_new < 1 or self.poll_every < 1:
            raise ValueError("max_prompt, max_new and poll_every must be at least 1")
        self.model = model
        # quantised once per session ("int8"), or the caller's snapshot; None: bf16
        self.weights = quant.resolve_weights(model, weights)
        self.stats = dict(captures=0, replays=0)
        self.dec = None
        self._key = None
        self._graphs, self._all, self._st = {}, [], {}
        dev = next(model.parameters()).device
        self._finalizer = weakref.finalize(self, _release_graphs, self._all, self._st, dev)

    @property
    def closed(self) -> bool:
        return not self._finalizer.alive

    def close(self):
        """Drain the device, reset the captured graphs and drop the buffers (idempotent).  A
        call after close() raises."""
        if self.closed:
            return
        self._finalizer()
        self._graphs, self.dec = {}, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check_call(self, prompt_ids, n_new, z, prompt_lens):
        """Everything that can refuse a call, before any launch.  -> (n_new, lens)."""
        if self.closed:
            raise RuntimeError(f"{type(self).__name__}.__call__ after close()")
        if prompt_ids.dim() != 2 or prompt_ids.shape[0] < 1 or prompt_ids.shape[1] < 1:
            raise ValueError("prompt_ids must be [B, P] with B, P >= 1")
        B, P = prompt_ids.shape
        n_new = self.max_new if n_new is None else int(n_new)
        if P > self.max_prompt:
            raise ValueError(f"a prompt of P = {P} tokens exceeds max_prompt = {self.max_prompt}")
        if not 1 <= n_new <= self.max_new:
            raise ValueError(f"n_new = {n_new} outside 1..max_new = {self.max_new}")
        key = (B, None if z is None else tuple(z.shape))
        if self._key is not None and key != self._key:
            raise ValueError(f"batch / image-token shape {key} differs from the captured "
                             f"{self._key}")
        block = (self.model.gpt if hasattr(self.model, "gpt") else self.model).config.block_size
        if prompt_lens is None:
            if P + n_new - 1 > block:
                raise ValueError(f"a prompt of {P} tokens + {n_new} new tokens exceeds block_size "
                                 f"{block}")
            lens = torch.full((B,), P, dtype=torch.int64)
        else:
            lens = check_prompt_lens(prompt_ids, prompt_lens, n_new, block)
        self._key = key
        return n_new, lens

    def _counters(self, dev):
        st = self._st
        st["t"] = torch.zeros(1, dtype=torch.int32, device=dev)
        st["step"] = torch.zeros(1, dtype=torch.int32, device=dev)
        st["step64"] = torch.zeros(1, dtype=torch.int64, device=dev)

    def _token(self):
        """One token for all rows: the decoder pass on the tokens chosen last, then the choice."""
        st, dec = self._st, self.dec
        logits = dec.step_dev(st["last"], st["t"])
        st["t"].add_(1)
        dec.pos.add_(1)
        self._choose(logits)

    def _graph_for(self, S):
        """The graph whose frozen prefix length serves S, captured now if there is none: a
        warm-up token on a side stream (allocator and kernel caches warm), the state it moved
        put back, then the capture (which runs nothing)."""
        g = self._graphs.get(S)
        if g is not None:
            return g
        dev = self._st["t"].device
        K._gemm_workspace(dev)
        K._gemm_tickets(dev)
        moved = [self._st[k] for k in self.RESTORE] + [self.dec.pos]
        saved = [v.clone() for v in moved]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            self._token()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        for v, s in zip(moved, saved):
            v.copy_(s)
        g = torch.cuda.CUDAGraph()
        pool = self._all[0].pool() if self._all else None
        with torch.cuda.graph(g, pool=pool):
            self._token()
        self._all.append(g)
        self._graphs[S] = g
        self.stats["captures"] += 1
        return g

    def _replay(self, g, n, done):
        """Up to n replays; done() (a host read) is asked every poll_every of them."""
        for i in range(1, n + 1):
            g.replay()
            self.stats["replays"] += 1
            if done is not None and i < n and i % self.poll_every == 0 and done():
                break


class GraphedGenerate(_GraphedSession):
    """generate() with every token after the first replayed as one captured graph.

    The prefill runs eagerly into the session's static cache and the first token is chosen on
    its logits; the graph then holds one token for all rows (embed at pos, every block with
    gvl_attn_decode_step, ln_f, lm_head, the logits record, gvl_logits_process_dev, gvl_sample
    on u[step], gvl_spec_accept at Q = 1 for the eos / lengths bookkeeping, the counters) and
    the host only replays it, reading `done` once every poll_every replays when eos is given.
    Finished rows keep emitting eos, so the extra replays change no output.  Results equal
    generate()'s on the same inputs bit for bit.  Sampling draws the n_new uniforms of a call up
    front (the values generate() consumes step by step): the generator ends advanced by n_new
    draws even when eos ended the loop early.

    The first call fixes the batch and the image-token shape; later calls need those,
    P <= max_prompt and n_new <= max_new, else ValueError before any launch.  stats: captures,
    replays.  close() (or the finalizer) resets the graph and drops the buffers."""

    RESTORE = ("t", "step", "step64", "n", "lengths", "last")  # what a warm-up token moves

    def __init__(self, model, max_prompt, max_new, *, greedy=False, temperature=1.0, top_k=0,
                 top_p=1.0, eos=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_new_tokens=0, bad_tokens=None, penalize_prompt=True, return_logits=False,
                 poll_every=8, weights=None, kv_cache=None):
        super().__init__(model, max_prompt, max_new, poll_every, weights, kv_cache)
        if greedy:
            temperature, top_k, top_p = 1.0, 1, 1.0
        self.greedy, self.samp = greedy, (float(temperature), int(top_k), float(top_p))
        self.eos, self.return_logits = eos, return_logits
        self.ctl_args = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos,
                         bad_tokens, penalize_prompt)
        if self.max_prompt + self.max_new > 4096:
            raise ValueError("max_prompt + max_new exceeds 4096")

    def _setup(self, B, V, dev):
        st, cap = self._st, self.max_new
        i32 = dict(dtype=torch.int32, device=dev)
        self._counters(dev)
        st["last"] = torch.zeros(B, dtype=torch.int64, device=dev)
        st["x"] = torch.zeros(B, dtype=torch.int64, device=dev)
        st["n"] = torch.zeros(B, **i32)
        st["lengths"] = torch.zeros(B, **i32)
        st["junk"] = torch.zeros(2, B, **i32)  # gvl_spec_accept's kv_len and pos: unused here
        st["out"] = torch.zeros(B, cap, dtype=torch.int64, device=dev)
        st["u"] = torch.zeros(cap, B, dtype=torch.float32, device=dev)
        st["hist"] = torch.zeros(cap, B, dtype=torch.int64, device=dev)
        if self.return_logits:
            st["lg"] = torch.zeros(B, cap, V, dtype=torch.float32, device=dev)
        # the controls over a prompt buffer of max_prompt columns: a shorter prompt is moved up
        # against the generated tokens behind entries of -1 (ragged_prompt_for_controls)
        ctl = _Controls(torch.zeros(B, self.max_prompt, dtype=torch.int64, device=dev),
                        *self.ctl_args)
        self.ctl = ctl
        self.ctl_on = ctl.always or ctl.min_new > 0
        if ctl.prompt is not None:
            st["prompt"] = ctl.prompt

    def _choose(self, logits):
        st, ctl = self._st, self.ctl
        B = logits.shape[0]
        if self.return_logits:
            st["lg"].index_copy_(1, st["step64"], logits.to(torch.float32).unsqueeze(1))
        if self.ctl_on:
            K.logits_process_dev(logits, st["hist"], st["step"], self.max_new,
                                 prompt=st.get("prompt"), repetition_penalty=ctl.pen,
                                 no_repeat_ngram_size=ctl.ngram, eos=ctl.eos, min_new=ctl.min_new,
                                 bad_tokens=ctl.bad)
        u = st["u"].index_select(0, st["step64"]).view(B)
        K.sample(logits, u, *self.samp, out=st["x"])
        K.spec_accept(st["x"].view(B, 1), None, st["n"], st["junk"][0], st["junk"][1],
                      st["lengths"], st["last"], st["out"], self.eos)
        if self.ctl_on:  # the step's row of the history: eos for a row that is done, as in generate
            st["hist"].index_copy_(0, st["step64"], st["last"].view(1, B))
        st["step"].add_(1)
        st["step64"].add_(1)

    @torch.no_grad()
    def __call__(self, prompt_ids, n_new=None, *, z=None, prompt_lens=None, generator=None,
                 return_lengths=False):
        """-> what generate() returns for these inputs and the session's settings."""
        n_new, lens = self._check_call(prompt_ids, n_new, z, prompt_lens)
        B, P = prompt_ids.shape
        if self.dec is None:
            self.dec = _StaticKV(self.model, B, n_new, weights=self.weights,
                                 kv_cache=self.kv_cache)
            self.dec._init_static(self.max_prompt, self.max_new)
        dec = self.dec
        dec.max_new = n_new
        logits = dec.start(prompt_ids, z, lens)
        dev, st = logits.device, self._st
        if not st:
            self._setup(B, logits.shape[1], dev)
        S = dec.t
        # a call with every row at P tokens needs no gap: any captured gap end serves it
        ragged = prompt_lens is not None
        if not ragged and self._graphs and S not in self._graphs:
            dec.gap_hi = next(iter(self._graphs))
            dec.gap_lo.fill_(dec.gap_hi)
        st["t"].fill_(S)
        st["step"].zero_()
        st["step64"].zero_()
        st["n"].zero_()
        st["lengths"].fill_(n_new)
        if self.greedy:
            st["u"].zero_()
        else:
            for i in range(n_new):
                st["u"][i] = torch.rand(B, generator=generator, device=dev, dtype=torch.float32)
        if "prompt" in st:
            st["prompt"].fill_(-1)
            st["prompt"][:, self.max_prompt - P:] = ragged_prompt_for_controls(prompt_ids, lens)
        self._choose(logits)
        if n_new > 1:
            g = self._graph_for(dec.gap_hi)
            done = None
            if self.eos is not None:
                done = lambda: bool((st["n"] >= self.max_new).all())
            self._replay(g, n_new - 1, done)
        out = [st["out"][:, :n_new].clone()]
        if self.return_logits:
            steps = n_new if self.eos is None else int(st["lengths"].max())
            out.append(st["lg"][:, :steps].clone())
        if return_lengths:
            out.append(st["lengths"].clone())
        return out[0] if len(out) == 1 else tuple(out)


class GraphedBeamSearch(_GraphedSession):
    """beam_search() with every step after the first replayed as one captured graph.

    As GraphedGenerate, with the token choice of beam search: gvl_logits_process_dev through the
    beam table, gvl_beam_step_dev into a second set of score / flen / table buffers, which are
    copied back so that every launch of every step names the same addresses (the results do not
    depend on which buffer a step wrote), and the step's tokens into the history.  With an end
    token the host reads "every hypothesis finished" once every poll_every replays; finished
    hypotheses only carry over, in their order, so the extra steps change no output.  The
    table's t0 is the prefix length: a call with another P captures its own graph."""

    RESTORE = ("t", "step", "step64", "score", "flen", "src", "tok")

    def __init__(self, model, max_prompt, max_new, *, num_beams=4, eos=50256, length_penalty=1.0,
                 repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, bad_tokens=None,
                 penalize_prompt=True, poll_every=8, weights=None, kv_cache=None):
        super().__init__(model, max_prompt, max_new, poll_every, weights, kv_cache)
        if not 1 <= num_beams <= 8:
            raise ValueError(f"beams={num_beams}: 1..8 supported")
        self.Kb, self.eos, self.length_penalty = int(num_beams), eos, float(length_penalty)
        self.ctl_args = (repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos,
                         bad_tokens, penalize_prompt)
        if self.max_prompt + self.max_new > 4096:
            raise ValueError("max_prompt + max_new exceeds 4096")

    def _setup(self, B, V, dtype, dev):
        st, cap, Kb = self._st, self.max_new, self.Kb
        R = B * Kb
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self._counters(dev)
        st["logits0"] = torch.empty(R, V, dtype=dtype, device=dev)
        st["len_norm"] = torch.arange(cap + 2, dtype=torch.float32).clamp_(min=1.0).pow_(
            -self.length_penalty).to(dev)
        st["score"], st["score_o"] = torch.empty(R, **f32), torch.empty(R, **f32)
        st["flen"], st["flen_o"] = torch.zeros(R, **i32), torch.zeros(R, **i32)
        st["src"] = torch.zeros(R, self.dec.Tmax, **i32)
        st["src_o"] = torch.zeros(R, self.dec.Tmax, **i32)
        st["tok"] = torch.zeros(R, dtype=torch.int64, device=dev)
        st["last"] = st["tok"]  # what the next decoder pass is fed
        st["parent"] = torch.zeros(R, **i32)
        nws = K._L().gvl_beam_step_workspace_size(B, Kb)
        st["ws"] = torch.empty(max(nws, 8) // 4, **f32)
        st["hist"] = torch.zeros(cap, R, dtype=torch.int64, device=dev)
        ctl = _Controls(torch.zeros(B, self.max_prompt, dtype=torch.int64, device=dev),
                        *self.ctl_args)
        self.ctl = ctl
        self.ctl_on = ctl.always or ctl.min_new > 0
        if ctl.prompt is not None:
            st["prompt"] = ctl.prompt

    def _choose(self, logits):
        st, ctl, Kb = self._st, self.ctl, self.Kb
        R = logits.shape[0]
        t0 = self.dec.gap_hi
        if self.ctl_on:
            K.logits_process_dev(logits, st["hist"], st["step"], self.max_new, src=st["src"],
                                 t0=t0, prompt=st.get("prompt"), rows_per_item=Kb,
                                 repetition_penalty=ctl.pen, no_repeat_ngram_size=ctl.ngram,
                                 eos=ctl.eos, min_new=ctl.min_new, bad_tokens=ctl.bad,
                                 flen=st["flen"])
        K.beam_step_dev(logits, st["score"], st["flen"], st["len_norm"], st["src"], Kb, st["step"],
                        self.max_new, self.eos, t0,
                        (st["tok"], st["parent"], st["score_o"], st["flen_o"], st["src_o"]),
                        st["ws"])
        st["score"].copy_(st["score_o"])
        st["flen"].copy_(st["flen_o"])
        st["src"].copy_(st["src_o"])
        st["hist"].index_copy_(0, st["step64"], st["tok"].view(1, R))
        st["step"].add_(1)
        st["step64"].add_(1)

    @torch.no_grad()
    def __call__(self, prompt_ids, n_new=None, *, z=None, prompt_lens=None, return_all=False):
        """-> what beam_search() returns for these inputs and the session's settings."""
        n_new, lens = self._check_call(prompt_ids, n_new, z, prompt_lens)
        B, P = prompt_ids.shape
        Kb, eos = self.Kb, self.eos
        R = B * Kb
        if self.dec is None:
            self.dec = _StaticBeam(self.model, B, Kb, n_new, weights=self.weights,
                                   kv_cache=self.kv_cache)
            self.dec._init_static(self.max_prompt, self.max_new)
        dec = self.dec
        dec.max_new = n_new
        first = dec.start(prompt_ids, z, lens)
        dev, st, V = first.device, self._st, first.shape[1]
        if not st:
            self._setup(B, V, first.dtype, dev)
        S = t0 = dec.t
        st["t"].fill_(S)
        st["step"].zero_()
        st["step64"].zero_()
        st["logits0"].view(B, Kb, V)[:, 0] = first  # slots 1.. start empty (score -inf)
        st["score"].fill_(float("-inf"))
        st["score"].view(B, Kb)[:, 0] = 0.0
        st["flen"].zero_()
        st["src"].copy_(dec.initial_src(dev))
        dec.src = st["src"]
        if "prompt" in st:
            st["prompt"].fill_(-1)
            st["prompt"][:, self.max_prompt - P:] = ragged_prompt_for_controls(prompt_ids, lens)
        self._choose(st["logits0"])
        if n_new > 1:
            g = self._graph_for(S)
            done = None
            if eos is not None:
                done = lambda: bool(((st["flen"] > 0) | (st["score"] == float("-inf"))).all())
            self._replay(g, n_new - 1, done)
        dec.src = None
        # beam_search()'s ending, on the steps that ran (more than it runs when the poll came
        # late: those steps emitted eos for every hypothesis, which is its padding)
        Sn = int(st["step"])
        score, flen, src = st["score"], st["flen"], st["src"]
        ids = st["hist"][:Sn].t().gather(0, src[:, t0:t0 + Sn].long())
        if Sn < n_new:
            ids = torch.cat([ids, ids.new_full((R, n_new - Sn), eos)], dim=1)
        live = torch.where(score == float("-inf"), 0, Sn).to(torch.int32)
        lengths = torch.where(flen > 0, flen, live)
        ids, lengths, scores = ids.view(B, Kb, n_new), lengths.view(B, Kb), score.view(B, Kb)
        if return_all:
            return ids, lengths, scores.clone()
        return ids[:, 0], lengths[:, 0], scores[:, 0].clone()
