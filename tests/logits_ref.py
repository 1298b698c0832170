"""numpy restatement of the logits processors (include/gvl.h gvl_logits_process).

Row r's sequence s = its item's prompt, then its generated tokens g_i = hist[i, row_i], row_i = r
or src[r, t0 + i] clamped into [0, R).  A row with flen[r] > 0 is left alone.  Otherwise:
repetition penalty once per distinct in-range token of s (x < 0 ? x * p : x / p in float32), then
the bans, which win: the no-repeat n-gram rule, the end token, the bad tokens.  The penalty is
computed in float32 and, for bf16 logits, rounded once through torch, so a kernel that follows the
header can be compared bit for bit.
"""
import numpy as np
import torch


def sequences(R, hist, n_hist, src=None, t0=0, prompt=None, rows_per_item=1):
    """The token sequence of every row: a list of R lists of ints."""
    out = []
    for r in range(R):
        s = [] if prompt is None else [int(v) for v in prompt[r // rows_per_item]]
        for i in range(n_hist):
            row = r if src is None else min(max(int(src[r, t0 + i]), 0), R - 1)
            s.append(int(hist[i, row]))
        out.append(s)
    return out


def banned_by_ngram(s, n):
    """Tokens the no-repeat rule forbids after sequence s (out-of-range ones included)."""
    L = len(s)
    if n <= 0:
        return set()
    if n == 1:
        return set(s)
    if L < n:
        return set()
    tail = s[L - n + 1:]
    return {s[i + n - 1] for i in range(L - n + 1) if s[i:i + n - 1] == tail}


def logits_ref(logits, hist, n_hist, *, src=None, t0=0, prompt=None, rows_per_item=1,
               repetition_penalty=1.0, no_repeat_ngram_size=0, eos=None, ban_eos=False,
               bad_tokens=None, flen=None, V=None):
    """logits: a torch tensor [R, ld] (bfloat16 or float32) whose first V columns are the
    vocabulary (V=None: all of them); hist [>= n_hist, >= R], src [R, >= t0 + n_hist], prompt
    [R / rows_per_item, P], bad_tokens, flen: arrays or tensors of integers (or None).
    -> the edited copy, same dtype and shape; columns [V, ld) are never changed."""
    as_np = lambda a: None if a is None else np.asarray(torch.as_tensor(a).cpu())
    hist, src, prompt, bad, flen = (as_np(a) for a in (hist, src, prompt, bad_tokens, flen))
    R, ld = logits.shape
    V = ld if V is None else V
    bf16 = logits.dtype == torch.bfloat16
    x = logits.detach().cpu().float().numpy().copy()  # float32, exact for bf16
    p = np.float32(repetition_penalty)
    seqs = sequences(R, hist, n_hist, src, t0, prompt, rows_per_item)
    for r in range(R):
        if flen is not None and flen[r] > 0:
            continue
        s = seqs[r]
        if p != np.float32(1.0):
            for v in sorted({v for v in s if 0 <= v < V}):
                a = x[r, v]
                x[r, v] = a * p if a < 0 else a / p  # float32 ops, one rounding each
        if bf16:  # the stored value: one round-to-nearest-even
            x[r, :V] = torch.from_numpy(x[r, :V]).to(torch.bfloat16).float().numpy()
        bans = banned_by_ngram(s, no_repeat_ngram_size)
        if ban_eos and eos is not None:
            bans.add(int(eos))
        if bad is not None:
            bans.update(int(v) for v in bad)
        for v in bans:
            if 0 <= v < V:
                x[r, v] = -np.inf
    out = torch.from_numpy(x)
    return out.to(torch.bfloat16) if bf16 else out
