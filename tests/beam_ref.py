"""fp64 numpy restatement of one beam-search step (include/gvl.h gvl_beam_step).

Row r = b*K + j.  A live row (flen 0, finite score) offers (r, v) for every v with
raw = score[r] + log_softmax(logits[r])[v] and length step + 1, finished when v == eos; a
finished row offers (r, eos) with its own raw and length; an empty row (score -inf) nothing.
key = raw * len_norm[length]; the K largest keys of an item win, ties to the lower parent slot,
then the lower token id — a stable descending sort over the flat candidate index
parent * V + token.  Slots past the last candidate are empty.
"""
import numpy as np


def _candidates(lg, sc, fl, len_norm, step, eos, K, V):
    """Flat-index-ordered candidate arrays of one item: key, raw, parent, tok, flen."""
    key, raw, par, tok, fln = [], [], [], [], []
    for j in range(K):
        if sc[j] == -np.inf:
            continue
        if fl[j] > 0:
            key.append(np.array([sc[j] * len_norm[fl[j]]]))
            raw.append(np.array([sc[j]]))
            par.append(np.array([j]))
            tok.append(np.array([max(eos, 0)]))
            fln.append(np.array([fl[j]]))
            continue
        x = lg[j] - lg[j].max()
        logp = x - np.log(np.exp(x).sum())
        r = sc[j] + logp
        f = np.zeros(V, dtype=np.int64)
        if eos >= 0:
            f[eos] = step + 1
        key.append(r * len_norm[step + 1])
        raw.append(r)
        par.append(np.full(V, j))
        tok.append(np.arange(V))
        fln.append(f)
    if not key:
        z = np.zeros(0)
        return z, z, z.astype(np.int64), z.astype(np.int64), z.astype(np.int64)
    return tuple(np.concatenate(a) for a in (key, raw, par, tok, fln))


def beam_step_ref(logits, score, flen, len_norm, step, eos, t0, src, K):
    """logits [R, V], score [R], flen [R], len_norm [>= step + 2], src [R, ld] (any numeric
    dtypes; computed in fp64); eos None or -1: no end token.
    -> dict(tok, parent, score, flen, src, gap): the outputs of gvl_beam_step and the smallest
    key gap between consecutive candidates among the top 2K + 1 of any item, pairs that tie by
    construction (same row and equal logit, or rows with identical score and logits) not
    counted; inf when no pair counts."""
    lg = np.asarray(logits, dtype=np.float64)
    sc = np.asarray(score, dtype=np.float64)
    fl = np.asarray(flen, dtype=np.int64)
    ln = np.asarray(len_norm, dtype=np.float64)
    src = np.asarray(src)
    eos = -1 if eos is None else int(eos)
    R, V = lg.shape
    assert R % K == 0
    T = t0 + step
    out = dict(tok=np.zeros(R, np.int64), parent=np.zeros(R, np.int32), score=np.zeros(R, np.float32),
               flen=np.zeros(R, np.int32), src=src.copy(), gap=np.inf)
    for b in range(R // K):
        rows = slice(b * K, (b + 1) * K)
        key, raw, par, tok, fln = _candidates(lg[rows], sc[rows], fl[rows], ln, step, eos, K, V)
        order = np.argsort(-key, kind="stable")  # flat index order breaks ties
        top = order[:2 * K + 1]
        for a, c in zip(top[:-1], top[1:]):
            same_row = par[a] == par[c] and fl[b * K + par[a]] == 0 and \
                lg[b * K + par[a], tok[a]] == lg[b * K + par[c], tok[c]]
            twin_rows = par[a] != par[c] and tok[a] == tok[c] and \
                sc[b * K + par[a]] == sc[b * K + par[c]] and fl[b * K + par[a]] == fl[b * K + par[c]] and \
                (fl[b * K + par[a]] > 0 or np.array_equal(lg[b * K + par[a]], lg[b * K + par[c]]))
            if not (same_row or twin_rows):
                out["gap"] = min(out["gap"], float(key[a] - key[c]))
        for i in range(K):
            r = b * K + i
            if i < len(order):
                c = order[i]
                out["tok"][r], out["parent"][r] = tok[c], par[c]
                out["score"][r], out["flen"][r] = raw[c], fln[c]
            else:
                out["tok"][r], out["parent"][r] = max(eos, 0), i
                out["score"][r], out["flen"][r] = -np.inf, 0
            out["src"][r, :T] = src[b * K + out["parent"][r], :T]
            out["src"][r, T] = r
    return out
