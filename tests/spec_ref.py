"""Plain-Python references for speculative decoding (include/gvl.h gvl_ngram_draft,
gvl_spec_accept, gvl.decode.speculative_generate), CPU only.

  * ngram_draft: the prompt-lookup draft of one row, as lists.
  * spec_accept: one accept step on a dict of per-row state lists.
  * simulate: the whole accept loop of speculative_generate for rows whose "true" tokens are
    known (the tokens the model emits whatever was drafted), with the draft taken from
    draft_ids alone: how many rounds run and how many guesses are made / accepted.
"""


def ngram_draft(prompt, emitted, ngram, D, n_new, given=None):
    """prompt, emitted: lists of ids (emitted: the n tokens so far); given: None or a list of
    n_new ids (-1: none).  -> D ids, -1 where there is no guess."""
    n = len(emitted)
    if n >= n_new:
        return [-1] * D
    s = list(prompt) + list(emitted)
    L = len(s)
    draft = [-1] * D
    for g in range(ngram, 0, -1):
        hit = [i for i in range(0, L - g) if s[i:i + g] == s[L - g:]]  # i + g <= L - 1
        if hit:
            i = max(hit)
            for j in range(D):
                if i + g + j < L:
                    draft[j] = s[i + g + j]
            break
    if given is not None:
        for j in range(D):
            if n + j < n_new and given[n + j] >= 0:
                draft[j] = given[n + j]
    return draft


def spec_accept(x, draft, st, n_new, eos=-1):
    """x [B][Q], draft [B][Q-1]; st: dict of lists n, kv_len, pos, lengths, last, drafted,
    accepted and out [B][n_new], edited in place."""
    for b in range(len(x)):
        n = st["n"][b]
        if n >= n_new:
            continue
        Q = len(x[b])
        a = 0
        while a < Q - 1 and draft[b][a] == x[b][a]:
            a += 1
        m = min(a + 1, n_new - n)
        ended = False
        if eos >= 0:
            for e in range(m):
                if x[b][e] == eos:
                    m, ended = e + 1, True
                    break
        st["out"][b][n:n + m] = x[b][:m]
        if ended:
            st["lengths"][b] = n + m
            st["out"][b][n + m:] = [eos] * (n_new - n - m)
            st["n"][b] = n_new
        else:
            st["n"][b] = n + m
        st["kv_len"][b] += m
        st["pos"][b] += m
        st["last"][b] = x[b][m - 1]
        st["drafted"][b] += sum(1 for d in draft[b] if d >= 0)
        st["accepted"][b] += m - 1


def simulate(true, given, draft_len, eos=-1, prompts=None, ngram=0):
    """true [B][n_new]: the token each row emits at every index as long as what it was fed is its
    own prefix (a deterministic model); given [B][n_new]: the draft (-1: none).  prompts None:
    `given` is the only source of guesses; else the rows' real prompts [B][len_b], and the draft
    is ngram_draft's (lookup with `ngram`, overridden by `given`, which may then be None).  Runs
    the rounds of speculative_generate: the first on the prefill's logits (one row, no draft),
    then passes of Q = draft_len + 1 rows until every row is done.
    -> dict(steps, drafted [B], accepted [B], out [B][n_new], lengths [B])."""
    B, n_new = len(true), len(true[0])
    st = dict(n=[0] * B, kv_len=[0] * B, pos=[0] * B, lengths=[n_new] * B, last=[0] * B,
              drafted=[0] * B, accepted=[0] * B, out=[[0] * n_new for _ in range(B)])
    spec_accept([[true[b][0]] for b in range(B)], [[] for _ in range(B)], st, n_new, eos)
    steps = 1
    while min(st["n"]) < n_new:
        draft = []
        for b in range(B):
            n = st["n"][b]
            if prompts is None:  # no lookup: only what `given` supplies
                draft.append([given[b][n + j] if n + j < n_new else -1 for j in range(draft_len)])
            else:
                draft.append(ngram_draft(prompts[b], st["out"][b][:min(n, n_new)], ngram,
                                         draft_len, n_new, None if given is None else given[b]))
        x = []
        for b in range(B):
            n = st["n"][b]
            row = []
            ok = True  # the fed tokens so far are the row's own prefix
            for j in range(draft_len + 1):
                if n + j < n_new and ok:
                    row.append(true[b][n + j])
                    ok = j < draft_len and draft[b][j] == true[b][n + j]
                else:
                    row.append(-2)  # whatever the model says after a wrong guess: never kept
            x.append(row)
        spec_accept(x, draft, st, n_new, eos)
        steps += 1
    return dict(steps=steps, drafted=st["drafted"], accepted=st["accepted"], out=st["out"],
                lengths=st["lengths"])
