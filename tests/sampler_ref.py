"""References for gvl_sample (csrc/decode.hip sample_kernel), CPU only.

  * draw_ok: the acceptance predicate of every sampler test.  With dist the float64 filtered
    distribution (oracle/ops.py sampling_distribution) and cdf its cumulative in token-index
    order, a draw `got` for the uniform u is right iff dist[got] > 0 and
    cdf[prev] - tol <= u <= cdf[got] + tol, prev the kept token in front of got (0 for the
    first).  tol = 1e-5 is what fp32 sums of <= 65536 probabilities may move a boundary by; it
    is tied to the boundaries NEXT TO the drawn token, not to any boundary of the row.
  * boundary_sweep: the uniforms that sit on and next to every CDF boundary of a row.
  * ScanEmulation: sample_kernel's draw restated in numpy float32 (block_exscan's shuffle scan,
    the per-thread claim test, the walk), in the form the kernel had (`fixed=False`: thread i
    claims pre_i <= target < fl(pre_i + s_i), which leaves gaps between neighbouring threads,
    and an unclaimed target falls back to the last kept token) and in the form it has now
    (`fixed=True`: the owner is the last thread with pre_i <= target).  numpy's exp stands in
    for the device's exp2, so counts differ from the hardware's; the mechanism does not.
  * edge_cases: the rows of the kept-set / per-token test with the conditions under which fp32
    and float64 agree on the kept set (case_conditions).
"""
import numpy as np
import torch

from oracle import ops as O

TOL = 1e-5
BF = torch.bfloat16
NT = 1024  # SMP_NT: threads per row
U_LAST = np.nextafter(np.float32(1), np.float32(0))  # the largest uniform: 1 - 2**-24


def row_values(t):
    """A logits tensor (bf16 or fp32) as the float64 values the kernel reads."""
    return t.detach().to(torch.float64).cpu().numpy()


def cdf64(dist):
    return np.cumsum(np.asarray(dist, dtype=np.float64))


def draw_edges(dist, cdf, got):
    """(lo, hi): the reference CDF interval of every drawn token (arrays like got)."""
    got = np.asarray(got, dtype=np.int64)
    kept = np.nonzero(dist > 0)[0]
    pos = np.searchsorted(kept, got)  # for a kept token: its rank among the kept ones
    pos = np.clip(pos, 0, kept.size - 1)
    lo = np.where(pos > 0, cdf[kept[np.maximum(pos - 1, 0)]], 0.0)
    return lo, cdf[got]


def draw_ok(dist, cdf, got, u, tol=TOL):
    """The predicate above, elementwise over the arrays got / u (one row's distribution)."""
    got = np.asarray(got, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    inside = (got >= 0) & (got < dist.size)
    g = np.where(inside, got, 0)
    lo, hi = draw_edges(dist, cdf, g)
    return inside & (dist[g] > 0) & (lo - tol <= u) & (u <= hi + tol)


def edge_distance(dist, cdf, got, u):
    """|u - the nearer edge of the drawn token's interval| (0 inside it is not needed: this is
    read only for draws that differ from the float64 inverse CDF)."""
    lo, hi = draw_edges(dist, cdf, np.asarray(got, dtype=np.int64))
    u = np.asarray(u, dtype=np.float64)
    return np.minimum(np.abs(u - lo), np.abs(u - hi))


def old_boundary_rule(cdf, u, tol=TOL):
    """What test_sampler_matches_reference_distribution granted a mismatching draw before:
    u within tol of ANY boundary of the row."""
    return np.min(np.abs(cdf[None, :] - np.asarray(u, dtype=np.float64)[:, None]), axis=1) < tol


def oracle_draws(dist, u):
    """O.inverse_cdf_index for an array of uniforms (one cumulative sum for all of them)."""
    cdf = np.cumsum(dist)
    i = np.searchsorted(cdf, np.asarray(u, dtype=np.float64) * cdf[-1], side="right")
    return np.minimum(i, np.nonzero(dist > 0)[0][-1]).astype(np.int64)


# ------------------------------------------------------------------------ boundary sweep
SWEEP_V, SWEEP_SEED, SWEEP_NEIGHBOURS = 1000, 1234, 16
SWEEP_BIG_V, SWEEP_BIG_BOUNDARIES = 50257, 2000


def sweep_row(V=SWEEP_V, dtype=torch.float32, seed=SWEEP_SEED):
    """Seeded Gaussian logits x 1.5 (temperature 1, no filter)."""
    g = torch.Generator().manual_seed(seed + V)
    return (torch.randn(V, generator=g) * 1.5).to(dtype)


def boundary_sweep(cdf, which=None, k=SWEEP_NEIGHBOURS):
    """fl32(c_i) and its k fp32 neighbours on each side for the boundaries c_i = cdf[i],
    i < V - 1 (or i in `which`), without any u >= 1 -> (u float32 [n], boundary index [n])."""
    idx = np.arange(cdf.size - 1) if which is None else np.asarray(which)
    c = cdf[idx].astype(np.float32)
    bits = c.view(np.int32).astype(np.int64)[:, None] + np.arange(-k, k + 1)[None, :]
    ok = bits > 0  # positive floats: the bit pattern orders like the value
    u = np.where(ok, bits, 1).astype(np.int32).view(np.float32)
    ok &= u < np.float32(1.0)
    bi = np.broadcast_to(idx[:, None], u.shape)
    return np.ascontiguousarray(u[ok]), np.ascontiguousarray(bi[ok])


def sweep_big_boundaries(V=SWEEP_BIG_V, n=SWEEP_BIG_BOUNDARIES, seed=SWEEP_SEED):
    return np.sort(np.random.default_rng(seed).permutation(V - 1)[:n])


def thread_boundaries(V=SWEEP_BIG_V):
    """The boundaries between the chunks of neighbouring threads (E = ceil(V / 1024) tokens
    each): the only ones at which the per-thread intervals of the scan meet."""
    E = -(-V // NT)
    return np.arange(E - 1, V - 1, E)


# ------------------------------------------------------------------ fp32 restatement
class ScanEmulation:
    """The unfiltered draw of sample_kernel in numpy float32 for one row of logits."""

    def __init__(self, logits, inv_temp=1.0):
        x = np.asarray(logits, dtype=np.float32)
        V = x.size
        E = -(-V // NT)
        self.V, self.E = V, E
        with np.errstate(invalid="ignore"):
            x = x * np.float32(inv_temp)
            p = np.where(np.isneginf(x), np.float32(0), np.exp(x - x.max())).astype(np.float32)
        self.p = np.zeros(NT * E, dtype=np.float32)
        self.p[:V] = p
        self.p = self.p.reshape(NT, E)
        s = np.zeros(NT, dtype=np.float32)
        for j in range(E):
            s = s + self.p[:, j]
        self.s = s
        kept = self.p > 0
        self.last = np.where(kept.any(1), E - 1 - np.argmax(kept[:, ::-1], axis=1), 0)
        xs = s.reshape(NT // 64, 64).copy()  # block_exscan: shuffle scan inside each wave
        o = 1
        while o < 64:
            y = xs.copy()
            xs[:, o:] = y[:, o:] + y[:, :-o]
            o *= 2
        sh = xs[:, 63]
        base = np.zeros(NT // 64, dtype=np.float32)
        tot = np.float32(0)
        for i in range(NT // 64):
            base[i] = tot
            tot = tot + sh[i]
        self.tot = np.float32(tot)
        self.pre = ((base[:, None] + xs) - s.reshape(NT // 64, 64)).reshape(NT)
        acc = self.pre.copy()  # the walk: acc += x[j] over the thread's elements
        self.walk = np.empty((NT, E), dtype=np.float32)
        for j in range(E):
            acc = acc + self.p[:, j]
            self.walk[:, j] = acc
        self.fallback = int(np.max(np.where(s > 0, np.arange(NT) * E + self.last, 0)))

    def _pick(self, t, target):
        """The token thread t returns for `target` (arrays of pairs)."""
        hit = (self.walk[t] > target[:, None]) & (self.p[t] > 0)
        j = np.where(hit.any(1), np.argmax(hit, axis=1), self.last[t])
        return t * self.E + j

    def draw(self, u, fixed):
        """-> (token [n], fell_back [n]) for the float32 uniforms u."""
        u = np.asarray(u, dtype=np.float32)
        out = np.full(u.size, self.fallback, dtype=np.int64)
        fell = np.ones(u.size, dtype=bool)
        live = self.s > 0
        for a in range(0, u.size, 4096):
            target = u[a:a + 4096] * self.tot
            below = live[None, :] & (self.pre[None, :] <= target[:, None])
            if fixed:
                below &= (target < self.tot)[:, None]
                has = below.any(1)
                owner = NT - 1 - np.argmax(below[:, ::-1], axis=1)
                n = np.nonzero(has)[0]
                out[a + n] = self._pick(owner[n], target[n])
                fell[a + n] = False
            else:
                claim = below & (target[:, None] < (self.pre + self.s)[None, :])
                n, t = np.nonzero(claim)
                tok = self._pick(t, target[n])
                best = np.full(target.size, np.iinfo(np.int64).max)
                np.minimum.at(best, n, tok)
                has = claim.any(1)
                out[a:a + target.size][has] = best[has]
                fell[a:a + target.size][has] = False
        return out, fell


# -------------------------------------------------------------------------- edge cases
def _bf16_values(x):
    """float tensor -> the same values rounded to bf16, as float32 (exact in both dtypes)."""
    return x.to(BF).float()


def _plain(V, seed):
    """Logits whose every probability is wider than 4 tol with no filter (V <= 1025)."""
    g = torch.Generator().manual_seed(9000 + seed)
    return _bf16_values(torch.randn(V, generator=g) * 0.5)


def _headed(V, seed, n_head=80):
    """V > 1024: low Gaussian noise under n_head scattered tokens with distinct logits in
    [8, 8 + n_head / 16): a top-k <= 64 cut is clear (6 % between neighbours) and every kept
    interval wide.  The heads include the first and the last token of the row."""
    g = torch.Generator().manual_seed(9100 + seed)
    x = torch.randn(V, generator=g)
    at = torch.randperm(V - 2, generator=g)[:n_head - 2] + 1
    at = torch.cat([torch.tensor([0, V - 1]), at])
    x[at] = 8.0 + torch.randperm(n_head, generator=g).float() / 16.0
    return _bf16_values(x)


TIE5 = [3, 70, 200, 640, 999]
TIE6 = [10, 80, 150, 300, 700, 990]


def _topk_tie_row(V, seed):
    """Four distinct tokens above five that tie (different threads, different waves), noise
    far below."""
    g = torch.Generator().manual_seed(9200 + seed)
    x = torch.randn(V, generator=g) * 0.25 - 6.0
    scale = V // 1000
    x[[t * scale for t in TIE5]] = 2.0
    x[[17 * scale, 333 * scale, 555 * scale, 901 * scale]] = torch.tensor([3.0, 3.5, 2.5, 4.0])
    return _bf16_values(x)


def _topp_tie_row(seed=0):
    """Token 500 (logit 3) above six that tie at 2, noise around -6: sorted cumulative
    probabilities 0.30, 0.41, 0.52, 0.63, 0.74, 0.85, 0.96, then the noise."""
    g = torch.Generator().manual_seed(9300 + seed)
    x = torch.randn(1000, generator=g) * 0.25 - 6.0
    x[TIE6] = 2.0
    x[500] = 3.0
    return _bf16_values(x)


def _peaked_row():
    """For temperature 0.05: five head tokens 0.7 and more above everything else, so that all
    other probabilities are below 1e-6 and most underflow to 0 in fp32."""
    g = torch.Generator().manual_seed(9400)
    x = (torch.randn(1000, generator=g)).clamp(max=2.0)
    x[[5, 64, 511, 512, 998]] = torch.tensor([3.0, 2.9375, 2.875, 2.8125, 2.75])
    return _bf16_values(x)


def _masked_row(V, n_finite, seed):
    g = torch.Generator().manual_seed(9500 + seed)
    x = _plain(V, 50 + seed)
    keep = torch.randperm(V, generator=g)[:n_finite]
    y = torch.full((V,), float("-inf"))
    y[keep] = x[keep]
    return y


def edge_cases():
    """[(name, logits float32 [V] of bf16-representable values, temperature, top_k, top_p,
    narrow_ok)]: every case runs in fp32 and in bf16 on the same values.  narrow_ok marks the
    one row that has kept tokens narrower than 4 tol by design (temperature 0.05)."""
    c = []
    for V in (1, 63, 1000, 1024, 1025):
        c.append((f"plain-V{V}", _plain(V, V), 1.0, 0, 1.0, False))
    c.append(("headed-V50257-k64", _headed(50257, 1), 1.0, 64, 1.0, False))
    c.append(("headed-V65536-k50", _headed(65536, 2), 1.0, 50, 1.0, False))
    c.append(("headed-V50257-k64-p0.7", _headed(50257, 3), 1.0, 64, 0.7, False))
    # top-k ties
    c.append(("topk-tie5-keep2-V1000", _topk_tie_row(1000, 0), 1.0, 6, 1.0, False))
    c.append(("topk-tie5-keep2-V50257", _topk_tie_row(50257, 1), 1.0, 6, 1.0, False))
    t = _plain(1000, 77).clamp(max=1.0)
    t[[100, 400]] = 2.0
    c.append(("topk-1-on-a-tie", t, 1.0, 1, 1.0, False))
    low = _plain(63, 78)
    low[31] = -3.0
    c.append(("topk-V", low, 1.0, 63, 1.0, False))
    c.append(("topk-above-V", low, 1.0, 70, 1.0, False))
    c.append(("topk-V-1", low, 1.0, 62, 1.0, False))
    # top-p ties
    c.append(("topp-cross-mid-tie", _topp_tie_row(), 1.0, 0, 0.58, False))
    c.append(("topp-cross-first-of-tie", _topp_tie_row(), 1.0, 0, 0.35, False))
    c.append(("topp-only-top", _topp_tie_row(), 1.0, 0, 0.05, False))
    c.append(("topp-just-below-1", _plain(63, 79), 1.0, 0, 0.999, False))
    c.append(("topk5-topp0.6-tie", _topp_tie_row(), 1.0, 5, 0.6, False))
    # -inf logits
    c.append(("neginf-900-of-1000", _masked_row(1000, 100, 0), 1.0, 0, 1.0, False))
    c.append(("neginf-topk-above-finite", _masked_row(1000, 100, 1), 1.0, 200, 1.0, False))
    c.append(("neginf-single-finite", _masked_row(63, 1, 2), 1.0, 0, 1.0, False))
    c.append(("neginf-50257-k64", _neginf_big(), 1.0, 64, 1.0, False))
    # temperature
    c.append(("temp-0.05-peaked", _peaked_row(), 0.05, 0, 1.0, True))
    c.append(("temp-5", sweep_row().to(BF).float(), 5.0, 0, 1.0, False))
    return c


def _neginf_big():
    x = _headed(50257, 4)
    g = torch.Generator().manual_seed(9600)
    ban = torch.randperm(50257, generator=g)[:25000]
    ban = ban[x[ban] < 7.0]  # the noise only: the heads stay
    x[ban] = float("-inf")
    return x


def case_reference(case):
    """-> dict(dist, cdf, kept, wide, mids, first, last) of one edge case (float64)."""
    _, logits, temperature, top_k, top_p, _ = case
    dist = O.sampling_distribution(logits.double().numpy(), temperature, top_k, top_p)
    cdf = cdf64(dist)
    kept = np.nonzero(dist > 0)[0]
    wide = kept[dist[kept] > 4 * TOL]
    mids = cdf[wide] - 0.5 * dist[wide]
    # u = 0 and u = nextafter(1, 0) by the float64 inverse CDF: the first and the last kept
    # token in every case but the peaked one (narrow_ok)
    return dict(dist=dist, cdf=cdf, kept=kept, wide=wide, mids=mids,
                first=O.inverse_cdf_index(dist, 0.0), last=O.inverse_cdf_index(dist, float(U_LAST)))


def case_conditions(case):
    """The conditions under which fp32 and float64 agree on the kept set, as a dict of
    measured figures (tests/test_sampler_ref_cpu.py asserts them):
      narrow_count / narrow_mass: kept tokens not wider than 4 tol and their total mass;
      topk_gap: relative gap between the k-th and the (k+1)-th probability (inf: no cut,
        0.0 with topk_tie: identical logits, an exact tie the kernel orders by index);
      topp_gap: the least |cumulative - top_p| over the sorted list that top-p walks."""
    _, logits, temperature, top_k, top_p, _ = case
    x = logits.double().numpy()
    ref = case_reference(case)
    dist, kept = ref["dist"], ref["kept"]
    narrow = kept[dist[kept] <= 4 * TOL]
    out = dict(narrow_count=int(narrow.size), narrow_mass=float(dist[narrow].sum()),
               topk_gap=np.inf, topk_tie=False, topp_gap=np.inf)
    pr = O.sampling_distribution(x, temperature, 0, 1.0)
    if 0 < top_k < x.size:
        order = np.argsort(-pr, kind="stable")
        a, b = order[top_k - 1], order[top_k]
        out["topk_tie"] = bool(x[a] == x[b])
        out["topk_gap"] = float((pr[a] - pr[b]) / pr[a]) if pr[a] > 0 else 0.0
    if top_p < 1.0:
        pk = O.sampling_distribution(x, temperature, top_k, 1.0)
        cum = np.cumsum(pk[np.argsort(-pk, kind="stable")])
        out["topp_gap"] = float(np.min(np.abs(cum - top_p)))
    return out
