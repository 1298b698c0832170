"""The device-stepped decode entry points without a GPU (gvl_attn_decode_step,
gvl_logits_process_dev, gvl_beam_step_dev): every refusal happens on the host before any launch,
returns -1 with a message naming the argument and leaves every output as it was.  The arrays
are host memory: a call that got past its checks would fail with the launch's error instead of
the message."""
import numpy as np

SENT16 = 0x40E0  # bf16 7.0
H, C, R, TMAX = 2, 128, 2, 16


def _lib():
    from gvl import _lib
    return _lib.load()


def _host(n, dtype, fill):
    """A 64-byte-aligned host array of n elements."""
    item = np.dtype(dtype).itemsize
    raw = np.empty(n * item + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n * item].view(dtype)
    a[:] = fill
    return a


def test_binding_and_header_name_the_new_entry_points():
    from gvl import _lib
    from tests.test_capi import declared
    names = {"gvl_attn_decode_step", "gvl_logits_process_dev", "gvl_beam_step_dev"}
    assert names <= set(declared()) and names <= set(_lib.SIGNATURES)
    assert _lib.load().gvl_abi_version() == 14  # new symbols, no version bump


def test_attn_decode_step_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    qkv = _host(R * 3 * C, np.uint16, 0x3F80)
    cache = _host(R * TMAX * 3 * C + 8, np.uint16, SENT16)
    o = _host(R * C, np.uint16, SENT16)
    t = _host(1, np.int32, 3)
    src = _host(R * TMAX, np.int32, 0)
    gap = _host(R, np.int32, 0)
    P = lambda a, byte_off=0: a.ctypes.data + byte_off

    def call(qkvp=P(qkv), cachep=P(cache), tp=P(t), op=P(o), sb=TMAX * 3 * C, Tmax=TMAX, o_ld=C,
             srcp=None, src_ld=0, gapp=None, gap_hi=0, rows=R):
        return lib.gvl_attn_decode_step(qkvp, cachep, sb, Tmax, tp, op, o_ld, rows, H, 0.125, srcp,
                                        src_ld, gapp, gap_hi, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (cache == SENT16).all() and (o == SENT16).all()

    for name in ("qkvp", "cachep", "op"):
        refused(call(**{name: None}), b"gvl_attn_decode_step: null buffer")
    refused(call(tp=None), b"gvl_attn_decode_step: null t")
    refused(call(Tmax=4097, sb=4097 * 3 * C), b"Tmax=4097 out of range")
    refused(call(Tmax=0), b"Tmax=0 out of range")
    refused(call(sb=TMAX * 3 * C + 4), b"cache_sb=%d is no stride" % (TMAX * 3 * C + 4))
    refused(call(sb=TMAX * 3 * C - 8), b"is no stride")            # rows would overlap
    refused(call(o_ld=C - 8), b"o_ld=%d < C" % (C - 8))
    refused(call(cachep=P(cache, 8)), b"16-byte aligned")
    refused(call(qkvp=P(qkv, 2)), b"16-byte aligned")
    refused(call(srcp=P(src), src_ld=TMAX - 1), b"src_ld=%d < Tmax=%d" % (TMAX - 1, TMAX))
    refused(call(gapp=P(gap), gap_hi=TMAX + 1), b"gap_hi=%d outside 0..Tmax" % (TMAX + 1))
    refused(call(gapp=P(gap), gap_hi=-1), b"gap_hi=-1 outside")
    refused(call(rows=65536), b"R=65536")
    assert call(rows=0) == 0  # nothing to do: no launch either
    assert (cache == SENT16).all() and (o == SENT16).all()


def test_logits_process_dev_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    V, Rr = 16, 2
    logits = _host(Rr * V, np.float32, 7.0)
    hist = _host(8 * Rr, np.int64, 1)
    step = _host(1, np.int32, 0)
    prompt = _host(Rr * 4096, np.int64, 1)
    src = _host(Rr * 16, np.int32, 0)
    bad = _host(2, np.int32, 3)
    P = lambda a: a.ctypes.data

    def call(lg=P(logits), ld=V, histp=P(hist), hist_ld=Rr, stepp=P(step), cap=8, srcp=None,
             src_ld=0, t0=0, pr=None, pr_ld=0, Pn=0, rpi=1, pen=1.3, ngram=2, min_new=0, badp=None,
             n_bad=0):
        return lib.gvl_logits_process_dev(lg, ld, 1, Rr, V, histp, hist_ld, stepp, cap, srcp,
                                          src_ld, t0, pr, pr_ld, Pn, rpi, pen, ngram, 3, min_new,
                                          badp, n_bad, None, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (logits == 7.0).all()

    refused(call(lg=None), b"gvl_logits_process_dev: null logits")
    refused(call(stepp=None), b"gvl_logits_process_dev: null step")
    refused(call(histp=None), b"null hist with hist_cap=8")
    refused(call(cap=-1), b"hist_cap=-1 is negative")
    refused(call(pr=P(prompt), pr_ld=4096, Pn=4089), b"L = P + hist_cap = 4097 exceeds 4096")
    refused(call(cap=4097), b"L = P + hist_cap = 4097 exceeds 4096")
    refused(call(hist_ld=Rr - 1), b"hist_ld=1 < R=2")
    refused(call(srcp=P(src), src_ld=10, t0=3), b"does not hold t0 + hist_cap = 11 columns")
    refused(call(Pn=4), b"null prompt with P=4")
    refused(call(ld=V - 1), b"ld=15 < V=16")
    refused(call(rpi=0), b"rows_per_item=0")
    refused(call(pen=0.0), b"rep_penalty=0")
    refused(call(ngram=17), b"ngram=17")
    refused(call(n_bad=2), b"null bad with n_bad=2")
    # every control off: no launch, nothing read
    assert call(pen=1.0, ngram=0) == 0 and (logits == 7.0).all()


def test_beam_step_dev_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    K, V, B = 2, 16, 1
    f32 = lambda n, v: _host(n, np.float32, v)
    i32 = lambda n, v: _host(n, np.int32, v)
    a = dict(logits=f32(B * K * V, 0.5), score=f32(B * K, 0.0), flen=i32(B * K, 0),
             len_norm=f32(8, 1.0), step=i32(1, 0), src_in=i32(B * K * 8, 0),
             tok=_host(B * K, np.int64, -9), parent=i32(B * K, -9), score_out=f32(B * K, 7.0),
             flen_out=i32(B * K, -9), src_out=i32(B * K * 8, -9), ws=f32(64, 7.0))

    def call(null=None, K=K, V=V, ld=None, max_steps=4, t0=1, src_ld=8, same_src=False):
        p = {n: (None if n == null else v.ctypes.data) for n, v in a.items()}
        if same_src:
            p["src_out"] = p["src_in"]
        return lib.gvl_beam_step_dev(p["logits"], V if ld is None else ld, 1, B, K, V, p["score"],
                                     p["flen"], p["len_norm"], p["step"], max_steps, -1, t0,
                                     p["src_in"], src_ld, p["tok"], p["parent"], p["score_out"],
                                     p["flen_out"], p["src_out"], p["ws"], None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (a["tok"] == -9).all() and (a["parent"] == -9).all() and (a["flen_out"] == -9).all()
        assert (a["score_out"] == 7.0).all() and (a["src_out"] == -9).all()
        assert (a["ws"] == 7.0).all()

    refused(call(null="step"), b"gvl_beam_step_dev: null step")
    for name in ("logits", "len_norm", "src_out", "ws", "tok"):
        refused(call(null=name), b"gvl_beam_step_dev: null buffer")
    refused(call(max_steps=0), b"max_steps=0 must be at least 1")
    refused(call(max_steps=-3), b"max_steps=-3 must be at least 1")
    for k in (0, 9):
        refused(call(K=k), b"K=%d out of range" % k)
    refused(call(V=65537), b"V=65537")
    refused(call(ld=8), b"ld=8")
    # the furthest step the counter may reach must fit the table: t0 + max_steps - 1 < src_ld
    refused(call(max_steps=8, t0=1, src_ld=8), b"position t0 + step = 8 outside the src table")
    refused(call(same_src=True), b"distinct tables")
