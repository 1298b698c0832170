"""The drop-in boundary: libgvl.so loads on a CPU-only host and exports exactly the
symbols include/gvl.h declares, and the ctypes binding covers all of them."""
import ctypes
import os
import re

from tests.conftest import ROOT

HDR = os.path.join(ROOT, "include", "gvl.h")
LIB = os.path.join(ROOT, "gpt2-vision-language_amd", "gvl", "libgvl.so")


def declared():
    txt = open(HDR).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w]+\s*\*?\s*(gvl_\w+)\s*\(", txt, re.M)))


def test_header_declares_api():
    names = declared()
    assert "gvl_gemm" in names and "gvl_attn_bwd" in names and len(names) >= 20


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "libgvl.so not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert not missing, missing
    lib.gvl_abi_version.restype = ctypes.c_int
    assert lib.gvl_abi_version() == 14


def test_library_links_no_vendor_blas():
    """Since ABI v10 every GEMM runs on libgvl's own kernels: the library has no hipBLASLt /
    rocBLAS dependency (round 4's gvl_gemm_lib_route is gone)."""
    import subprocess
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "-d", LIB], capture_output=True,
                         text=True, check=True).stdout
    needed = [ln for ln in out.splitlines() if "NEEDED" in ln]
    assert needed and not any("blas" in ln.lower() for ln in needed), needed


def test_library_reads_no_environment():
    """The settled A/B switches are frozen: libgvl imports no getenv, so no routing decision can
    depend on the environment (gvl_gemm_tune is the only handle on it)."""
    import subprocess
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "-W", LIB],
                         capture_output=True, text=True, check=True).stdout
    syms = [ln.split()[-1].split("@")[0] for ln in out.splitlines() if " UND " in ln]
    assert any(s.startswith("hip") for s in syms), syms[:8]  # (the listing is the imports)
    assert [s for s in syms if "getenv" in s] == []


def test_package_reads_only_the_kept_variables():
    """The gvl package reads exactly these GVL_* variables (the library path, the documented id
    check, and the data-parallel overlap / trace handles)."""
    import glob
    pat = re.compile(r"""(?:environ(?:\.get)?|getenv)\s*[\[(]\s*["'](GVL_[A-Z0-9_]+)["']""")
    found = set()
    for path in glob.glob(os.path.join(ROOT, "gpt2-vision-language_amd", "gvl", "*.py")):
        found |= set(pat.findall(open(path).read()))
    assert found == {"GVL_LIB", "GVL_CHECK_IDS", "GVL_DP_OVERLAP_BLOCKS", "GVL_TRACE_BUCKETS"}


def test_binding_covers_header():
    from gvl import _lib
    assert sorted(_lib.SIGNATURES) == declared()
    lib = _lib.load()  # binds every symbol with its argtypes
    assert lib.gvl_abi_version() == 14


def test_rejects_bad_arguments_without_gpu():
    """Argument validation runs on the host before any launch (no device needed)."""
    from gvl import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()
    d.a = d.b = d.c = 16
    d.m, d.n, d.k = 8, 8, 7  # K not a multiple of 8
    d.lda = d.ldb = d.ldc = 8
    rc = lib.gvl_gemm(ctypes.byref(d), None)
    assert rc == -1 and b"multiple of 8" in lib.gvl_last_error()
    rc = lib.gvl_layernorm_fwd(None, 4, None, None, None, 4, None, None, 1, 2048, 1e-5, None)
    assert rc == -1 and b"cols" in lib.gvl_last_error()


SENT16 = 0x40E0  # bf16 7.0


def _host(n, dtype, fill):
    """A 64-byte-aligned host array of n elements: the refused calls below never launch, so
    no pointer is ever dereferenced and host memory stands in for the device's."""
    import numpy as np
    item = np.dtype(dtype).itemsize
    raw = np.empty(n * item + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    a = raw[off:off + n * item].view(dtype)
    a[:] = fill
    assert a.ctypes.data % 64 == 0
    return a


def test_layernorm_bwd_refuses_bad_arguments_before_any_launch():
    """Every GVL_REQUIRE of ln_bwd_launch: a width above 1024 or no multiple of 8, a leading
    dimension (dy, x, dx, residual) that is no multiple of 8, a dx or residual off the 16-byte
    grid, a null residual, dw / db / deferral without a workspace.  Each returns -1 with its
    message and writes nothing: dx, dw, db and the workspace keep their sentinels.  A call that
    got past its check would fail here with the launch's error instead of the message."""
    import numpy as np
    from gvl import _lib
    lib = _lib.load()
    rows, ld = 4, 1040
    dy, x, res = (_host(rows * ld, np.uint16, 0x3F80) for _ in range(3))
    w = _host(ld, np.uint16, 0x3F80)
    mean, rstd = _host(rows, np.float32, 0.0), _host(rows, np.float32, 1.0)
    dx = _host(rows * ld + 8, np.uint16, SENT16)
    dw, db = _host(ld, np.uint16, SENT16), _host(ld, np.uint16, SENT16)
    ws = _host(2 * ld, np.float32, 7.0)
    P = lambda a, byte_off=0: a.ctypes.data + byte_off

    def bwd(cols=16, lddy=16, ldx=16, lddx=16, dxp=None, acc_dx=0, dwp=None, dbp=None, acc_wb=0,
            wsp=None):
        return lib.gvl_layernorm_bwd(P(dy), lddy, P(x), ldx, P(w), P(mean), P(rstd),
                                     P(dx) if dxp is None else dxp, lddx, acc_dx, dwp, dbp, acc_wb,
                                     wsp, rows, cols, None)

    def res_(cols=16, ldr=16, rp=P(res), lddx=16):
        return lib.gvl_layernorm_bwd_res(P(dy), 16, P(x), 16, P(w), P(mean), P(rstd), rp, ldr,
                                         P(dx), lddx, P(dw), P(db), 0, P(ws), rows, cols, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (dx == SENT16).all() and (dw == SENT16).all() and (db == SENT16).all()
        assert (ws == 7.0).all()

    shape = b"gvl_layernorm_bwd: cols unsupported"
    refused(bwd(cols=1032, lddy=1032, ldx=1032, lddx=1032), shape)
    refused(bwd(cols=12), shape)
    refused(bwd(cols=0), shape)
    refused(bwd(lddy=20), shape)
    refused(bwd(ldx=20), shape)
    refused(bwd(lddx=20), shape)
    refused(bwd(lddx=12, acc_dx=1), shape)
    refused(bwd(dxp=P(dx, 8)), shape)   # 8-byte aligned only
    refused(bwd(dxp=P(dx, 2)), shape)
    refused(res_(ldr=20), shape)
    refused(res_(rp=P(res, 8)), shape)
    refused(res_(rp=None), b"null residual")
    refused(res_(cols=1032, ldr=1032, lddx=1032), shape)
    need = b"dw/db need a workspace"
    refused(bwd(dwp=P(dw)), need)
    refused(bwd(dbp=P(db)), need)
    refused(bwd(dwp=P(dw), dbp=P(db), acc_wb=1), need)
    refused(bwd(acc_wb=2), need)        # deferred partials with nowhere to leave them


def test_layernorm_finalize_batched_refuses_bad_arguments_before_any_launch():
    """gvl_layernorm_bwd_finalize_batched: 65 items (one more than a launch holds; the Python
    wrapper splits), a block count of 513 or -1, a null workspace item (first or last), null
    lists, a width of 0 or 1032, a negative count: -1 with the message, no output written."""
    import numpy as np
    from gvl import _lib
    lib = _lib.load()
    C_, n = 16, 65
    ws = _host(512 * 2 * C_, np.float32, 1.0)
    outs = _host(2 * n * C_, np.uint16, SENT16)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32

    def call(count, cols=C_, nblk=None, null_ws=None, ws_list=True, nb_list=True):
        wsl = (vp * n)(*[None if i == null_ws else ws.ctypes.data for i in range(n)])
        nbl = (i32 * n)(*[(nblk or {}).get(i, 512) for i in range(n)])
        dwl = (vp * n)(*[outs.ctypes.data + 2 * C_ * (2 * i) for i in range(n)])
        dbl = (vp * n)(*[outs.ctypes.data + 2 * C_ * (2 * i + 1) for i in range(n)])
        return lib.gvl_layernorm_bwd_finalize_batched(wsl if ws_list else None,
                                                      nbl if nb_list else None, count, cols, dwl,
                                                      dbl, 1, None)

    def refused(rc, text):
        assert rc == -1 and text in lib.gvl_last_error(), (rc, lib.gvl_last_error())
        assert (outs == SENT16).all() and (ws == 1.0).all()

    bad = b"gvl_layernorm_bwd_finalize_batched: bad arguments"
    refused(call(65), bad)
    refused(call(-1), bad)
    refused(call(2, cols=1032), bad)
    refused(call(2, cols=0), bad)
    refused(call(2, ws_list=False), bad)
    refused(call(2, nb_list=False), bad)
    refused(call(3, nblk={2: 513}), b"item 2: null workspace or bad block count")
    refused(call(3, nblk={0: -1}), b"item 0: null workspace or bad block count")
    refused(call(3, null_ws=0), b"item 0: null workspace or bad block count")
    refused(call(64, null_ws=63), b"item 63: null workspace or bad block count")
    assert call(0) == 0  # nothing to do: no launch either
    assert (outs == SENT16).all()
