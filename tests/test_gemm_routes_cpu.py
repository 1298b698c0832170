"""The GEMM route table (tests/data/gemm_routes.json, written by tools/gemm_routes.py): the
kernel instance gvl_gemm_kernel_name reports for every descriptor of the table under every tune
setting, with and without workspace + tickets.  The name comes from the leaf that would launch
(csrc/gemm.hip gemm_dispatch), so a routing change shows here as a changed cell; cells whose
name was corrected when the name query moved onto the dispatch carry the earlier name in "was".
No GPU: the query touches no device."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gemm_routes as R  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "data", "gemm_routes.json")


def test_gemm_routes_match_table():
    from gvl import _lib
    want = json.load(open(TABLE))
    got = R.table(_lib.load())
    assert got["settings"] == want["settings"]
    assert len(got["rows"]) == len(want["rows"]) >= 300
    have, bad = R.cells(got), []
    for key, name in R.cells(want).items():
        if have.get(key) != name:
            bad.append((key, name, have.get(key)))
    assert not bad, f"{len(bad)} cells differ, first: {bad[:5]}"


def test_table_covers_every_family_and_marks_corrections():
    t = json.load(open(TABLE))
    fam = {n.split("<")[0] for n in t["names"]}
    assert fam >= {"gemm_w4x_kernel", "gemm_w4_kernel", "gemm_w4m_kernel", "gemm_w4n_kernel", "gemm_w4r_kernel",
                   "gemm_w4d_kernel", "gemm_pp3_kernel", "gemm_ring_kernel", "gemm_pp_kernel", "gemm_lds_kernel",
                   "gemm_bf16_kernel"}, fam
    cur = R.cells(t)
    for r in t["rows"]:
        for cell, old in r.get("was", {}).items():
            s, w = cell.split("/")
            new = cur[(r["m"], r["n"], r["k"], r["a_mn"], r["b_mn"], r["epi"], s, w)]
            assert new != old
            # the three corrected classes: MN-contiguous A with K-contiguous B never ran the AGPR
            # kernel; tune (3, 12) tries the four-wave kernels after it; ring configs 6-9 fall
            # back to 128 x 128 tiles for the layouts they have no instance for
            assert ((old.startswith("gemm_w4x_kernel") and r["a_mn"] and not r["b_mn"])
                    or (s == "3:12" and new.startswith("gemm_w4"))
                    or (s in ("2:6", "2:7", "2:8", "2:9") and (r["a_mn"] or r["b_mn"])
                        and new.startswith("gemm_ring_kernel<128, 128, 2, 2, 4, 1"))), (r, cell, old, new)
