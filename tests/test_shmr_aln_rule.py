"""CPU-side checks of the shimmer chain alignment (pgx_shmr_aln_batch): the restatement of tests/shmr_aln_util.py against every case of
the fixture the real shmr_aln wrote, the fixture's provenance, and the boundary -- the symbol is declared, listed with argument types and
exported, shmr_aln itself is not, and a call without pgx_init answers PGX_ESTATE and touches nothing."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import shmr_aln_util as A
from peregrine_amd import _lib, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["empty_0", "empty_1", "empty_both", "no_shared", "one_shared", "one_shared_opposite", "rep1_at", "rep1_over", "rep3_at", "rep3_over",
         "twice_in_list1", "before_last", "diff_below", "diff_at", "dist_below", "dist_at", "tie_earlier", "later_smaller", "best_1_of_129",
         "best_64_of_129", "best_65_of_129", "best_128_of_129", "best_129_of_129", "near_2_31", "stop_4810", "no_stop_4810"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_the_restatement_gives_the_references_chains_on_every_case():
    cases = A.load_cases()
    assert [c.name for c in cases][:len(NAMES)] == NAMES
    for c in cases:
        chains, _ = A.shmr_aln(c.mm0, c.mm1, **c.params)
        assert len(chains) == len(c.chains), c.name
        for k, (mine, ref) in enumerate(zip(chains, c.chains)):
            assert mine == ref, (c.name, k)


def test_the_cases_are_what_they_are_named_for():
    by = {c.name: c for c in A.load_cases()}
    assert by["one_shared"].chains == [([1], [1])] and by["one_shared_opposite"].chains == []
    assert by["rep1_at"].chains == [([1], [0]), ([1], [2])] and by["rep3_at"].chains == [([1, 2, 3], [0, 0, 0]), ([1, 2, 3], [2, 2, 2])]
    assert by["rep1_at"].params["max_repeat"] == 1 and by["rep3_over"].params["max_repeat"] == 3 and by["rep3_over"].chains == []
    assert by["twice_in_list1"].chains == [([0, 0], [0, 1])]
    assert by["before_last"].chains == [([1], [0]), ([0], [1])]
    assert by["diff_below"].chains == [([0, 1], [0, 1])] and by["diff_at"].chains == [([0], [0]), ([1], [1])]
    assert by["dist_below"].chains == [([0, 1], [0, 1])] and by["dist_at"].chains == [([0], [0]), ([1], [1])]
    assert by["tie_earlier"].chains == [([1, 2], [0, 2]), ([0], [1])] and by["later_smaller"].chains == [([1], [0]), ([0, 2], [1, 2])]
    for k in (1, 64, 65, 128, 129):
        ch = by[f"best_{k}_of_129"].chains
        assert len(ch) == 129 and [len(a) for a, _ in ch] == [1] * (k - 1) + [2] + [1] * (129 - k) and ch[k - 1] == ([129 - k, 129], [k - 1, 129])
    assert int(A.positions(by["near_2_31"].mm0).max()) == 2**31 - 1 and by["near_2_31"].chains == [([0, 1], [0, 1]), ([2, 3], [2, 3])]
    stop, twin = by["stop_4810"], by["no_stop_4810"]
    assert len(stop.mm1) == 4810 and len(stop.chains) == 4802 and stop.chains[-1] == ([4801], [4801])   # the scan of shimmer 4,801 saw 4,801 small chains
    assert len(twin.chains) == 4810 and sum(len(a) for a, _ in twin.chains) == len(twin.mm1) == 4850 and sum(len(a) == 3 for a, _ in twin.chains) == 20
    fwd = by["real_fwd"].chains
    longest = max(fwd, key=lambda c: len(c[0]))
    d = A.positions(by["real_fwd"].mm0)[longest[0]] - A.positions(by["real_fwd"].mm1)[longest[1]]
    assert len(longest[0]) >= 20 and set(d.tolist()) == {-A.REAL["shift"]}
    assert by["real_rc"].chains == [] and len(by["real_self"].chains) == 1


def test_provenance():
    prov = json.load(open(A.PROVENANCE))
    assert prov["generator"] == "tests/golden/make_golden_shmr_aln.py" and prov["direction"] == 0 and prov["real"] == A.REAL
    assert set(prov["sources"]) == {"shmr_align.c", "shmr_utils.c", "kalloc.c", "shimmer.h", "kvec.h", "khash.h", "kalloc.h"}
    assert all(re.fullmatch(r"[0-9a-f]{64}", h) for h in prov["sources"].values())
    cases = A.load_cases()
    assert prov["cases"] == [c.name for c in cases]
    for c in cases:
        s = prov["summary"][c.name]
        assert (s["n0"], s["n1"], s["chains"], s["elements"]) == (len(c.mm0), len(c.mm1), len(c.chains), sum(len(a) for a, _ in c.chains)), c.name
    assert prov["summary"]["stop_4810"]["stopped"] is True and prov["summary"]["stop_4810"]["walked"] == 4802
    assert prov["summary"]["no_stop_4810"]["stopped"] is False
    assert hashlib.sha256(open(A.GOLDEN, "rb").read()).hexdigest() == prov["sha256"]
    assert os.path.getsize(A.GOLDEN) < 500_000


def test_the_symbol_is_declared_listed_and_exported_and_shmr_aln_is_not(lib, tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    name = "pgx_shmr_aln_batch"
    assert re.search(r"\bint %s\s*\(" % name, hdr) and "pgx_shmr_aln_pair" in hdr and "pgx_shmr_aln_stats" in hdr
    assert name in exported and name in _lib.EXPORTS and hasattr(lib, name) and len(getattr(lib, name).argtypes) == 17
    for ref_name in ("shmr_aln", "free_shmr_alns"):
        assert ref_name not in exported and ref_name not in _lib.EXPORTS and not re.search(r"\b%s\s*\(" % ref_name, hdr), ref_name
    assert callable(shimmer.shimmer_alns) and callable(shimmer.get_shimmer_alns)
    # the header compiles as C and the stats have the layout their ctypes mirror assumes
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(pgx_shmr_aln_stats), '
                   'offsetof(pgx_shmr_aln_stats, n_stopped), offsetof(pgx_shmr_aln_stats, unroll_ms), sizeof(pgx_shmr_aln_pair)); '
                   'return sizeof(&pgx_shmr_aln_batch) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    S = _lib.ShmrAlnStats
    want = [C.sizeof(S), S.n_stopped.offset, S.unroll_ms.offset, _lib.SHMR_ALN_PAIR_DTYPE.itemsize]
    assert want == [80, 40, 72, 8] and [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_a_call_without_init_answers_estate_and_touches_nothing():
    """in a fresh process (pgx_init never called there)"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "import numpy as np\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "off = np.zeros(2, np.uint64); pr = np.zeros(1, _lib.SHMR_ALN_PAIR_DTYPE)\n"
            "outs = [C.c_void_p(5) for _ in range(4)]\n"
            "st = _lib.ShmrAlnStats(); st.n_pairs = 7\n"
            "rc = lib.pgx_shmr_aln_batch(None, off.ctypes.data, 1, None, off.ctypes.data, 1, pr.ctypes.data, 1, 0, 100, 1200, 1, "
            "*[C.byref(o) for o in outs], C.byref(st))\n"
            "print(rc, st.n_pairs, *[o.value for o in outs], lib.pgx_last_error().decode())\n") % (ROOT,)
    out = subprocess.check_output([sys.executable, "-c", code], text=True)
    assert out.split()[:6] == [str(_lib.PGX_ESTATE), "7", "5", "5", "5", "5"] and "pgx_init" in out, out
