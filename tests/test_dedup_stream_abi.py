"""The streaming shmr_dedup without a GPU: its four entry points are declared, exported and callable and there is no CPU fall-back;
the formatting torture fixture (tests/golden/dedup_format_cases.npz, the real reference's stdout) is pinned against the oracle."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import golden_util as G
import oracle_util as U
from peregrine_amd import _lib
from peregrine_amd.formats import OVLP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_dedup_open", "pgx_dedup_feed", "pgx_dedup_feed_dev", "pgx_dedup_close")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_stream_entry_points_are_declared_exported_and_callable(lib):
    import subprocess
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    exported = {ln.split()[-1].split("@")[0] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True).splitlines() if ln.strip()}
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr), n
        assert n in exported and n in _lib.EXPORTS and getattr(lib, n).argtypes, n
    assert "typedef struct pgx_dedup_stream pgx_dedup_stream;" in hdr
    # null arguments are refused before anything touches a device
    assert lib.pgx_dedup_open(0, None) == -1 and b"null" in lib.pgx_last_error()
    text, tl = C.c_void_p(), C.c_size_t(7)
    assert lib.pgx_dedup_feed(None, None, 0, C.byref(text), C.byref(tl)) == -1 and b"pgx_dedup_feed: null" in lib.pgx_last_error()
    assert lib.pgx_dedup_feed_dev(None, None, 0, C.byref(text), C.byref(tl)) == -1 and b"pgx_dedup_feed_dev: null" in lib.pgx_last_error()
    assert lib.pgx_dedup_close(None, None, None) == -1 and not text.value
    # the caller's output variables may hold anything (uninitialised, or the last feed's released text): an error clears them and
    # never reads what they held
    for fn in (lib.pgx_dedup_feed, lib.pgx_dedup_feed_dev):
        junk, jl = C.c_void_p(0xDEAD0000BEEF), C.c_size_t(123)
        assert fn(None, None, 3, C.byref(junk), C.byref(jl)) == -1 and not junk.value and jl.value == 0


def test_open_has_no_cpu_fallback(lib, monkeypatch):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.pgx_init(0) != 0
    h = C.c_void_p()
    assert lib.pgx_dedup_open(0, C.byref(h)) != 0 and not h.value
    msg = lib.pgx_last_error()
    assert b"HIP" in msg or b"device" in msg, msg
    from peregrine_amd.shimmer import DedupStream
    monkeypatch.setattr(_lib, "_inited", None)
    with pytest.raises(_lib.PgxError):
        DedupStream()


def test_format_fixture_is_the_oracles_text():
    z = G.load("dedup_format_cases.npz")
    recs, ref = z["recs"], z["text"].tobytes()
    assert recs.dtype == OVLP_DTYPE
    text, nu = U.orc_dedup(recs)
    assert text == ref and nu == ref.count(b"\n")
    prov = json.loads(str(z["provenance"]))
    assert prov["n_records"] == len(recs) and prov["n_lines"] == nu and prov["n_ties"] == 1806 and prov["n_grid"] == 1_130_250
    # what the set is there for: ties both ways, the sign of small values, the host's inf / nan, wide and negative fields, recurring pairs
    lines = ref.split(b"\n")[:-1]
    by_pair = {(int(ln.split()[0]), int(ln.split()[1])): ln.split() for ln in lines}
    m = recs["m_size"].astype(np.int64)
    d = recs["dist"].astype(np.int64)
    rid0 = (recs["y0"] >> np.uint64(32)).astype(np.int64)
    i = int(np.flatnonzero((m == 400) & (d == 1) & (rid0 >= 1000) & (rid0 < 1_000_000))[0])
    assert by_pair[int(rid0[i]), int(rid0[i]) + 1][3] == b"99.8"          # 99.75: tie, to even upwards
    i = int(np.flatnonzero((m == 80) & (d == 3) & (rid0 >= 1000) & (rid0 < 1_000_000))[0])
    assert by_pair[int(rid0[i]), int(rid0[i]) + 1][3] == b"96.2"          # 96.25: tie, to even downwards
    cols3 = {ln.split()[3] for ln in lines}
    assert {b"-0.0", b"inf", b"-inf"} <= cols3 and any(b"nan" in c for c in cols3)
    assert any(ln.startswith(b"-2147483648 ") for ln in lines) and any(ln.startswith(b"-00000001 ") for ln in lines)
    assert any(ln.split()[2] == b"-2147483647" for ln in lines) and any(ln.split()[2] == b"2147483647" for ln in lines)
    assert any(ln.split()[5].startswith(b"-") for ln in lines) and {ln.split()[-1] for ln in lines} == {b"overlap", b"contains", b"contained"}
    assert len(recs) - nu > 900                                             # recurring pairs, never printed
    assert '%0.1f' % (100.0 - 100.0 * 1 / 400) == "99.8" and '%0.1f' % (100.0 - 100.0 * 3 / 80) == "96.2"
