"""CPU-side checks of the compaction entry points (pgx_seqdb_compact_bytes, pgx_seqdb_side_bytes, pgx_seqdb_read_bytes): declared, exported,
bound -- and no CPU fallback: without a GPU they fail loudly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from peregrine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_seqdb_compact_bytes", "pgx_seqdb_side_bytes", "pgx_seqdb_read_bytes")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_compaction_symbols_are_declared_exported_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for n in NAMES:
        assert n in _lib.EXPORTS and n in exported and re.search(r"\b%s\s*\(" % n, hdr), n
        assert getattr(lib, n).argtypes, n
    assert lib.pgx_seqdb_side_bytes.restype is C.c_uint64
    from peregrine_amd.shimmer import ResidentDB
    assert callable(ResidentDB.compact_bytes) and isinstance(ResidentDB.side_bytes, property)
    assert lib.pgx_seqdb_side_bytes(None) == 0          # (a null database holds nothing; no device needed to say so)


def test_compaction_has_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.pgx_init(0) != 0
    assert lib.pgx_seqdb_compact_bytes(None) == _lib.PGX_ESTATE and b"pgx_init" in lib.pgx_last_error()
    out = np.zeros(8, np.uint8)
    assert lib.pgx_seqdb_read_bytes(None, 0, out.ctypes.data_as(C.c_void_p), 8) == _lib.PGX_ESTATE
    from peregrine_amd import formats
    from peregrine_amd.shimmer import ResidentDB
    enc = np.array([0x81, 0x42, 0x24, 0x18] * 8, np.uint8)
    db = formats.SeqDB(enc, np.zeros(1, np.uint32), np.array([len(enc)], np.uint32), np.zeros(1, np.uint64), None)
    _lib._inited = None
    with pytest.raises(_lib.PgxError):
        ResidentDB(db, 0).compact_bytes()
