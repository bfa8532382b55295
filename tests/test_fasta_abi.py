"""pgx_seqdb_from_fasta and pgx_seqdb_save at the drop-in boundary: declared in include/pgx.h, exported through libpgx.map, listed in
_lib.EXPORTS, with their ctypes argument types set."""
import ctypes as C
import os
import re
import subprocess

import pytest

from peregrine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_seqdb_from_fasta", "pgx_seqdb_save")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_prototypes_are_in_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    assert ("int pgx_seqdb_from_fasta(const char *text, size_t len, int on_device, pgx_seqdb **out, char **names, size_t *names_len, "
            "uint64_t *n_reads, uint64_t *n_bases);") in flat
    assert "int pgx_seqdb_save(pgx_seqdb *db, const char *names, size_t names_len, const char *seqdb_prefix);" in flat


def test_symbols_are_exported_and_listed(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for n in NAMES:
        assert n in _lib.EXPORTS and n in exported and hasattr(lib, n), n
    m = open(os.path.join(ROOT, "peregrine_amd", "csrc", "libpgx.map")).read()
    assert "pgx_*;" in m and "local: *;" in m


def test_ctypes_argument_types_are_set(lib):
    assert lib.pgx_seqdb_from_fasta.argtypes == [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.pgx_seqdb_save.argtypes == [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p]


def test_python_surface_exists():
    from peregrine_amd import shimmer
    assert callable(shimmer.ResidentDB.from_fasta) and callable(shimmer.ResidentDB.save)
    assert callable(shimmer.polish) and callable(shimmer.assemble)
