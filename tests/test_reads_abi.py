"""The read-database builder at the drop-in boundary: declared in include/pgx.h, exported through libpgx.map, listed in _lib.EXPORTS, with
their ctypes argument types set; without a GPU every entry point answers an error code and a message."""
import ctypes as C
import os
import re
import subprocess

import pytest

from peregrine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_seqdb_builder_open", "pgx_seqdb_builder_feed", "pgx_seqdb_builder_finish", "pgx_seqdb_builder_close", "pgx_seqdb_from_files",
         "pgx_seqdb_read_lengths")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_prototypes_are_in_the_header():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    for proto in ("typedef struct pgx_seqdb_builder pgx_seqdb_builder;",
                  "int pgx_seqdb_builder_open(uint64_t reserve_bases, pgx_seqdb_builder **out);",
                  "int pgx_seqdb_builder_feed(pgx_seqdb_builder *b, const char *text, size_t len, int on_device, int ends_file);",
                  "int pgx_seqdb_builder_finish(pgx_seqdb_builder *b, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads, "
                  "uint64_t *n_bases);",
                  "void pgx_seqdb_builder_close(pgx_seqdb_builder *b);",
                  "int pgx_seqdb_from_files(const char *seq_dataset_path, pgx_seqdb **out, char **names, size_t *names_len, uint64_t *n_reads, "
                  "uint64_t *n_bases);",
                  "int pgx_seqdb_read_lengths(const pgx_seqdb *db, uint32_t *rlen_by_rid, size_t cap);"):
        assert proto in flat, proto


def test_symbols_are_exported_and_listed(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for n in NAMES:
        assert n in _lib.EXPORTS and n in exported and hasattr(lib, n), n


def test_ctypes_argument_types_are_set(lib):
    assert lib.pgx_seqdb_builder_open.argtypes == [C.c_uint64, C.c_void_p]
    assert lib.pgx_seqdb_builder_feed.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    assert lib.pgx_seqdb_builder_finish.argtypes == [C.c_void_p] * 6
    assert lib.pgx_seqdb_builder_close.argtypes == [C.c_void_p] and lib.pgx_seqdb_builder_close.restype is None
    assert lib.pgx_seqdb_from_files.argtypes == [C.c_char_p] + [C.c_void_p] * 5
    assert lib.pgx_seqdb_read_lengths.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t]


def test_python_surface_exists():
    from peregrine_amd import shimmer
    assert callable(shimmer.ResidentDB.from_reads) and callable(shimmer.ResidentDB.save) and callable(shimmer.assemble)
    src = open(os.path.join(ROOT, "bin", "pg_asm")).read()
    assert "--reads-on-gpu" in src and "from_reads" in src


def test_null_arguments_are_refused_with_a_message(lib):
    """with or without a device: nothing is dereferenced, every call answers a code and says why"""
    lib.pgx_seqdb_builder_close(None)
    assert lib.pgx_seqdb_read_lengths(None, None, 0) != 0 and b"pgx_seqdb_read_lengths" in lib.pgx_last_error()
    assert lib.pgx_seqdb_builder_open(0, None) != 0 and b"pgx_seqdb_builder_open" in lib.pgx_last_error()


def test_no_cpu_fallback_without_gpu(lib, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.pgx_init(0) != 0
    b, h, names, nl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t(0)

    def says_why():
        return any(w in lib.pgx_last_error() for w in (b"device", b"HIP", b"pgx_init"))
    assert lib.pgx_seqdb_builder_open(1 << 20, C.byref(b)) != 0 and not b.value
    assert b"pgx_seqdb_builder_open" in lib.pgx_last_error() and b"device" in lib.pgx_last_error()
    text = b"@r\nACGT\n+\nIIII\n"
    for rc in (lib.pgx_seqdb_builder_feed(None, text, len(text), 0, 1),
               lib.pgx_seqdb_builder_finish(None, C.byref(h), C.byref(names), C.byref(nl), None, None)):
        assert rc != 0 and says_why()
    fq = tmp_path / "r.fq"
    fq.write_bytes(text)
    (tmp_path / "r.lst").write_text(str(fq) + "\n")
    assert lib.pgx_seqdb_from_files(os.fsencode(str(tmp_path / "r.lst")), C.byref(h), C.byref(names), C.byref(nl), None, None) != 0
    assert not h.value and says_why()
    from peregrine_amd import shimmer
    _lib._inited = None
    with pytest.raises(_lib.PgxError):
        shimmer.ResidentDB.from_reads([text])
    _lib._inited = None
    with pytest.raises(_lib.PgxError):
        shimmer.ResidentDB.from_reads(str(tmp_path / "r.lst"))
