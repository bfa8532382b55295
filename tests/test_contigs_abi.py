"""CPU-side checks of the contig-layout boundary (pgx_align_batch2, pgx_contigs_resident, pgx_contigs_chunk): the header compiles, the
symbols are exported, a call without pgx_init answers PGX_ESTATE, and the golden fixture is what a numpy statement of the layout over the
oracle's ovlp_match gives."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contig_util as CU
import oracle_util as U
from peregrine_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "contig_cases.npz")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_compiles_and_the_structs_have_the_mirrored_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pgx_align_key2), '
                   'offsetof(pgx_align_key2, t_off), offsetof(pgx_align_key2, dir0), sizeof(pgx_tile_row), offsetof(pgx_tile_row, s), '
                   'offsetof(pgx_tile_row, strand0)); return (int)(sizeof(&pgx_contigs_chunk) + sizeof(&pgx_contigs_resident) + sizeof(&pgx_align_batch2)) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    K, R = _lib.ALIGN_KEY2_DTYPE, _lib.TILE_ROW_DTYPE
    want = [K.itemsize, K.fields["t_off"][1], K.fields["dir0"][1], R.itemsize, R.fields["s"][1], R.fields["strand0"][1]]
    assert want == [20, 12, 16, 24, 12, 20]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_new_symbols_are_exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for name in ("pgx_align_batch2", "pgx_contigs_resident", "pgx_contigs_chunk"):
        assert name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    exe = os.path.join(ROOT, "bin", "native", "path_to_contig.py")
    assert os.path.exists(exe), "build() did not produce bin/native/path_to_contig.py"
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"seqdb_prefix tiling_path" in r.stderr and r.stdout == b""


def test_calls_without_init_answer_estate(tmp_path):
    """in a fresh process (pgx_init never called there): every new entry point answers PGX_ESTATE and touches nothing"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "t, l, off = C.c_void_p(), C.c_uint64(0), (C.c_uint64 * 2)()\n"
            "a = lib.pgx_align_batch2(None, None, 0, 100, None)\n"
            "b = lib.pgx_contigs_resident(None, None, 0, 0, C.byref(t), off, C.byref(l))\n"
            "c = lib.pgx_contigs_chunk(b'nothing', b'nothing.path', %r, None, None)\n"
            "print(a, b, c, lib.pgx_last_error().decode())\n") % (ROOT, str(tmp_path / "out.fa").encode())
    out = subprocess.check_output([os.sys.executable, "-c", code], text=True)
    assert out.split()[:3] == [str(_lib.PGX_ESTATE)] * 3 and "pgx_init" in out, out
    assert not (tmp_path / "out.fa").exists()


def test_fixture_is_the_layout_over_the_oracle():
    """the stored reference output, re-derived: liboracle.so's ovlp_match + the numpy statement of the layout"""
    g = np.load(GOLDEN)
    db = CU.make_db()
    assert CU.seqdb_sha256(db) == str(g["seqdb_sha256"])
    for tag in ("bio", "adv"):
        text = str(g["path_" + tag])
        assert CU.layout(db, text, U.orc_ovlp_match) == g["fasta_" + tag].tobytes(), tag
    rows, names = CU.parse_path(str(g["path_adv"]))
    assert names == ["advA", "one", "advB"] and [r[0] for r in rows] != sorted(r[0] for r in sorted(rows, key=lambda r: r[7]))[::-1]
    assert sum(1 for r in rows if r[0] == 1) == 1                                         # a one-row contig
    assert [r[0] for r in sorted(rows, key=lambda r: r[7])][-1] == 0                        # advA comes back at the end of the file
