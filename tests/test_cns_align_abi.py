"""CPU-side checks of the aligner's boundary (pgx_falcon_align, pgx_cns_pieces): the header compiles, the structs have the layout the
ctypes and numpy mirrors assume, the symbols are declared, listed with argument types and exported, and a call without pgx_init answers
PGX_ESTATE."""
import ctypes as C
import os
import re
import subprocess

import pytest

from peregrine_amd import _lib, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_falcon_align", "pgx_cns_pieces")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_compiles_and_the_structs_have_the_mirrored_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(pgx_faln_req), sizeof(pgx_faln_res), sizeof(pgx_cns_piece), sizeof(pgx_cns_read), offsetof(pgx_faln_req, band), '
                   'offsetof(pgx_faln_res, aln_t_e), offsetof(pgx_faln_res, str_off), offsetof(pgx_cns_read, read_shift), sizeof(pgx_faln_stats), '
                   'offsetof(pgx_faln_stats, gpu_ms), sizeof(pgx_cns_pieces_stats), offsetof(pgx_cns_pieces_stats, call)); '
                   'return (int)(sizeof(&pgx_falcon_align) + sizeof(&pgx_cns_pieces)) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    Q, R, P, D, S, PS = _lib.FALN_REQ_DTYPE, _lib.FALN_RES_DTYPE, _lib.CNS_PIECE_DTYPE, _lib.CNS_READ_DTYPE, _lib.FalnStats, _lib.CnsPiecesStats
    want = [Q.itemsize, R.itemsize, P.itemsize, D.itemsize, Q.fields["band"][1], R.fields["aln_t_e"][1], R.fields["str_off"][1], D.fields["read_shift"][1],
            C.sizeof(S), S.gpu_ms.offset, C.sizeof(PS), PS.call.offset]
    assert want[:4] == [32, 32, 16, 24] and want[4:8] == [24, 20, 24, 16]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert [n for n, _ in _lib.FALN_RES_DTYPE.descr[:6]] == ["aln_str_size", "dist", "aln_q_s", "aln_q_e", "aln_t_s", "aln_t_e"]


def test_new_symbols_are_declared_listed_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for name, nargs in zip(NAMES, (9, 11)):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert callable(shimmer.falcon_align) and callable(shimmer.consensus_reads)


def test_calls_without_init_answer_estate():
    """in a fresh process (pgx_init never called there): both entry points answer PGX_ESTATE and touch nothing"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "q, t, n, off = C.c_void_p(), C.c_void_p(), C.c_uint64(7), (C.c_uint64 * 2)()\n"
            "a = lib.pgx_falcon_align(None, 0, None, 0, None, C.byref(q), C.byref(t), C.byref(n), None)\n"
            "b = lib.pgx_cns_pieces(None, 0, None, 0, None, 0, 1, C.byref(t), off, None, None)\n"
            "print(a, b, q.value, t.value, n.value, lib.pgx_last_error().decode())\n") % (ROOT,)
    out = subprocess.check_output([os.sys.executable, "-c", code], text=True)
    assert out.split()[:5] == [str(_lib.PGX_ESTATE)] * 2 + ["None", "None", "7"] and "pgx_init" in out, out
