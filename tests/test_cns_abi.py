"""CPU-side checks of the consensus boundary (pgx_cns_call, pgx_cns_call_dev, pgx_cns_tags): the header compiles, the structs have the
layout the ctypes and numpy mirrors assume, the symbols are declared, listed and exported, and a call without pgx_init answers PGX_ESTATE."""
import ctypes as C
import os
import re
import subprocess

import pytest

from peregrine_amd import _lib, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_cns_call", "pgx_cns_call_dev", "pgx_cns_tags")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_compiles_and_the_structs_have_the_mirrored_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(pgx_cns_aln), offsetof(pgx_cns_aln, s2), offsetof(pgx_cns_aln, str_off), offsetof(pgx_cns_aln, str_len), sizeof(pgx_cns_tag), '
                   'offsetof(pgx_cns_tag, p_t_pos), offsetof(pgx_cns_tag, p_q_base), sizeof(pgx_cns_stats), offsetof(pgx_cns_stats, gpu_ms)); '
                   'return (int)(sizeof(&pgx_cns_call) + sizeof(&pgx_cns_call_dev) + sizeof(&pgx_cns_tags)) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    A, T, S = _lib.CNS_ALN_DTYPE, _lib.CNS_TAG_DTYPE, _lib.CnsStats
    want = [A.itemsize, A.fields["s2"][1], A.fields["str_off"][1], A.fields["str_len"][1], T.itemsize, T.fields["p_t_pos"][1], T.fields["p_q_base"][1],
            C.sizeof(S), S.gpu_ms.offset]
    assert want == [32, 12, 16, 24, 12, 4, 11, 80, 40]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_new_symbols_are_declared_listed_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
    assert callable(shimmer.consensus) and callable(shimmer.align_tags)


def test_calls_without_init_answer_estate():
    """in a fresh process (pgx_init never called there): every new entry point answers PGX_ESTATE and touches nothing"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "t, off = C.c_void_p(), (C.c_uint64 * 2)()\n"
            "a = lib.pgx_cns_call(None, 0, None, None, 0, None, 0, 1, C.byref(t), off, None)\n"
            "b = lib.pgx_cns_call_dev(None, 0, None, None, 0, None, 0, 1, C.byref(t), off, None)\n"
            "c = lib.pgx_cns_tags(None, 0, None, None, 0, C.byref(t), off)\n"
            "print(a, b, c, t.value, lib.pgx_last_error().decode())\n") % (ROOT,)
    out = subprocess.check_output([os.sys.executable, "-c", code], text=True)
    assert out.split()[:4] == [str(_lib.PGX_ESTATE)] * 3 + ["None"] and "pgx_init" in out, out
