"""CPU-side checks of the consensus job's boundary (pgx_cns_layout, pgx_cns_job_resident, pgx_cns_job): the header compiles, the structs
have the layout the ctypes and numpy mirrors assume, the symbols are declared, listed with argument types and exported, a call without
pgx_init answers PGX_ESTATE, the tool is one of the native drop-ins and both drop-ins print their usage without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import cnsjob_util as J
from peregrine_amd import _lib, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pgx_cns_layout", 8), ("pgx_cns_job_resident", 14), ("pgx_cns_job", 7))
USAGE = b"Usage: pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_compiles_and_the_structs_have_the_mirrored_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(pgx_cns_job_piece), sizeof(pgx_cns_job_read), offsetof(pgx_cns_job_piece, read_first), offsetof(pgx_cns_job_read, read_shift), '
                   'sizeof(pgx_cns_job_stats), offsetof(pgx_cns_job_stats, text_bytes), offsetof(pgx_cns_job_stats, stitch_ms), '
                   'offsetof(pgx_cns_job_stats, align), offsetof(pgx_cns_job_stats, call)); '
                   'return (int)(sizeof(&pgx_cns_layout) + sizeof(&pgx_cns_job_resident) + sizeof(&pgx_cns_job)) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    P, R, S = _lib.CNS_JOB_PIECE_DTYPE, _lib.CNS_JOB_READ_DTYPE, _lib.CnsJobStats
    want = [P.itemsize, R.itemsize, P.fields["read_first"][1], R.fields["read_shift"][1], C.sizeof(S), S.text_bytes.offset, S.stitch_ms.offset, S.align.offset,
            S.call.offset]
    assert want[:4] == [32, 16, 20, 8]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert P == J.JOB_PIECE_DTYPE and R == J.JOB_READ_DTYPE


def test_new_symbols_are_declared_listed_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for name, nargs in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert "pgx_cns_job_stats" in hdr
    assert callable(shimmer.cns_layout) and callable(shimmer.pg_asm_cns) and callable(shimmer.cns_job_resident)


def test_calls_without_init_answer_estate():
    """in a fresh process (pgx_init never called there): the three entry points answer PGX_ESTATE and touch nothing"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "p, r, n, m = C.c_void_p(), C.c_void_p(), C.c_uint64(7), C.c_uint64(7)\n"
            "a = lib.pgx_cns_layout(None, 0, None, 0, C.byref(p), C.byref(n), C.byref(r), C.byref(m))\n"
            "b = lib.pgx_cns_job_resident(None, None, None, 0, 1, 0, None, None, 0, C.byref(p), C.byref(r), C.byref(n), C.byref(m), None)\n"
            "c = lib.pgx_cns_job(b'x', b'y', b'z', 1, 0, None, None)\n"
            "print(a, b, c, p.value, r.value, n.value, m.value, lib.pgx_last_error().decode())\n") % (ROOT,)
    out = subprocess.check_output([sys.executable, "-c", code], text=True)
    assert out.split()[:7] == [str(_lib.PGX_ESTATE)] * 3 + ["None", "None", "7", "7"] and "pgx_init" in out, out


def test_the_tool_is_a_native_drop_in_and_both_print_their_usage(lib):
    mk = open(os.path.join(ROOT, "peregrine_amd", "csrc", "Makefile")).read()
    tools = re.search(r"^TOOLS := (.*)$", mk, flags=re.M).group(1).split()
    assert "pg_asm_cns.py" in tools
    native = os.path.join(ROOT, "bin", "native", "pg_asm_cns.py")
    assert os.path.islink(native) and os.readlink(native) == "pgx_cli", "build() did not link bin/native/pg_asm_cns.py"
    r = subprocess.run([os.path.join(ROOT, "bin", "native", "pgx_cli")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"pg_asm_cns.py" in r.stderr
    for exe in ([native], [sys.executable, os.path.join(ROOT, "bin", "pg_asm_cns.py")]):
        for args in ([], ["a", "b", "c", "3"], ["a", "b", "c", "x", "0"]):
            r = subprocess.run(exe + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(USAGE), (exe, args, r.stderr)
