"""CPU-side checks of the map merge's boundary (pgx_map_merge_dev, pgx_map_merge_rows, pgx_map_merge, pgx_map_rows, pgx_map_rows_chunk):
the header compiles, the stats struct has the layout its ctypes mirror assumes, the symbols are declared, listed with argument types and
exported, a call without pgx_init answers PGX_ESTATE and touches nothing, the tool is one of the native drop-ins and both drop-ins print
their usage without a GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from peregrine_amd import _lib, shimmer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = (("pgx_map_merge_dev", 4), ("pgx_map_merge_rows", 4), ("pgx_map_merge", 4), ("pgx_map_rows", 11), ("pgx_map_rows_chunk", 7))
USAGE = b"usage: shmr_map_merge [FILE...] [-o OUT]"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_header_compiles_and_the_stats_have_the_mirrored_layout(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(pgx_map_merge_stats), offsetof(pgx_map_merge_stats, longest_run), offsetof(pgx_map_merge_stats, rows_lsd), '
                   'offsetof(pgx_map_merge_stats, parse_ms), offsetof(pgx_map_merge_stats, format_ms)); '
                   'return (int)(sizeof(&pgx_map_merge_dev) + sizeof(&pgx_map_merge_rows) + sizeof(&pgx_map_merge) + sizeof(&pgx_map_rows) + '
                   'sizeof(&pgx_map_rows_chunk)) == 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    S = _lib.MapMergeStats
    want = [C.sizeof(S), S.longest_run.offset, S.rows_lsd.offset, S.parse_ms.offset, S.format_ms.offset]
    assert want == [96, 24, 48, 56, 88]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want


def test_new_symbols_are_declared_listed_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {l.split()[-1].split("@")[0] for l in out.splitlines() if l.strip()}
    for name, nargs in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in exported and name in _lib.EXPORTS and hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == nargs, name
    assert "pgx_map_merge_stats" in hdr
    assert callable(shimmer.map_merge) and callable(shimmer.map_rows) and callable(shimmer.consensus_branch)


def test_calls_without_init_answer_estate():
    """in a fresh process (pgx_init never called there): the five entry points answer PGX_ESTATE and touch nothing"""
    code = ("import ctypes as C, sys; sys.path.insert(0, %r)\n"
            "import os; os.environ['PGX_NO_TORCH'] = '1'\n"
            "from peregrine_amd import _lib; lib = _lib.load()\n"
            "st = _lib.MapMergeStats(); st.n_rows = 7\n"
            "p, n = C.c_void_p(), C.c_uint64(7)\n"
            "paths = (C.c_char_p * 1)(b'/nonexistent/x')\n"
            "a = lib.pgx_map_merge_dev(None, 0, None, C.byref(st))\n"
            "b = lib.pgx_map_merge_rows(None, 0, None, C.byref(st))\n"
            "c = lib.pgx_map_merge(paths, 1, b'/nonexistent/out', C.byref(st))\n"
            "d = lib.pgx_map_rows(None, 0, None, 0, None, 0, None, 0, None, C.byref(p), C.byref(n))\n"
            "e = lib.pgx_map_rows_chunk(b'r', b'm', b'p', b'l', None, C.byref(p), C.byref(n))\n"
            "print(a, b, c, d, e, st.n_rows, p.value, n.value, lib.pgx_last_error().decode())\n") % (ROOT,)
    out = subprocess.check_output([sys.executable, "-c", code], text=True)
    assert out.split()[:8] == [str(_lib.PGX_ESTATE)] * 5 + ["7", "None", "7"] and "pgx_init" in out, out


def test_the_tool_is_a_native_drop_in_and_both_print_their_usage(lib):
    mk = open(os.path.join(ROOT, "peregrine_amd", "csrc", "Makefile")).read()
    tools = re.search(r"^TOOLS := (.*)$", mk, flags=re.M).group(1).split()
    assert "shmr_map_merge" in tools
    native = os.path.join(ROOT, "bin", "native", "shmr_map_merge")
    assert os.path.islink(native) and os.readlink(native) == "pgx_cli", "build() did not link bin/native/shmr_map_merge"
    r = subprocess.run([os.path.join(ROOT, "bin", "native", "pgx_cli")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"shmr_map_merge" in r.stderr
    for exe in ([native], [sys.executable, os.path.join(ROOT, "bin", "shmr_map_merge")]):
        for args in (["-x"], ["a", "-o"], ["-o", "a", "-o", "b"]):
            r = subprocess.run(exe + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(USAGE), (exe, args, r.stderr)
