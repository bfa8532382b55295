"""The tiling-path entry points without a GPU: declared in include/pgx.h, exported by libpgx.so, listed in _lib.EXPORTS; pgx_tiling_stats_t
as a C compiler lays it out equals shimmer._TILING_STATS; without a device context the builders answer PGX_ESTATE and write nothing;
pgx_tiling_free(NULL) is accepted."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_sgraph_parse", "pgx_tiling_build", "pgx_tiling_stats", "pgx_tiling_rows", "pgx_tiling_names", "pgx_tiling_text", "pgx_tiling_contigs", "pgx_tiling_free", "pgx_tiling_chunk")
STATS = ("sg_lines", "g_edges", "utg_simple", "utg_contained", "utg_compound", "ctg_kept", "ctg_skipped", "ctg_empty", "p_rows", "a_rows", "alternates",
         "compound_tie_rounds", "host_us")


def _lib_built():
    from peregrine_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_entry_points_are_declared_exported_and_listed():
    _lib = _lib_built()
    lib = _lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pgx.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, hdr) and n in _lib.EXPORTS and getattr(lib, n).argtypes, n
    from peregrine_amd import shimmer
    for name in ("TilingPaths", "graph_to_path", "parse_sg_edges_list", "TILING_FILES"):
        assert hasattr(shimmer, name), name
    assert hasattr(shimmer.StringGraph, "tiling")
    for m in ("rows", "names", "text", "write", "contigs", "close"):
        assert hasattr(shimmer.TilingPaths, m), m
    assert os.access(os.path.join(ROOT, "bin", "graph_to_path.py"), os.X_OK)
    assert "graph_to_path.py" in re.search(r"^TOOLS := (.*)$", open(os.path.join(ROOT, "peregrine_amd", "csrc", "Makefile")).read(), re.M).group(1).split()


def test_struct_layout_matches_the_python_mirror(tmp_path):
    from peregrine_amd import shimmer
    src = tmp_path / "sz.c"
    prints = "".join('  printf("%%zu\\n", offsetof(pgx_tiling_stats_t, %s));\n' % f for f in STATS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) {\n  printf("%zu\\n%zu\\n", sizeof(pgx_tiling_stats_t), sizeof(pgx_tile_row));\n'
                   + prints + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    assert shimmer._TILING_STATS == STATS
    assert got == [8 * len(STATS), 24] + [8 * k for k in range(len(STATS))]


def test_without_a_device_context_the_builders_answer_estate(tmp_path):
    _lib = _lib_built()
    for fn in ("sg", "utg", "ctg"):
        (tmp_path / fn).write_text("")
    code = ("import ctypes as C, sys\nfrom peregrine_amd import _lib\nlib = _lib.load()\nd = sys.argv[1].encode()\n"
            "t, e, n = C.c_void_p(0xDEAD0000BEEF), C.c_void_p(0xDEAD0000BEEF), C.c_uint64(7)\n"
            "print(lib.pgx_tiling_build(d + b'/sg', None, b'', 0, b'', 0, C.byref(t)), t.value, lib.pgx_last_error().decode())\n"
            "print(lib.pgx_sgraph_parse(d + b'/sg', C.byref(e), None, C.byref(n)), e.value, n.value, lib.pgx_last_error().decode())\n"
            "print(lib.pgx_tiling_chunk(d + b'/sg', d + b'/utg', d + b'/ctg', d + b'/p', d + b'/a', None), lib.pgx_last_error().decode())\n"
            "print(lib.pgx_tiling_free(None))\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         env=dict(os.environ, PGX_NO_TORCH="1", PYTHONPATH=ROOT), timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0].startswith("%d None pgx_tiling_build: no device context" % _lib.PGX_ESTATE), out.stdout
    assert lines[1].startswith("%d None 0 pgx_sgraph_parse: no device context" % _lib.PGX_ESTATE), out.stdout
    assert lines[2].startswith("%d pgx_tiling_chunk: no device context" % _lib.PGX_ESTATE) and lines[3] == "0", out.stdout
    assert not (tmp_path / "p").exists() and not (tmp_path / "a").exists()
