"""The unitig entry points without a GPU: declared in include/pgx.h, exported by libpgx.so, listed in _lib.EXPORTS; pgx_unitig and
pgx_unitigs_stats_t as a C compiler lays them out equal the numpy mirrors of shimmer.py; without a device context the builders answer
PGX_ESTATE."""
import os
import re
import subprocess
import sys

import utg_util as UT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_sgraph_unitigs", "pgx_unitigs_build", "pgx_unitigs_stats", "pgx_unitigs_table", "pgx_unitigs_paths", "pgx_unitigs_text", "pgx_unitigs_free")
FIELDS = ("s_rid", "t_rid", "via_rid", "s_end", "t_end", "via_end", "circular", "n_edges", "first", "length", "score")
STATS = ("g_edges", "unitigs", "circular", "longest_edges")


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
    for name in ("Unitigs", "unitigs", "read_sg_edges_list", "UNITIG_DTYPE"):
        assert hasattr(shimmer, name), name
    assert hasattr(shimmer.StringGraph, "unitigs")


def test_struct_sizes_and_offsets_match_the_numpy_mirrors(tmp_path):
    from peregrine_amd import shimmer
    src = tmp_path / "sz.c"
    prints = "".join('  printf("%%zu\\n", offsetof(pgx_unitig, %s));\n' % f for f in FIELDS) + \
        "".join('  printf("%%zu\\n", offsetof(pgx_unitigs_stats_t, %s));\n' % f for f in STATS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) {\n  printf("%zu\\n%zu\\n", sizeof(pgx_unitig), sizeof(pgx_unitigs_stats_t));\n'
                   + prints + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    d = shimmer.UNITIG_DTYPE
    assert d == UT.UNITIG_DTYPE
    want = [d.itemsize, 8 * len(shimmer._UNITIGS_STATS)] + [d.fields[f][1] for f in FIELDS] + [8 * k for k in range(len(STATS))]
    assert got == want and d.itemsize == 48 and shimmer._UNITIGS_STATS == STATS


def test_without_a_device_context_the_builders_answer_estate():
    _lib = _lib_built()
    code = ("import ctypes as C\nfrom peregrine_amd import _lib\nlib = _lib.load()\nfor f, a in ((lib.pgx_sgraph_unitigs, (None,)), (lib.pgx_unitigs_build, (None, 0))):\n"
            "    u = C.c_void_p(0xDEAD0000BEEF)\n    print(f(*a, C.byref(u)), u.value, lib.pgx_last_error().decode())\nprint(lib.pgx_unitigs_free(None))\n")
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, PGX_NO_TORCH="1", PYTHONPATH=ROOT), timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0].startswith("%d None pgx_sgraph_unitigs: no device context" % _lib.PGX_ESTATE), out.stdout
    assert lines[1].startswith("%d None pgx_unitigs_build: no device context" % _lib.PGX_ESTATE) and lines[2] == "0", out.stdout
