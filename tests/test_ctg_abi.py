"""The contig-path entry points without a GPU: declared in include/pgx.h, exported by libpgx.so, listed in _lib.EXPORTS; pgx_ctg_unitig and
pgx_ctg_paths_stats_t as a C compiler lays them out equal the numpy mirrors of shimmer.py and of tests/ctg_util.py; without a device
context the builders answer PGX_ESTATE; both forms of shmr_sgraph know --utg-data and --ctg-paths and refuse them without a file name."""
import os
import re
import subprocess
import sys

import ctg_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pgx_unitigs_contig_paths", "pgx_ctg_paths_build", "pgx_ctg_paths_stats", "pgx_ctg_paths_table", "pgx_ctg_paths_rows", "pgx_ctg_paths_utg_text",
         "pgx_ctg_paths_ctg_text", "pgx_ctg_paths_free")


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
    assert set(re.findall(r"\b(pgx_ctg_paths_[a-z_]+|pgx_unitigs_contig_paths)\s*\(", hdr)) == set(NAMES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert {ln.split()[-1] for ln in out.splitlines() if "ctg_paths" in ln or "contig_paths" in ln} == set(NAMES)
    from peregrine_amd import shimmer
    for name in ("ContigPaths", "contig_paths", "CTG_UNITIG_DTYPE", "CTG_TYPES", "CTG_NONE"):
        assert hasattr(shimmer, name), name
    assert hasattr(shimmer.Unitigs, "contig_paths")
    for m in ("table", "rows", "utg_text", "ctg_text", "write", "tiling", "close"):
        assert hasattr(shimmer.ContigPaths, m), m
    assert tuple(t.encode() for t in shimmer.CTG_TYPES) == CU.TYPE_NAMES and shimmer.CTG_NONE == CU.NONE


def test_struct_sizes_and_offsets_match_the_numpy_mirrors(tmp_path):
    from peregrine_amd import shimmer
    src = tmp_path / "sz.c"
    prints = "".join('  printf("%%zu\\n", offsetof(pgx_ctg_paths_stats_t, %s));\n' % f for f in CU.STATS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pgx.h"\nint main(void) {\n'
                   '  printf("%zu\\n%zu\\n%zu\\n%zu\\n", sizeof(pgx_ctg_unitig), offsetof(pgx_ctg_unitig, type), offsetof(pgx_ctg_unitig, dual), sizeof(pgx_ctg_paths_stats_t));\n'
                   '  printf("%d %d %d %d %d %d %u\\n", PGX_CTG_SIMPLE, PGX_CTG_SPUR2, PGX_CTG_SIMPLE_DUP, PGX_CTG_CONTAINED, PGX_CTG_REPEAT_BRIDGE, PGX_CTG_COMPOUND, PGX_CTG_NONE);\n'
                   + prints + "  return 0;\n}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    d = shimmer.CTG_UNITIG_DTYPE
    assert d == CU.CTG_UNITIG_DTYPE and shimmer._CTG_PATHS_STATS == CU.STATS
    want = [d.itemsize, d.fields["type"][1], d.fields["dual"][1], 8 * len(CU.STATS)] + [CU.SIMPLE, CU.SPUR2, CU.SIMPLE_DUP, CU.CONTAINED, CU.REPEAT_BRIDGE, CU.COMPOUND, CU.NONE] + \
        [8 * k for k in range(len(CU.STATS))]
    assert got == want and d.itemsize == 8


def test_without_a_device_context_the_builders_answer_estate():
    _lib = _lib_built()
    code = ("import ctypes as C\nfrom peregrine_amd import _lib\nlib = _lib.load()\nfor f, a in ((lib.pgx_unitigs_contig_paths, (None,)), (lib.pgx_ctg_paths_build, (None, 0))):\n"
            "    c = C.c_void_p(0xDEAD0000BEEF)\n    print(f(*a, C.byref(c)), c.value, lib.pgx_last_error().decode())\nprint(lib.pgx_ctg_paths_free(None))\n")
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=dict(os.environ, PGX_NO_TORCH="1", PYTHONPATH=ROOT), timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0].startswith("%d None pgx_unitigs_contig_paths: no device context" % _lib.PGX_ESTATE), out.stdout
    assert lines[1].startswith("%d None pgx_unitigs_build: no device context" % _lib.PGX_ESTATE) and lines[2] == "0", out.stdout


def test_both_commands_parse_the_new_flags():
    _lib_built()
    native = [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_sgraph"]
    script = [sys.executable, os.path.join(ROOT, "bin", "shmr_sgraph")]
    for cmd in (native, script):
        for flag in ("--utg-data", "--ctg-paths"):
            r = subprocess.run(cmd + [flag], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
            assert r.returncode == 2 and flag.encode() in r.stderr and r.stdout == b"", (cmd, flag, r.stderr)
        r = subprocess.run(cmd + ["--utg-dat", "x"] if cmd is native else cmd + ["--no-such", "x"], input=b"", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 2 and b"--utg-data" in r.stderr and b"--ctg-paths" in r.stderr, r.stderr      # the usage names them
