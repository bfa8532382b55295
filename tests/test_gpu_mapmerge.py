"""The map merge on the GPU (pgx_map_merge_dev / _rows / pgx_map_merge, shmr_map_merge) against the rule of tests/mapmerge_util.py, byte
for byte: digit-length boundaries in every field, run lengths around the bounds of the three tie paths (the stats say which path took
which rows), runs placed every way, the file level with its pieces, its drop-ins and each of its refusals, the fixture GNU sort wrote, the
consensus job behind the merge, the whole branch in one process, and shmr_map's rows in place of its text."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cnsjob_util as J
import golden_util as G
import mapmerge_util as M
from peregrine_amd import _lib, formats, shimmer, simreads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = [os.path.join(ROOT, "bin", "native", "shmr_map_merge")]
SCRIPT = [sys.executable, os.path.join(ROOT, "bin", "shmr_map_merge")]
pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _merge_rows(lines, **env):
    """(the merged lines, the stats) of the rows form"""
    st = {}
    with _env(**env):
        out = shimmer.map_merge(M.rows_of(lines), stats=st)
    return M.lines_of(out), st


def _merge_files(tmp_path, texts, name="merged.out", **env):
    """(the merged file's bytes, the stats) of the file form over files holding `texts`"""
    paths = []
    for k, t in enumerate(texts):
        paths.append(str(tmp_path / f"in_{name}_{k}.dat"))
        open(paths[-1], "wb").write(t)
    out = str(tmp_path / name)
    with _env(**env):
        st = shimmer.map_merge(paths, out=out)
    return open(out, "rb").read(), st


def test_digit_boundaries_in_every_field(tmp_path):
    rng = np.random.default_rng(20261102)
    lines = M.boundary_lines(rng, 3000)
    want = M.rule_sorted(lines)
    assert want != sorted(lines, key=lambda l: [int(x) for x in l.split()])   # text order and numeric order disagree here
    got, st = _merge_rows(lines)
    assert got == want and st["n_rows"] == 3000 and st["n_runs"] == len({tuple(l.split()[:2]) for l in lines})
    text, st = _merge_files(tmp_path, [M.text_of(lines)])
    assert text == M.text_of(want) and st["n_rows"] == 3000


@pytest.mark.parametrize("run_max,lengths", [(128, [1, 2, 63, 64, 65, 127, 128, 129]), (None, [1, 64, 65, 1023, 1024, 1025])])
def test_run_lengths_reach_every_tie_path(run_max, lengths):
    rng = np.random.default_rng(20261103)
    lines = M.run_lines(rng, lengths)
    got, st = _merge_rows(lines, **({"PGX_MERGE_RUN_MAX": run_max} if run_max else {}))
    assert got == M.rule_sorted(lines)
    bound = run_max or 1024
    assert st["rows_wave"] == sum(n for n in lengths if 2 <= n <= 64) > 0
    assert st["rows_group"] == sum(n for n in lengths if 64 < n <= bound) > 0
    assert st["rows_lsd"] == sum(n for n in lengths if n > bound) > 0
    assert (st["n_runs"], st["n_tie_runs"], st["longest_run"]) == (len(lengths), sum(n > 1 for n in lengths), max(lengths))


def test_runs_placed_every_way():
    rng = np.random.default_rng(20261104)
    for n, path in ((40, "rows_wave"), (100, "rows_group"), (300, "rows_lsd")):   # one run that is the whole input
        lines = M.run_lines(rng, [n], wide=True)
        got, st = _merge_rows(lines, PGX_MERGE_RUN_MAX=128)
        assert got == M.rule_sorted(lines) and st[path] == n and st["n_runs"] == 1
    for n in (50, 100, 200):   # all lines identical
        lines = ["3 14 15 9 2 6 1 5 3"] * n
        assert _merge_rows(lines, PGX_MERGE_RUN_MAX=128)[0] == lines
    for differ in ((8,), (2,)):   # runs that differ in the last field only, and in the first tie field only
        lines = M.run_lines(rng, [30, 64, 90, 140, 1, 200], differ=differ)
        got, st = _merge_rows(lines, PGX_MERGE_RUN_MAX=128)
        assert got == M.rule_sorted(lines) and st["rows_lsd"] == 340
    lines = M.run_lines(rng, [200, 3, 150, 1, 129, 70])   # several long runs beside the others
    got, st = _merge_rows(lines, PGX_MERGE_RUN_MAX=128)
    assert got == M.rule_sorted(lines) and st["rows_lsd"] == 479
    got, st = _merge_rows(lines, PGX_MERGE_RUN_MAX=1)   # the hook at 1: every tie run through the LSD sort
    assert got == M.rule_sorted(lines) and (st["rows_wave"], st["rows_group"], st["rows_lsd"]) == (0, 0, 552)
    got, st = _merge_rows(lines, PGX_MERGE_RUN_MAX=10)   # below 64 it bounds the wavefront's runs too
    assert got == M.rule_sorted(lines) and (st["rows_wave"], st["rows_group"], st["rows_lsd"]) == (3, 0, 549)
    assert _merge_rows([])[0] == [] and _merge_rows(["7 7 7 7 7 7 7 7 7"])[0] == ["7 7 7 7 7 7 7 7 7"]
    lines = M.mapped_lines(rng, 20000)   # as a job has them: about 30 rows a run
    got, st = _merge_rows(lines)
    assert got == M.rule_sorted(lines) and st["rows_wave"] > 15000


def test_rows_on_the_device_and_the_rows_forms_refusals():
    import torch
    rng = np.random.default_rng(20261105)
    lines = M.boundary_lines(rng, 500) + M.run_lines(rng, [70, 200])
    rows = M.rows_of(lines)
    d_in = torch.from_numpy(rows.astype(np.uint32).view(np.int32)).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    st = _lib.MapMergeStats()
    with _env(PGX_MERGE_RUN_MAX=128):
        _lib.check(_lib.load().pgx_map_merge_dev(C.c_void_p(d_in.data_ptr()), len(rows), C.c_void_p(d_out.data_ptr()), C.byref(st)), "pgx_map_merge_dev")
    assert M.lines_of(d_out.cpu().numpy().view(np.uint32).astype(np.int64)) == M.rule_sorted(lines)
    assert st.n_rows == len(rows) and st.rows_lsd == 200
    for bad in (-1, 1 << 32):
        wrong = rows.copy()
        wrong[123, 4] = bad
        with pytest.raises(_lib.PgxError) as e:
            shimmer.map_merge(wrong)
        assert "code -6" in str(e.value) and "pgx_map_merge_rows" in str(e.value) and "row 123 " in str(e.value), str(e.value)
    assert M.lines_of(shimmer.map_merge(rows)) == M.rule_sorted(lines)


def test_files_pieces_and_drop_ins_give_the_same_bytes(tmp_path):
    rng = np.random.default_rng(20261106)
    lines = M.boundary_lines(rng, 400) + M.mapped_lines(rng, 1500)
    a, b = lines[:700], lines[700:]
    texts = [M.text_of(a), b"", M.text_of(b)[:-1]]   # one file empty, one without its last newline
    want = M.text_of(M.rule_sorted(lines))
    got, st = _merge_files(tmp_path, texts)
    assert got == want and st["n_rows"] == len(lines)
    for piece in (64, 1000, 4096):   # lines straddle the pieces of the file; the text leaves in pieces too
        assert _merge_files(tmp_path, texts, name=f"piece{piece}.out", PGX_MERGE_PIECE=piece)[0] == want, piece
    paths = [str(tmp_path / f"in_merged.out_{k}.dat") for k in range(3)]
    for exe in (NATIVE, SCRIPT):
        out = str(tmp_path / "tool.out")
        r = subprocess.run(exe + paths + ["-o", out], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want, (exe, r.stderr[-500:])
        os.remove(out)
        r = subprocess.run(exe + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0 and r.stdout == want, (exe, r.stderr[-500:])
        r = subprocess.run(exe, input=b"".join(texts), stdout=subprocess.PIPE, stderr=subprocess.PIPE)   # the pipeline's `cat ... |` form
        assert r.returncode == 0 and r.stdout == want, (exe, r.stderr[-500:])
    for none in ([b"", b""], []):   # no rows at all: an empty output file
        got, st = _merge_files(tmp_path, none, name="none.out")
        assert got == b"" and st["n_rows"] == 0


REFUSED = (("sign", "1 2 -3 4 5 6 0 8 9"), ("plus", "1 2 +3 4 5 6 0 8 9"), ("leading zero", "1 2 03 4 5 6 0 8 9"), ("tab", "1 2\t3 4 5 6 0 8 9"),
           ("carriage return", "1 2 3 4 5 6 0 8 9\r"), ("blank line", ""), ("eight fields", "1 2 3 4 5 6 0 8"), ("ten fields", "1 2 3 4 5 6 0 8 9 10"),
           ("2^32", "1 2 3 4294967296 5 6 0 8 9"), ("two blanks", "1 2  3 4 5 6 0 8 9"), ("a blank in front", " 1 2 3 4 5 6 0 8 9"),
           ("a blank behind", "1 2 3 4 5 6 0 8 9 "), ("a word", "1 2 x 4 5 6 0 8 9"), ("eleven digits", "1 2 10000000000 4 5 6 0 8 9"))


@pytest.mark.parametrize("what,bad", REFUSED, ids=[w for w, _ in REFUSED])
def test_each_refusal_names_the_file_and_the_line_and_writes_nothing(tmp_path, what, bad):
    rng = np.random.default_rng(20261107)
    good = M.mapped_lines(rng, 300)
    first, second = str(tmp_path / "first.dat"), str(tmp_path / "second.dat")
    open(first, "wb").write(M.text_of(good[:100]))
    open(second, "wb").write(M.text_of(good[100:217] + [bad] + good[217:]))
    out = str(tmp_path / "never.out")
    for env in ({}, {"PGX_MERGE_PIECE": 512}):
        with _env(**env), pytest.raises(_lib.PgxError) as e:
            shimmer.map_merge([first, second], out=out)
        msg = str(e.value)
        assert "code -6" in msg and "pgx_map_merge" in msg and f"{second}: line 117 " in msg, msg
        assert not os.path.exists(out)
    r = subprocess.run(NATIVE + [first, second], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout == b"" and b"second.dat: line 117 " in r.stderr, r.stderr
    r = subprocess.run(SCRIPT + ["-o", out], input=M.text_of([bad] + good), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stdout == b"" and b"<stdin>: line 0 " in r.stderr and not os.path.exists(out), r.stderr
    # ... and the library goes on
    shimmer.map_merge([first], out=out)
    assert open(out, "rb").read() == M.text_of(M.rule_sorted(good[:100]))


def test_the_fixture_merges_to_gnu_sorts_file(tmp_path):
    maps, merged = M.load_fixture()
    got, st = _merge_files(tmp_path, maps)
    assert got == merged and st["n_rows"] == merged.count(b"\n")
    rows = np.concatenate([M.rows_of(m.decode().splitlines()) for m in maps])
    assert M.text_of(M.lines_of(shimmer.map_merge(rows))) == merged


def test_the_consensus_job_behind_the_merge(tmp_path):
    """the `edges` case of cnsjob_cases.npz: its map lines dealt into 3 files, merged, and pg_asm_cns on the result for chunk 3_0 against the
    CPU restatement on the rule-sorted text"""
    case = next(c for c in J.load_cases() if c.name == "edges")
    lines = case.map_text.splitlines()
    merged, _ = _merge_files(tmp_path, [M.text_of(lines[k::3]) for k in range(3)], name="reads2ref_all.out")
    want_map = M.text_of(M.rule_sorted(lines))
    assert merged == want_map
    rp, cp = str(tmp_path / "reads"), str(tmp_path / "ref")
    formats.write_seqdb(rp, case.read_db)
    formats.write_seqdb(cp, case.ref_db)
    out = str(tmp_path / "cns_3_0.fa")
    shimmer.pg_asm_cns(rp, cp, str(tmp_path / "reads2ref_all.out"), 3, 0, out=out)
    assert open(out, "rb").read() == J.job(case.read_db, case.ref_db, want_map.decode(), 3, 0)


@pytest.fixture(scope="module")
def branch_files(tmp_path_factory):
    """the tiny set's reads with their two-chunk level-2 index, and three contigs of the reads' genome with theirs, as files: the inputs of
    test_gpu_parity's map test with the contigs' database beside them"""
    d = tmp_path_factory.mktemp("branch")
    q, mmers, mc, rlen = G.query_fixture()
    t = G.load("tiny_stage.npz")
    pre, sp = str(d / "sd"), str(d / "ix-L2")
    (d / "sd.seqdb").write_bytes(t["seqdb"].tobytes())
    (d / "sd.idx").write_bytes(t["idx_text"].tobytes())
    for c in (1, 2):
        formats.write_mmlist(f"{sp}-{c:02d}-of-02.dat", t[f"ix2l2_L2_{c}"])
        m = np.zeros(len(t[f"ix2l2_L2MC_{c}"]), formats.MC_DTYPE)
        m["mer"], m["count"] = t[f"ix2l2_L2MC_{c}"][:, 0], t[f"ix2l2_L2MC_{c}"][:, 1]
        formats.write_mm_count(f"{sp}-MC-{c:02d}-of-02.dat", m)
    formats.write_mmlist(str(d / "ref-L2-01-of-01.dat"), q["ref_l2"])
    cfg = dict(simreads.WORKLOADS["tiny"])
    g = simreads.make_genome(cfg["genome_len"], cfg["genome_seed"])
    contigs = [g[:30000], (3 - g[24000:])[::-1], g[10000:10900]]   # (tests/golden/make_golden_query.py)

    def enc(codes):
        codes = np.asarray(codes, np.uint8)
        return ((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4))).astype(np.uint8)

    lens = np.array([len(c) for c in contigs], np.uint32)
    assert np.array_equal(lens, q["ref_rlen"])
    formats.write_seqdb(str(d / "ref"), formats.SeqDB(np.concatenate([enc(c) for c in contigs]), np.arange(3, dtype=np.uint32), lens,
                                                       np.concatenate([[0], np.cumsum(lens.astype(np.uint64))[:-1]]).astype(np.uint64), ["ctg0", "ctg1", "ctg2"]))
    return dict(q=q, mmers=mmers, mc=mc, rlen=rlen, reads=pre, read_index=sp, ctg=str(d / "ref"), ctg_index=str(d / "ref-L2"), dir=d)


def test_map_rows_are_shmr_maps_lines(branch_files):
    f = branch_files
    for (c, T, lo, hi) in ((1, 1, 1, 240), (2, 2, 1, 240), (1, 1, 2, 4)):
        want = f["q"][f"map_c{c}t{T}lo{lo}hi{hi}"].tobytes()
        rows = shimmer.map_rows(f["ctg_index"], f["reads"], f["read_index"], f["ctg"], T, c, lo, hi)
        assert rows.dtype == np.int64 and rows.shape == (want.count(b"\n"), 9) and M.text_of(M.lines_of(rows)) == want, (c, T, lo, hi)
        rows2 = shimmer.map_rows_of(f["q"]["ref_l2"], f["mmers"], f["mc"], f["rlen"], T, c, lo, hi)
        assert np.array_equal(rows2, rows)
        assert shimmer.shmr_map(f["ctg_index"], f["reads"], f["read_index"], f["ctg"], T, c, lo, hi)[0] == want   # the text path as it was


def test_consensus_branch_equals_the_commands_one_by_one(branch_files, tmp_path):
    f = branch_files
    n_map, n_cns = 3, 2
    paths = []
    for c in range(1, n_map + 1):   # shmr_map per chunk, the merge, pg_asm_cns per chunk: the pipeline's files
        paths.append(str(tmp_path / f"reads2ref-{c:02d}.dat"))
        shimmer.shmr_map(f["ctg_index"], f["reads"], f["read_index"], f["ctg"], n_map, c, out_path=paths[-1])
    merged = str(tmp_path / "reads2ref_all.out")
    shimmer.map_merge(paths, out=merged)
    assert open(merged, "rb").read() == M.text_of(M.rule_sorted(b"".join(open(p, "rb").read() for p in paths).decode().splitlines()))
    want = b""
    for my in range(1, n_cns + 1):
        out = str(tmp_path / f"cns_{my}.fa")
        shimmer.pg_asm_cns(f["reads"], f["ctg"], merged, n_cns, my, out=out)
        want += open(out, "rb").read()
    assert want.count(b">") >= 2   # (both chunks answer contigs)
    assert shimmer.consensus_branch(f["reads"], f["read_index"], f["ctg"], f["ctg_index"], n_map, n_cns) == want
    out = str(tmp_path / "branch.fa")
    assert shimmer.consensus_branch(f["reads"], f["read_index"], f["ctg"], f["ctg_index"], n_map, n_cns, out=out) == len(want)
    assert open(out, "rb").read() == want
