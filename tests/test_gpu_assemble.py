"""shimmer.assemble, shimmer.polish and bin/pg_asm against the existing drop-ins of bin/ run as commands on files, in the same
configuration: 3 index chunks, 2 overlap chunks, 2 mapping chunks, 2 consensus chunks, with the alternate contigs.  The commands are each
pinned to the reference by their own tests; here their chain is the expectation, byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from peregrine_amd import _lib, formats, shimmer, simreads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INDEX, N_OVLP, N_MAP, N_CNS = 3, 2, 2, 2
MC_LOWER, MC_UPPER = 2, 240   # pg_run.py hands the same two to shmr_overlap and to shmr_map


def _cmd(tool, *args, cwd=None, stdin=None):
    """a drop-in of bin/ as a command: the native multi-call binary, through its per-tool link when the link survived the copy"""
    exe = os.path.join(ROOT, "bin", "native", tool)
    cmd = [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), tool]
    return subprocess.run([*cmd, *map(str, args)], cwd=cwd, check=True, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stdout


def _chain_from_overlaps(d, sd, cat, tag, ordered):
    """shmr_sgraph ... pg_asm_cns.py in directory d/tag; answers dict(p_ctg, a_ctg, p_ctg_cns, ctg prefixes)"""
    w = d / tag
    w.mkdir()
    flags = ("--chimer_bridge_ordered",) if ordered else ()
    (w / "sg_edges_list").write_bytes(_cmd("shmr_sgraph", *flags, "--utg-data", "utg_data", "--ctg-paths", "ctg_paths", cwd=w, stdin=cat))
    _cmd("graph_to_path.py", cwd=w)
    p_ctg = _cmd("path_to_contig.py", sd, "p_ctg_tiling_path", cwd=w)
    a_ctg = _cmd("path_to_contig.py", sd, "a_ctg_tiling_path", cwd=w)
    (w / "p_ctg.fa").write_bytes(p_ctg)
    (w / "ctg.lst").write_text(str(w / "p_ctg.fa") + "\n")
    _cmd("shmr_mkseqdb", "-p", w / "ctg", "-d", w / "ctg.lst")
    _cmd("shmr_index", "-p", w / "ctg", "-t", 1, "-c", 1, "-o", w / "ctg")
    maps = []
    for c in range(1, N_MAP + 1):
        maps.append(w / f"reads2ref-{c:02d}.dat")
        maps[-1].write_bytes(_cmd("shmr_map", "-r", w / "ctg", "-m", w / "ctg-L2", "-p", sd, "-l", d / "shmr-L2", "-M", MC_UPPER, "-n", MC_LOWER, "-t", N_MAP, "-c", c))
    _cmd("shmr_map_merge", *maps, "-o", w / "reads2ref_all.out")
    cns = b"".join(_cmd("pg_asm_cns.py", sd, w / "ctg", w / "reads2ref_all.out", N_CNS, my) for my in range(1, N_CNS + 1))
    return dict(p_ctg=p_ctg, a_ctg=a_ctg, p_ctg_cns=cns, ctg=str(w / "ctg"), ctg_index=str(w / "ctg-L2"))


def read_set():
    """two haplotypes of a 300 kb genome at 12x each, the second with 9 kb inserted in the middle, so that the graph holds a bubble and the
    job alternate contigs; the error rate of tests/test_gpu_pipeline.py.  Chosen on the GPU with the drop-ins, seeds fixed: their chain
    gives one primary contig of some 320 kb, two alternate contigs and one polished contig."""
    g = simreads.make_genome(300_000, 41)
    h = np.concatenate([g[:150_000], simreads.make_genome(9_000, 44), g[150_000:]])
    a = simreads.simulate_reads(g, coverage=12.0, seed=17, mean_len=8000, sd_len=1500, err=0.01)
    b = simreads.simulate_reads(h, coverage=12.0, seed=18, mean_len=8000, sd_len=1500, err=0.01)
    rlen = np.concatenate([a.rlen, b.rlen])
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return formats.SeqDB(np.concatenate([a.seqdb, b.seqdb]), np.arange(len(rlen), dtype=np.uint32), rlen, roff, None)


def build_job(d, db):
    """the command chain's files for read set db in directory d, with and without the chimer bridge step"""
    sd = str(d / "seq_dataset")
    formats.write_seqdb(sd, db)
    for c in range(1, N_INDEX + 1):
        _cmd("shmr_index", "-p", sd, "-t", N_INDEX, "-c", c, "-o", d / "shmr")
    for c in range(1, N_OVLP + 1):
        _cmd("shmr_overlap", "-p", sd, "-l", d / "shmr-L2", "-m", MC_LOWER, "-M", MC_UPPER, "-t", N_OVLP, "-c", c, "-o", d / f"ovlp.{c:02d}")
    cat = b"".join((d / f"ovlp.{c:02d}").read_bytes() for c in range(1, N_OVLP + 1))
    out = dict(dir=d, db=db, sd=sd, read_index=str(d / "shmr-L2"))
    out["ordered"] = _chain_from_overlaps(d, sd, cat, "ordered", True)
    out["plain"] = _chain_from_overlaps(d, sd, cat, "plain", False)
    return out


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    return build_job(tmp_path_factory.mktemp("asm"), read_set())


def _lengths(fasta: bytes):
    return [len(s) for s in fasta.split(b"\n")[1::2]]


def test_the_job_has_a_long_contig_and_a_polished_one(job):
    for k in ("ordered", "plain"):
        lens, cns = _lengths(job[k]["p_ctg"]), _lengths(job[k]["p_ctg_cns"])
        print(k, "p_ctg", lens, "a_ctg", _lengths(job[k]["a_ctg"]), "p_ctg_cns", cns)
        assert max(lens, default=0) >= 50_000
        assert len(cns) >= 1 and max(cns) >= 50_000
        assert len(_lengths(job[k]["a_ctg"])) >= 1   # (with_alt compares something)


@pytest.mark.parametrize("ordered", [True, False], ids=["chimer_ordered", "chimer_off"])
def test_assemble_equals_the_commands(job, ordered, tmp_path):
    want = job["ordered" if ordered else "plain"]
    got = shimmer.assemble(job["sd"], N_INDEX, N_OVLP, N_MAP, N_CNS, with_alt=True, mc_lower=MC_LOWER, mc_upper=MC_UPPER, chimer_ordered=ordered,
                           out_dir=str(tmp_path / "out"))
    for k in ("p_ctg", "a_ctg", "p_ctg_cns"):
        assert got[k] == want[k], k
        assert (tmp_path / "out" / (k + ".fa")).read_bytes() == want[k], k
    st = got["stats"]
    assert len(st["index"]) == N_INDEX and len(st["overlap"]) == N_OVLP and st["tiling"]["ctg_kept"] >= 1
    assert set(st["ms"]) == {"load", "index", "overlap", "graph", "contigs", "polish"}


def test_assemble_without_consensus_and_alternates(job):
    got = shimmer.assemble(job["sd"], N_INDEX, N_OVLP, mc_lower=MC_LOWER, mc_upper=MC_UPPER)
    assert got["p_ctg"] == job["ordered"]["p_ctg"] and got["a_ctg"] is None and got["p_ctg_cns"] is None


def test_polish_equals_consensus_branch(job, tmp_path):
    want = shimmer.consensus_branch(job["sd"], job["read_index"], job["ordered"]["ctg"], job["ordered"]["ctg_index"], N_MAP, N_CNS, MC_LOWER, MC_UPPER)
    assert want == job["ordered"]["p_ctg_cns"]
    rdb = shimmer.ResidentDB(formats.read_seqdb(job["sd"]), 0)
    try:
        ixs = [rdb.index(N_INDEX, c) for c in range(1, N_INDEX + 1)]
        top, counts = np.concatenate([ix.top for ix in ixs]), np.concatenate([ix.top_mc for ix in ixs])
        assert shimmer.polish(rdb, top, counts, job["ordered"]["p_ctg"], N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER) == want
        out = str(tmp_path / "cns.fa")
        assert shimmer.polish(rdb, top, counts, job["ordered"]["p_ctg"], N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER, out=out) == len(want)
        assert open(out, "rb").read() == want
    finally:
        rdb.close()


def test_handles_are_closed_when_a_stage_raises(job, monkeypatch):
    """the first stage raising (the index refuses k = 99) and the last one (polish, made to raise with every handle of the job open): the
    device memory the job held is given back"""
    import gc
    gc.collect()
    shimmer.assemble(job["sd"], N_INDEX, N_OVLP, N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER)   # (the library's grow-only workspaces are at their size)
    before = _lib.mem_ledger()["live_bytes"]
    with pytest.raises(_lib.PgxError, match="w > k"):
        shimmer.assemble(job["sd"], N_INDEX, N_OVLP, N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER, kmer=99)
    assert _lib.mem_ledger()["live_bytes"] <= before

    def refuse(*a, **k):
        raise _lib.PgxError("polish refused")
    monkeypatch.setattr(shimmer, "polish", refuse)
    with pytest.raises(_lib.PgxError, match="polish refused"):
        shimmer.assemble(job["sd"], N_INDEX, N_OVLP, N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER)
    assert _lib.mem_ledger()["live_bytes"] <= before


def test_pg_asm_writes_the_same_three_files(job, tmp_path):
    fa = tmp_path / "reads.fa"
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    db = job["db"]
    with open(fa, "wb") as f:
        for r, n, o in zip(db.rid, db.rlen, db.roff):
            f.write(b">read%06d\n" % r + lut[db.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes() + b"\n")
    (tmp_path / "reads.lst").write_text(str(fa) + "\n")
    exe = [sys.executable, os.path.join(ROOT, "bin", "pg_asm")]
    r = subprocess.run([*exe, str(tmp_path / "reads.lst"), str(N_INDEX), str(N_OVLP), str(N_MAP), str(N_CNS), "--with-alt", "--output", str(tmp_path / "wd")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    for k in ("p_ctg", "a_ctg", "p_ctg_cns"):
        assert (tmp_path / "wd" / (k + ".fa")).read_bytes() == job["ordered"][k], k
    (tmp_path / "bad.lst").write_text(str(tmp_path / "no_such_file.fa") + "\n")
    r = subprocess.run([*exe, str(tmp_path / "bad.lst"), "1", "1", "--output", str(tmp_path / "bad")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"no_such_file.fa" in r.stderr
    assert not any((tmp_path / "bad" / (k + ".fa")).exists() for k in ("p_ctg", "a_ctg", "p_ctg_cns"))
