"""The whole job with homopolymer-compressed shimmers: shimmer.assemble(hpc=True) and bin/pg_asm --hpc against the drop-in commands
chained with -H on both index steps (reads and contigs), byte for byte, as tests/test_gpu_assemble.py does for the default."""
import os
import subprocess
import sys

import numpy as np
import pytest

from peregrine_amd import formats, shimmer, simreads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INDEX, N_OVLP, N_MAP, N_CNS = 2, 1, 1, 1
MC_LOWER, MC_UPPER = 2, 240


def _cmd(tool, *args, cwd=None, stdin=None):
    return subprocess.run([os.path.join(ROOT, "bin", "native", "pgx_cli"), tool, *map(str, args)], cwd=cwd, check=True, input=stdin,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600).stdout


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """a 100 kb genome with a few planted homopolymer runs at 15x, and the command chain's three FASTA files"""
    d = tmp_path_factory.mktemp("hpcasm")
    g = simreads.make_genome(100_000, 43)
    rng = np.random.default_rng(6)
    for n in (280, 60, 30, 20, 12, 12):
        s = int(rng.integers(0, len(g) - n))
        g[s:s + n] = int(rng.integers(0, 4))
    db = simreads.simulate_reads(g, coverage=15.0, seed=19, mean_len=7000, sd_len=1000, err=0.01)
    sd = str(d / "seq_dataset")
    formats.write_seqdb(sd, db)
    for c in range(1, N_INDEX + 1):
        _cmd("shmr_index", "-p", sd, "-t", N_INDEX, "-c", c, "-H", "-o", d / "shmr")
    cat = b""
    for c in range(1, N_OVLP + 1):
        _cmd("shmr_overlap", "-p", sd, "-l", d / "shmr-L2", "-m", MC_LOWER, "-M", MC_UPPER, "-t", N_OVLP, "-c", c, "-o", d / f"ovlp.{c:02d}")
        cat += (d / f"ovlp.{c:02d}").read_bytes()
    (d / "sg_edges_list").write_bytes(_cmd("shmr_sgraph", "--chimer_bridge_ordered", "--utg-data", "utg_data", "--ctg-paths", "ctg_paths", cwd=d, stdin=cat))
    _cmd("graph_to_path.py", cwd=d)
    p_ctg = _cmd("path_to_contig.py", sd, "p_ctg_tiling_path", cwd=d)
    (d / "p_ctg.fa").write_bytes(p_ctg)
    (d / "ctg.lst").write_text(str(d / "p_ctg.fa") + "\n")
    _cmd("shmr_mkseqdb", "-p", d / "ctg", "-d", d / "ctg.lst")
    _cmd("shmr_index", "-p", d / "ctg", "-t", 1, "-c", 1, "-H", "-o", d / "ctg")
    maps = []
    for c in range(1, N_MAP + 1):
        maps.append(d / f"reads2ref-{c:02d}.dat")
        maps[-1].write_bytes(_cmd("shmr_map", "-r", d / "ctg", "-m", d / "ctg-L2", "-p", sd, "-l", d / "shmr-L2", "-M", MC_UPPER, "-n", MC_LOWER, "-t", N_MAP, "-c", c))
    _cmd("shmr_map_merge", *maps, "-o", d / "reads2ref_all.out")
    cns = b"".join(_cmd("pg_asm_cns.py", sd, d / "ctg", d / "reads2ref_all.out", N_CNS, my) for my in range(1, N_CNS + 1))
    return dict(d=d, db=db, sd=sd, p_ctg=p_ctg, p_ctg_cns=cns)


def _lengths(fasta: bytes):
    return [len(s) for s in fasta.split(b"\n")[1::2]]


def test_assemble_hpc_equals_the_commands_with_H(job, tmp_path):
    print("p_ctg", _lengths(job["p_ctg"]), "p_ctg_cns", _lengths(job["p_ctg_cns"]))
    assert max(_lengths(job["p_ctg"]), default=0) >= 50_000 and len(job["p_ctg_cns"]) > 0
    got = shimmer.assemble(job["sd"], N_INDEX, N_OVLP, N_MAP, N_CNS, mc_lower=MC_LOWER, mc_upper=MC_UPPER, out_dir=str(tmp_path / "out"), hpc=True)
    assert got["p_ctg"] == job["p_ctg"] and got["p_ctg_cns"] == job["p_ctg_cns"]
    assert (tmp_path / "out" / "p_ctg.fa").read_bytes() == job["p_ctg"]
    plain = shimmer.assemble(job["sd"], N_INDEX, N_OVLP, mc_lower=MC_LOWER, mc_upper=MC_UPPER)
    assert [s["shimmers"] for s in got["stats"]["index"]] != [s["shimmers"] for s in plain["stats"]["index"]]   # (the flag reaches the index)


def test_pg_asm_hpc_writes_the_same_files(job, tmp_path):
    fa = tmp_path / "reads.fa"
    lut = np.full(16, ord("N"), np.uint8)
    lut[[1, 2, 4, 8]] = [ord(c) for c in "ACGT"]
    db = job["db"]
    with open(fa, "wb") as f:
        for r, n, o in zip(db.rid, db.rlen, db.roff):
            f.write(b">read%06d\n" % r + lut[db.seqdb[int(o):int(o) + int(n)] & 0x0F].tobytes() + b"\n")
    (tmp_path / "reads.lst").write_text(str(fa) + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", "pg_asm"), str(tmp_path / "reads.lst"), str(N_INDEX), str(N_OVLP), str(N_MAP), str(N_CNS),
                        "--hpc", "--output", str(tmp_path / "wd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "wd" / "p_ctg.fa").read_bytes() == job["p_ctg"]
    assert (tmp_path / "wd" / "p_ctg_cns.fa").read_bytes() == job["p_ctg_cns"]
