"""Overlap and map on homopolymer-compressed (hpc) lists against the REAL reference: our shmr_index -H files go into oracle/_ref/shmr_overlap
and oracle/_ref/shmr_map unchanged, and our stages on the same lists must give their streams -- the record stream under
formats.ovlp_fields_equal (default dispatch and device replay), the map text byte for byte.  Nothing after the index assumes span == k."""
import os
import subprocess

import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import formats, simreads
from peregrine_amd.shimmer import ResidentDB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not U.have_ref() or not os.path.exists(os.path.join(U.REF_DIR, "shmr_map")),
                                                  reason="needs the prebuilt reference binaries (oracle/_ref)")]


def _native(tool, *args, **kw):
    return subprocess.run([os.path.join(ROOT, "bin", "native", "pgx_cli"), tool, *map(str, args)], check=True, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=600, **kw).stdout


def genome():
    """300 kb with homopolymer runs of 300, 260, 40, 20, 20, 12, 12 and 12 bases planted at seeded places"""
    g = simreads.make_genome(300_000, 7)
    rng = np.random.default_rng(3)
    for n in (300, 260, 40, 20, 20, 12, 12, 12):
        s = int(rng.integers(0, len(g) - n))
        g[s:s + n] = int(rng.integers(0, 4))
    return g


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """the read set, its files, our -H index of it (one chunk), and a resident copy"""
    d = tmp_path_factory.mktemp("hpc")
    g = genome()
    db = simreads.simulate_reads(g, coverage=20, mean_len=6000, sd_len=800, seed=5)
    pre = str(d / "rd")
    formats.write_seqdb(pre, db)
    _native("shmr_index", "-p", pre, "-t", 1, "-c", 1, "-m", 0, "-H", "-o", d / "ix")
    rdb = ResidentDB(db, 0)
    yield dict(d=d, g=g, db=db, pre=pre, rdb=rdb, top=formats.read_mmlist(str(d / "ix-L2-01-of-01.dat")),
               mc=formats.read_mm_count(str(d / "ix-L2-MC-01-of-01.dat")))
    rdb.close()


def test_the_lists_are_hpc(job):
    spans = job["top"]["x"] & np.uint64(0xFF)
    assert len(job["top"]) > 8000 and (spans > 16).mean() > 0.9     # (11,792 elements; nearly every span is above k)
    assert np.array_equal(job["top"], job["rdb"].index(hpc=True).top)


def test_overlap_stream_equals_the_reference(job, monkeypatch):
    """oracle/_ref/shmr_overlap -t 1 -c 1 on our -H files (9,923 records when this was written; fewer than 1,000 fails) against our
    overlap stage: the default dispatch, the device replay forced, and the native drop-in on the files"""
    d = job["d"]
    U.ref_run("shmr_overlap", "-p", job["pre"], "-l", d / "ix-L2", "-t", 1, "-c", 1, "-o", d / "ref.ov")
    want = formats.read_ovlp(str(d / "ref.ov"))
    print("reference records on hpc lists:", len(want))
    assert len(want) >= 1000
    got, st = job["rdb"].overlap(job["top"], job["mc"])
    assert formats.ovlp_fields_equal(got, want)
    monkeypatch.setenv("PGX_GPU_REPLAY", "1")
    got2, st2 = job["rdb"].overlap(job["top"], job["mc"])
    assert st2["device_replay"] == 1 and formats.ovlp_fields_equal(got2, want)
    monkeypatch.delenv("PGX_GPU_REPLAY")
    _native("shmr_overlap", "-p", job["pre"], "-l", d / "ix-L2", "-t", 1, "-c", 1, "-o", d / "our.ov")
    assert formats.ovlp_fields_equal(formats.read_ovlp(str(d / "our.ov")), want)


def test_map_text_equals_the_reference(job):
    """three slices of the genome as contigs, indexed with -H -t 1 -c 1: oracle/_ref/shmr_map against our shmr_map on the two hpc indexes,
    byte for byte (the reference must give at least 100 rows; it gave 3,739 when this was written)"""
    d, g = job["d"], job["g"]
    slices = [g[10_000:110_000], g[120_000:200_000], g[205_000:295_000]]
    enc = [(np.uint8(1) << s) | ((np.uint8(8) >> s[::-1]) << np.uint8(4)) for s in slices]
    rlen = np.array([len(s) for s in slices], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    cpre = str(d / "ctg")
    formats.write_seqdb(cpre, formats.SeqDB(np.concatenate(enc).astype(np.uint8), np.arange(3, dtype=np.uint32), rlen, roff, ["c0", "c1", "c2"]))
    _native("shmr_index", "-p", cpre, "-t", 1, "-c", 1, "-m", 0, "-H", "-o", d / "ctg")
    args = ["-r", cpre, "-m", str(d / "ctg-L2"), "-p", job["pre"], "-l", str(d / "ix-L2"), "-t", "1", "-c", "1"]
    want = subprocess.run([os.path.join(U.REF_DIR, "shmr_map"), *args], check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
    print("reference map rows on hpc lists:", want.count(b"\n"))
    assert want.count(b"\n") >= 100
    assert _native("shmr_map", *args) == want
