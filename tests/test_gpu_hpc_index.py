"""The index stage with homopolymer-compressed shimmers (hpc): ResidentDB.index / index_dev / index_overlap(hpc=True), shmr_index -H
in both drop-ins and through `pgx_cli serve`, against the compiled reference's mm_sketch(is_hpc=1) + mm_reduce per read (the reference
itself where oracle/_ref is present, else its record in tests/golden/hpc_cases.npz).  The database is the fixture's w = 80, k = 16
strings: directed edge cases, reads with ambiguous bases, reads that outgrow their slabs.  All comparisons are exact."""
import os
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

import hpc_util as H
import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.shimmer import ResidentDB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "native", "pgx_cli")
pytestmark = pytest.mark.gpu


def _cat(parts):
    return np.concatenate(parts) if len(parts) else np.zeros(0, formats.MM_DTYPE)


def _counts(mm):
    """the count table of a list as sorted (mer, count) pairs: the multiset of x >> 8"""
    mer, cnt = np.unique(mm["x"] >> np.uint64(8), return_counts=True)
    return np.stack([mer.astype(np.uint64), cnt.astype(np.uint64)], axis=1)


class Work:
    """the database and the expected per-read lists of every level: made once, never changed"""

    def __init__(self):
        self.cases = [c for c in H.golden_cases() if (c.w, c.k) == (H.W, H.K)]
        self.db = H.seqdb_of([c.seq for c in self.cases])
        self.lv = {0: [], 1: [], 2: []}
        for rid, c in enumerate(self.cases):
            if U.have_ref():
                l0 = H.ref_sketch_hpc(c.seq, H.W, H.K, rid)
                l1 = U.ref_reduce(l0, H.R)
                l2 = U.ref_reduce(l1, H.R)
            else:
                l0, l1, l2 = (c.with_rid(a, rid) for a in (c.l0, c.l1, c.l2))
            for lv, a in ((0, l0), (1, l1), (2, l2)):
                self.lv[lv].append(a)
        self.rdb = ResidentDB(self.db, 0)

    def want(self, level, keep=lambda rid: True):
        return _cat([a for rid, a in enumerate(self.lv[level]) if keep(rid)])


@pytest.fixture(scope="module")
def work():
    wk = Work()
    yield wk
    wk.rdb.close()


class Sim:
    """a small simulated read set for the tests that go on into the overlap stage"""

    def __init__(self):
        self.db = simreads.simulate_reads(simreads.make_genome(60_000, 3), coverage=8.0, seed=4, mean_len=5000, sd_len=500)
        self.rdb = ResidentDB(self.db, 0)
        self.plain = self.rdb.index()
        self.hpc = self.rdb.index(hpc=True)


@pytest.fixture(scope="module")
def sim():
    s = Sim()
    yield s
    s.rdb.close()


def test_the_database_is_worth_indexing(work):
    assert len(work.cases) > 90 and len(work.want(0)) > 2000 and len(work.want(1)) > 300 and len(work.want(2)) > 50
    assert any(b"N" in c.seq for c in work.cases)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("want_l0", [False, True], ids=["top", "top+l0"])
def test_index_hpc(work, levels, want_l0):
    a = work.rdb.index(levels=levels, want_l0=want_l0, hpc=True)
    top = work.want(levels)
    assert np.array_equal(a.top, top)
    assert np.array_equal(formats.mc_as_sorted_pairs(a.top_mc), _counts(top))
    assert a.reads == len(work.cases) and a.bases == int(work.db.rlen.sum())
    assert a.reads_literal >= 2          # the low-complexity reads outgrew their slabs and were sketched again into exact ones
    if want_l0:
        assert np.array_equal(a.l0, work.want(0))
        assert np.array_equal(formats.mc_as_sorted_pairs(a.l0_mc), _counts(work.want(0)))
    else:
        assert a.l0 is None


def test_three_chunks_hold_what_the_one_holds(work):
    one = work.rdb.index(hpc=True).top
    parts = [work.rdb.index(total_chunk=3, mychunk=c, hpc=True) for c in (1, 2, 3)]
    for c, p in zip((1, 2, 3), parts):
        sel = work.want(2, lambda rid: rid % 3 == c % 3)
        assert np.array_equal(p.top, sel), c
        assert np.array_equal(formats.mc_as_sorted_pairs(p.top_mc), _counts(sel)), c
    both = _cat([p.top for p in parts])
    order = np.argsort(both["y"] >> np.uint64(32), kind="stable")
    assert np.array_equal(both[order], one)


def test_the_device_hand_over(work):
    top = work.want(2)
    ix, d_top, n_top, d_mc, n_mc = work.rdb.index_dev(hpc=True)
    assert n_top == len(top) and n_mc == len(_counts(top)) and d_top and d_mc


def test_the_one_call_pipeline(sim):
    """index_overlap(hpc=True): the hpc index's lists, and the records the overlap stage makes of them"""
    assert len(sim.hpc.top) > 100 and not np.array_equal(sim.hpc.top, sim.plain.top)
    if U.have_ref():
        db = sim.db
        want = _cat([U.ref_reduce(U.ref_reduce(H.ref_sketch_hpc(U.ref_decode(db.seqdb[int(o):int(o) + int(n)], 0), H.W, H.K, int(r)), H.R), H.R)
                     for r, n, o in zip(db.rid, db.rlen, db.roff)])
        assert np.array_equal(sim.hpc.top, want)
    ix, ov, st = sim.rdb.index_overlap(want_index_arrays=True, hpc=True)
    assert np.array_equal(ix.top, sim.hpc.top) and np.array_equal(formats.mc_as_sorted_pairs(ix.top_mc), formats.mc_as_sorted_pairs(sim.hpc.top_mc))
    want, _ = sim.rdb.overlap(sim.hpc.top, sim.hpc.top_mc)
    assert len(want) > 100 and formats.ovlp_fields_equal(ov, want)


def test_the_plain_index_is_what_it_was(work):
    """hpc=False before and after hpc calls in the same process: the same lists, and the CPU oracle's"""
    db = work.db
    l0 = _cat([U.orc_sketch_seqdb(db.seqdb[int(o):int(o) + int(n)], H.W, H.K, int(r)) for r, n, o in zip(db.rid, db.rlen, db.roff)])
    top = U.orc_reduce(U.orc_reduce(l0, H.R), H.R)
    before = work.rdb.index()
    before_l0 = work.rdb.index(want_l0=True)
    work.rdb.index(hpc=True), work.rdb.index(want_l0=True, hpc=True)
    after = work.rdb.index()
    after_l0 = work.rdb.index(want_l0=True)
    for a in (before, before_l0, after, after_l0):
        assert np.array_equal(a.top, top)
        assert np.array_equal(formats.mc_as_sorted_pairs(a.top_mc), formats.mc_as_sorted_pairs(U.orc_count(top)))
    assert np.array_equal(before_l0.l0, l0) and np.array_equal(after_l0.l0, l0)
    assert not np.array_equal(top, work.want(2))


def _check_files(work, prefix, levels, l0):
    top = work.want(levels)
    assert np.array_equal(formats.read_mmlist(f"{prefix}-L{levels}-01-of-01.dat"), top)
    assert np.array_equal(formats.mc_as_sorted_pairs(formats.read_mm_count(f"{prefix}-L{levels}-MC-01-of-01.dat")), _counts(top))
    assert os.path.exists(f"{prefix}-L0-01-of-01.dat") == l0
    if l0:
        assert np.array_equal(formats.read_mmlist(f"{prefix}-L0-01-of-01.dat"), work.want(0))
        assert np.array_equal(formats.mc_as_sorted_pairs(formats.read_mm_count(f"{prefix}-L0-MC-01-of-01.dat")), _counts(work.want(0)))


@pytest.mark.parametrize("tool", ["python", "native"])
def test_shmr_index_H_writes_the_lists(work, tmp_path, tool):
    """both drop-ins: -H with the default -m 1 (L0 files too) and two levels, with -m 0 -l 1; without -H the plain lists"""
    pre = str(tmp_path / "sd")
    formats.write_seqdb(pre, work.db)
    cmd = [sys.executable, os.path.join(ROOT, "bin", "shmr_index")] if tool == "python" else [os.path.join(ROOT, "bin", "native", "shmr_index")]
    run = lambda *a: subprocess.run(cmd + ["-p", pre, *a], check=True, capture_output=True, timeout=300)
    run("-H", "-o", str(tmp_path / "a"))
    _check_files(work, str(tmp_path / "a"), 2, True)
    run("-o", str(tmp_path / "b"), "-m", "0", "-l", "1", "-H")
    _check_files(work, str(tmp_path / "b"), 1, False)
    run("-o", str(tmp_path / "c"), "-m", "0")
    assert np.array_equal(formats.read_mmlist(str(tmp_path / "c-L2-01-of-01.dat")), work.rdb.index().top)


def test_shmr_index_H_through_the_server(work, sim, tmp_path):
    """`pgx_cli serve` parses the same argv: -H lists under the usual names, then plain lists under the SAME names -- an overlap command
    after each must read that command's lists (the server's device copies of the files it wrote are replaced with them)"""
    pre = str(tmp_path / "sd")
    formats.write_seqdb(pre, sim.db)
    plain, hpc = sim.plain, sim.hpc
    srv = subprocess.Popen([CLI, "serve", "-p", pre], stderr=subprocess.PIPE, text=True)
    try:
        for _ in range(600):
            if os.path.exists(pre + ".pgx.sock") or srv.poll() is not None:
                break
            time.sleep(0.1)
        assert srv.poll() is None and os.path.exists(pre + ".pgx.sock"), srv.stderr.read() if srv.poll() is not None else "no socket"
        run = lambda tool, *a: subprocess.run([CLI, tool, "-p", pre, *a], cwd=tmp_path, check=True, capture_output=True, text=True, timeout=300)
        for flag, ix, name in ((["-H"], hpc, "ov.hpc"), ([], plain, "ov.plain"), (["-H"], hpc, "ov.hpc2")):
            r = run("shmr_index", "-m", "0", "-o", "ix", *flag)
            assert "resident: pgx_cli serve" in r.stderr
            assert np.array_equal(formats.read_mmlist(str(tmp_path / "ix-L2-01-of-01.dat")), ix.top)
            run("shmr_overlap", "-l", "ix-L2", "-o", name)
            want, _ = sim.rdb.overlap(ix.top, ix.top_mc)
            assert formats.ovlp_fields_equal(formats.read_ovlp(str(tmp_path / name)), want), name
        run("shmr_index", "-o", "l0", "-H")
        assert np.array_equal(formats.read_mmlist(str(tmp_path / "l0-L2-01-of-01.dat")), hpc.top)
        assert np.array_equal(formats.read_mmlist(str(tmp_path / "l0-L0-01-of-01.dat")), sim.rdb.index(want_l0=True, hpc=True).l0)
    finally:
        srv.send_signal(signal.SIGTERM)
        srv.wait(timeout=30)


def test_hpc_needs_the_bytes():
    """after release_bytes (no ambiguous base) and after compact_bytes (with one) the hpc sketch answers PGX_ESTATE, as w / k other than
    80 / 16 do; the database stays usable"""
    g = simreads.make_genome(30_000, 3)
    db = simreads.simulate_reads(g, coverage=6.0, seed=4, mean_len=3000, sd_len=300)
    rdb = ResidentDB(db, 0)
    try:
        before = rdb.index()
        hpc = rdb.index(hpc=True)
        assert len(hpc.top) > 0 and not np.array_equal(hpc.top, before.top)
        assert rdb.release_bytes() is True
        for call in (lambda: rdb.index(hpc=True), lambda: rdb.index(hpc=True, want_l0=True), lambda: rdb.sketch([0, 1], hpc=True), lambda: rdb.index_dev(hpc=True)):
            with pytest.raises(_lib.PgxError, match=r"code -5\).*bytes were released or compacted"):
                call()
        assert np.array_equal(rdb.index().top, before.top)
    finally:
        rdb.close()
    withn = formats.SeqDB(db.seqdb.copy(), db.rid, db.rlen, db.roff, db.names)
    for r in (2, 7):
        withn.seqdb[int(db.roff[r]) + 500] = 0     # an ambiguous base: neither nibble set
    rdb = ResidentDB(withn, 0)
    try:
        before = rdb.index()
        assert rdb.compact_bytes() is True
        with pytest.raises(_lib.PgxError, match=r"code -5\)"):
            rdb.index(hpc=True)
        assert np.array_equal(rdb.index().top, before.top)
    finally:
        rdb.close()
