#!/usr/bin/env python3
"""Times a FASTA text -> resident database, two routes on one GPU, on the same texts:

  new : ResidentDB.from_fasta(text) (pgx_seqdb_from_fasta: the text uploaded, parsed, compacted and encoded on the GPU)
  old : pgx_mkseqdb to <shm>/x.seqdb + x.idx, then pgx_seqdb_load of the two files (the route before from_fasta)

Texts (single-line records, as path_to_contig writes contigs): one contig of 100 Mb; 3 Gb in contigs of 1 to 50 Mb; 1 Gb of 15 kb reads
(--scale shrinks all three; a scaled run is recorded as such).  Per text and route: the median of --runs calls after --warmup warm-ups,
host clock around the calls, files in --shm; the HBM peak of the new route from the library's ledger.  Then the stage table of
shimmer.assemble on a small two-haplotype job (its wall time per stage, one run after a warm-up).
    python tools/fasta_db_bench.py [--scale 1.0] [--runs 5] [--warmup 2] [--shm /dev/shm] [--out profiles/fasta_db.txt]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def text_of(lengths, seed):
    """>name\\nbases\\n per record, built in one buffer"""
    rng = np.random.default_rng(seed)
    heads = [b">ctg%06d\n" % i for i in range(len(lengths))]
    total = sum(map(len, heads)) + int(sum(lengths)) + len(lengths)
    out = np.empty(total, np.uint8)
    at = 0
    for h, n in zip(heads, lengths):
        out[at:at + len(h)] = np.frombuffer(h, np.uint8)
        at += len(h)
        out[at:at + n] = ACGT[rng.integers(0, 4, n, dtype=np.uint8)]
        out[at + n] = 10
        at += n + 1
    return out.tobytes()


def texts(scale):
    rng = np.random.default_rng(1)
    mixed, left = [], int(3e9 * scale)
    while left > 0:
        n = min(int(rng.integers(int(1e6 * scale) + 1, int(50e6 * scale) + 2)), left)
        mixed.append(n)
        left -= n
    return (("one contig of %.0f Mb" % (100 * scale), [int(100e6 * scale)]),
            ("%.2f Gb in %d contigs of 1 to 50 Mb (scaled alike)" % (3 * scale, len(mixed)), mixed),
            ("%.2f Gb of 15 kb single-line reads" % scale, [15000] * int(1e9 * scale / 15000)))


def timed(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shm", default="/dev/shm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fasta_db.txt"))
    a = ap.parse_args()
    import ctypes as C
    from peregrine_amd import _lib, formats, shimmer, simreads
    _lib.init(0)
    lib = _lib.load()
    d = tempfile.mkdtemp(prefix="pgx_fasta_bench_", dir=a.shm)
    lines = ["FASTA text -> resident database on one MI355X: median (min, max) of %d calls after %d warm-ups, host clock, files in %s%s"
             % (a.runs, a.warmup, a.shm, "" if a.scale == 1.0 else "; SCALED RUN, --scale %g" % a.scale),
             "%-52s %10s %28s %28s %8s %12s" % ("text", "MB", "from_fasta ms", "pgx_mkseqdb + load ms", "ratio", "HBM peak MB")]
    try:
        for k, (what, lengths) in enumerate(texts(a.scale)):
            text = text_of(lengths, 100 + k)
            fa, lst, pre = (os.path.join(d, n) for n in ("x.fa", "x.lst", "x"))
            with open(fa, "wb") as f:
                f.write(text)
            with open(lst, "w") as f:
                f.write(fa + "\n")

            def new():
                shimmer.ResidentDB.from_fasta(text, 0).close()

            def old():
                shimmer.shmr_mkseqdb(lst, pre)
                h = C.c_void_p()
                _lib.check(lib.pgx_seqdb_load(pre.encode(), C.byref(h)), "pgx_seqdb_load")
                lib.pgx_seqdb_free(h)
            new()
            _lib.mem_ledger(reset_peak=True)
            tn = timed(new, a.runs, max(a.warmup - 1, 0))
            peak = _lib.mem_ledger()["peak_live_bytes"]
            print(what, "new", tn, flush=True)
            to = timed(old, a.runs, a.warmup)
            print(what, "old", to, flush=True)
            rdb = shimmer.ResidentDB.from_fasta(text, 0)   # the two routes give the same files
            rdb.save(os.path.join(d, "y"))
            rdb.close()
            for ext in (".seqdb", ".idx"):
                with open(pre + ext, "rb") as f, open(os.path.join(d, "y") + ext, "rb") as g:
                    assert f.read() == g.read(), ext
            lines.append("%-52s %10.1f %28s %28s %7.1fx %12.1f" % (what, len(text) / 1e6, "%.1f (%.1f, %.1f)" % tuple(1e3 * t for t in tn),
                                                                  "%.1f (%.1f, %.1f)" % tuple(1e3 * t for t in to), to[0] / tn[0], peak / 1e6))
            lines.append("%-52s from_fasta: %.2f GB/s of text" % ("", len(text) / tn[0] / 1e9))
            del text
        # the stage table of assemble on a small job (tests/test_gpu_assemble.py's read set)
        g = simreads.make_genome(300_000, 41)
        h = np.concatenate([g[:150_000], simreads.make_genome(9_000, 44), g[150_000:]])
        x = simreads.simulate_reads(g, coverage=12.0, seed=17, mean_len=8000, sd_len=1500, err=0.01)
        y = simreads.simulate_reads(h, coverage=12.0, seed=18, mean_len=8000, sd_len=1500, err=0.01)
        rlen = np.concatenate([x.rlen, y.rlen])
        roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
        db = formats.SeqDB(np.concatenate([x.seqdb, y.seqdb]), np.arange(len(rlen), dtype=np.uint32), rlen, roff, None)
        formats.write_seqdb(os.path.join(d, "job"), db)
        run = lambda: shimmer.assemble(os.path.join(d, "job"), 3, 2, 2, 2, with_alt=True)
        run()
        t0 = time.perf_counter()
        r = run()
        wall = time.perf_counter() - t0
        st = r["stats"]
        lines.append("")
        lines.append("shimmer.assemble, %d reads / %.1f Mbases (two haplotypes of 300 kb at 12x), 3 index, 2 overlap, 2 mapping, 2 consensus chunks, with_alt; second run: %.0f ms"
                     % (db.n_reads, db.n_bases / 1e6, 1e3 * wall))
        lines.append("  " + "  ".join("%s %.1f ms" % kv for kv in st["ms"].items()))
        lines.append("  polish: " + "  ".join("%s %.1f ms" % kv for kv in st["polish"]["ms"].items()))
        lines.append("  p_ctg %d bytes, a_ctg %d bytes, p_ctg_cns %d bytes.  The share of these stages in a 30x human job: not measured."
                     % (len(r["p_ctg"]), len(r["a_ctg"]), len(r["p_ctg_cns"])))
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = "\n".join(lines) + "\n"
    print(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
