#!/usr/bin/env python3
"""Times reads -> resident database, two routes on one GPU, on the same files:

  new : ResidentDB.from_reads(list) (pgx_seqdb_from_files: files read / inflated on the host in pieces, parsed and encoded on the GPU)
  old : pgx_mkseqdb to <shm>/x.seqdb + x.idx, then pgx_seqdb_load of the two files (the route of the parent commit; never the new code)

Inputs: --gbases (default 1.0) Gb of 15 kb reads as four-line FASTQ in four plain files, and the same four files as .gz.  Per input and
route: the median of --runs calls after --warmup warm-ups, host clock around the calls, files in --shm.  The new route's wall time is split
with the library's timers into upload (reads.upload), kernels (reads) and the rest -- reading, inflating, the host's share; its HBM peak comes
from the ledger, in bytes per text byte.  Both routes' databases are compared through .save().  Then bin/pg_asm with and without
--reads-on-gpu on the plain files (--job 0 leaves it out: the assembly of 1 Gb of random reads finds no overlaps, the stages behind the
database cost the same on both sides).
    python tools/reads_db_bench.py [--gbases 1.0] [--runs 5] [--warmup 2] [--shm /dev/shm] [--job 1] [--out profiles/reads_db.txt]
"""
import argparse
import gzip
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ACGT = np.frombuffer(b"ACGT", np.uint8)
QUAL = np.frombuffer(b"~{zI@>5", np.uint8)   # ('@' and '>' are common quality values of accurate long reads)


def fastq_of(n_reads, rlen, seed, first):
    rng = np.random.default_rng(seed)
    heads = [b"@read%08d ccs\n" % (first + i) for i in range(n_reads)]
    total = sum(map(len, heads)) + n_reads * (2 * rlen + 4)
    out = np.empty(total, np.uint8)
    at = 0
    for h in heads:
        out[at:at + len(h)] = np.frombuffer(h, np.uint8)
        at += len(h)
        out[at:at + rlen] = ACGT[rng.integers(0, 4, rlen, dtype=np.uint8)]
        out[at + rlen:at + rlen + 3] = (10, 43, 10)
        at += rlen + 3
        out[at:at + rlen] = QUAL[rng.integers(0, len(QUAL), rlen, dtype=np.uint8)]
        out[at + rlen] = 10
        at += rlen + 1
    return out.tobytes()


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
    ap.add_argument("--gbases", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shm", default="/dev/shm")
    ap.add_argument("--job", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reads_db.txt"))
    a = ap.parse_args()
    import ctypes as C
    from peregrine_amd import _lib, shimmer
    _lib.init(0)
    lib = _lib.load()
    d = tempfile.mkdtemp(prefix="pgx_reads_bench_", dir=a.shm)
    rlen, per_file = 15000, int(a.gbases * 1e9 / 15000 / 4)
    lines = ["reads -> resident database on one MI355X: median (min, max) of %d calls after %d warm-ups, host clock, files in %s; "
             "%.2f Gb of 15 kb reads as four-line FASTQ in four files" % (a.runs, a.warmup, a.shm, 4 * per_file * rlen / 1e9),
             "%-12s %9s %26s %26s %7s   %s" % ("files", "text MB", "from_reads ms", "pgx_mkseqdb + load ms", "ratio", "from_reads: upload / kernels / host rest ms; HBM peak B per text byte")]
    try:
        plain, gz, text_bytes = [], [], 0
        for k in range(4):
            t = fastq_of(per_file, rlen, 50 + k, k * per_file)
            text_bytes += len(t)
            plain.append(os.path.join(d, "reads%d.fastq" % k))
            with open(plain[-1], "wb") as f:
                f.write(t)
            gz.append(plain[-1] + ".gz")
            with gzip.open(gz[-1], "wb", compresslevel=1) as f:
                f.write(t)
            del t
        pre, verdicts = os.path.join(d, "x"), []
        for what, files in (("plain", plain), ("gz", gz)):
            lst = os.path.join(d, what + ".lst")
            with open(lst, "w") as f:
                f.write("\n".join(files) + "\n")

            def new():
                shimmer.ResidentDB.from_reads(lst, 0).close()

            def old():
                shimmer.shmr_mkseqdb(lst, pre)
                h = C.c_void_p()
                _lib.check(lib.pgx_seqdb_load(pre.encode(), C.byref(h)), "pgx_seqdb_load")
                lib.pgx_seqdb_free(h)
            for _ in range(a.warmup):
                new()
            _lib.mem_ledger(reset_peak=True)
            _lib.timing_reset()
            tn = timed(new, a.runs, 0)
            peak = _lib.mem_ledger()["peak_live_bytes"]
            up, kern = _lib.timing("reads.upload")[0] / a.runs, _lib.timing("reads")[0] / a.runs
            print(what, "new", tn, flush=True)
            to = timed(old, a.runs, a.warmup)
            print(what, "old", to, flush=True)
            rdb = shimmer.ResidentDB.from_reads(lst, 0)   # the two routes give the same files
            rdb.save(os.path.join(d, "y"))
            rdb.close()
            for ext in (".seqdb", ".idx"):
                with open(pre + ext, "rb") as f, open(os.path.join(d, "y") + ext, "rb") as g:
                    assert f.read() == g.read(), ext
            size = sum(os.path.getsize(f) for f in files)
            lines.append("%-12s %9.1f %26s %26s %6.2fx   %.1f / %.1f / %.1f; %.2f" % (
                what, size / 1e6, "%.1f (%.1f, %.1f)" % tuple(1e3 * t for t in tn), "%.1f (%.1f, %.1f)" % tuple(1e3 * t for t in to), to[0] / tn[0],
                up, kern, 1e3 * tn[0] - up - kern, peak / text_bytes))
            spread = max(tn[2] - tn[1], to[2] - to[1])
            verdicts.append("%s: the new median is %.1f ms below the old one; the larger spread (max - min) of the two routes' runs is %.1f ms: %s"
                            % (what, 1e3 * (to[0] - tn[0]), 1e3 * spread, "condition met" if to[0] - tn[0] > spread else "CONDITION NOT MET"))
        lines += verdicts
        lines.append("text of the inflated files: %.1f MB; both routes' .seqdb and .idx equal on both inputs" % (text_bytes / 1e6))
        if a.job:
            exe = [sys.executable, os.path.join(ROOT, "bin", "pg_asm"), os.path.join(d, "plain.lst"), "4", "4"]
            for flag in ([], ["--reads-on-gpu"]):
                ts = []
                for _ in range(2):
                    shutil.rmtree(os.path.join(d, "wd"), ignore_errors=True)
                    t0 = time.perf_counter()
                    r = subprocess.run(exe + flag + ["--output", os.path.join(d, "wd")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                    ts.append(time.perf_counter() - t0)
                if r.returncode != 0:
                    lines.append("pg_asm %s: exit %d, %s" % (" ".join(flag) or "(files)", r.returncode, r.stderr.decode().strip().split("\n")[-1]))
                    continue
                lines.append("pg_asm %-15s 4 index / 4 overlap chunks, process wall of the second of two runs: %.2f s; %s"
                             % (" ".join(flag) or "(files)", ts[1], r.stderr.decode().strip().split("\n")[-1]))
        lines.append("a full 93-Gbase read set: unmeasured")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out = "\n".join(lines) + "\n"
    print(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
