#!/usr/bin/env python3
"""Times `shmr_dedup < stream > out` of the native drop-in at job scale.

One input: the overlap records of a multi-chunk simulated job produced by the library itself, repeated under shifted read ids until
the stream holds --records records (default 100 M = 6.4 GB), written to --dir (default /dev/shm).  Legs, 5 repeats each after one
warm-up, all in this session on this machine:
  (a) --parent <path to the PARENT commit's bin/native/pgx_cli>   (optional; a second checkout, built)
  (b) this tree's bin/native/pgx_cli
  (c) this tree's with the host formatter forced (PGX_DEDUP_HOST_TEXT=1)
Reports per leg: median / min / max wall seconds, records and lines per second, the child's peak resident size, and whether the three
outputs are byte-equal; for (b) also the library's peak HBM (pgx_mem_ledger, from an in-process run of the same pieces) and the wall
time of a plain read + write of the same bytes (`cat stream > out` and writing the text), the share of (b) that is file traffic.
    python tools/dedup_bench.py [--records N] [--parent PATH] [--piece RECORDS] [--out profiles/dedup_stream.txt]
A kernel trace of (b) is taken in a run of its own (--keep-stream leaves the input where it is):
    rocprofv3 --kernel-trace --memory-copy-trace --stats -- bin/native/pgx_cli shmr_dedup < stream > out
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_stream(path, n_records):
    from peregrine_amd import simreads
    from peregrine_amd.shimmer import ResidentDB
    g = simreads.make_genome(1_500_000, 21, repeat_families=2, repeat_len=3000, repeat_copies=4, divergence=0.02, tandem=2)
    db = simreads.simulate_reads(g, coverage=50.0, seed=3, mean_len=7000, sd_len=1500, err=0.01, n_files=1)
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    base = np.concatenate([np.array(rdb.overlap(ix.top, ix.top_mc, total_chunk=4, mychunk=c)[0]) for c in (1, 2, 3, 4)])
    rdb.close()
    shift = int(db.n_reads)
    written = 0
    with open(path, "wb") as f:
        k = 0
        while written < n_records:
            s = base.copy()
            s["y0"] += np.uint64((k * shift) << 32)
            s["y1"] += np.uint64((k * shift) << 32)
            s[: n_records - written].tofile(f)
            written += min(len(s), n_records - written)
            k += 1
    return written


def run(cmd, stream, out, env):
    with open(stream, "rb") as fi, open(out, "wb") as fo:
        t0 = time.perf_counter()
        p = subprocess.Popen(cmd, stdin=fi, stdout=fo, env=env)
        _, status, ru = os.wait4(p.pid, 0)
        dt = time.perf_counter() - t0
        p.returncode = os.waitstatus_to_exitcode(status)
    if p.returncode:
        raise SystemExit(f"{cmd} exited with {p.returncode}")
    return dt, ru.ru_maxrss * 1024


def digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--piece", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--keep-stream", action="store_true", help="leave the input in --dir (for a profiler run of its own)")
    a = ap.parse_args()
    stream, out = os.path.join(a.dir, "pgx_dedup_bench.dat"), os.path.join(a.dir, "pgx_dedup_bench.ovl")
    lines_out = []

    def say(s):
        print(s, flush=True)
        lines_out.append(s)

    try:
        n = make_stream(stream, a.records)
        say(f"stream: {n} records, {n * 64 / 1e9:.2f} GB")
        env = dict(os.environ)
        if a.piece:
            env["PGX_DEDUP_PIECE"] = str(a.piece)
        mine = [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_dedup"]
        legs = [("b: this tree", mine, env), ("c: this tree, host formatter", mine, dict(env, PGX_DEDUP_HOST_TEXT="1"))]
        if a.parent:
            legs.insert(0, ("a: parent commit", [a.parent, "shmr_dedup"], env))
        digests = {}
        for name, cmd, e in legs:
            run(cmd, stream, out, e)   # warm-up
            res = [run(cmd, stream, out, e) for _ in range(a.repeats)]
            ts = [r[0] for r in res]
            n_lines = sum(1 for _ in open(out, "rb"))
            digests[name] = digest(out)
            med = statistics.median(ts)
            say(f"{name}: median {med:.3f} s (min {min(ts):.3f}, max {max(ts):.3f}, spread {max(ts) - min(ts):.3f}); "
                f"{n / med / 1e6:.1f} M records/s, {n_lines / med / 1e6:.1f} M lines/s ({n_lines} lines, {os.path.getsize(out) / 1e9:.2f} GB); "
                f"peak resident {max(r[1] for r in res) / 2**20:.0f} MiB")
        say("outputs byte-equal: %s" % (len(set(digests.values())) == 1))
        # file traffic alone: the same bytes read and written without any work in between
        t0 = time.perf_counter()
        with open(stream, "rb") as f:
            while f.read(1 << 26):
                pass
        t_read = time.perf_counter() - t0
        text = open(out, "rb").read()
        t0 = time.perf_counter()
        with open(out + ".copy", "wb") as f:
            f.write(text)
        t_write = time.perf_counter() - t0
        os.unlink(out + ".copy")
        say(f"plain read of the stream {t_read:.3f} s, plain write of the text {t_write:.3f} s")
        # peak HBM of the stream (in process, the same pieces)
        from peregrine_amd import _lib
        from peregrine_amd.formats import OVLP_DTYPE
        from peregrine_amd.shimmer import DedupStream, dedup_piece_records
        piece = a.piece or dedup_piece_records()
        _lib.init()
        _lib.mem_ledger(reset_peak=True)
        with DedupStream() as ds, open(stream, "rb") as f:
            while True:
                r = np.fromfile(f, OVLP_DTYPE, piece)
                if len(r):
                    ds.feed(r)
                if len(r) < piece:
                    break
        led = _lib.mem_ledger()
        say(f"peak HBM of the stream: {led['peak_live_bytes'] / 2**20:.0f} MiB live ({led['peak_by_tag']})")
    finally:
        for p in (out,) if a.keep_stream else (stream, out):
            if os.path.exists(p):
                os.unlink(p)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    main()
