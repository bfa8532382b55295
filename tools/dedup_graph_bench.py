#!/usr/bin/env python3
"""What the dedup stream's graph mode removes and costs on one workload's overlap stream.

The stream: the overlap records of a simulated job produced by the library itself (a --genome-base genome with repeat families, reads at
--coverage, all chunks of a --chunks-chunk overlap stage, concatenated).  It goes, in pieces of --piece records, through a plain stream
(each feed's text taken) and through a graph-mode stream (fed, then drained); one warm-up and --repeats timed runs each, in this process.
Written to --out:
  lines kept / lines total, marked reads / reads named; the two outputs checked against each other with the rule in plain Python
  peak HBM booked to the dedup streams (pgx_mem_ledger, tag `dedup`) in either mode: the difference is the row store and the bitmap
  median / min / max wall seconds of either mode
    python tools/dedup_graph_bench.py [--genome 1500000] [--coverage 30] [--chunks 4] [--piece 65536] [--out profiles/dedup_graph_filter.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def make_stream(genome, coverage, chunks):
    from peregrine_amd import simreads
    from peregrine_amd.shimmer import ResidentDB
    g = simreads.make_genome(genome, 21, repeat_families=2, repeat_len=3000, repeat_copies=4, divergence=0.02, tandem=2)
    db = simreads.simulate_reads(g, coverage=coverage, seed=3, mean_len=7000, sd_len=1500, err=0.01, n_files=1)
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    recs = np.concatenate([np.array(rdb.overlap(ix.top, ix.top_mc, total_chunk=chunks, mychunk=c)[0]) for c in range(1, chunks + 1)])
    rdb.close()
    return recs, int(db.n_reads)


def run(recs, piece, graph):
    from peregrine_amd import _lib
    from peregrine_amd.shimmer import DedupStream
    _lib.mem_ledger(reset_peak=True)
    t0 = time.perf_counter()
    with DedupStream(graph_ready=graph) as ds:
        parts = [ds.feed(recs[a:a + piece]) for a in range(0, len(recs), piece)]
        if graph:
            parts = list(ds.drain(piece))
        stats = ds.stats if graph else None
    dt = time.perf_counter() - t0
    return b"".join(parts), dt, _lib.mem_ledger()["peak_by_tag"].get("dedup", 0), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=1_500_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--piece", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dedup_graph_filter.txt"))
    a = ap.parse_args()
    import dedup_graph_util as DG
    recs, n_reads = make_stream(a.genome, a.coverage, a.chunks)
    rows = {}
    for graph in (False, True):
        run(recs, a.piece, graph)   # warm-up: workspaces, pinned buffers
        times = []
        for _ in range(a.repeats):
            text, dt, peak, stats = run(recs, a.piece, graph)
            times.append(dt)
        rows[graph] = (text, times, peak, stats)
    plain, kept = rows[False][0], rows[True][0]
    same = DG.select_graph_lines(plain) == kept
    st = rows[True][3]
    named = len({f for ln in plain.split(b"\n")[:-1] for f in ln.split()[:2]})
    with open(a.out, "w") as f:
        def p(s):
            print(s)
            f.write(s + "\n")
        p(f"tools/dedup_graph_bench.py --genome {a.genome} --coverage {a.coverage:g} --chunks {a.chunks} --piece {a.piece} --repeats {a.repeats}")
        p(f"stream: {len(recs)} overlap records of {n_reads} simulated reads, {len(recs) * 64 / 1e6:.1f} MB, {-(-len(recs) // a.piece)} feeds")
        p(f"lines kept / lines total: {st['lines_kept']} / {st['lines_total']} = {st['lines_kept'] / max(1, st['lines_total']):.4f}   "
          f"(text {len(kept)} / {len(plain)} bytes)")
        p(f"marked reads: {st['contained_reads']} of {named} named in the text ({n_reads} in the job)")
        p(f"graph-mode text equals the rule applied to the plain text (tests/dedup_graph_util.py): {same}")
        p(f"peak HBM booked to `dedup`: plain {rows[False][2]} bytes, graph mode {rows[True][2]} bytes; the row store and the bitmap: {rows[True][2] - rows[False][2]} bytes")
        for graph, name in ((False, "plain stream, text per feed"), (True, "graph mode, feeds + drain ")):
            t = rows[graph][1]
            p(f"{name}: median {statistics.median(t):.4f} s, min {min(t):.4f} s, max {max(t):.4f} s over {len(t)} runs (wall, in process, host arrays in and out)")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
