#!/usr/bin/env python3
"""Times the GFA stage (Unitigs.gfa() + its text) on chains, rings and bubbles of reads of growing size, without a read database, and
on one simulated read set with one.  The shapes are edge arrays built here (an edge and its reverse, pair after pair), so the stage
runs from host records: the route with the two extra sorts for the reverse-edge search.  Per size and shape: the unitigs once, then
`runs` times the GFA and its text -- device time of the stage and of each part (pgx_timing_get: gfa_dual, _rows, _links, _text),
medians with the spread, the peak of the `gfa` ledger tag.  The read set (two haplotypes, the second with an insertion: a bubble) runs
through index, overlap, graph and unitigs once, then the GFA with the resident reads: the `gfa` timer holds the layout too, so the
layout's share is what the four parts leave.  Last, shimmer.assemble on that read set with gfa=False and with gfa=True, wall ms.

    python tools/gfa_bench.py [--sizes 10000 100000 1000000] [--runs 3] [--genome 300000] [--out profiles/gfa.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

SIZES = [10_000, 100_000, 1_000_000]
PARTS = ("gfa_dual", "gfa_rows", "gfa_links", "gfa_text")


def edges_of(v_rid, w_rid, seed):
    """the edges v:E -> w:E, each followed by its reverse w:B -> v:B, the pairs shuffled"""
    from peregrine_amd.shimmer import SGRAPH_EDGE_DTYPE
    order = np.random.default_rng(seed).permutation(len(v_rid))
    v, w = v_rid[order].astype(np.uint32), w_rid[order].astype(np.uint32)
    e = np.zeros(2 * len(v), SGRAPH_EDGE_DTYPE)
    e["v_rid"][0::2], e["w_rid"][0::2], e["v_end"][0::2], e["w_end"][0::2], e["sp"][0::2], e["tp"][0::2] = v, w, 1, 1, 7800, 9000
    e["v_rid"][1::2], e["w_rid"][1::2], e["v_end"][1::2], e["w_end"][1::2], e["sp"][1::2], e["tp"][1::2] = w, v, 0, 0, 1200, 0
    e["label_rid"], e["score"], e["idt_tenths"] = e["w_rid"], 5000, 990
    return e


def shapes(n):
    """name -> edge records over about n reads"""
    k = np.arange(n)
    chain = k[k % 1000 != 999]
    hub = np.arange(0, n - 4, 4)                                     # hub, two arms, the next hub: a bubble every four reads
    return {"chains of 1000": edges_of(chain, chain + 1, n),
            "rings of 1000": edges_of(k, k - k % 1000 + (k + 1) % 1000, n + 1),
            "bubbles": edges_of(np.concatenate([hub, hub, hub + 1, hub + 2]), np.concatenate([hub + 1, hub + 2, hub + 4, hub + 4]), n + 2)}


def med(xs):
    return "%8.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def read_set(genome):
    """tests/test_gpu_assemble.read_set at a genome of `genome` bases: two haplotypes at 12x, the second with 3 % inserted in the middle"""
    from peregrine_amd import formats, simreads
    g = simreads.make_genome(genome, 41)
    h = np.concatenate([g[:genome // 2], simreads.make_genome(genome * 3 // 100, 44), g[genome // 2:]])
    a = simreads.simulate_reads(g, coverage=12.0, seed=17, mean_len=8000, sd_len=1500, err=0.01)
    b = simreads.simulate_reads(h, coverage=12.0, seed=18, mean_len=8000, sd_len=1500, err=0.01)
    rlen = np.concatenate([a.rlen, b.rlen])
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return formats.SeqDB(np.concatenate([a.seqdb, b.seqdb]), np.arange(len(rlen), dtype=np.uint32), rlen, roff, None)


def timed(runs, make, tag="gfa"):
    """runs + 1 times make() -> Gfa, its text drawn; the first warms the workspaces up and is dropped"""
    from peregrine_amd import _lib
    wall, dev, parts, peak, st, nbytes = [], [], {p: [] for p in PARTS}, 0, None, 0
    for k in range(runs + 1):
        _lib.timing_reset()
        _lib.mem_ledger(reset_peak=True)
        t0 = time.perf_counter()
        with make() as f:
            nbytes, st = len(f.text()), f.stats
        t1 = time.perf_counter()
        if k == 0:
            continue
        wall.append((t1 - t0) * 1e3)
        dev.append(_lib.timing(tag)[0])
        for p in PARTS:
            parts[p].append(_lib.timing(p)[0])
        peak = _lib.mem_ledger()["peak_by_tag"].get(tag, 0)
    return wall, dev, parts, peak, st, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--genome", type=int, default=300_000, help="bases of the simulated genome (0: no read set)")
    ap.add_argument("--out")
    a = ap.parse_args()
    from peregrine_amd import formats, shimmer
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("GPU: Unitigs.gfa(edges) + its text, no read database, from shuffled host edge records; device ms (the `gfa` timer and its parts), median of %d (min .. max)" % a.runs)
    head = "%-15s %9s %9s %9s %9s %9s %9s %26s %26s %26s %26s %26s %26s %9s"
    emit(head % ("shape", "reads", "G edges", "segments", "links", "text MB", "bases MB", "wall: gfa + text", "gfa (device)", "dual", "rows", "links", "text", "peak MiB"))
    row = "%-15s %9d %9d %9d %9d %9.1f %9.1f %26s %26s %26s %26s %26s %26s %9.1f"
    for n in a.sizes:
        for name, edges in shapes(n).items():
            with shimmer.unitigs(edges) as u:
                wall, dev, parts, peak, st, nbytes = timed(a.runs, lambda: u.gfa(edges))
            emit(row % (name, n, len(edges), st["segments"], st["links"], nbytes / 1e6, 0.0, med(wall), med(dev), *(med(parts[p]) for p in PARTS), peak / 2**20))
    if a.genome:
        db = read_set(a.genome)
        rdb = shimmer.ResidentDB(db, 0)
        try:
            ix = rdb.index()
            recs, _ = rdb.overlap(ix.top, ix.top_mc)
            with shimmer.string_graph(recs, chimer_ordered=True) as g, g.unitigs() as u:
                emit("")
                emit("GPU: Unitigs.gfa(graph, reads) + its text on %d simulated reads (%.1f Mb, two haplotypes of %d bases); the `gfa` timer holds the contig layout, whose share is "
                     "what the four parts leave" % (len(db.rlen), int(db.rlen.sum()) / 1e6, a.genome))
                emit(head % ("shape", "reads", "G edges", "segments", "links", "text MB", "bases MB", "wall: gfa + text", "gfa (device)", "dual", "rows", "links", "text", "peak MiB"))
                wall, dev, parts, peak, st, nbytes = timed(a.runs, lambda: u.gfa(g, rdb))
                emit(row % ("read set", len(db.rlen), u.stats["g_edges"], st["segments"], st["links"], nbytes / 1e6, st["bases"] / 1e6, med(wall), med(dev),
                            *(med(parts[p]) for p in PARTS), peak / 2**20))
                own = sum(statistics.median(parts[p]) for p in PARTS)
                emit("the layout's share of the stage's device time: %.2f of %.2f ms (%.0f %%); the stage's own parts: %.2f ms" %
                     (statistics.median(dev) - own, statistics.median(dev), 100 * (statistics.median(dev) - own) / max(statistics.median(dev), 1e-9), own))
        finally:
            rdb.close()
        with tempfile.TemporaryDirectory() as d:
            sd = os.path.join(d, "seq_dataset")
            formats.write_seqdb(sd, db)
            for flag in (False, True):
                wall = []
                for k in range(a.runs + 1):
                    t0 = time.perf_counter()
                    r = shimmer.assemble(sd, 3, 2, gfa=flag)
                    if k:
                        wall.append((time.perf_counter() - t0) * 1e3)
                emit("shimmer.assemble(3 index chunks, 2 overlap chunks, no consensus, gfa=%s): wall ms %s%s" %
                     (flag, med(wall), "; its gfa stage %.1f ms" % r["stats"]["ms"]["gfa"] if flag else ""))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
