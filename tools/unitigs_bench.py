#!/usr/bin/env python3
"""Times the unitig stage (StringGraph.unitigs() + all of its text) on chains and rings of reads of growing size.  The inputs are
record streams in the manner of tests/dedup_graph_util.rec (dovetails of read i into read i + 1), built here as arrays; nothing else
is read.  Per size: the graph, then `runs` times the unitigs and their text -- device time of the stage and of each part
(pgx_timing_get: unitigs_links, _rank, _paths, _text), medians with the spread, the peak of the `unitigs` ledger tag.

    python tools/unitigs_bench.py [--sizes 10000 100000 1000000] [--runs 5] [--out profiles/unitigs.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

SIZES = [10_000, 100_000, 1_000_000]
PARTS = ("unitigs_links", "unitigs_rank", "unitigs_paths", "unitigs_text")


def dovetails(f, g, rl=9000):
    """records: read f[i] to the left of read g[i] on the same strand, overhangs and scores varying with i"""
    from peregrine_amd.formats import OVLP_DTYPE
    n = len(f)
    i = np.arange(n)
    r = np.zeros(n, OVLP_DTYPE)
    r["y0"] = (f.astype(np.uint64) << np.uint64(32)) | np.uint64(200)
    r["y1"] = (g.astype(np.uint64) << np.uint64(32)) | np.uint64(200)
    r["rl0"] = r["rl1"] = rl
    r["m_size"], r["dist"] = 5000 + i % 13, 20
    r["q_bgn"], r["q_end"], r["t_bgn"], r["t_end"] = 1000 + (i % 7) * 10, rl, 0, rl - 1200 - (i % 5) * 10
    r["t_m_end"], r["q_m_end"] = r["t_end"], r["q_end"]
    return r


def shapes(n):
    """name -> records over about n reads, shuffled"""
    rng = np.random.default_rng(n)
    i = np.arange(n - 1)
    one = dovetails(i, i + 1)                                        # one chain
    k = np.arange(n)
    many = dovetails(k[k % 1000 != 999], k[k % 1000 != 999] + 1)     # chains of 1,000 reads
    ring = dovetails(k, (k + 1) % n)                                 # one ring
    rings = dovetails(k, k - k % 1000 + (k + 1) % 1000)              # rings of 1,000 reads
    out = {"one chain": one, "chains of 1000": many, "one ring": ring, "rings of 1000": rings}
    for v in out.values():
        rng.shuffle(v)
    return out


def med(xs):
    return "%8.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    from peregrine_amd import _lib, shimmer
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    emit("GPU: StringGraph.unitigs() + all of its text on the graph of shuffled dovetail records; device ms (the `unitigs` timer and its parts), median of %d (min .. max)" % a.runs)
    emit("%-15s %9s %9s %8s %9s %10s %26s %26s %26s %26s %26s %26s %9s" % ("shape", "reads", "G edges", "unitigs", "longest", "text MB", "wall: unitigs + text", "unitigs (device)",
                                                                       "links", "rank", "paths", "text", "peak MiB"))
    for n in a.sizes:
        for name, recs in shapes(n).items():
            with shimmer.string_graph(recs) as g:
                wall, dev, parts = [], [], {p: [] for p in PARTS}
                for k in range(a.runs + 1):      # (the first run warms the workspaces up and is dropped)
                    _lib.timing_reset()
                    _lib.mem_ledger(reset_peak=True)
                    t0 = time.perf_counter()
                    with g.unitigs() as u:
                        nbytes = sum(len(p) for p in u.text())
                        st = u.stats
                    t1 = time.perf_counter()
                    if k == 0:
                        continue
                    wall.append((t1 - t0) * 1e3)
                    dev.append(_lib.timing("unitigs")[0])
                    for p in PARTS:
                        parts[p].append(_lib.timing(p)[0])
                    peak = _lib.mem_ledger()["peak_by_tag"].get("unitigs", 0)
            emit("%-15s %9d %9d %8d %9d %10.1f %26s %26s %26s %26s %26s %26s %9.1f" % (name, n, st["g_edges"], st["unitigs"], st["longest_edges"], nbytes / 1e6, med(wall), med(dev),
                                                                                 *(med(parts[p]) for p in PARTS), peak / 2**20))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
