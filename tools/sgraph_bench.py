#!/usr/bin/env python3
"""Times the string graph stage on record streams of growing size (tests/dedup_graph_util.make_records, the dense fixture's density:
genome = 19 bases per read).

    python tools/sgraph_bench.py                 # GPU: shimmer.string_graph(records) + its whole text, medians of 5 with the spread,
                                                 # the share of each part (pgx_timing_get) and the peak of the `sgraph` ledger tag
    python tools/sgraph_bench.py --reference S   # CPU, only where the reference tree is (S = its py/scripts): the real generate_string_graph
                                                 # (disable_chimer_bridge_removal=True, lfc=False) on the texts of the same records

    python tools/sgraph_bench.py --chimer [--reference S]   # the same streams plus chimeric reads (tests/chimer_util.chimeric_sim, a chimeric
                                                 # read per 4 reads): the stage without and with chimer_ordered, part by part; with --reference the
                                                 # real function with the chimer bridge step, bfs_nodes popping the smallest (rid, end)

All print a table; --out appends it to a file (profiles/sgraph.txt, profiles/sgraph_chimer.txt)."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import dedup_graph_util as DG  # noqa: E402

SIZES = [260, 520, 1040, 2080]
MIN_LEN, MIN_IDT = 2000, 96.0
PARTS = ("sgraph_edges", "sgraph_adj", "sgraph_tr", "sgraph_chimer", "sgraph_spur", "sgraph_best", "sgraph_text")
CHIMER = False     # --chimer: the streams get chimeric reads, and the GPU table has a row without and a row with the step


def records(n_reads):
    if CHIMER:
        import chimer_util
        return chimer_util.chimeric_sim(seed=7, n_reads=n_reads, genome=n_reads * 5000 // 260, n_chimers=n_reads // 4)
    return DG.make_records(seed=7, n_reads=n_reads, genome=n_reads * 5000 // 260, contained_share=0.0)


def med(xs):
    return "%9.1f (%.1f .. %.1f)" % (statistics.median(xs), min(xs), max(xs))


def gpu(sizes, runs, emit):
    from peregrine_amd import _lib, shimmer
    emit("GPU: shimmer.string_graph(records, min_len=%d) + all of its text; ms, median of %d (min .. max); build+text = the `sgraph` timer" % (MIN_LEN, runs))
    emit("%8s %9s %8s %7s %28s %28s %10s  %s" % ("reads", "records", "edges", "maxdeg", "one-shot call + text", "build + text (device)", "peak MiB", "share of build+text: " + " ".join(p[7:] for p in PARTS)))
    for n, chimer in [(n, c) for n in sizes for c in ((False, True) if CHIMER else (False,))]:
        recs = records(n)
        wall, dev, parts = [], [], {p: 0.0 for p in PARTS}
        for k in range(runs + 1):        # (the first run warms the workspaces up and is dropped)
            _lib.timing_reset()
            _lib.mem_ledger(reset_peak=True)
            t0 = time.perf_counter()
            with shimmer.string_graph(recs, MIN_LEN, MIN_IDT, **(dict(chimer_ordered=True) if chimer else {})) as g:
                nbytes = sum(len(p) for p in g.text())
                st = g.stats
                ch = g.chimer_stats if chimer else None
            t1 = time.perf_counter()
            if k == 0:
                continue
            wall.append((t1 - t0) * 1e3)
            dev.append(_lib.timing("sgraph")[0])
            for p in PARTS:
                parts[p] += _lib.timing(p)[0]
            peak = _lib.mem_ledger()["peak_by_tag"].get("sgraph", 0)
        tot = sum(dev)
        emit("%8d %9d %8d %7d %28s %28s %10.1f  %s" % (n, len(recs), st["edges"], st["max_out_degree"], med(wall), med(dev), peak / 2**20,
                                                     " ".join("%s %.0f%%" % (p[7:], 100 * parts[p] / tot) for p in PARTS)))
        if chimer:
            emit("%8s chimer_ordered: sgraph_chimer %.2f ms per run; %s" % ("", parts["sgraph_chimer"] / runs, ch))
        assert nbytes > 0


def reference(scripts, sizes, runs, emit):
    sys.path.insert(0, scripts)
    import ovlp_to_graph
    if CHIMER:      # the pinned pop order, as the fixtures' generator binds it
        sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
        import make_golden_chimer
        ovlp_to_graph.set = make_golden_chimer.policy_set("smallest")
    ref = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
    emit("reference: generate_string_graph (ovlp_to_graph.py, CPython %s, one thread) on the reference shmr_dedup's text of the same records; s, median of %d (min .. max)"
         % (sys.version.split()[0], runs))
    emit("%8s %9s %9s %8s %28s" % ("reads", "records", "lines", "edges", "generate_string_graph"))
    for n in sizes:
        recs = records(n)
        text = subprocess.run([ref], input=recs.tobytes(), stdout=subprocess.PIPE, check=True).stdout
        ts = []
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            try:
                with open("preads.ovl", "wb") as f:
                    f.write(text + b"-\n")
                for _ in range(runs):
                    t0 = time.perf_counter()
                    ovlp_to_graph.generate_string_graph(types.SimpleNamespace(overlap_file="preads.ovl", min_len=MIN_LEN, min_idt=MIN_IDT, lfc=False,
                                                                              disable_chimer_bridge_removal=not CHIMER))
                    ts.append(time.perf_counter() - t0)
                edges = open("sg_edges_list", "rb").read().count(b"\n")
            finally:
                os.chdir(cwd)
        emit("%8d %9d %9d %8d %28s" % (n, len(recs), text.count(b"\n"), edges, "%9.2f (%.2f .. %.2f)" % (statistics.median(ts), min(ts), max(ts))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", metavar="SCRIPTS", help="the reference tree's py/scripts: time the real function instead")
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--chimer", action="store_true", help="streams with chimeric reads; the GPU rows without and with chimer_ordered, the reference with the step")
    a = ap.parse_args()
    global CHIMER
    CHIMER = a.chimer
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.reference:
        reference(a.reference, a.sizes, a.runs, emit)
    else:
        gpu(a.sizes, a.runs, emit)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
