#!/usr/bin/env python3
"""Times the contig-path stage (Unitigs.contig_paths() + both of its texts) on hand-made string graphs of growing size: a chain with a
short side branch every 50 reads (each branch a `spur:2`, the chain one contig of many unitigs) and a chain of bubbles (each a compound
unitig).  The inputs are edge records built here as arrays; nothing else is read.  Per size: the unitigs, then `runs` times the contig
paths and their texts -- device time of the stage and of each part (pgx_timing_get: ctg_paths_graph, _clean, _walk, _text; _clean is
host work between two events, _walk the device walks plus the host's claim), host_us of the statistics, medians with the spread, the peak of the `ctg_paths` ledger tag.

    python tools/ctg_paths_bench.py [--sizes 10000 100000 1000000] [--runs 3] [--out profiles/ctg_paths.txt]
    python tools/ctg_paths_bench.py --reference SCRIPTS_DIR [--sizes 10000 100000]     (no GPU: the second half of the reference's
        ovlp_to_graph.py on the same graphs, run in place with its string graph loaded from the sg_edges_list text; CPU seconds of
        whatever machine this runs on -- not a same-machine ratio)
"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np  # noqa: E402

SIZES = [10_000, 100_000, 1_000_000]
PARTS = ("ctg_paths_graph", "ctg_paths_clean", "ctg_paths_walk", "ctg_paths_text")
EDGE_DTYPE = np.dtype([("v_rid", "<u4"), ("w_rid", "<u4"), ("label_rid", "<u4"), ("sp", "<i4"), ("tp", "<i4"), ("v_end", "u1"), ("w_end", "u1"),
                       ("type", "u1"), ("pad", "u1"), ("score", "<i8"), ("idt_tenths", "<i8")])   # pgx_sgraph_edge


def edges_of(a, b, length):
    """G edge records: read a[i]'s E end -> read b[i]'s E end, each followed by its reverse"""
    n = len(a)
    e = np.zeros(2 * n, EDGE_DTYPE)
    e["v_rid"][0::2], e["w_rid"][0::2], e["v_end"][0::2], e["w_end"][0::2], e["tp"][0::2] = a, b, 1, 1, length
    e["v_rid"][1::2], e["w_rid"][1::2], e["sp"][1::2] = b, a, length
    e["label_rid"], e["idt_tenths"] = e["w_rid"], 999
    e["score"] = np.repeat(length.astype(np.int64) - np.arange(n) % 97, 2)
    return e


def shapes(n):
    """name -> edge records of about n G edges"""
    half = n // 2
    # a chain of reads 0 .. c with a branch (2 reads, 2,000 each) into every 50th read
    c = half * 50 // 52
    k = np.arange(50, c, 50)
    a = np.concatenate([np.arange(c), c + 1 + 2 * np.arange(len(k)), c + 2 + 2 * np.arange(len(k))])
    b = np.concatenate([np.arange(1, c + 1), c + 2 + 2 * np.arange(len(k)), k])
    ln = np.concatenate([np.full(c, 30000), np.full(2 * len(k), 2000)])
    spurs = edges_of(a, b, ln)
    # bubbles: s -> x1 -> x2 -> t and s -> y1 -> y2 -> t (3,000 and 3,100 an edge), then t -> . -> the next s (30,000 each): 8 edges, 7 reads apiece
    m = half // 8
    base = 7 * np.arange(m)
    a = (base[:, None] + np.array([0, 1, 2, 0, 3, 4, 5, 6])).ravel()
    b = (base[:, None] + np.array([1, 2, 5, 3, 4, 5, 6, 7])).ravel()
    ln = np.tile(np.array([3000, 3000, 3000, 3100, 3100, 3100, 30000, 30000]), m)
    bubbles = edges_of(a, b, ln)
    return {"chain + spurs": spurs, "bubbles": bubbles}


def med(xs):
    return "%9.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def sg_text(e) -> bytes:
    nm = lambda r, end: "%09d:%s" % (r, "BE"[end])   # noqa: E731
    return "".join("%s %s %09d %5d %5d %5d %5.2f G\n" % (nm(x["v_rid"], x["v_end"]), nm(x["w_rid"], x["w_end"]), x["label_rid"], x["sp"], x["tp"], x["score"], 99.9) for x in e).encode()


LOADER = '''
def _load(args):
    import networkx as nx
    g, edge_data = nx.DiGraph(), {}
    for ln in open("sg_edges_list"):
        v, w, rid, sp, tp, score, idt, ty = ln.split()
        if ty != "G":
            continue
        sp, tp, score = int(sp), int(tp), int(score)
        g.add_edge(v, w, label="%s:%d-%d" % (rid, sp, tp), length=abs(sp - tp), score=score)
        edge_data[(v, w)] = (rid, sp, tp, abs(sp - tp), score, float(idt), ty)
        g.nodes[w]["best_in"] = v
    return g, g.reverse(), edge_data
'''


def reference(scripts, sizes, emit):
    emit("CPU, this machine (%d cores; one is used): the second half of the reference's ovlp_to_graph.py (from its loaded string graph to utg_data and ctg_paths), "
         "run in place, wall seconds of the function alone" % os.cpu_count())
    for n in sizes:
        for name, e in shapes(n).items():
            with tempfile.TemporaryDirectory() as tmp:
                with open(os.path.join(tmp, "sg_edges_list"), "wb") as f:
                    f.write(sg_text(e))
                code = ("import os, runpy, sys, time\nos.chdir(%r)\ng = runpy.run_path(%r, run_name='ref')\nfn = g['ovlp_to_graph']\n%s\nsg = _load(None)\n"
                        "fn.__globals__['generate_string_graph'] = lambda a: sg\nt0 = time.perf_counter()\nfn(None)\nsys.stderr.write('%%.2f' %% (time.perf_counter() - t0))\n"
                        % (tmp, os.path.join(scripts, "ovlp_to_graph.py"), LOADER))
                p = subprocess.run([sys.executable, "-c", code], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=dict(os.environ, PYTHONHASHSEED="1"))
                emit("%-15s %9d G edges %10s s" % (name, len(e), p.stderr.strip().split("\n")[-1] if p.returncode == 0 else "failed"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--reference", metavar="SCRIPTS_DIR")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.reference:
        reference(a.reference, a.sizes, emit)
    else:
        from peregrine_amd import _lib, shimmer
        emit("GPU: Unitigs.contig_paths() + utg_data + ctg_paths of hand-made edge records; device ms (the `ctg_paths` timer and its parts; clean is host work, walk the device walks plus the claim on the host), "
             "median of %d (min .. max)" % a.runs)
        emit("%-15s %9s %8s %8s %8s %9s %8s %30s %30s %30s %30s %30s %30s %30s %9s" % ("shape", "G edges", "unitigs", "spur:2", "compound", "ctg lines", "text MB", "wall: paths + texts",
                                                                                  "ctg_paths (device)", "graph", "clean", "walk", "text", "host_us / 1000", "peak MiB"))
        for n in a.sizes:
            for name, e in shapes(n).items():
                with shimmer.unitigs(e) as u:
                    wall, dev, host, parts = [], [], [], {p: [] for p in PARTS}
                    for k in range(a.runs + 1):      # (the first run warms the workspaces up and is dropped)
                        _lib.timing_reset()
                        _lib.mem_ledger(reset_peak=True)
                        t0 = time.perf_counter()
                        with u.contig_paths() as c:
                            nbytes = sum(len(p) for p in c.utg_pieces()) + sum(len(p) for p in c.ctg_pieces())
                            st = c.stats
                        t1 = time.perf_counter()
                        if k == 0:
                            continue
                        wall.append((t1 - t0) * 1e3)
                        dev.append(_lib.timing("ctg_paths")[0])
                        host.append(st["host_us"] / 1e3)
                        for p in PARTS:
                            parts[p].append(_lib.timing(p)[0])
                        peak = _lib.mem_ledger()["peak_by_tag"].get("ctg_paths", 0)
                emit("%-15s %9d %8d %8d %8d %9d %8.1f %30s %30s %30s %30s %30s %30s %30s %9.1f" % (name, len(e), st["unitigs"], st["spur2"], st["compound"], st["ctg_lines"], nbytes / 1e6,
                                                                                              med(wall), med(dev), *(med(parts[p]) for p in PARTS), med(host), peak / 2**20))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
