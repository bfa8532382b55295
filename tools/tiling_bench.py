#!/usr/bin/env python3
"""Times the tiling-path stage (shimmer.graph_to_path: sg_edges_list, utg_data, ctg_paths -> the two tiling path files) on synthetic
chains and bubbles of growing size.  The three files are built here, deterministically from the size, so that two machines time the same
input; half of the lines of sg_edges_list are TR lines, as in a real file.

    python tools/tiling_bench.py [--sizes 100000 1000000 10000000] [--runs 3] [--out profiles/tiling.txt]
        on a GPU: device ms of the stage and of each part (pgx_timing_get: tiling_parse, _index, _paths, _text), the host's time over the
        two small files and the bundles (statistics: host_us), wall time, the peak of the `tiling` ledger tag; medians
    python tools/tiling_bench.py --script path/to/graph_to_path.py [...]
        on a CPU: the wall time of that script on the same files, run as a child process in the files' directory
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
SIZES = [100_000, 1_000_000, 10_000_000]
PARTS = ("tiling_parse", "tiling_index", "tiling_paths", "tiling_text")
CHAIN = 1000   # edges of a unitig


def nm(r, end="E"):
    return "%09d:%s" % (r, end)


def build(n_lines, shape, d):
    """about n_lines lines of sg_edges_list: contigs of 10 unitigs of CHAIN edges; `bubbles`: a two-way bubble between any two unitigs"""
    sg, utg, ctg = [], [], []
    rid, n_g, c = 1, 0, 0
    while 2 * n_g < n_lines:
        utgs, first = [], rid
        for k in range(10):
            nodes = list(range(rid, rid + CHAIN + 1))
            rid += CHAIN
            for a, b in zip(nodes[:-1], nodes[1:]):
                s = 1000 + (a * 7919) % 5000
                sg.append("%s %s %09d %5d %5d %5d %5.2f G\n" % (nm(a), nm(b), b, s, s + 500 + a % 1500, 4000 + (a * 31) % 3000, 96 + (a % 40) / 10.0))
                sg.append("%s %s %09d %5d %5d %5d %5.2f TR\n" % (nm(a), nm(b + 2), b + 2, s, s + 2500, 3000, 97.5))
            n_g += CHAIN
            utgs.append("%s~%s~%s" % (nm(nodes[0]), nm(nodes[1]), nm(nodes[-1])))
            utg.append("%s %s %s simple %d %d %s\n" % (nm(nodes[0]), nm(nodes[1]), nm(nodes[-1]), 0, 0, "~".join(nm(x) for x in nodes)))
            if shape == "bubbles" and k < 9:
                s_, t_, subs = rid, rid + 5, []
                for way, inner in enumerate(([rid + 1, rid + 2], [rid + 3, rid + 4])):
                    path = [s_] + inner + [t_]
                    for a, b in zip(path[:-1], path[1:]):
                        sg.append("%s %s %09d %5d %5d %5d %5.2f G\n" % (nm(a), nm(b), b, 100, 900 + way, 5000 + 100 * way + (a + b) % 97, 99.0))
                    n_g += 3
                    subs.append("%s~%s~%s" % (nm(path[0]), nm(path[1]), nm(path[-1])))
                    utg.append("%s %s %s simple 0 0 %s\n" % (nm(path[0]), nm(path[1]), nm(path[-1]), "~".join(nm(x) for x in path)))
                utg.append("%s NA %s compound 0 0 %s\n" % (nm(s_), nm(t_), "|".join(subs)))
                utgs.append("%s~NA~%s" % (nm(s_), nm(t_)))
                rid += 5
        ctg.append("%06dF ctg_linear %s %s 0 0 %s\n" % (c, utgs[0], nm(rid), "|".join(utgs)))
        rid += 10
        c += 1
    for fn, lines in (("sg_edges_list", sg), ("utg_data", utg), ("ctg_paths", ctg)):
        with open(os.path.join(d, fn), "w") as f:
            f.write("".join(lines))
    return len(sg), [os.path.getsize(os.path.join(d, fn)) for fn in ("sg_edges_list", "utg_data", "ctg_paths")]


def med(xs):
    return "%9.2f (%.2f .. %.2f)" % (statistics.median(xs), min(xs), max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--script", help="time this graph_to_path.py on the CPU instead of the library on the GPU")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    if a.script:
        emit("CPU: %s on the same files; wall s, median of %d (min .. max)" % (os.path.basename(a.script), a.runs))
        emit("%-8s %10s %10s %28s" % ("shape", "sg lines", "sg MB", "wall s"))
    else:
        from peregrine_amd import _lib, shimmer
        emit("GPU: shimmer.graph_to_path (files in, both files out); device ms (the `tiling` timer and its parts), host ms over utg_data, ctg_paths and the bundles; median of %d (min .. max)"
             % a.runs)
        emit("%-8s %10s %8s %8s %10s %28s %28s %28s %28s %28s %28s %28s %9s" % ("shape", "sg lines", "sg MB", "small MB", "p+a rows", "wall ms", "tiling (device)", "parse", "index", "paths",
                                                                          "text", "host ms", "peak MiB"))
    for n in a.sizes:
        for shape in ("chains", "bubbles"):
            with tempfile.TemporaryDirectory() as d:
                n_sg, sizes = build(n, shape, d)
                inputs = [os.path.join(d, fn) for fn in ("sg_edges_list", "utg_data", "ctg_paths")]
                if a.script:
                    wall = []
                    for _ in range(a.runs):
                        t0 = time.perf_counter()
                        subprocess.run([sys.executable, os.path.abspath(a.script)], cwd=d, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                        wall.append(time.perf_counter() - t0)
                    emit("%-8s %10d %10.1f %28s" % (shape, n_sg, sizes[0] / 1e6, med(wall)))
                    continue
                wall, dev, host, parts = [], [], [], {p: [] for p in PARTS}
                for k in range(a.runs + 1):      # (the first run warms the workspaces up and is dropped)
                    _lib.timing_reset()
                    _lib.mem_ledger(reset_peak=True)
                    t0 = time.perf_counter()
                    st = shimmer.graph_to_path(*inputs, os.path.join(d, "p"), os.path.join(d, "a"))
                    t1 = time.perf_counter()
                    if k == 0:
                        continue
                    wall.append((t1 - t0) * 1e3), dev.append(_lib.timing("tiling")[0]), host.append(st["host_us"] / 1e3)
                    for p in PARTS:
                        parts[p].append(_lib.timing(p)[0])
                    peak = _lib.mem_ledger()["peak_by_tag"].get("tiling", 0)
                emit("%-8s %10d %8.1f %8.1f %10d %28s %28s %28s %28s %28s %28s %28s %9.1f" % (shape, n_sg, sizes[0] / 1e6, (sizes[1] + sizes[2]) / 1e6, st["p_rows"] + st["a_rows"], med(wall),
                                                                                        med(dev), *(med(parts[p]) for p in PARTS), med(host), peak / 2**20))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
