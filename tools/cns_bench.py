#!/usr/bin/env python3
"""Times pgx_cns_call on a seeded batch of synthetic pieces (tests/cns_util.synthetic_piece: the back-bone and `--reads` reads per piece,
alignment columns drawn without an aligner) and reports device time per piece and per tag.  The generator and seed are the ones whose
first pieces tests/golden/make_golden_cns.py timed on the reference (one CPU thread; cns_cases.provenance.json, "bench"): the two sets
of numbers come from different machines and are set side by side in profiles/cns_call.txt, not divided.

    python tools/cns_bench.py [--pieces 256] [--t-len 50000] [--reads 30] [--reps 3] [--check 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cns_util as CU  # noqa: E402
from peregrine_amd import shimmer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=256)
    ap.add_argument("--t-len", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=30)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=1, help="pieces whose consensus is compared with the integer restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    t0 = time.perf_counter()
    pieces = [CU.synthetic_piece(rng, a.t_len, a.reads) for _ in range(a.pieces)]
    gen_s = time.perf_counter() - t0
    runs = []
    for rep in range(a.reps + 1):     # the first run is dropped (block cache, workspaces)
        st = {}
        t0 = time.perf_counter()
        cns = shimmer.consensus(pieces, 1, stats=st)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        if rep:
            runs.append(st)
        print(f"run {rep}: device {st['gpu_ms']:.1f} ms (tags {st['tags_ms']:.1f}, sort {st['sort_ms']:.1f}, score {st['score_ms']:.1f}, back {st['back_ms']:.1f}), wall {st['wall_ms']:.0f} ms",
              file=sys.stderr, flush=True)
    for p in range(min(a.check, a.pieces)):
        assert cns[p] == CU.consensus(*pieces[p]), f"piece {p} differs from the restatement"
    med = lambda k: float(np.median([r[k] for r in runs]))
    st = runs[-1]
    lines = [
        f"pgx_cns_call: {a.pieces} pieces of {a.t_len} bases, back-bone + {a.reads} reads each (cns_util.synthetic_piece, seed {a.seed}); median of {a.reps} runs after one dropped",
        f"  alignments {st['n_aln']}  tags {st['n_tags']}  edges {st['n_edges']}  nodes {st['n_nodes']}  consensus bytes {st['text_bytes']}  ({min(a.check, a.pieces)} piece(s) equal to the restatement)",
        f"  device ms: whole call {med('gpu_ms'):.1f}  tags + keys {med('tags_ms'):.1f}  sorts + edges {med('sort_ms'):.1f}  scoring {med('score_ms'):.1f}  back-track {med('back_ms'):.1f}",
        f"  per piece {med('gpu_ms') / a.pieces:.3f} ms   per tag {med('gpu_ms') * 1e6 / max(1, st['n_tags']):.3f} ns   wall of the call (uploads of {sum(len(x[0]) for _, al in pieces for x in al) * 2 / 1e6:.0f} MB of strings included) {med('wall_ms'):.0f} ms",
        f"  (the batch took {gen_s:.1f} s to draw on the host)",
    ]
    try:
        b = json.load(open(CU.PROVENANCE))["bench"]
        if (b["seed"], b["t_len"], b["reads"]) == (a.seed, a.t_len, a.reads):
            lines.append(f"  reference, same generator and seed, first {b['pieces']} pieces, on {b['machine']}: "
                         f"{b['reference_seconds_per_piece']} s per piece for {b['tags_per_piece']} tags (get_align_tags + get_cns_from_align_tags)")
    except (OSError, KeyError):
        pass
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
