#!/usr/bin/env python3
"""Times pgx_cns_pieces -- falcon.align with trace-back, the acceptance rule and the consensus call, all on the device -- on a seeded
batch of pieces as pg_asm_cns.py meets them (tests/aln_util.bench_piece: a template, and `--cov` times its length in reads of
`--read-len` bases drawn from it and its flanks, mutated at `--rate`), and reports the device time of the aligner's counting pass,
filling pass and trace-back, of the consensus call, the trace cells per read and the device memory at the peak.  The generator and seed
are the ones whose first pieces tests/golden/make_golden_aln.py timed on the reference's align (one CPU thread; aln_cases.provenance.json,
"bench"): those numbers come from another machine and are set beside these, not divided.

    python tools/cns_align_bench.py [--pieces 256] [--t-len 50000] [--cov 30] [--read-len 15000] [--rate 0.01] [--reps 3] [--check 1] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import aln_util as AU  # noqa: E402
from peregrine_amd import _lib, shimmer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=256)
    ap.add_argument("--t-len", type=int, default=50_000)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check", type=int, default=1, help="pieces whose consensus and accepted reads are compared with the integer restatement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    t0 = time.perf_counter()
    pieces = [AU.bench_piece(rng, a.t_len, a.cov, a.read_len, a.rate) for _ in range(a.pieces)]
    gen_s = time.perf_counter() - t0
    n_reads = sum(len(r) for _, r in pieces)
    runs, peak = [], {}
    for rep in range(a.reps + 1):     # the first run is dropped (block cache, workspaces)
        st, used = {}, []
        _lib.init()
        _lib.mem_ledger(reset_peak=True)
        t0 = time.perf_counter()
        cns = shimmer.consensus_reads(pieces, 1, stats=st, used=used)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        peak = _lib.mem_ledger()["peak_by_tag"]
        if rep:
            runs.append(st)
        al, cl = st["align"], st["call"]
        print(f"run {rep}: align {al['gpu_ms']:.1f} ms (count {al['count_ms']:.1f}, fill {al['fill_ms']:.1f}, trace-back {al['back_ms']:.1f}), call {cl['gpu_ms']:.1f} ms, "
              f"wall {st['wall_ms']:.0f} ms", file=sys.stderr, flush=True)
    for p in range(min(a.check, a.pieces)):
        want, want_used, _ = AU.consensus_reads(*pieces[p], 1)
        assert cns[p] == want and used[p].tolist() == want_used, f"piece {p} differs from the restatement"
    med = lambda f: float(np.median([f(r) for r in runs]))
    st = runs[-1]
    al = st["align"]
    align_ms, call_ms = med(lambda r: r["align"]["gpu_ms"]), med(lambda r: r["call"]["gpu_ms"])
    lines = [
        f"pgx_cns_pieces: {a.pieces} pieces of {a.t_len} bases, {n_reads} reads of {a.read_len} at {a.rate * 100:g} % (aln_util.bench_piece, seed {a.seed}); "
        f"median of {a.reps} runs after one dropped",
        f"  alignments {al['n_req']} (aligned {al['n_aligned']})  reads accepted {st['n_accepted']} rejected {st['n_rejected']}  pieces by the low-coverage rule "
        f"{st['n_by_rule']} called {st['n_called']}  ({min(a.check, a.pieces)} piece(s) equal to the restatement)",
        f"  device ms, aligner: whole {align_ms:.1f}  counting {med(lambda r: r['align']['count_ms']):.1f}  filling {med(lambda r: r['align']['fill_ms']):.1f}  "
        f"trace-back {med(lambda r: r['align']['back_ms']):.1f}   consensus call: {call_ms:.1f}",
        f"  per piece: aligner {align_ms / a.pieces:.3f} ms, call {call_ms / a.pieces:.3f} ms   per alignment: {align_ms * 1e3 / al['n_req']:.2f} us",
        f"  trace cells {al['n_cells']} = {al['n_cells'] / al['n_req']:.0f} per alignment ({4 * al['n_cells'] / al['n_req']:.0f} bytes)  string bytes {al['str_bytes']} x 2  "
        f"consensus bytes {st['call']['text_bytes']}",
        f"  device memory at the peak, by owner: " + ", ".join(f"{k} {v / 2**20:.0f} MiB" for k, v in sorted(peak.items()) if v),
        f"  wall of the call (upload of {sum(len(t) + sum(len(r) for r, _ in rs) for t, rs in pieces) / 1e6:.0f} MB of sequence included) {med(lambda r: r['wall_ms']):.0f} ms"
        f"   (the batch took {gen_s:.1f} s to draw on the host)",
    ]
    try:
        b = json.load(open(AU.PROVENANCE))["bench"]
        if (b["seed"], b["t_len"], b["cov"], b["read_len"], b["rate"]) == (a.seed, a.t_len, a.cov, a.read_len, a.rate):
            lines.append(f"  reference's align, same generator and seed, first {b['pieces']} pieces, on {b['machine']} -- ANOTHER machine, not to be divided: "
                         f"{b['with_strings']} s per piece with strings, {b['without_strings']} s without, for {b['alignments_per_piece']} alignments "
                         f"(mean dist {b['mean_dist']})")
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
