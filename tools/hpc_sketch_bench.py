#!/usr/bin/env python3
"""The homopolymer-compressed (hpc) sketch against its yardstick, the plain general index path on the same reads:
ResidentDB.index(want_l0=True) at w = 80, k = 16 (sketch kernel, one list-wide reduce per level, counts; no fused kernel) with and
without hpc=True.  gpu_ms of the call, median of 5 runs after 2 warm-ups; L0 / L2 sizes of both; the overlap records one chunk makes
of each L2 list.  The read set is the c4s recipe (repeat families, tandem arrays, homopolymer runs, 30x) on a genome of genome_mb Mb
(default 40: 1.2 Gbases).   python tools/hpc_sketch_bench.py [genome_mb=40] [overlap=1]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from peregrine_amd import simreads   # noqa: E402
from peregrine_amd.shimmer import ResidentDB   # noqa: E402

gmb = float(sys.argv[1]) if len(sys.argv) > 1 else 40.0
with_overlap = (int(sys.argv[2]) if len(sys.argv) > 2 else 1) != 0
seq, total, rlen = simreads.make_workload_resident("c4s", genome_mb=gmb)
rid = np.arange(len(rlen), dtype=np.uint32)
roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
rdb = ResidentDB.adopt_device(seq, total, rid, rlen, roff, 0)
print(f"read set: c4s recipe on {gmb:g} Mb, {len(rlen)} reads, {total} bases", flush=True)
out = dict(genome_mb=gmb, reads=int(len(rlen)), bases=int(total))
# plain: the yardstick (at w = 80 its sketch is k_sketch_wave, the in-register closed form); plain_w81: the same path one window size
# further, where the sketch is k_sketch_general -- the kernel k_sketch_hpc shares its shape and its window passes with
for name, hpc, w in (("plain", False, 80), ("plain_w81", False, 81), ("hpc", True, 80)):
    ms = []
    for it in range(7):
        ix = rdb.index(want_l0=True, hpc=hpc, window=w)
        if it >= 2:
            ms.append(ix.ms)
    spans = ix.l0["x"] & np.uint64(0xFF)
    out[name] = dict(gpu_ms=[round(m, 2) for m in ms], median_ms=round(statistics.median(ms), 2), l0=int(len(ix.l0)), l2=int(len(ix.top)),
                     redone_reads=int(ix.reads_literal), span_min=int(spans.min()), span_max=int(spans.max()), span_above_k=round(float((spans > 16).mean()), 4))
    print(f"{name}: index(want_l0=True) gpu_ms {out[name]['gpu_ms']} median {out[name]['median_ms']}  L0 {len(ix.l0)}  L2 {len(ix.top)}  "
          f"reads sketched a second time {ix.reads_literal}  spans {spans.min()}..{spans.max()}, above k: {100 * (spans > 16).mean():.1f} %", flush=True)
    if with_overlap and w == 80:
        ov, st = rdb.overlap(ix.top, ix.top_mc)
        out[name]["overlap_records"] = int(len(ov))
        print(f"{name}: overlap records (one chunk, default parameters) {len(ov)}", flush=True)
    del ix
out["ratio"] = round(out["hpc"]["median_ms"] / out["plain"]["median_ms"], 3)
out["ratio_w81"] = round(out["hpc"]["median_ms"] / out["plain_w81"]["median_ms"], 3)
print(f"hpc / plain at w = 81 (k_sketch_general): {out['ratio_w81']:.3f} x")
print(f"hpc / plain: {out['ratio']:.3f} x   ({total / out['hpc']['median_ms'] / 1e6:.2f} vs {total / out['plain']['median_ms'] / 1e6:.2f} Gbases/s)")
print(json.dumps(out))
rdb.close()
