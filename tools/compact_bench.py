#!/usr/bin/env python
"""Overlap-stage time and HBM of a read set WITH ambiguous bases, bytes kept versus compacted (pgx_seqdb_compact_bytes).

Builds a named workload (default c4s: bench.py's recipe), gives --n-reads reads one ambiguous base each (both nibbles zero, and the mirror
image on the reverse strand), indexes it once, runs one warm-up overlap stage (which builds the 2-bit packs) and then --steps timed ones.
--mode keep: the database keeps its bytes (the only choice before compaction existed); --mode compact: compact_bytes() after the warm-up.
Prints one JSON line: ms per step (each step, median, min, max), the record count and stream checksum of the last step, and the library's
live device memory by owner (pgx_mem_ledger).  PGX_TRACE=2 in the environment shows where a step's time goes."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from peregrine_amd import _lib, formats, simreads   # noqa: E402
from peregrine_amd.shimmer import ResidentDB         # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="c4s")
    ap.add_argument("--n-reads", type=int, default=100, help="reads given an ambiguous base")
    ap.add_argument("--mode", choices=("keep", "compact"), required=True)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    sp = dict(levels=2, mc_upper=240)
    sp.update({k: v for k, v in simreads.STAGE_PARAMS.get(a.workload, {}).items() if k in sp})
    db = simreads.make_workload_torch(a.workload) if a.workload in simreads.TORCH_WORKLOADS else simreads.make_workload(a.workload)
    sd = np.array(db.seqdb, np.uint8, copy=True)
    rng = np.random.default_rng(20)
    for s in rng.choice(db.n_reads, a.n_reads, replace=False):
        o, n = int(db.roff[s]), int(db.rlen[s])
        p = int(rng.integers(0, n))
        sd[o + p] = 0
        sd[o + n - 1 - p] &= 0x0F
    db = formats.SeqDB(sd, db.rid, db.rlen, db.roff, None)
    rdb = ResidentDB(db, 0)
    ix = rdb.index(levels=sp["levels"])
    rdb.overlap(ix.top, ix.top_mc, mc_upper=sp["mc_upper"])          # warm-up: builds the packs
    compacted = False
    if a.mode == "compact":
        compacted = rdb.compact_bytes()
        assert compacted and not rdb.has_bytes
    ms = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        ov, st = rdb.overlap(ix.top, ix.top_mc, mc_upper=sp["mc_upper"])
        ms.append((time.perf_counter() - t0) * 1e3)
    _lib.mem_ledger(reset_peak=True)
    led = _lib.mem_ledger()
    print(json.dumps(dict(workload=a.workload, bases=int(db.rlen.sum(dtype=np.uint64)), reads=int(db.n_reads), reads_with_ambiguous_base=a.n_reads,
                          mode=a.mode, compacted=bool(compacted), overlap_ms=[round(x, 2) for x in ms], median_ms=round(float(np.median(ms)), 2),
                          min_ms=round(min(ms), 2), max_ms=round(max(ms), 2), n_records=int(len(ov)), stream_checksum=int(st.get("stream_checksum", 0)),
                          side_bytes=int(getattr(rdb, "side_bytes", 0)), live_bytes=int(led["live_bytes"]),
                          by_owner={k: int(v) for k, v in led["peak_by_tag"].items() if v})))
    rdb.close()


if __name__ == "__main__":
    main()
