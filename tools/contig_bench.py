#!/usr/bin/env python3
"""Times the contig layout (pgx_contigs_resident) on chains over the overlap records of a simulated read set.

  1. reads: simreads, HiFi-like (err 5e-5), --mbases of them (default 4500 = the size of configs[2]; a smaller value is recorded as such);
     one index + overlap stage on the GPU; every dovetail record whose target runs >= 300 bases beyond the overlap becomes a tiling-path row
     v = (rid0, strand0), w = (rid1, strand1), s / e = the part of w beyond t_end; rows are cut into contigs of --chain rows.  (The rows are
     valid input for the stage and exercise it at the reference's shapes -- 500-base query, a target of a few kb -- they are not a string graph.)
  2. pgx_contigs_resident: one warm-up, then the median / min / max of 5 calls (host clock around the call, which ends in a device
     synchronise and the download of the contig bytes); the library's per-kernel device times of the timed calls (pgx_timing_get).
  3. what a user does without this stage: the reference script's per-row loop over this library's single-call `ovlp_match` and
     `decode_biseq` symbols (ctypes), on the first --subset rows, one host thread.
  4. with --trace-child: only step 2 once (the command to put under `rocprofv3 --kernel-trace --stats --`).
Writes rows/s, output GB/s, the alignment and k_stitch shares of the device time, and k_stitch's bytes (2 per output base: each source byte
read, each output byte written) over its device time against --hbm-gbs (the peak of MI355X_MICROARCH, 8000) to --out.
    python tools/contig_bench.py [--mbases N] [--chain 40] [--subset 2000] [--out profiles/contig_layout.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = 500


def build(mbases, chain):
    from peregrine_amd import _lib, simreads
    from peregrine_amd.shimmer import ResidentDB
    glen = max(int(mbases * 1e6 / 30), 200_000)
    db = simreads.simulate_reads(simreads.make_genome(glen, 17), coverage=30.0, seed=9, mean_len=12000, sd_len=1500, err=5e-5)
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    ov, _ = rdb.overlap(ix.top, ix.top_mc)
    ov = np.array(ov)
    rid0, rid1 = (ov["y0"] >> np.uint64(32)).astype(np.int64), (ov["y1"] >> np.uint64(32)).astype(np.int64)
    l0, l1, x = ov["rl0"].astype(np.int64), ov["rl1"].astype(np.int64), ov["t_end"].astype(np.int64)
    keep = (ov["ovlp_type"] == 0) & (l0 >= H) & (x >= H) & (l1 - x >= 300) & (l1 < 60000)
    rid0, rid1, l1, x, s0, s1 = rid0[keep], rid1[keep], l1[keep], x[keep], ov["strand0"][keep], ov["strand1"][keep]
    n = len(x) // chain * chain
    rows = np.zeros(n, _lib.TILE_ROW_DTYPE)
    rows["ctg"] = np.arange(n) // chain
    rows["rid0"], rows["rid1"], rows["strand0"], rows["strand1"] = rid0[:n], rid1[:n], s0[:n], s1[:n]
    rows["s"] = np.where(s1[:n] == 0, x[:n], l1[:n] - x[:n])
    rows["e"] = np.where(s1[:n] == 0, l1[:n], 0)
    return db, rdb, rows


def reference_loop(db, rows):
    """path_to_contig.py's row loop over libpgx's shimmer4py symbols: returns seconds and the contigs' total length"""
    from peregrine_amd import _lib
    lib = _lib.load()
    lib.ovlp_match.restype = C.POINTER(C.c_int32 * 8)
    lib.ovlp_match.argtypes = [C.c_char_p, C.c_int32, C.c_uint8, C.c_char_p, C.c_int32, C.c_uint8, C.c_int32]
    lib.free_ovlp_match.argtypes = [C.c_void_p]
    lib.decode_biseq.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint8]
    rl, ro = db.by_rid()
    seq = db.seqdb
    read = lambda r: seq[int(ro[r]):int(ro[r]) + int(rl[r])].tobytes()
    t0 = time.perf_counter()
    total, ctg, ctg_len, segs = 0, -1, 0, []

    def flush():
        nonlocal total
        if segs:
            a = np.full(ctg_len, ord("N"), np.uint8)
            for st, b in segs:
                a[st:st + len(b)] = list(b)          # (the script assigns a list, byte by byte)
            "".join(chr(c) for c in a)
            total += ctg_len
    for r in rows:
        b0, b1, l0_, l1_ = read(r["rid0"]), read(r["rid1"]), int(rl[r["rid0"]]), int(rl[r["rid1"]])
        if r["ctg"] != ctg:
            flush()
            ctg, segs = r["ctg"], []
            buf = C.create_string_buffer(l0_)
            lib.decode_biseq(b0, buf, l0_, int(r["strand0"]))
            segs.append((0, buf.raw))
            ctg_len = l0_
        s, e = int(r["s"]), int(r["e"])
        o2 = l1_ - abs(e - s) - H
        m = lib.ovlp_match(b0[l0_ - H:], H, int(r["strand0"]), b1[o2:], l1_ - o2, int(r["strand1"]), 100)
        t_m_end, q_m_end = m.contents[6], m.contents[7]
        lib.free_ovlp_match(m)
        if r["strand1"]:
            s, e = l1_ - s, l1_ - e
        sg = e - s + H - t_m_end
        buf = C.create_string_buffer(max(sg, 1))
        lib.decode_biseq(b1[e - sg:e], buf, sg, int(r["strand1"]))
        st = ctg_len - H + q_m_end
        segs.append((st, buf.raw[:sg]))
        ctg_len = st + sg
    flush()
    return time.perf_counter() - t0, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbases", type=float, default=4500)
    ap.add_argument("--chain", type=int, default=40)
    ap.add_argument("--subset", type=int, default=2000)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--trace-child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contig_layout.txt"))
    a = ap.parse_args()
    from peregrine_amd import _lib
    db, rdb, rows = build(a.mbases, a.chain)
    data, off = rdb.contigs(rows)                       # warm-up
    if a.trace_child:
        print(f"traced call: {len(rows)} rows, {len(data)} contig bytes")
        return
    _lib.timing_reset()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        d2, _ = rdb.contigs(rows)
        times.append(time.perf_counter() - t0)
        assert d2 == data
    kt = {k: _lib.timing(k) for k in ("align1t", "tile_geom", "stitch")}
    dev_ms = sum(v[0] for v in kt.values()) / 5
    med = statistics.median(times)
    sub = rows[:a.subset // a.chain * a.chain]
    ref_s, ref_bases = reference_loop(db, sub)
    dsub, osub = rdb.contigs(sub)
    assert len(dsub) == ref_bases, (len(dsub), ref_bases)
    stitch_ms = kt["stitch"][0] / 5
    lines = [
        f"contig layout: {db.n_bases / 1e6:.0f} Mbases of reads ({db.n_reads} reads), {len(rows)} rows in {int(rows['ctg'].max()) + 1} contigs of {a.chain}, {len(data) / 1e6:.1f} MB of contigs",
        f"pgx_contigs_resident, 5 calls after a warm-up: median {med * 1e3:.1f} ms (min {min(times) * 1e3:.1f}, max {max(times) * 1e3:.1f}) = {len(rows) / med:.0f} rows/s, {len(data) / med / 1e9:.3f} GB/s of output (host clock, download included)",
        f"device time per call: align1t {kt['align1t'][0] / 5:.2f} ms ({100 * kt['align1t'][0] / 5 / dev_ms:.0f} %), tile_geom + scan {kt['tile_geom'][0] / 5:.2f} ms, k_stitch {stitch_ms:.2f} ms ({100 * stitch_ms / dev_ms:.0f} %)",
        f"k_stitch: 2 x {len(data) / 1e6:.1f} MB in {stitch_ms:.3f} ms = {2 * len(data) / stitch_ms / 1e6:.0f} GB/s = {100 * 2 * len(data) / stitch_ms / 1e6 / a.hbm_gbs:.1f} % of {a.hbm_gbs:.0f} GB/s",
        f"the script's row loop over libpgx's ovlp_match / decode_biseq, first {len(sub)} rows ({ref_bases / 1e6:.2f} MB of contigs), one host thread: {ref_s:.2f} s = {len(sub) / ref_s:.0f} rows/s; ratio of the rows/s: {len(rows) / med / (len(sub) / ref_s):.0f}x",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
