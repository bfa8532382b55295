#!/usr/bin/env python3
"""Times pgx_cns_job -- pg_asm_cns.py from files to FASTA: map text to rows, layout, decode of templates and reads into the ASCII pool, the
inner loop (pgx_cns_pieces' device form) and the stitch, all on the device -- on a seeded job sized like tools/cns_align_bench.py's batch:
`--contigs` contigs of `--ctg-len` bases (a piece per 50 kb of contig), `--cov` times their length in reads of `--read-len` bases on both
strands, mutated at `--rate`, map rows every `--every` bases of a read at its true place, a few bases off.  Reports the host-clock parts
of the job (layout, decode, inner loop, stitch), the device time of the aligner and of the consensus call inside the inner loop, the pool
bytes and the device memory at the peak; and beside them pgx_cns_pieces (host arrays in, text out) on the same pieces and reads, which
is what a caller had to drive with a layout of their own before.  `--pieces-root DIR` times that entry point of ANOTHER built checkout of
the project (the parent commit's, say) on the same pieces, in a child process that imports the package from DIR.  `--batch N` cuts the job
into batches of N pieces (PGX_CNS_JOB_BATCH) instead of the library's own cut.

    python tools/cns_job_bench.py [--contigs 32] [--ctg-len 400500] [--cov 30] [--read-len 15000] [--rate 0.01] [--reps 3] [--batch N]
                                  [--pieces-too 1] [--pieces-root DIR] [--out FILE]
"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = len(sys.argv) == 5 and sys.argv[1] == "--pieces-child"     # (the child imports the package of the OTHER checkout, and nothing of this one)
if not CHILD:
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import cnsjob_util as J  # noqa: E402
    from peregrine_amd import _lib, formats, shimmer  # noqa: E402


def pieces_child(root, path, reps):
    """pgx_cns_pieces of the checkout at `root` on the pickled pieces at `path`: one JSON line of the runs' stats"""
    sys.path[:0] = [root]
    from peregrine_amd import shimmer as other
    assert os.path.abspath(os.path.dirname(os.path.dirname(other.__file__))) == os.path.abspath(root), other.__file__
    pieces = pickle.load(open(path, "rb"))
    runs = []
    for rep in range(reps + 1):
        ps = {}
        t0 = time.perf_counter()
        other.consensus_reads(pieces, 1, stats=ps)
        ps["wall_ms"] = (time.perf_counter() - t0) * 1e3
        if rep:
            runs.append(ps)
    print(json.dumps(runs))


def main():
    if CHILD:
        return pieces_child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=32)
    ap.add_argument("--ctg-len", type=int, default=400_500)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--rate", type=float, default=0.01)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="pieces per batch (PGX_CNS_JOB_BATCH); 0: the library's own cut")
    ap.add_argument("--pieces-too", type=int, default=1, help="also time pgx_cns_pieces on the same pieces")
    ap.add_argument("--pieces-root", default=None, help="another built checkout of the project whose pgx_cns_pieces is timed on the same pieces")
    ap.add_argument("--pieces-label", default=None, help="what the report calls that checkout (default: its path)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.batch:
        os.environ["PGX_CNS_JOB_BATCH"] = str(a.batch)
    t0 = time.perf_counter()
    b = J.Builder(a.seed, a.rate)
    for _ in range(a.contigs):
        c = b.contig(a.ctg_len, polish=0.0)
        for _ in range(a.cov * a.ctg_len // a.read_len):
            pos = int(b.rng.integers(0, a.ctg_len - a.read_len + 1))
            b.mapped(c, pos, a.read_len, int(b.rng.integers(0, 2)), every=a.every)
    text = b.map_text(b.rng.permutation(len(b.rows)))
    rdb, cdb = b.dbs()
    gen_s = time.perf_counter() - t0
    runs, peak, fasta = [], {}, b""
    with tempfile.TemporaryDirectory() as tmp:
        rp, cp, mp, out = (os.path.join(tmp, n) for n in ("reads", "ref", "map", "cns.fa"))
        formats.write_seqdb(rp, rdb)
        formats.write_seqdb(cp, cdb)
        open(mp, "w").write(text)
        for rep in range(a.reps + 1):     # the first run is dropped (block cache, workspaces)
            _lib.init()
            _lib.mem_ledger(reset_peak=True)
            t0 = time.perf_counter()
            st = shimmer.pg_asm_cns(rp, cp, mp, 1, 0, out=out)
            st["wall_ms"] = (time.perf_counter() - t0) * 1e3
            peak = _lib.mem_ledger()["peak_by_tag"]
            if rep:
                runs.append(st)
            print(f"run {rep}: job {st['total_ms']:.0f} ms (layout {st['layout_ms']:.1f}, decode {st['decode_ms']:.1f}, inner loop {st['pieces_ms']:.1f}, stitch "
                  f"{st['stitch_ms']:.1f}), wall with the databases' load {st['wall_ms']:.0f} ms", file=sys.stderr, flush=True)
        fasta = open(out, "rb").read()
    med = lambda f: float(np.median([f(r) for r in runs]))
    st = runs[-1]
    cut = f", batches of {a.batch} pieces" if a.batch else ""
    lines = [
        f"pgx_cns_job: {a.contigs} contigs of {a.ctg_len} bases, {rdb.n_reads} reads of {a.read_len} at {a.rate * 100:g} %, {len(b.rows)} map rows of "
        f"{len(text) / 1e6:.0f} MB (cnsjob_util.Builder, seed {a.seed}){cut}; median of {a.reps} runs after one dropped",
        f"  rows kept {st['n_rows']}  contigs {st['n_contigs']}  pieces {st['n_pieces']} (by the low-coverage rule {st['n_by_rule']}, called {st['n_called']})  read entries "
        f"{st['n_reads']} (accepted {st['n_accepted']})  batches {st['n_batches']}  FASTA bytes {len(fasta)}",
        f"  host clock around the parts, ms: job {med(lambda r: r['total_ms']):.1f} = layout {med(lambda r: r['layout_ms']):.1f} + decode {med(lambda r: r['decode_ms']):.1f} "
        f"+ inner loop {med(lambda r: r['pieces_ms']):.1f} + stitch and FASTA {med(lambda r: r['stitch_ms']):.1f}",
        f"  device ms inside the inner loop and the stitch: aligner {med(lambda r: r['align']['gpu_ms']):.1f}  consensus call {med(lambda r: r['call']['gpu_ms']):.1f}",
        f"  pool bytes decoded {st['pool_bytes']} ({st['pool_bytes'] / max(1, st['n_batches']) / 2**20:.0f} MiB per batch; a read is decoded once per entry)",
        f"  device memory at the peak, by owner: " + ", ".join(f"{k} {v / 2**20:.0f} MiB" for k, v in sorted(peak.items()) if v),
        f"  wall of the file-level call (both databases loaded from files, the map parsed, the FASTA written) {med(lambda r: r['wall_ms']):.0f} ms"
        f"   (the job took {gen_s:.1f} s to draw on the host)",
    ]
    if a.pieces_too or a.pieces_root:
        # the same pieces through the exported pgx_cns_pieces: layout and decode on the host (not timed), ASCII pool uploaded by the call
        t0 = time.perf_counter()
        lay = J.layout(J.parse_map(text), {int(r): int(n) for r, n in zip(cdb.rid, cdb.rlen)})
        pieces, cache = [], {}
        for c in lay:
            ctg = J.seq_of(cdb, c["ctg"])
            for g in c["groups"]:
                reads = []
                for rd, strand, shift in g["entries"]:
                    if (rd, strand) not in cache:
                        cache[(rd, strand)] = J.seq_of(rdb, rd, strand)
                    reads.append((cache[(rd, strand)], shift))
                pieces.append((ctg[g["left"] - J.FLANK:g["right"]], reads))
        host_s = time.perf_counter() - t0
        pruns = []
        for rep in range(a.reps + 1 if a.pieces_too else 0):
            ps = {}
            t0 = time.perf_counter()
            shimmer.consensus_reads(pieces, 1, stats=ps)
            ps["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if rep:
                pruns.append(ps)
        pm = lambda f: float(np.median([f(r) for r in pruns]))
        if a.pieces_root:
            with tempfile.TemporaryDirectory() as tmp:
                path = os.path.join(tmp, "pieces.pickle")
                pickle.dump(pieces, open(path, "wb"), protocol=4)
                env = {k: v for k, v in os.environ.items() if k not in ("PGX_LIB", "PGX_CNS_JOB_BATCH")}
                out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--pieces-child", os.path.abspath(a.pieces_root), path, str(a.reps)], env=env)
            oruns = json.loads(out.decode().strip().splitlines()[-1])
            om = lambda f: float(np.median([f(r) for r in oruns]))
            lines.append(f"  pgx_cns_pieces of {a.pieces_label or 'the checkout at ' + a.pieces_root} on the same {len(pieces)} pieces and {sum(len(r) for _, r in pieces)} entries, in a child "
                         f"process: wall {om(lambda r: r['wall_ms']):.0f} ms, aligner {om(lambda r: r['align']['gpu_ms']):.1f} ms, consensus call "
                         f"{om(lambda r: r['call']['gpu_ms']):.1f} ms")
    if a.pieces_too:
        lines.append(f"  pgx_cns_pieces on the same {len(pieces)} pieces and {sum(len(r) for _, r in pieces)} entries (host arrays in, text out): wall {pm(lambda r: r['wall_ms']):.0f} ms, "
                     f"aligner {pm(lambda r: r['align']['gpu_ms']):.1f} ms, consensus call {pm(lambda r: r['call']['gpu_ms']):.1f} ms   (layout and decode in Python on "
                     f"the host took {host_s:.1f} s, not counted)")
    out_text = "\n".join(lines) + "\n"
    sys.stdout.write(out_text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(out_text)


if __name__ == "__main__":
    main()
