#!/usr/bin/env python3
"""The shimmer chain alignment of a back-bone against its reads: pgx_shmr_aln_batch on the GPU against the REAL shmr_aln on one CPU thread.

The workload is the one py/peregrine/utils.py's get_cns_from_reads sets up: a seeded back-bone (default 50 kb) and reads of it (default 300 of
15 kb, uniformly placed, 1 % error: substitutions, insertions and deletions in equal parts), all sketched on the device with w = 80, k = 16
and reduced twice by 3 (the script's level-2 shimmers), then list 0 = the back-bone against every read with the script's defaults
(max_diff 100, max_dist 1200, max_repeat 1).  Timed, on the same lists:
  - shimmer.shimmer_alns, host clock around the call (it ends in a synchronisation), and the library's own split of it: upload + index of
    side 0, bounds + walk, CSR + download.  The first call of the process is made and dropped.
  - shmr_aln + free_shmr_alns of oracle/_ref/libshimmer_ref.so (the reference's src/shmr_align.c as `make -C oracle ref` compiles it),
    pair after pair on one thread through ctypes, the lists already in memory.
The chains of both are compared element for element.  No threshold is set; the report says what was measured.

  python tools/shmr_aln_bench.py [--backbone 50000] [--reads 300] [--read-len 15000] [--error 0.01] [--reps 5] [--out profiles/shmr_aln.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from peregrine_amd import shimmer  # noqa: E402
from peregrine_amd.formats import SeqDB  # noqa: E402

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libshimmer_ref.so")


class KVec(C.Structure):   # kvec_t(T): {size_t n, m; T *a}
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class ShmrAln(C.Structure):   # shmr_aln_t
    _fields_ = [("idx0", KVec), ("idx1", KVec)]


def mutate(rng, codes, rate):
    """codes (0..3) with substitutions, insertions and deletions, rate / 3 each"""
    r = rng.random(len(codes))
    out = []
    for c, x in zip(codes.tolist(), r.tolist()):
        if x < rate / 3:
            out.append((c + int(rng.integers(1, 4))) % 4)
        elif x < 2 * rate / 3:
            out.append(c), out.append(int(rng.integers(0, 4)))
        elif x >= rate:
            out.append(c)
    return np.array(out, np.int64)


def encode(codes):
    """the seqdb bytes of a sequence of codes: the base in the low nibble, the reverse complement's base at the same place in the high one"""
    codes = np.asarray(codes, np.int64)
    return ((np.uint8(1) << codes.astype(np.uint8)) | ((np.uint8(8) >> codes[::-1].astype(np.uint8)) << np.uint8(4))).astype(np.uint8)


def make_workload(seed, backbone, n_reads, read_len, error):
    rng = np.random.default_rng(seed)
    bb = rng.integers(0, 4, backbone)
    seqs = [bb]
    for _ in range(n_reads):
        a = int(rng.integers(0, max(1, backbone - read_len + 1)))
        seqs.append(mutate(rng, bb[a:a + read_len], error))
    lens = np.array([len(s) for s in seqs], np.uint32)
    off = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return SeqDB(np.concatenate([encode(s) for s in seqs]), np.arange(len(seqs), dtype=np.uint32), lens, off, [f"s{i}" for i in range(len(seqs))])


def level2_lists(db, w=80, k=16, r=3):
    """every sequence's level-2 shimmers, sketched and reduced on the device"""
    rdb = shimmer.ResidentDB(db, None)
    try:
        mm = shimmer.mm_reduce(shimmer.mm_reduce(rdb.sketch(np.arange(db.n_reads), w, k), r), r)
    finally:
        rdb.close()
    rid = (mm["y"] >> np.uint64(32)).astype(np.int64)
    return [np.ascontiguousarray(mm[rid == i]) for i in range(db.n_reads)]


def load_reference():
    if not os.path.exists(REF_SO):
        raise SystemExit(f"{REF_SO} is not there: `make -C oracle ref` builds it where the reference's sources are")
    lib = C.CDLL(REF_SO)
    lib.shmr_aln.restype = C.POINTER(KVec)
    lib.shmr_aln.argtypes = [C.POINTER(KVec), C.POINTER(KVec), C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.free_shmr_alns.argtypes = [C.POINTER(KVec)]
    return lib


def reference_run(lib, mm0, lists1, keep, max_diff=100, max_dist=1200, max_repeat=1):
    """shmr_aln + free_shmr_alns per pair on this thread: the seconds of the loop (keep: the chains instead, untimed)"""
    v0 = KVec(len(mm0), len(mm0), mm0.ctypes.data)
    vs = [KVec(len(m), len(m), m.ctypes.data) for m in lists1]
    chains = []
    t = time.perf_counter()
    for v1 in vs:
        alns = lib.shmr_aln(C.byref(v0), C.byref(v1), 0, max_diff, max_dist, max_repeat)
        if keep:
            arr = C.cast(alns.contents.a, C.POINTER(ShmrAln))
            take = lambda kv: np.ctypeslib.as_array(C.cast(kv.a, C.POINTER(C.c_uint32)), (kv.n,)).tolist() if kv.n else []
            chains.append([(take(arr[i].idx0), take(arr[i].idx1)) for i in range(alns.contents.n)])
        lib.free_shmr_alns(alns)
    return chains if keep else time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", type=int, default=50_000)
    ap.add_argument("--reads", type=int, default=300)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=20261121)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the report to this file")
    a = ap.parse_args()
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    ref = load_reference()
    lists = level2_lists(make_workload(a.seed, a.backbone, a.reads, a.read_len, a.error))
    mm0, lists1 = lists[0], lists[1:]
    say(f"shmr_aln: a back-bone of {a.backbone} bases ({len(mm0)} level-2 shimmers, w 80, k 16, reduced twice by 3) against {a.reads} reads of {a.read_len} at "
        f"{100 * a.error:g} % error ({sum(len(m) for m in lists1)} shimmers, {min(len(m) for m in lists1)} .. {max(len(m) for m in lists1)} a read), seed {a.seed}; "
        f"max_diff 100, max_dist 1200, max_repeat 1")
    shimmer.shimmer_alns(mm0, lists1)   # the first call of the process: dropped
    best = None
    for rep in range(a.reps):
        st = {}
        t = time.perf_counter()
        got = shimmer.shimmer_alns(mm0, lists1, stats=st)
        ms = (time.perf_counter() - t) * 1e3
        say(f"  shimmer.shimmer_alns, run {rep + 1}: wall {ms:.2f} ms; in the library {st['gpu_ms']:.2f} ms = upload + index of side 0 {st['index_ms']:.2f} + bounds + walk "
            f"{st['walk_ms']:.2f} + CSR + download {st['unroll_ms']:.2f}")
        best = (ms, st) if best is None or ms < best[0] else best
    st = best[1]
    say(f"    pairs {st['n_pairs']}  candidates bound {st['n_candidates']}  chains {st['n_chains']}  elements {st['n_elems']}  pairs stopped by the small-chain count {st['n_stopped']}")
    ref_s = [reference_run(ref, mm0, lists1, False) for _ in range(a.reps)]
    for rep, s in enumerate(ref_s):
        say(f"  the reference's shmr_aln + free_shmr_alns, {a.reads} pairs on one thread, run {rep + 1}: {s * 1e3:.2f} ms")
    want = reference_run(ref, mm0, lists1, True)
    same = [[(x.tolist(), y.tolist()) for x, y in ch] for ch in got] == want
    say(f"  the chains of the two are {'identical' if same else 'DIFFERENT'}; the longest chain of a pair has {max((max((len(x) for x, _ in ch), default=0) for ch in want), default=0)} elements, "
        f"{sum(len(ch) for ch in want) / max(1, len(want)):.1f} chains a pair")
    say(f"  reference / shimmer_alns, the best run of each: {min(ref_s) * 1e3 / best[0]:.2f} (wall), {min(ref_s) * 1e3 / best[1]['gpu_ms']:.2f} (against the library's own time)")
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(report) + "\n")
    if not same:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
