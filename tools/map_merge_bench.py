#!/usr/bin/env python3
"""The map merge against GNU sort on synthetic map text: for each size, lines as shmr_map writes them with about 30 rows per
(ref_id, ref_bgn) are drawn from a seed and written to a file; `pgx_map_merge` (file to file) and `pgx_map_merge_dev` (rows resident on the
device to rows on the device) are timed against `LC_ALL=C sort -S 8g --parallel 16 -k 1 -g -k 2 -g` on the same file on this host, and the
two merged files are compared byte for byte.  Times are host clocks around calls that end in a synchronisation; the first call of the
process (block cache, first launches) is made on a small input and dropped.

  python tools/map_merge_bench.py [--sizes 1000000,10000000,100000000] [--dir DIR] [--out profiles/map_merge.txt] [--run-max N] [--per-key N]
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from peregrine_amd import _lib, shimmer  # noqa: E402

BLOCK = 2_000_000


def draw(rng, n, per_key=30):
    """n rows (n x 9 uint32): keys of about per_key rows each, the other fields of the widths a job has"""
    n_keys = max(1, n // per_key)
    ctg = rng.integers(0, 2000, n_keys, dtype=np.int64)
    pos = rng.integers(0, 20_000_000, n_keys, dtype=np.int64)
    k = rng.integers(0, n_keys, n)
    rb = rng.integers(0, 40_000, n)
    span = rng.integers(100, 3000, n)
    cols = [ctg[k], pos[k], pos[k] + span, rng.integers(0, 5_000_000, n), rb, rb + span, rng.integers(0, 2, n), rng.integers(1, 100, n), rng.integers(1, 100, n)]
    return np.stack(cols, axis=1).astype(np.uint32)


def text_of(rows) -> bytes:
    """the rows as map lines, with numpy alone: every number right-aligned in 10 places, the places in front of it dropped"""
    n = len(rows)
    buf = np.zeros((n, 9, 11), np.uint8)
    v = rows.astype(np.int64)
    nd = np.ones(v.shape, np.int64)
    for d in range(1, 10):
        nd += v >= 10 ** d
    for d in range(10):
        digit = (v // 10 ** (9 - d)) % 10
        buf[:, :, d] = np.where(10 - d <= nd, digit + ord("0"), 0)
    buf[:, :, 10] = ord(" ")
    buf[:, 8, 10] = ord("\n")
    flat = buf.reshape(-1)
    return flat[flat != 0].tobytes()


def write_case(path, n, seed, keep_rows, per_key=30):
    """the file of n lines; returns the rows (uint32, n x 9) where keep_rows"""
    rng = np.random.default_rng(seed)
    kept = []
    with open(path, "wb") as f:
        # drawn block by block, every block with contig ids of its own: ties stay inside a block
        for at in range(0, n, BLOCK):
            rows = draw(rng, min(BLOCK, n - at), per_key)
            rows[:, 0] += np.uint32(2000 * (at // BLOCK))
            f.write(text_of(rows))
            if keep_rows:
                kept.append(rows)
    return np.concatenate(kept) if keep_rows else None


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--dir", default=None, help="where the files go (default: a temporary directory)")
    ap.add_argument("--out", default=None, help="append the report to this file")
    ap.add_argument("--run-max", type=int, default=0, help="PGX_MERGE_RUN_MAX for the run (0: the library's bound)")
    ap.add_argument("--reps", type=int, default=2, help="runs of every contender (the file is in the page cache from the second on)")
    ap.add_argument("--per-key", type=int, default=30, help="rows per (ref_id, ref_bgn) on average")
    ap.add_argument("--no-sort", action="store_true", help="leave GNU sort out (a second run with another --run-max)")
    ap.add_argument("--sort-mem", default="8g")
    ap.add_argument("--sort-threads", type=int, default=16)
    a = ap.parse_args()
    import torch
    if a.run_max:
        os.environ["PGX_MERGE_RUN_MAX"] = str(a.run_max)
    d = a.dir or tempfile.mkdtemp(prefix="mapmerge_")
    os.makedirs(d, exist_ok=True)
    lib = _lib.load()
    _lib.init()
    warm = draw(np.random.default_rng(1), 100_000)
    shimmer.map_merge(warm.astype(np.int64))
    report = []

    def say(s):
        print(s, flush=True)
        report.append(s)

    sort_exe = None if a.no_sort else shutil.which("sort")
    for n in [int(x) for x in a.sizes.split(",")]:
        src, ours, theirs = os.path.join(d, f"map_{n}.dat"), os.path.join(d, f"merged_{n}.out"), os.path.join(d, f"sorted_{n}.out")
        rows, gen_ms = timed(lambda: write_case(src, n, 20261100 + n % 97, True, a.per_key))
        size = os.path.getsize(src)
        say(f"map merge: {n} lines, {size / 1e6:.0f} MB of text, about {a.per_key} rows per (ref_id, ref_bgn) (seed {20261100 + n % 97}; drawn and written in {gen_ms / 1e3:.1f} s)"
            + (f", PGX_MERGE_RUN_MAX={a.run_max}" if a.run_max else ""))
        # file to file
        ours_best = None
        for rep in range(a.reps):
            st, ms = timed(lambda: shimmer.map_merge([src], out=ours))
            ours_best = ms if ours_best is None else min(ours_best, ms)
            say(f"  pgx_map_merge file to file, run {rep + 1}: wall {ms:.0f} ms = parse {st['parse_ms']:.0f} + keys {st['key_ms']:.1f} + sort {st['sort_ms']:.1f} + ties {st['ties_ms']:.1f}"
                f" + format and write {st['format_ms']:.0f}")
        say(f"    rows {st['n_rows']}  runs {st['n_runs']} (of two rows and more {st['n_tie_runs']}, the longest {st['longest_run']})  rows by tie path: wavefront {st['rows_wave']}"
            f"  workgroup {st['rows_group']}  LSD {st['rows_lsd']}")
        # rows to rows, resident on the device
        d_in = torch.from_numpy(rows.view(np.int32)).cuda()
        d_out = torch.empty_like(d_in)
        torch.cuda.synchronize()
        for rep in range(a.reps):
            ms_st = _lib.MapMergeStats()
            _, ms = timed(lambda: _lib.check(lib.pgx_map_merge_dev(C.c_void_p(d_in.data_ptr()), n, C.c_void_p(d_out.data_ptr()), C.byref(ms_st)), "pgx_map_merge_dev"))
            say(f"  pgx_map_merge_dev rows to rows on the device, run {rep + 1}: wall {ms:.1f} ms = keys {ms_st.key_ms:.1f} + sort {ms_st.sort_ms:.1f} + ties and gather {ms_st.ties_ms:.1f}")
        del d_in, d_out, rows
        torch.cuda.empty_cache()
        if sort_exe:
            env = {"LC_ALL": "C", "PATH": os.environ.get("PATH", "")}
            cmd = [sort_exe, "-T", d, "-S", a.sort_mem, "--parallel", str(a.sort_threads), "-k", "1", "-g", "-k", "2", "-g", "-o", theirs, src]
            best = None
            for rep in range(a.reps):
                _, ms = timed(lambda: subprocess.run(cmd, check=True, env=env))
                say(f"  LC_ALL=C sort -S {a.sort_mem} --parallel {a.sort_threads} -k 1 -g -k 2 -g, run {rep + 1}: wall {ms:.0f} ms")
                best = ms if best is None else min(best, ms)
            same = subprocess.run(["cmp", "-s", ours, theirs]).returncode == 0
            say(f"  the two merged files are {'identical' if same else 'DIFFERENT'}; sort / pgx_map_merge, the best run of each: {best / ours_best:.1f}")
            os.remove(theirs)
        os.remove(src), os.remove(ours)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(report) + "\n")
    if not a.dir:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
