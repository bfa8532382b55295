#!/usr/bin/env python3
"""bench.py -- SHIMMER index + read-overlap hot path on MI355X.

One "step" = one full pass of the hot path over the synthetic read set: index stage (sketch L0 -> L1 -> L2 + counts)
then overlap stage (pair build, bucket order, greedy best-n with GPU banded O(ND) confirmation), with the seqdb
already resident in HBM.

Two families of workloads:
  * c4 (BASELINE configs[3] at FULL size, the configuration the metric is quoted on: a 3.1 Gb repeat-seeded genome x 30x = 93 Gbases,
    index_nchunk = ovlp_nchunk = 8 as pg_run.py runs it): ONE read set, every rank holds the whole seqdb in HBM, the job's 8 index
    chunks + 8 overlap chunks are dealt round-robin to the N ranks (N = 1: all 16 stages one after the other on the one GPU; N = 8: one
    index + one overlap chunk per rank, pair records routed by the RCCL all-to-all) -- total work is fixed: "scaling": "strong";
  * c3 / ecoli / c4s / c5s (one chunk per rank): N ranks = N index chunks + N overlap chunks over an N-times larger read set
    ("scaling": "weak"), the count tables / pair records exchanged between the stages over RCCL.

A plain run sets up, warms up, times the steps, writes the last timed step's outputs if --dump-outputs DIR is given and prints the
result line.  --full adds what the headline figure does not need (hashes and pins, the replay's kernel timing and the roofline, the
reference CPU leg, the end-to-end leg).

  python bench.py --gpus 1 --steps 5 --warmup 1
  python bench.py --gpus 1 --steps 5 --warmup 1 --full
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
SKETCH_BYTES_PER_BASE = 1.04     # 1 B seqdb + 16 B/408 L2 + MC  (-m 0)
ALIGN_BYTES_PER_PAIR = 21664.0   # 2 x 10.8 kB read + 64 B written
LEVELS = 2
DEFAULT_WORKLOAD = "c4"
BUDGET_S = 540                   # --full: seconds from the start the legs after the timed steps plan with (PGX_BENCH_BUDGET_S)
DUMP_RECORDS = 1 << 18           # --dump-outputs: records sampled over the job's overlap chunks (18 float64 columns: 37.7 MB)
DUMP_SEED = 20240917
DUMP_COLUMNS = ("index", "y0_hi", "y0_lo", "y1_hi", "y1_lo", "rl0", "rl1", "strand0", "strand1", "ovlp_type",
                "m_size", "dist", "q_bgn", "q_end", "t_bgn", "t_end", "t_m_end", "q_m_end")
WORKLOAD_TEXT = {
    "c4": "BASELINE configs[3] at FULL size (the configuration the metric is quoted on): 3.1 Gb genome seeded with 207 families of 300 copies "
          "of a 6 kb unit at 1 % divergence, 31 k tandem arrays and 31 k homopolymer runs (CHM13 is not obtainable offline) x 30x",
    "c5": "BASELINE configs[4] at FULL size: the configs[3] read set (3.1 Gb repeat-seeded genome x 30x) with -l 1 (dense L1 shimmers) and mc_upper 240",
    "c3": "BASELINE configs[2], uniform-random 150 Mb genome x 30x",
    "ecoli": "BASELINE configs[1], E. coli-size uniform-random genome (4,639,675 bp), 4,984 reads",
    "c4s": "BASELINE configs[3] scaled to one GPU, 300 Mb genome seeded with 6 kb x 300-copy repeat families, tandem arrays and homopolymers x 30x",
    "c5s": "BASELINE configs[4] scaled to one GPU, the c4s read set with -l 1 (L1 shimmers) and mc_upper 240",
}


_T0 = time.perf_counter()


def log(msg):
    """progress on stderr (stdout carries only the JSON line)"""
    if int(os.environ.get("RANK", "0")) == 0:
        sys.stderr.write("[bench +%.1f s] %s\n" % (time.perf_counter() - _T0, msg))
        sys.stderr.flush()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 3 for the c4 family -- a step is 8 + 8 chunks, ~11 s -- else 10)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps before them (default: 1 for the c4 family, else 2)")
    ap.add_argument("--two-stage", action="store_true",
                    help="N=1 only: hand the shimmer list from the index to the overlap stage through host arrays (as the "
                         "multi-GPU path must, around its all-gather) instead of leaving it in HBM")
    ap.add_argument("--workload", default=DEFAULT_WORKLOAD,
                    help="c4 (BASELINE configs[3] at full size: 3.1 Gb repeat-seeded genome x 30x = 93 Gbases, 8 index + 8 overlap chunks; "
                         "the configuration the metric is quoted on) | c3 (configs[2]: 150 Mb x 30x, 4.5 Gbases, one chunk) | ecoli "
                         "(configs[1]) | c4s | c5s (repeat-seeded, scaled configs[3]/[4], one chunk) | small | tiny")
    ap.add_argument("--chunks", type=int, default=0, help="c4 family: index_nchunk = ovlp_nchunk of the job (default 8); must be a multiple of --gpus")
    ap.add_argument("--genome-mb", type=float, default=0, help="c4 family: genome size in Mb (default 3100; the repeat content scales with it)")
    ap.add_argument("--ambiguous-frac", type=float, default=0.0,
                    help="one-chunk workloads: this fraction of the reads gets 1-3 ambiguous bases (both strands' nibbles zeroed, seeded): the index "
                         "stage then takes those reads run by run (pgx_sketch_n.hip), the packed alignment kernel hands their candidates on")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", default=None, choices=("full", "sample", "whole_chunks"),
                    help="one-chunk workloads -- full (default): the reference binaries on the WHOLE workload: one process on one core (its "
                         "ovlp_t stream is compared field by field with the timed GPU output) and N processes over N chunks for N in 24, 64, "
                         "128; sample: a 10 Mb x 30x set of the same recipe (count check only).  c4 family -- full: the reference as 24 "
                         "processes over 24 index chunks, then 24 overlap chunks, of the WHOLE 93 Gbases; sample (default): a bounded "
                         "sample of it, 24 processes over chunks 1..24 of 192; either way the streams of two of those chunks are compared "
                         "field by field with the GPU's; whole_chunks (default of c5): the reference indexes all of the job's chunks, then runs 8 of "
                         "its overlap chunks whole, their streams hashed and compared with the GPU's")
    ap.add_argument("--end-to-end", action="store_true", default=None,
                    help="c4 family: after the timed steps run the job's CHUNKS index + CHUNKS overlap commands through bin/native/* attached to a "
                         "`pgx_cli serve` process, files on /dev/shm (file -> kernels -> D2H -> file): `gpu_end_to_end` in the line.  Default at N = 1 "
                         "and full size where the command's time budget (PGX_BENCH_BUDGET_S) has ~3 minutes left after the other legs")
    ap.add_argument("--no-end-to-end", dest="end_to_end", action="store_false")
    ap.add_argument("--check-ref", action="store_true",
                    help="c4 family, small --genome-mb only: after the timed steps every rank compares the ovlp_t stream of each of its "
                         "chunks, field by field, with oracle/_ref/shmr_overlap -t CHUNKS -c c on files rank 0 writes")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: the read set's hash, one more step whose streams are SHA-256'd and "
                         "compared with the pins, the device replay's kernel-timing step and the roofline, the reference CPU leg and the "
                         "end-to-end leg, within PGX_BENCH_BUDGET_S (default %d s).  --check-ref, --cpu-baseline and --end-to-end imply it" % BUDGET_S)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed to DIR: per overlap chunk, records_chunkCC_of_TT.npy "
                         "(float64, one row per record of a seeded sample of at most %d records of the job, columns %s) and "
                         "stream_chunkCC_of_TT.npy (float64: records in the chunk's whole stream, its 64-bit stream checksum as high and "
                         "low 32 bits)" % (DUMP_RECORDS, ", ".join(DUMP_COLUMNS)))
    a = ap.parse_args()
    if a.check_ref or a.cpu_baseline or a.end_to_end:
        a.full = True
    big = a.workload in ("c4", "c5") and not a.genome_mb
    if a.steps is None:
        a.steps = 3 if big else 10
    if a.warmup is None:
        a.warmup = 1 if big else 2
    return a


def budget_s():
    """the command's time budget for the --full legs, from the process's start"""
    return float(os.environ.get("PGX_BENCH_BUDGET_S", str(BUDGET_S)))


def dump_sample(ov, c, n_chunks):
    """--dump-outputs: a seeded sample of overlap chunk c's records (the same rows from run to run for the same stream length),
    copied out of the library's array -> (positions in the stream, records)"""
    n, k = len(ov), max(1, DUMP_RECORDS // n_chunks)
    idx = np.arange(n) if n <= k else np.unique(np.random.default_rng([DUMP_SEED, c]).integers(0, n, k))
    return idx, ov[idx]


def write_dump(d, rows, checks, n_chunks):
    """--dump-outputs: the sampled records as float64 columns (DUMP_COLUMNS; the 64-bit y0 / y1 split into exact 32-bit halves) and every
    chunk's record count and stream checksum"""
    os.makedirs(d, exist_ok=True)
    lo32 = np.uint64(0xFFFFFFFF)
    for c, (idx, rec) in sorted(rows.items()):
        cols = [idx, rec["y0"] >> np.uint64(32), rec["y0"] & lo32, rec["y1"] >> np.uint64(32), rec["y1"] & lo32]
        cols += [rec[f] for f in DUMP_COLUMNS[5:]]
        tag = "chunk%02d_of_%02d" % (c, n_chunks)
        np.save(os.path.join(d, f"records_{tag}.npy"), np.stack([np.asarray(x, np.float64) for x in cols], axis=1))
        n, ck = checks[c]
        np.save(os.path.join(d, f"stream_{tag}.npy"), np.array([n, ck >> 32, ck & 0xFFFFFFFF], np.float64))


def _pair_keys(ov):
    r0 = ov["y0"] >> np.uint64(32)
    r1 = ov["y1"] >> np.uint64(32)
    return (np.minimum(r0, r1) << np.uint64(32)) | np.maximum(r0, r1)


def _scratch_dir(need_bytes):
    """a directory with room for the seqdb file + the reference's outputs (page-cache backed either way)"""
    best, free = None, -1
    for d in (os.environ.get("PGX_BENCH_TMP"), "/dev/shm", tempfile.gettempdir()):
        if d and os.path.isdir(d):
            try:
                st = os.statvfs(d)
            except OSError:
                continue
            f = st.f_bavail * st.f_frsize
            if f > free:
                best, free = d, f
    return best if free >= need_bytes else None


def cpu_baseline(db, ov_gpu, tag, levels=2, mc_upper=240):
    """The REAL reference (oracle/_ref: /root/reference/src compiled in the build container; falls back to the oracle port
    when the prebuilt binaries are absent) on the host cores of this box, same input files, whole workload:
      (1) one process, one core: shmr_index -t 1 -c 1, shmr_overlap -t 1 -c 1 -- the configuration the GPU step ran; its ovlp_t
          stream is compared FIELD BY FIELD, in order, with the records of the timed GPU steps;
      (2) N processes over N index chunks, then N processes over N overlap chunks, for N = 24 (the reference's own practical
          ceiling, /root/reference/README.md:127-137), 64 and 128 where the host has the cores, one leg after the other -- raw
          records/s and unique pairs/s per leg; the headline `value` is the fastest leg.
    Also times the GPU drop-in executables end to end (file -> H2D -> kernels -> D2H -> file) on the same files.
    Checker / baseline only: nothing here is on the product path."""
    import concurrent.futures as cf
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as U
    from peregrine_amd import formats
    need = int(db.seqdb.size * 1.1) + 64 * len(ov_gpu) * 8 + (1 << 30)
    base = _scratch_dir(need)
    if base is None:
        return {"value": None, "unit": "overlaps/s", "cores": 0, "kind": "none", "sample": f"no scratch directory with {need >> 30} GiB free"}
    d = tempfile.mkdtemp(prefix="pgx_bench_", dir=base)
    try:
        pre = os.path.join(d, "sd")
        formats.write_seqdb(pre, db)
        have = U.have_ref()
        kind = "reference" if have else "port"
        # ---- GPU, end to end through the drop-in executables on these files (file -> H2D -> kernels -> D2H -> file), FIRST:
        # the 24 / 64 / 128-process CPU legs below leave the host's caches and clocks in another state
        e2e_best = None
        exe = os.path.join(ROOT, "bin", "native")
        if os.path.exists(os.path.join(exe, "shmr_index")):
            try:
                env = dict(os.environ)
                for rep in range(3):    # the later runs have the executable, the library and the files in the page cache
                    t0 = time.perf_counter()
                    subprocess.run([os.path.join(exe, "shmr_index"), "-p", pre, "-t", "1", "-c", "1", "-m", "0", "-l", str(levels), "-o", os.path.join(d, "gx")],
                                   check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    t1 = time.perf_counter()
                    subprocess.run([os.path.join(exe, "shmr_overlap"), "-p", pre, "-l", os.path.join(d, "gx-L%d" % levels), "-t", "1", "-c", "1",
                                    "-M", str(mc_upper), "-o", os.path.join(d, "gov")], check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                    t2 = time.perf_counter()
                    if e2e_best is None or t2 - t0 < e2e_best[0] + e2e_best[1]:
                        e2e_best = (t1 - t0, t2 - t1)
            except Exception as e:   # the drop-ins fail loudly without a GPU; the baseline figures stand on their own
                e2e_best = repr(e)
        ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        N = max(1, min(ncpu, 24))

        def run_index(total, c, out):
            if have:
                U.ref_run("shmr_index", "-p", pre, "-t", total, "-c", c, "-m", 0, "-l", levels, "-o", out)
            else:
                subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import oracle_util as U; "
                                "U.orc_index_chunk(%r, %r, %d, %d, %d, 6, 0, 80, 16)" % (os.path.join(ROOT, "tests"), pre, out, total, c, levels)], check=True)

        def run_overlap(total, c, lpre, out):
            if have:
                U.ref_run("shmr_overlap", "-p", pre, "-l", lpre, "-t", total, "-c", c, "-M", mc_upper, "-o", out)
            else:
                subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import oracle_util as U; "
                                "U.orc_overlap_chunk(%r, %r, %r, %d, %d, 4, 2, %d)" % (os.path.join(ROOT, "tests"), pre, lpre, out, total, c, mc_upper)], check=True)

        def one_core():
            t0 = time.perf_counter()
            run_index(1, 1, os.path.join(d, "ix1"))
            t1 = time.perf_counter()
            run_overlap(1, 1, os.path.join(d, "ix1-L%d" % levels), os.path.join(d, "ov1"))
            t2 = time.perf_counter()
            return t1 - t0, t2 - t1

        def n_cores(N):
            nd = os.path.join(d, "n%d" % N)
            os.makedirs(nd, exist_ok=True)
            t0 = time.perf_counter()
            with cf.ThreadPoolExecutor(N) as ex:
                list(ex.map(lambda c: run_index(N, c, os.path.join(nd, "ix")), range(1, N + 1)))
            t1 = time.perf_counter()
            with cf.ThreadPoolExecutor(N) as ex:
                list(ex.map(lambda c: run_overlap(N, c, os.path.join(nd, "ix-L%d" % levels), os.path.join(nd, "ov.%03d" % c)), range(1, N + 1)))
            t2 = time.perf_counter()
            raw, keys = 0, []
            for c in range(1, N + 1):
                o = formats.read_ovlp(os.path.join(nd, "ov.%03d" % c))
                raw += len(o)
                keys.append(_pair_keys(o))
            uniq = int(len(np.unique(np.concatenate(keys)))) if keys else 0
            shutil.rmtree(nd, ignore_errors=True)
            return {"cores": N, "index_s": t1 - t0, "overlap_s": t2 - t1, "records": int(raw), "unique_pairs": uniq,
                    "value": raw / (t2 - t0), "unit": "overlaps/s", "index_bases_per_s": db.n_bases / (t1 - t0),
                    "overlap_records_per_s": raw / (t2 - t1), "unique_pairs_per_s": uniq / (t2 - t0)}

        # The legs run ONE AFTER THE OTHER (side by side they share LLC and DRAM bandwidth and the 1-core time comes
        # out inflated).  N-process legs: 24 (the reference's own practical ceiling, README.md:127-137) and, to show where THIS
        # box's plateau is instead of asserting it, 64 and 128 where the host has the cores.
        i1, o1 = one_core()
        ref1 = formats.read_ovlp(os.path.join(d, "ov1"))
        fields_equal = bool(formats.ovlp_fields_equal(np.asarray(ov_gpu), ref1))
        uniq1 = int(len(np.unique(_pair_keys(ref1))))
        want = [n for n in (24, 64, 128) if n <= ncpu] or [N]
        if os.environ.get("PGX_BENCH_CPU_LEGS"):
            want = [int(v) for v in os.environ["PGX_BENCH_CPU_LEGS"].split(",") if int(v) <= ncpu] or [N]
        legs = [n_cores(n) for n in want] if ncpu > 1 else []
        if not legs:
            legs = [{"cores": 1, "index_s": i1, "overlap_s": o1, "records": int(len(ref1)), "unique_pairs": uniq1, "value": len(ref1) / (i1 + o1),
                     "unit": "overlaps/s", "index_bases_per_s": db.n_bases / i1, "overlap_records_per_s": len(ref1) / o1,
                     "unique_pairs_per_s": uniq1 / (i1 + o1)}]
        best = max(legs, key=lambda l: l["value"])
        out = dict(best)
        out.update({
            "kind": kind,
            "sample": f"whole workload {tag} ({db.n_reads} reads, {db.n_bases} bases): N processes over N index chunks, then N processes over N "
                      f"overlap chunks (raw ovlp_t records of all chunks / wall time of both stages), N in {[l['cores'] for l in legs]} one after "
                      f"the other -- the headline is the fastest (N = {best['cores']}); host has {ncpu} usable cores; every leg runs alone",
            "legs": legs,
            "one_core": {"value": len(ref1) / (i1 + o1), "unit": "overlaps/s", "cores": 1, "index_s": i1, "overlap_s": o1,
                         "records": int(len(ref1)), "unique_pairs": uniq1, "index_bases_per_s": db.n_bases / i1,
                         "overlap_records_per_s": len(ref1) / o1,
                         "sample": "1 index chunk + 1 overlap chunk, 1 process (the chunking of the timed GPU step), run alone"},
            "records_match_gpu": fields_equal,
            "records_match_gpu_means": "every field of every ovlp_t record of the timed GPU steps equals the reference's 1-chunk "
                                       "stream, in order (formats.ovlp_fields_equal; padding bytes masked)",
        })
        # ---- GPU, end to end through the drop-in executables on the same files: timed before the CPU legs (e2e_best), compared here
        if e2e_best is not None and not isinstance(e2e_best, str):
            gov = formats.read_ovlp(os.path.join(d, "gov"))
            same_l2 = open(os.path.join(d, "gx-L%d-01-of-01.dat" % levels), "rb").read() == open(os.path.join(d, "ix1-L%d-01-of-01.dat" % levels), "rb").read()
            out["gpu_end_to_end"] = {
                "what": "bin/native/shmr_index + bin/native/shmr_overlap as separate processes on the same files: process start, "
                        "HIP context, file read, H2D, kernels, D2H, file write (best of 3 runs, taken before the CPU legs)",
                "index_s": e2e_best[0], "overlap_s": e2e_best[1], "overlaps_per_s": len(gov) / (e2e_best[0] + e2e_best[1]),
                "index_bases_per_s": db.n_bases / e2e_best[0], "overlap_records_per_s": len(gov) / e2e_best[1],
                "l2_file_identical_to_reference": bool(same_l2), "ovlp_fields_equal_reference": bool(formats.ovlp_fields_equal(gov, ref1)),
            }
        elif e2e_best is not None:
            out["gpu_end_to_end"] = {"error": e2e_best}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def attach_counters(cands, kern, workload):
    """HBM traffic and SQ instruction counts from the PMC counters: collected in SEPARATE rocprofv3 passes of this same command ON THIS
    WORKLOAD (tools/pmc_profile.sh <workload>: kernel-trace + one --pmc group per pass, never with the other trace domains) and committed
    under profiles/; bench.py itself cannot run under two profilers.  A workload without its own collection reports traffic = null and
    no `valu` object."""
    VALU_CEILING = 0.5     # wave64 VALU instructions per cycle and SIMD: a SIMD is 32 lanes wide, a wave64 add / logic / shift holds it two cycles (measured
                           # 0.45-0.48); the four-cycle class (v_min / v_max / v_cmp / v_cndmask / v_alignbit / v_perm / DPP / SDWA) tops out at 0.23-0.32
                           # (profiles/r03_valu_issue.txt).  Rounds 3-4 priced the alignment kernel against 0.25 and read 0.22 as "93 % of the ceiling": it was
                           # the work counter's same-address atomic that held it there (round 4: DESIGN 4.4); with chunks of 8 it issues 0.31.
    N_SIMD = 1024          # 256 CUs x 4 SIMDs
    for tag in ("r06", "r05", "r04", "r03"):
        tfile = os.path.join("profiles", f"{tag}_traffic_{workload}.json")
        if os.path.exists(os.path.join(ROOT, tfile)):
            break
    try:
        tr = json.load(open(os.path.join(ROOT, tfile)))
        pmc_steps = tr.get("_steps", 1)
        if "replay" in cands and "k_update" in tr:   # a round = one evaluation kernel (k_eval or k_eval_rows) + one k_update
            tot = sum(tr[k]["hbm_bytes_per_launch"] * tr[k]["launches"] for k in ("k_eval", "k_eval_rows", "k_eval_big", "k_update") if k in tr)
            tr["replay"] = {"hbm_bytes_per_launch": tot / tr["k_update"]["launches"]}
        for nm, kks in (("sketch", ("k_sketch_blk", "k_sketch_wave")), ("align", ("k_align_ph", "k_align4")), ("align1", ("k_align1",)),
                        ("replay", ("replay",))):
            kk = next((k for k in kks if k in tr), None)
            if nm in cands and kk:
                # PER STEP (the PMC pass and the timed tree may split a step into different numbers of launches): what the counters
                # saw over one step of the PMC pass; `traffic` (the contract's per-launch figure) = that / THIS run's launches per step
                per_step = tr[kk]["hbm_bytes_per_launch"] * tr[kk]["launches"] / tr[kk].get("steps", pmc_steps)
                cands[nm]["traffic_bytes_per_step"] = per_step
                cands[nm]["traffic"] = per_step / (kern[nm]["launches"] / kern[nm]["steps"])
                cands[nm]["traffic_read_side_raw"] = tr[kk].get("FETCH_SIZE_KB_per_launch", 0) * 1024 if "FETCH_SIZE_KB_per_launch" in tr[kk] else None
                cands[nm]["traffic_source"] = tfile + " (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, bytes per launch; read side x2 for the streaming kernels, x1 for the alignment kernels' scattered 8- / 16-byte loads: profiles/r03_fetch_calib.txt)"
    except Exception:
        pass
    # the roofline that BINDS the sketch and alignment kernels: VALU issue (VERDICT r3 task 4).  From the committed SQ passes: wave64 VALU
    # instructions per unit and the issue rate they were executed at, against the four-cycle class's ceiling
    for tag in ("r06", "r05", "r04", "r03"):
        vfile = os.path.join("profiles", f"{tag}_valu_{workload}.json")
        if os.path.exists(os.path.join(ROOT, vfile)):
            break
    try:
        vv = json.load(open(os.path.join(ROOT, vfile)))
        for nm, kks in (("sketch", ("k_sketch_blk",)), ("align", ("k_align_ph",))):
            kk = next((k for k in kks if k in vv), None)
            if nm in cands and kk:
                v = vv[kk]
                per_unit = v["SQ_INSTS_VALU"] / v["units"]
                rate = v["SQ_INSTS_VALU"] / N_SIMD / v["SQ_BUSY_CYCLES_per_se"]
                cands[nm]["valu"] = {"wave_instr_per_unit": per_unit, "salu_wave_instr_per_unit": v.get("SQ_INSTS_SALU", 0) / v["units"],
                                     "issue_rate": rate, "ceiling": VALU_CEILING, "ceiling_four_cycle_opcodes": 0.25, "frac": rate / VALU_CEILING,
                                     "unit": "wave64 VALU instructions per cycle and SIMD", "unit_name": cands[nm]["unit_name"],
                                     "units_per_s_at_ceiling": VALU_CEILING * N_SIMD * v["clock_hz"] / per_unit,
                                     "source": vfile + " (rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_BUSY_CYCLES ... pass of this command; ceiling: profiles/r03_valu_issue.txt)"}
    except Exception:
        pass


def check_vs_reference(seq, total, db, rank, world, CH, my_chunks, streams, levels, mc_upper, multi, xdev):
    """--check-ref (c4 family on a reduced genome; VERDICT r3 task 8): rank 0 writes the seqdb files and runs the REFERENCE index over
    all CH chunks; every rank then runs oracle/_ref/shmr_overlap -t CH -c c for each of ITS chunks and compares its last step's
    stream field by field, in order.  Returns (rank 0) {"all_equal": bool, "chunks": [...]}."""
    import shutil
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as U
    from peregrine_amd import formats, simreads
    if not U.have_ref():
        return {"all_equal": None, "error": "oracle/_ref is not in this tree"}
    d = os.path.join(_scratch_dir(int(total * 1.2) + (2 << 30)) or tempfile.gettempdir(), "pgx_checkref_%s" % os.environ.get("MASTER_PORT", "0"))
    if rank == 0:
        shutil.rmtree(d, ignore_errors=True)
        os.makedirs(d)
        simreads.write_seqdb_from_device(os.path.join(d, "sd"), seq, total, db.rid, db.rlen, db.roff)
        _run_many(min(CH, 24), [lambda c=c: U.ref_run("shmr_index", "-p", os.path.join(d, "sd"), "-t", CH, "-c", c, "-m", 0, "-l", levels, "-o", os.path.join(d, "ix")) for c in range(1, CH + 1)])
    if multi:
        dist.barrier()
    res = []
    for c in my_chunks:
        U.ref_run("shmr_overlap", "-p", os.path.join(d, "sd"), "-l", os.path.join(d, "ix-L%d" % levels), "-t", CH, "-c", c, "-M", mc_upper, "-o", os.path.join(d, "ov.%03d" % c))
        ref = formats.read_ovlp(os.path.join(d, "ov.%03d" % c))
        res.append((c, int(len(ref)), bool(len(ref) > 0 and formats.ovlp_fields_equal(np.asarray(streams[c]), ref))))
    flat = torch.zeros(3 * (CH // world), dtype=torch.int64, device=xdev)
    flat[:3 * len(res)] = torch.tensor([v for r in res for v in (r[0], r[1], int(r[2]))], dtype=torch.int64)
    if multi:
        allr = [torch.zeros_like(flat) for _ in range(world)]
        dist.all_gather(allr, flat)
        dist.barrier()
    else:
        allr = [flat]
    if rank == 0:
        shutil.rmtree(d, ignore_errors=True)
        rows = sorted((int(t[i]), int(t[i + 1]), bool(t[i + 2])) for t in allr for i in range(0, t.numel(), 3) if int(t[i]))
        return {"all_equal": all(r[2] for r in rows) and len(rows) == CH,
                "chunks": [{"chunk": "%d of %d" % (r[0], CH), "records": r[1], "equal_to_reference": r[2]} for r in rows],
                "means": "every rank's ovlp_t stream of each of its chunks == oracle/_ref/shmr_overlap -t %d -c c on the reference's own index files, field by field, in order" % CH}
    return None


def _run_many(n_workers, jobs):
    """jobs: callables; run n_workers at a time (one reference process each); returns the wall time"""
    import concurrent.futures as cf
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(n_workers) as ex:
        list(ex.map(lambda j: j(), jobs))
    return time.perf_counter() - t0


def cpu_baseline_chunked(seq, total, db, rdb, eng, tag, mode, levels, mc_upper, job_chunks, gpu_index_files, job_lists, stream_report=None, before_timing=None, files=None):
    """c4 family (one read set, CHUNKS index + overlap chunks): the REAL reference (oracle/_ref) on this box's host cores, on the same
    bytes (the device-resident seqdb written to files), 24 processes at a time (the reference's own practical ceiling,
    /root/reference/README.md:127-137):
      full   -- T = 24: 24 index chunks, then 24 overlap chunks of the WHOLE read set (what VERDICT r3 task 2 asks for);
      sample -- T = 192: index chunks 1..24 of 192 (1/8 of the reads; timed for the index rate) and overlap chunks 1..24 of 192 (1/8 of
                the first keys) over the 8 index-chunk files of the job as the GPU wrote them (byte-identical to the reference's own:
                tests/test_gpu_pipeline.py; shmr_overlap globs whatever index chunks exist, src/shmr_overlap.c:359-384);
      whole_chunks -- T = the job's own chunking (configs[4]: 24): the reference indexes all T chunks, then runs SOME of the job's overlap chunks
                whole (PGX_BENCH_CPU_CHUNKS, default 8 of them spread over 1..T, one process each side by side: a reference process at l = 1
                holds ~13 GB of lists and tables at full size); their streams are hashed like the GPU's (`reference_streams`: what
                tests/golden/c4_stream_pins.json pins) and compared with the hashed GPU step by record count + masked SHA-256.
    full / sample: the ovlp_t streams of overlap chunks 1 and 2 of T are compared FIELD BY FIELD, in order, with the GPU's stream for the
    same (T, c) over the same index lists -> records_match_gpu.  Checker / baseline only: nothing here is on the product path."""
    import shutil
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as U
    from peregrine_amd import _lib, formats, simreads
    if not U.have_ref():
        return {"value": None, "unit": "overlaps/s", "cores": 0, "kind": "none", "sample": "oracle/_ref (the compiled reference) is not in this tree"}
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    # 24 processes: the reference's own practical ceiling (README.md:127-137: 48 cores no faster than 24).  PGX_BENCH_CPU_PROCS = 48 | 64 runs the
    # whole-workload leg as that many processes over that many chunks instead -- the leg that says whether 24 is the best one on THIS host
    P = max(1, min(ncpu, int(os.environ.get("PGX_BENCH_CPU_PROCS", "24"))))
    if P > 24 and os.environ.get("PGX_BENCH_CPU_PROCS_FORCE") != "1":
        # (rounds 5 and 6: both attempts at a 48-process whole-workload leg lost the GPU box within minutes, whatever the host's free memory said)
        log(f"cpu baseline: {P} reference processes asked for; 24 is the most this leg runs (both 48-process attempts lost the GPU box: PGX_BENCH_CPU_PROCS_FORCE=1 overrides)")
        P = 24
    if os.environ.get("PGX_BENCH_CPU_PROCS") and mode == "full":
        # (round 5: 48 reference processes over the full-size set -- each holds every chunk's lists and its part of the pair map, ~13 GB at l = 2 --
        #  beside the 93 GB seqdb file in /dev/shm took the GPU box down.  A non-default process count must fit the host's free memory.)
        try:
            avail = next(int(l.split()[1]) * 1024 for l in open("/proc/meminfo") if l.startswith("MemAvailable"))
            per_proc = 14e9 * db.n_bases / 93.3e9 * (3.2 if levels == 1 else 1.0)
            fit = int((avail - total * 1.1 - 32e9) // max(per_proc, 1e8))
            if fit < P:
                log(f"cpu baseline: {P} reference processes would need ~{P * per_proc / 1e9:.0f} GB of host memory, {avail / 1e9:.0f} GB are available: {max(1, min(P, fit, 24))} instead")
                P = max(1, min(P, fit, 24))
        except Exception:
            P = min(P, 24)
    mem = {l.split(":")[0]: int(l.split()[1]) * 1024 for l in open("/proc/meminfo") if l.split(":")[0] in ("MemTotal", "MemAvailable")}
    # what the CONTAINER may use (its cgroup's limit) can be far below what /proc/meminfo reports for the host: a leg of 48 reference processes
    # (~13 GB each) took the GPU box down in round 5 AND in round 6 on a host with 3.2 TB of RAM, 3.0 TB of it "available"
    for f, g in (("/sys/fs/cgroup/memory.max", "/sys/fs/cgroup/memory.current"), ("/sys/fs/cgroup/memory/memory.limit_in_bytes", "/sys/fs/cgroup/memory/memory.usage_in_bytes")):
        try:
            lim = open(f).read().strip()
            if lim.isdigit() and int(lim) < (1 << 60):
                mem["CgroupLimit"] = int(lim)
                mem["MemAvailable"] = min(mem.get("MemAvailable", int(lim)), int(lim) - int(open(g).read().strip()))
            break
        except Exception:
            continue
    procs_limit_reason = ("24 = the reference's own practical ceiling (README.md:127-137); a 48-process leg was attempted in round 5 and in round 6 and lost the GPU "
                          "box both times within minutes (its container's memory limit, not the 3.2 TB the host reports); 64 / 128 processes were slower than 24 at configs[2] (round 3)"
                          if P == 24 and not os.environ.get("PGX_BENCH_CPU_PROCS")
                          else "PGX_BENCH_CPU_PROCS / host cores / host memory")
    T = P if mode == "full" else job_chunks if mode == "whole_chunks" else 192
    cs = list(range(1, min(T, P) + 1))
    ov_cs, P_ov = cs, P
    if mode == "whole_chunks":
        cs = list(range(1, T + 1))
        dflt = sorted({1, 2} | {1 + (i * (T - 1)) // 7 for i in range(8)})[:8] if T > 8 else list(range(1, T + 1))
        try:     # (the chunks tests/golden/c4_stream_pins.json pins for this workload, where it has them: the leg then re-checks the pins too)
            pinned = json.load(open(PINS_FILE)).get(tag) or {}
            if pinned.get("chunks") == T:
                dflt = sorted(int(r["chunk"].split()[0]) for r in pinned["streams"]) or dflt
        except Exception:
            pass
        ov_cs = [int(v) for v in os.environ.get("PGX_BENCH_CPU_CHUNKS", "").split(",") if v] or dflt
        per_proc = 13e9 * db.n_bases / 93.3e9      # (measured at full size: 12.4 GB at l = 1, T = 24; ~13 GB at l = 2, T = 8)
        fit = int((mem.get("MemAvailable", 0) - total * 1.1 - 32e9) // max(per_proc, 1e8))
        P_ov = max(1, min(len(ov_cs), ncpu, fit))
        procs_limit_reason = "one process per compared chunk (%d), host memory allows %d at ~%.0f GB each" % (len(ov_cs), fit, per_proc / 1e9)
    need = int(total * 1.02) + int(db.n_bases * (0.12 if mode == "full" else 0.2 if mode == "whole_chunks" and levels == 1 else 0.03)) + (8 << 30)
    if files is not None:      # the seqdb files are there already (shared with the end-to-end leg): this leg's outputs go to a directory of their own
        d = os.path.join(files["dir"], "cpu")
        os.makedirs(d, exist_ok=True)
    else:
        base = _scratch_dir(need)
        if base is None:
            return {"value": None, "unit": "overlaps/s", "cores": 0, "kind": "none", "sample": f"no scratch directory with {need >> 30} GiB free"}
        d = tempfile.mkdtemp(prefix="pgx_bench_", dir=base)
    try:
        if files is not None:
            pre, t_files = files["prefix"], files["seconds"]
        else:
            pre = os.path.join(d, "sd")
            t0 = time.perf_counter()
            simreads.write_seqdb_from_device(pre, seq, total, db.rid, db.rlen, db.roff)
            t_files = time.perf_counter() - t0
        log(f"cpu baseline ({mode}): seqdb files written in {t_files:.1f} s")
        if before_timing is not None:     # (nothing of this process runs beside the reference while it is timed -- the seqdb's SHA-256 thread ends here)
            before_timing()
        lv = "L%d" % levels
        if mode in ("full", "whole_chunks"):      # the reference indexes everything itself
            t_index = _run_many(P, [lambda c=c: U.ref_run("shmr_index", "-p", pre, "-t", T, "-c", c, "-m", 0, "-l", levels, "-o", os.path.join(d, "ix")) for c in cs])
            lpre, index_bases, index_chunking = os.path.join(d, "ix-" + lv), db.n_bases, T
        else:                   # the reference indexes 24 of 192 chunks (timed); the overlap sample reads the job's own index-chunk files
            t_index = _run_many(P, [lambda c=c: U.ref_run("shmr_index", "-p", pre, "-t", T, "-c", c, "-m", 0, "-l", levels, "-o", os.path.join(d, "cx")) for c in cs])
            index_bases = int(db.rlen[np.isin(db.rid % T, [c % T for c in cs])].sum(dtype=np.uint64))
            gpu_index_files(os.path.join(d, "ix"))
            lpre, index_chunking = os.path.join(d, "ix-" + lv), job_chunks
        log(f"cpu baseline: reference index leg {t_index:.1f} s")
        t_ovlp = _run_many(P_ov, [lambda c=c: U.ref_run("shmr_overlap", "-p", pre, "-l", lpre, "-t", T, "-c", c, "-M", mc_upper, "-o", os.path.join(d, "ov.%03d" % c)) for c in ov_cs])
        log(f"cpu baseline: reference overlap leg {t_ovlp:.1f} s ({P_ov} processes over chunks {ov_cs if mode == 'whole_chunks' else '1..%d' % len(ov_cs)} of {T})")
        if mode == "whole_chunks":
            return _whole_chunks_result(d, lv, T, cs, ov_cs, P, P_ov, t_index, t_ovlp, t_files, db, tag, ncpu, mem, procs_limit_reason, stream_report, job_lists, formats)
        # ---- the GPU on the same (T, c), same index chunking, for the first two chunks: field-for-field compare
        dev = torch.device("cuda", torch.cuda.current_device())
        if index_chunking == job_chunks and job_lists.get("mm") is not None:
            mm_all, mc_all = job_lists["mm"], job_lists["mc"]      # the timed steps' own lists (still in HBM)
        else:
            job_lists.clear()                                       # (their HBM is needed: 276-285 of 288 GB are in use at full size)
            torch.cuda.empty_cache()
            tops, mcs = [], []
            for c in range(1, index_chunking + 1):
                _, top, mc = eng.index(index_chunking, c, levels)
                _lib.stream_signal()
                tops.append(top.clone()); mcs.append(mc.clone())
            mm_all, mc_all = torch.cat(tops), torch.cat(mcs)
            del tops, mcs
        same_index = None
        if mode == "full":
            got = mm_all.cpu().numpy().view(formats.MM_DTYPE)
            n1 = os.path.getsize(os.path.join(d, "ix-%s-01-of-%02d.dat" % (lv, T))) // 16
            same_index = bool(np.array_equal(got[:n1], formats.read_mmlist(os.path.join(d, "ix-%s-01-of-%02d.dat" % (lv, T)))))
            del got
        _lib.stream_wait()
        match, compared = True, []
        for c in cs[:2]:     # (T != the job's chunking: the GPU on the CPU leg's chunking)
            ov, _ = rdb.overlap_dev(mm_all.data_ptr(), mm_all.numel() // 16, mc_all.data_ptr(), mc_all.numel() // 16, total_chunk=T, mychunk=c, mc_upper=mc_upper)
            ref = formats.read_ovlp(os.path.join(d, "ov.%03d" % c))
            ok = bool(formats.ovlp_fields_equal(np.asarray(ov), ref))
            compared.append({"chunk": "%d of %d" % (c, T), "records": int(len(ref)), "equal": ok})
            match = match and ok and len(ref) > 0
            del ov, ref
        del mm_all, mc_all
        log(f"cpu baseline: GPU streams of {[c['chunk'] for c in compared]} compared: {[c['equal'] for c in compared]}")
        raw, keys = 0, []
        for c in cs:
            o = formats.read_ovlp(os.path.join(d, "ov.%03d" % c))
            raw += len(o)
            keys.append(_pair_keys(o).view(np.int64))
            del o
        try:     # bookkeeping of the CPU leg's output; the whole-workload leg leaves ~0.5 G keys: sorted on the GPU
            uniq = int(len(np.unique(np.concatenate(keys)))) if raw <= 150_000_000 else int(torch.unique(torch.cat([torch.from_numpy(k).to(dev) for k in keys])).numel())
        except Exception:
            uniq = None
        del keys
        frac = 1.0 if mode == "full" else len(cs) / T
        out = {"value": raw / (t_index + t_ovlp), "unit": "overlaps/s", "cores": P, "kind": "reference",
               "sample": (f"WHOLE workload {tag} ({db.n_reads} reads, {db.n_bases} bases): {P} processes over {T} index chunks, then over {T} overlap chunks"
                          if mode == "full" else
                          f"bounded sample of {tag} ({db.n_reads} reads, {db.n_bases} bases): {P} processes over index chunks 1..24 of 192 ({index_bases} bases) and "
                          f"then over overlap chunks 1..24 of 192 (1/8 of the first keys; each process still loads all shimmer / count files and scans "
                          f"the whole list, as every reference overlap chunk does)") + f"; raw ovlp_t records / wall time of both stages; host has {ncpu} usable cores",
               "mode": mode, "chunking": T, "chunks_run": len(cs), "fraction_of_job": frac,
               "host_ram_gb": mem.get("MemTotal", 0) / 1e9, "host_ram_available_gb": mem.get("MemAvailable", 0) / 1e9, "cgroup_limit_gb": mem.get("CgroupLimit", 0) / 1e9 or None,
               "procs_limit_reason": procs_limit_reason,
               "index_s": t_index, "overlap_s": t_ovlp, "records": int(raw), "unique_pairs": uniq,
               "index_bases_per_s": index_bases / t_index, "overlap_records_per_s": raw / t_ovlp,
               "unique_pairs_per_s": uniq / (t_index + t_ovlp) if uniq else None,
               "seqdb_files_written_s": t_files, "one_core": None,
               "records_match_gpu": bool(match), "records_compared": compared, "index_list_chunk1_equals_reference": same_index,
               "records_match_gpu_means": "every field of every ovlp_t record of overlap chunks 1 and 2 of T (the CPU leg's chunking) equals the "
                                          "reference's stream for that chunk, in order, the GPU run on the same index lists (formats.ovlp_fields_equal; "
                                          "padding bytes masked)"}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _whole_chunks_result(d, lv, T, cs, ov_cs, P, P_ov, t_index, t_ovlp, t_files, db, tag, ncpu, mem, procs_limit_reason, stream_report, job_lists, formats):
    """mode whole_chunks of cpu_baseline_chunked: the reference ran SOME of the job's own overlap chunks whole (after indexing all T chunks itself)"""
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(8) as ex:
        shas = list(ex.map(lambda c: formats.masked_stream_sha256(os.path.join(d, "ov.%03d" % c)), ov_cs))
    ref_streams = [{"chunk": "%d of %d" % (c, T), "records": os.path.getsize(os.path.join(d, "ov.%03d" % c)) // 64, "masked_sha256": shas[i]} for i, c in enumerate(ov_cs)]
    gpu = {r["chunk"]: r for r in stream_report or []}
    compared = [{"chunk": r["chunk"], "records": r["records"],
                 "equal": bool(r["chunk"] in gpu and gpu[r["chunk"]]["records"] == r["records"] and gpu[r["chunk"]]["masked_sha256"] == r["masked_sha256"])} for r in ref_streams]
    same_index = None
    if job_lists.get("mm") is not None:      # the job's own L lists (all chunks, chunk order) against the reference's first chunk file
        n1 = os.path.getsize(os.path.join(d, "ix-%s-01-of-%02d.dat" % (lv, T))) // 16
        got = job_lists["mm"][:n1 * 16].cpu().numpy().view(formats.MM_DTYPE)
        same_index = bool(np.array_equal(got, formats.read_mmlist(os.path.join(d, "ix-%s-01-of-%02d.dat" % (lv, T)))))
    raw = sum(r["records"] for r in ref_streams)
    k = len(ov_cs)
    log(f"cpu baseline: reference streams of chunks {ov_cs} hashed; equal to the GPU's: {[c['equal'] for c in compared]}")
    return {"value": raw / (t_index * k / T + t_ovlp), "unit": "overlaps/s", "cores": P, "kind": "reference",
            "sample": (f"{k} WHOLE overlap chunks ({ov_cs} of {T}) of {tag} ({db.n_reads} reads, {db.n_bases} bases) after the reference indexed all {T} chunks itself "
                       f"({P} processes); {P_ov} overlap processes side by side; value = their raw ovlp_t records / (index time x {k}/{T} + overlap wall time); "
                       f"host has {ncpu} usable cores"),
            "mode": "whole_chunks", "chunking": T, "chunks_run": k, "overlap_chunks": ov_cs, "overlap_processes": P_ov, "index_processes": P, "fraction_of_job": k / T,
            "host_ram_gb": mem.get("MemTotal", 0) / 1e9, "host_ram_available_gb": mem.get("MemAvailable", 0) / 1e9, "procs_limit_reason": procs_limit_reason,
            "index_s": t_index, "overlap_s": t_ovlp, "records": int(raw), "unique_pairs": None, "index_bases_per_s": db.n_bases / t_index,
            "overlap_records_per_s": raw / t_ovlp, "unique_pairs_per_s": None, "seqdb_files_written_s": t_files, "one_core": None,
            "records_match_gpu": bool(compared and all(c["equal"] for c in compared)), "records_compared": compared,
            "index_list_chunk1_equals_reference": same_index, "reference_streams": ref_streams,
            "records_match_gpu_means": "record count and SHA-256 (padding bytes 27, 60..63 zeroed) of the reference's stream of each of these chunks of the JOB's own "
                                       "chunking equal the GPU's stream of the hashed step (whose checksums equal every timed step's)"}


def cpu_baseline_sample(sample):
    """bounded form (--cpu-baseline sample): the reference on one core on a small set of the same recipe; count only"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_util as U
    from peregrine_amd import formats
    with tempfile.TemporaryDirectory() as d:
        pre = os.path.join(d, "sd")
        formats.write_seqdb(pre, sample)
        kind = "reference" if U.have_ref() else "port"
        t0 = time.perf_counter()
        if U.have_ref():
            U.ref_run("shmr_index", "-p", pre, "-t", 1, "-c", 1, "-m", 0, "-o", os.path.join(d, "ix"))
            t1 = time.perf_counter()
            U.ref_run("shmr_overlap", "-p", pre, "-l", os.path.join(d, "ix-L2"), "-t", 1, "-c", 1, "-o", os.path.join(d, "ov"))
        else:
            U.orc_index_chunk(pre, os.path.join(d, "ix"), 1, 1, 2, 6, 0, 80, 16)
            t1 = time.perf_counter()
            U.orc_overlap_chunk(pre, os.path.join(d, "ix-L2"), os.path.join(d, "ov"), 1, 1)
        t2 = time.perf_counter()
        nrec = os.path.getsize(os.path.join(d, "ov")) // 64
    return {"value": nrec / (t2 - t0), "unit": "overlaps/s", "cores": 1, "kind": kind,
            "sample": f"10 Mb x 30x set of the same recipe ({sample.n_reads} reads, {sample.n_bases} bases), 1 chunk, 1 process",
            "index_s": t1 - t0, "overlap_s": t2 - t1, "records": int(nrec), "records_match_gpu": None}


def device_read_set_hash(seq, total):
    """EVERY byte of the resident seqdb in two 64-bit sums (position-dependent odd multipliers, wrap-around int64 arithmetic on the device):
    what the ranks compare instead of round 4's strided checksum.  Not cryptographic; the SHA-256 of the same bytes is `seqdb_sha256`."""
    import torch
    n8 = total // 8
    w_all = seq[:n8 * 8].view(torch.int64)
    h1 = torch.zeros((), dtype=torch.int64, device=seq.device)
    h2 = torch.zeros((), dtype=torch.int64, device=seq.device)
    B = 1 << 27
    for o in range(0, n8, B):
        w = w_all[o:o + B]
        i = torch.arange(o, o + w.numel(), dtype=torch.int64, device=seq.device)
        m = (i * -7046029254386353131) | 1                       # 0x9E3779B97F4A7C15 as int64, odd
        h1 += (w * m).sum()
        h2 += ((w ^ (w >> 29)) * ((i * -4417276706812531889) | 1)).sum()
        del w, i, m
    tail = int(seq[n8 * 8:total].to(torch.int64).sum()) if total > n8 * 8 else 0
    return "%016x%016x%02x" % (int(h1) & 0xFFFFFFFFFFFFFFFF, int(h2) & 0xFFFFFFFFFFFFFFFF, tail & 0xFF)


def seqdb_sha256_of_device(seq, total, piece=1 << 30):
    """SHA-256 of the resident seqdb bytes (= sha256sum of the .seqdb file written from them), piece by piece through the host"""
    import hashlib
    h = hashlib.sha256()
    for o in range(0, total, piece):
        h.update(memoryview(seq[o:min(total, o + piece)].cpu().numpy()))
    return h.hexdigest()


PINS_FILE = os.path.join(ROOT, "tests", "golden", "c4_stream_pins.json")


def end_to_end_served(seq, total, db, rdb, CH, levels, mc_upper, stream_report, release=None, files=None):
    """file -> H2D -> kernels -> D2H -> file at the metric's configuration (pg_run.py:232-244,305-317): the job's CH index + CH overlap
    chunk COMMANDS through bin/native/shmr_index / shmr_overlap attached to one `pgx_cli serve` process, everything on /dev/shm.  This process
    gives its HBM back first (two copies of a 93 GB database do not fit one GPU).  The output files are hashed like the resident streams."""
    import shutil
    import signal
    import torch
    from peregrine_amd import _lib, formats, simreads
    need = int(total * 1.02) + 64 * int(sum(r["records"] for r in stream_report or [])) + (8 << 30)
    if files is not None:
        base = os.path.dirname(files["dir"])
        d = os.path.join(files["dir"], "e2e")
        os.makedirs(d, exist_ok=True)
    else:
        base = _scratch_dir(need)
        if base is None:
            return {"error": f"no scratch directory with {need >> 30} GiB free"}
        d = tempfile.mkdtemp(prefix="pgx_e2e_", dir=base)
    cli = os.path.join(ROOT, "bin", "native", "pgx_cli")
    inflight = max(1, int(os.environ.get("PGX_BENCH_E2E_INFLIGHT", "2")))
    try:
        if files is not None:
            pre, t_files = files["prefix"], files["seconds"]
        else:
            pre = os.path.join(d, "sd")
            t0 = time.perf_counter()
            simreads.write_seqdb_from_device(pre, seq[0] if isinstance(seq, list) else seq, total, db.rid, db.rlen, db.roff)
            t_files = time.perf_counter() - t0
        rdb.close()
        _lib.shutdown()
        del seq
        if release is not None:
            release()          # (the caller's references to the resident seqdb and the lists)
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        log("end to end: %.1f GB of HBM still in use by this process" % ((torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9))
        log(f"end to end: seqdb files written in {t_files:.1f} s; this process's HBM released")
        t0 = time.perf_counter()
        tr = os.environ.get("PGX_BENCH_E2E_TRACE")     # a file: the server's PGX_TRACE=1 log (per command: lists, stage, file transfer)
        srv = subprocess.Popen([cli, "serve", "-p", pre], stderr=open(tr, "w") if tr else subprocess.DEVNULL, env=dict(os.environ, PGX_TRACE="1") if tr else None)
        while not os.path.exists(pre + ".pgx.sock") and srv.poll() is None:
            time.sleep(0.05)
        t_up = time.perf_counter() - t0
        try:
            t0 = time.perf_counter()
            def run(cmd):
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode:
                    raise RuntimeError("%s -> %d: %s" % (" ".join(cmd[1:6]), r.returncode, (r.stderr or "")[-600:]))
            for c in range(1, CH + 1):
                run([cli, "shmr_index", "-p", pre, "-t", str(CH), "-c", str(c), "-m", "0", "-l", str(levels), "-o", os.path.join(d, "ix")])
            t1 = time.perf_counter()
            # the job's overlap commands as a scheduler with `inflight` job slots issues them (pg_run.py hands its chunk commands to a job queue): the
            # server runs ONE stage at a time; a second command in flight lets its stage start while the first one's file is being completed
            _run_many(inflight, [lambda c=c: run([cli, "shmr_overlap", "-p", pre, "-l", os.path.join(d, "ix-L%d" % levels), "-t", str(CH), "-c", str(c), "-M", str(mc_upper),
                                                  "-o", os.path.join(d, "ov.%02d" % c)]) for c in range(1, CH + 1)])
            t2 = time.perf_counter()
        finally:
            srv.send_signal(signal.SIGTERM)
            srv.wait()
        nrec = sum(os.path.getsize(os.path.join(d, "ov.%02d" % c)) // 64 for c in range(1, CH + 1))
        res = {"what": "the job's %d index + %d overlap chunk commands through bin/native/shmr_index / shmr_overlap attached to one `pgx_cli serve` process "
                       "(the database resident there), files on %s: process start, socket, file reads, kernels, D2H, file writes; the index commands one after the "
                       "other, %d overlap command(s) in flight" % (CH, CH, base, inflight),
               "overlap_commands_in_flight": inflight,
               "index_s": t1 - t0, "overlap_s": t2 - t1, "records": int(nrec), "overlaps_per_s": nrec / (t2 - t0),
               "server_start_s": t_up, "overlaps_per_s_incl_server_start": nrec / (t2 - t0 + t_up), "seqdb_files_written_s": t_files}
        if stream_report:
            want = {r["chunk"]: r["masked_sha256"] for r in stream_report}
            got = {"%d of %d" % (c, CH): formats.masked_stream_sha256(os.path.join(d, "ov.%02d" % c)) for c in range(1, CH + 1)}
            res["files_equal_resident_streams"] = bool(got == want)
        return res
    except Exception as e:
        return {"error": repr(e)}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    a = parse()
    # stdout carries exactly ONE line, the JSON: everything else that writes to file descriptor 1 -- RCCL prints a version banner
    # there from C when a communicator is torn down -- is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist
    from peregrine_amd import _lib, formats, simreads
    from peregrine_amd.formats import MC_DTYPE, MM_DTYPE, SeqDB
    from peregrine_amd.parallel import GpuEngine, allgather_cat, allgather_ints, exchange_overlap, gather_seqdb
    from peregrine_amd.shimmer import ResidentDB

    assert torch.cuda.is_available(), "bench.py needs a GPU (there is no CPU fallback)"
    ngpu = torch.cuda.device_count()
    # PGX_BENCH_BACKEND=gloo: debugging aid that lets several ranks share one GPU (RCCL refuses that); the graded runs
    # use one rank per GPU over RCCL ("nccl")
    backend = os.environ.get("PGX_BENCH_BACKEND", "nccl")
    dev_index = local if backend == "nccl" else local % ngpu
    torch.cuda.set_device(dev_index)
    home = torch.device("cuda", dev_index)
    xdev = home if backend == "nccl" else torch.device("cpu")
    # PGX_FORCE_EXCHANGE=1: a one-rank job takes the multi-rank path too -- process group over RCCL, the seqdb gathered into an
    # adopted device buffer, count all-gather + record all-to-all(v) on device views, event hand-over between the streams --
    # which is how the RCCL path is executed (and checked against the single-chunk records) on a one-GPU box
    multi = world > 1 or os.environ.get("PGX_FORCE_EXCHANGE") == "1"
    if multi:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29533")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=home)
        else:
            dist.init_process_group(backend)
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"

    sp = dict(levels=2, mc_upper=240)
    sp.update(simreads.STAGE_PARAMS.get(a.workload, {}))
    global LEVELS
    LEVELS = sp["levels"]
    strong = a.workload in simreads.RESIDENT_WORKLOADS     # ONE read set, CHUNKS chunks dealt to the ranks; else one chunk per rank
    seq_dev = None
    read_set_hash = read_set_hash_equal = None
    if strong:
        # ---- synthetic input (untimed): EVERY rank generates the same seeded read set into its own HBM (11 s for 93 Gbases) ----
        CH = a.chunks or sp.get("chunks", 8)
        assert CH % world == 0, f"--chunks {CH} must be a multiple of --gpus {world}"
        my_chunks = [c for c in range(1, CH + 1) if (c - 1) % world == rank]
        seq_dev, total, rlen = simreads.make_workload_resident(a.workload, genome_mb=a.genome_mb or None)
        rid = np.arange(len(rlen), dtype=np.uint32)
        roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
        if a.full:
            read_set_hash = device_read_set_hash(seq_dev, total)    # every byte, on the device
        read_set_hash_equal = None
        if a.full and world > 1:    # same generator, same seeds, same device type: the ranks' copies must be the same bytes
            probe = [int(total), int(len(rlen)), int(read_set_hash[:15], 16), int(read_set_hash[15:30], 16), int(read_set_hash[30:], 16)]
            read_set_hash_equal = len({tuple(r) for r in allgather_ints(probe, world, device=home if backend == "nccl" else None)}) == 1
            assert read_set_hash_equal, "ranks generated different read sets"
        rdb = ResidentDB.adopt_device(seq_dev, total, rid, rlen, roff, dev_index)
        db = SeqDB(np.zeros(0, np.uint8), rid, rlen, roff, None)   # (sizes only: the bytes live in HBM)
    else:
        # ---- synthetic input (untimed): rank r simulates genome r; the union is the job's read set -----------------
        CH = world
        my_chunks = [rank + 1]
        cache = os.environ.get("PGX_BENCH_CACHE")   # a directory: the simulated set is kept there (the PMC passes of the repeat-rich workloads:
        cpath = os.path.join(cache, f"{a.workload}_r{rank}") if cache else None   # rocprofv3 --pmc aborts inside torch's generator kernels)
        if cpath and os.path.exists(cpath + ".seqdb.npy"):
            sq, rl = np.load(cpath + ".seqdb.npy", mmap_mode="r"), np.load(cpath + ".rlen.npy")
            roff0 = np.concatenate([[0], np.cumsum(rl.astype(np.uint64))[:-1]]).astype(np.uint64)
            mine = SeqDB(np.ascontiguousarray(sq), np.arange(len(rl), dtype=np.uint32), rl, roff0, None)
        elif a.workload in simreads.TORCH_WORKLOADS:
            mine = simreads.make_workload_torch(a.workload, rank)
            mine.names = None
            if cpath:
                os.makedirs(cache, exist_ok=True)
                np.save(cpath + ".seqdb.npy", np.asarray(mine.seqdb)), np.save(cpath + ".rlen.npy", np.asarray(mine.rlen))
        else:
            cfg = dict(simreads.WORKLOADS[a.workload])
            g = simreads.make_genome(cfg.pop("genome_len"), cfg.pop("genome_seed") + 7919 * rank)
            mine = simreads.simulate_reads(g, seed=42 + rank, **cfg)
        if a.ambiguous_frac > 0:
            rng = np.random.default_rng(777 + rank)
            sq = np.array(mine.seqdb, copy=True)
            picked = rng.choice(mine.n_reads, max(1, int(a.ambiguous_frac * mine.n_reads)), replace=False)
            for r in picked:
                o, n = int(mine.roff[r]), int(mine.rlen[r])
                for ppos in rng.integers(0, n, int(rng.integers(1, 4))):
                    sq[o + ppos] = 0                      # ambiguous on the forward strand ...
                    sq[o + n - 1 - ppos] &= 0x0F          # ... and its mirror image on the reverse strand's nibble
            mine = SeqDB(sq, mine.rid, mine.rlen, mine.roff, None)
            log(f"{len(picked)} reads with ambiguous bases")
        if multi:
            # the job's read set = the union of the ranks' sets, replicated in every GPU's HBM: every rank's bytes are
            # received over xGMI (RCCL) straight into their place in ONE device buffer, which the library adopts without a copy
            seq_all, total, rlen = gather_seqdb(mine.seqdb, mine.rlen, world, home)
            roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
            rid = np.arange(len(rlen), dtype=np.uint32)
            rdb = ResidentDB.adopt_device(seq_all, total, rid, rlen, roff, dev_index)
            db = SeqDB(mine.seqdb if world == 1 else np.zeros(0, np.uint8), rid, rlen, roff, None)   # (sizes only when the bytes live in HBM)
            del seq_all
        else:
            db = mine
            rdb = ResidentDB(db, dev_index)  # H2D once; the timed region starts with the seqdb resident in HBM
    log(f"input ready: {db.n_reads} reads, {db.n_bases} bases")
    eng = GpuEngine(rdb, home)
    ov_params = dict(mc_upper=sp["mc_upper"])
    SUM_KEYS = ("n_records", "n_pair_records", "n_buckets", "n_align_needed", "n_align_gpu", "n_seen_skip", "n_evaluations", "gpu_ms", "host_ms", "device_visit")
    keep_streams = {}

    shared_files = None   # the seqdb files of the reference CPU leg and the end-to-end leg ({"dir", "prefix", "seconds"})
    held = {}   # N = 1, several chunks: the concatenated lists live in ONE pair of buffers kept across the steps (sizes repeat)
    hash_streams = False     # set for ONE extra step after the timed region: every chunk's stream is SHA-256'd (padding masked) as it arrives
    hash_jobs, hash_keep = {}, []
    import concurrent.futures as _cf
    hash_pool = _cf.ThreadPoolExecutor(8)
    dump_rows = None    # --dump-outputs, the last timed step: {chunk: (positions, records)} sampled as each chunk's records arrive

    def index_my_chunks():
        """the rank's index chunks; the lists / count tables as device byte tensors (copies: the library reuses its buffers)"""
        tops, mcs, bases, ix = [], [], 0, None
        om = oc = 0
        for c in my_chunks:
            ix, top, mc = eng.index(CH, c, sp["levels"])
            bases += ix.bases
            if len(my_chunks) > 1:
                _lib.stream_signal()
                if "mm" in held and om + top.numel() <= held["mm"].numel() and oc + mc.numel() <= held["mc"].numel():
                    held["mm"][om:om + top.numel()].copy_(top), held["mc"][oc:oc + mc.numel()].copy_(mc)   # straight into place
                    top, mc = held["mm"][om:om + top.numel()], held["mc"][oc:oc + mc.numel()]
                else:
                    held.clear()
                    top, mc = top.clone(), mc.clone()
                om, oc = om + top.numel(), oc + mc.numel()
            tops.append(top)
            mcs.append(mc)
        ix.bases = bases
        if held and (om != held["mm"].numel() or oc != held["mc"].numel()):
            held.clear()
            tops, mcs = [t.clone() for t in tops], [t.clone() for t in mcs]
        return ix, tops, mcs

    def step_strong():
        """CHUNKS index chunks + CHUNKS overlap chunks of ONE read set, dealt round-robin to the ranks"""
        s0 = time.perf_counter()
        ix, tops, mcs = index_my_chunks()
        s1 = time.perf_counter()
        if world > 1 and len(my_chunks) == 1:       # one chunk per rank: count all-gather + pair-record all-to-all(v) on device views
            (ov, st), info = exchange_overlap(eng, rank, world, tops[0], mcs[0], **ov_params)
            st["exchange"] = info
            st["chunk_checksums"] = {my_chunks[0]: (len(ov), st["stream_checksum"])}
            if a.check_ref or hash_streams or dump_rows is not None:
                keep_streams[my_chunks[0]] = ov
            return ix, len(ov), st, s1 - s0
        if world > 1:       # several chunks per rank: the lists of ALL chunks, in chunk order, all-gathered round by round (round j = chunks j N + 1 .. j N + N)
            mm_all = torch.cat([allgather_cat(t, world)[0] for t in tops])
            mc_all = torch.cat([allgather_cat(t, world)[0] for t in mcs])
        elif held:
            mm_all, mc_all = held["mm"], held["mc"]
        elif len(tops) > 1:      # the first step: concatenate, keep the buffers, give the pieces back to the driver
            mm_all, mc_all = torch.cat(tops), torch.cat(mcs)
            held["mm"], held["mc"] = mm_all, mc_all
            del tops, mcs
            tops = mcs = None
            torch.cuda.empty_cache()
        else:
            mm_all, mc_all = tops[0], mcs[0]
        del tops, mcs
        _lib.stream_wait()
        tot, nrec, cks = None, 0, {}
        was_async = _lib.results_async(os.environ.get("PGX_BENCH_SYNC_RESULTS") != "1")    # a chunk's records travel to the host beside the next chunk's main alignment launch
        prev = None                             # (the array of the chunk before: freeing it would wait for its copy)
        prev_c = None
        for ci, c in enumerate(my_chunks):
            tc0 = time.perf_counter()
            ov, st = rdb.overlap_dev(mm_all.data_ptr(), mm_all.numel() // 16, mc_all.data_ptr(), mc_all.numel() // 16, total_chunk=CH, mychunk=c, **ov_params)
            if os.environ.get("PGX_BENCH_CHUNK_TIMES"):
                log("chunk %d: call %.1f ms (library: gpu %.1f + host %.1f), %d records, attempts %d" % (c, (time.perf_counter() - tc0) * 1e3, st["gpu_ms"], st["host_ms"], len(ov), st["replay_attempts"]))
            if dump_rows is not None and prev is not None:
                # the chunk before's records: a device replay that emitted records has waited for their copy before starting its own
                # (holding every chunk's array instead would take new pinned blocks in the middle of the step)
                if not (st.get("device_replay") == 1 and len(ov)):
                    _lib.results_wait()
                dump_rows[prev_c] = dump_sample(prev, prev_c, CH)
            nrec += len(ov)
            prev, prev_c = ov, c
            cks[c] = (len(ov), st["stream_checksum"])
            if a.check_ref:
                keep_streams[c] = ov
            if hash_streams:      # (the extra step after the timed region: the content is needed now, and the hashing runs beside the next chunk)
                _lib.results_wait()
                hash_jobs[c] = hash_pool.submit(formats.masked_stream_sha256, ov)
                hash_keep.append(ov)
            if tot is None:
                tot = dict(st)
            else:
                for k in SUM_KEYS:
                    tot[k] += st[k]
                tot["rounds"] = max(tot["rounds"], st["rounds"])
                tot["device_replay"] = min(tot["device_replay"], st["device_replay"])
            del ov
        _lib.results_wait()                     # the last chunk's records have arrived: the step is complete
        _lib.results_async(was_async)
        if dump_rows is not None and prev is not None:
            dump_rows[prev_c] = dump_sample(prev, prev_c, CH)
        del prev
        tot["chunks"] = len(my_chunks)
        tot["chunk_checksums"] = cks
        return ix, nrec, tot, s1 - s0

    def step_one_chunk():
        """one pass of the hot path: index chunk rank+1 of world, the exchange, overlap chunk rank+1 of world.
        Returns (IndexOut, ovlp records, stats, seconds of the index stage)."""
        s0 = time.perf_counter()
        if not multi and not a.two_stage:   # one chunk: the shimmer list and its counts stay in HBM between the stages
            ix, ov, st = rdb.index_overlap(levels=sp['levels'], mc_upper=sp['mc_upper'])
            keep_streams[1] = ov
            return ix, len(ov), st, ix.ms * 1e-3
        if not multi:
            ix = rdb.index(levels=sp['levels'])
            s1 = time.perf_counter()
            ov, st = rdb.overlap(ix.top, ix.top_mc, mc_upper=sp['mc_upper'])
            keep_streams[1] = ov
            return ix, len(ov), st, s1 - s0
        ix, top, mc = eng.index(world, rank + 1, sp['levels'])
        s1 = time.perf_counter()
        (ov, st), info = exchange_overlap(eng, rank, world, top, mc, **ov_params)   # counts all-gather + record all-to-all(v), on device
        st["exchange"] = info
        keep_streams[rank + 1] = ov
        return ix, len(ov), st, s1 - s0

    step = step_strong if strong else step_one_chunk

    def fence():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    log(f"{a.warmup} warm-up step(s) done")
    # The seqdb's BYTES out of HBM (VERDICT r5 task 5): the warm-up's first overlap stage has built the 2-bit packs (a quarter of the size, the same
    # information, laid out by locus), and every kernel of the timed path reads them -- so the timed steps run with the packs alone.  What needs
    # the bytes afterwards (the reference CPU leg's files, the seqdb's SHA-256, --check-ref, the end-to-end leg) gets them from the seeded
    # generator again (read_set_hash is re-checked).  PGX_BENCH_KEEP_BYTES=1: as through round 5.
    bytes_released = False
    if a.warmup >= 1 and os.environ.get("PGX_BENCH_KEEP_BYTES") != "1":
        bytes_released = bool(rdb.release_bytes())
        if bytes_released and seq_dev is not None:
            seq_dev = None
            import gc
            gc.collect()
            torch.cuda.empty_cache()
        log("seqdb bytes released: %s (%.1f GB of HBM in use)" % (bytes_released, (torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]) / 1e9))

    def seq_bytes():
        """the resident seqdb's bytes as a device tensor: the one the library still reads, or -- after the release -- the generator's output again"""
        nonlocal seq_dev
        if seq_dev is None and strong:
            t0 = time.perf_counter()
            seq_dev, total2, _ = simreads.make_workload_resident(a.workload, genome_mb=a.genome_mb or None)
            assert total2 == total and device_read_set_hash(seq_dev, total) == read_set_hash, "the regenerated read set differs from the one the steps ran on"
            log(f"seqdb bytes generated again in {time.perf_counter() - t0:.1f} s (same read_set_hash)")
        return seq_dev
    _lib.timing_reset()
    t_index = t_ovlp = 0.0
    fence()
    t0 = time.perf_counter()
    step_checksums = []
    for i in range(a.steps):
        if a.dump_outputs and i == a.steps - 1:
            dump_rows = {}
        s0 = time.perf_counter()
        ix, nrec, st, ti = step()
        t_index += ti
        t_ovlp += time.perf_counter() - s0 - ti
        step_checksums.append(st.get("chunk_checksums") or {my_chunks[0]: (int(nrec), int(st["stream_checksum"]))})
    fence()
    elapsed = time.perf_counter() - t0
    log(f"{a.steps} timed step(s): {elapsed:.2f} s")
    if dump_rows is not None:
        _lib.results_wait()
        for c in my_chunks:
            if c not in dump_rows:     # (the one-chunk forms keep the last step's whole stream)
                dump_rows[c] = dump_sample(np.asarray(keep_streams[c]), c, CH)
        write_dump(a.dump_outputs, dump_rows, step_checksums[-1], CH)
        dump_rows = None
        log(f"outputs of the last timed step written to {a.dump_outputs}")

    tot = torch.tensor([elapsed, float(nrec), float(ix.bases), t_index, t_ovlp], dtype=torch.float64, device=xdev)
    if multi:
        mx = tot.clone(); dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = tot.clone(); dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        elapsed, t_index, t_ovlp = float(mx[0]), float(mx[3]), float(mx[4])
        records, bases = float(sm[1]), float(sm[2])
    else:
        records, bases = float(nrec), float(ix.bases)

    ref_check = None
    if a.check_ref and strong:
        ref_check = check_vs_reference(seq_bytes(), total, db, rank, world, CH, my_chunks, keep_streams, sp["levels"], sp["mc_upper"], multi, xdev)

    # the library's kernel timers over exactly the timed steps (read before anything else runs)
    kern = {}
    for name in ("sketch", "sketch_redo", "sketch_nreads", "sketch_general", "sketch_gather", "reduce", "count", "pairs", "visit", "pack", "align", "align1"):
        ms, launches, units = _lib.timing(name)
        if launches:
            kern[name] = {"ms_total": ms, "launches": launches, "units": units, "avg_ms": ms / launches, "steps": a.steps}

    # ---- the streams, hashed (VERDICT r4 task 3).  Every timed step reports, per chunk, the 64-bit checksum k_emit adds up while
    # it writes the records (order-sensitive, all fields, padding excluded).  ONE more step after the timed region keeps every chunk's stream
    # and SHA-256s it with the padding bytes (27, 60..63) zeroed; its per-chunk checksums must equal those of every timed step, so the hashed
    # streams ARE the timed ones.  tests/golden/c4_stream_pins.json holds the same hashes of oracle/_ref/shmr_overlap's streams.
    stream_report = None
    if a.full and not os.environ.get("PGX_BENCH_NO_STREAM_HASH"):
        hash_streams = True
        hash_jobs.clear(), hash_keep.clear()
        _, _, st_h, _ = step()
        hash_streams = False
        if not strong or (world > 1 and len(my_chunks) == 1):      # one chunk per rank: the stream the step kept
            for c in my_chunks:
                hash_jobs[c] = hash_pool.submit(formats.masked_stream_sha256, np.asarray(keep_streams[c]))
        mine_rows = []
        for c in my_chunks:
            sha = hash_jobs[c].result()
            nrec_c, ck = st_h["chunk_checksums"][c] if "chunk_checksums" in st_h else (int(st_h["n_records"]), int(st_h["stream_checksum"]))
            same = all(sc is None or sc.get(c) == (nrec_c, ck) for sc in step_checksums) if step_checksums and step_checksums[0] is not None else None
            mine_rows.append([c, int(nrec_c), ck >> 32, ck & 0xFFFFFFFF, 1 if same else 0 if same is not None else -1] + [int(sha[i:i + 8], 16) for i in range(0, 64, 8)])
        hash_keep.clear(), hash_jobs.clear()
        flat = [v for r in mine_rows for v in r]
        allrows = allgather_ints(flat, world, device=home if backend == "nccl" else None) if multi else [flat]
        rows = sorted(tuple(r[i:i + 13]) for r in allrows for i in range(0, len(r), 13))
        stream_report = [{"chunk": "%d of %d" % (r[0], CH), "records": r[1], "stream_checksum": (r[2] << 32) | r[3],
                          "checksum_equal_in_every_timed_step": None if r[4] < 0 else bool(r[4]), "masked_sha256": "".join("%08x" % v for v in r[5:13])} for r in rows]
        log("streams of one more step hashed")

    # per rank: HBM in use, records through the exchange
    ex = st.get("exchange") or {}
    rank_row = [int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0]), int(ex.get("sent_records", 0)), int(ex.get("received_records", 0)), int(nrec), len(my_chunks)]
    rank_rows = allgather_ints(rank_row, world, device=home if backend == "nccl" else None) if multi else [rank_row]

    if rank == 0:
        if a.full and st.get("device_replay") and not multi and not os.environ.get("PGX_BENCH_NO_REPLAY_TIMING"):
            # the device replay's kernels (k_eval + k_update pairs) are timed in ONE EXTRA step, outside the timed region: a HIP
            # event pair around each of their ~40 launches per step would cost ~2 % of the step
            kern_timed = kern
            os.environ["PGX_REPLAY_TIMING"] = "1"
            _lib.timing_reset()
            _, _, st_x, _ = step()
            os.environ.pop("PGX_REPLAY_TIMING")
            rk = {}
            for nm, kname in (("replay_dense", "k_eval"), ("replay_rows", "k_eval_rows"), ("replay_big", "k_eval_big"), ("replay_update", "k_update"),
                              ("replay_misc", "table clears + k_setup + k_count_a/b + k_file + k_settle"), ("replay_emit", "k_emit + records to the host")):
                ms, launches, units = _lib.timing(nm)
                if launches:
                    rk[kname] = {"ms_total": ms, "launches": launches, "avg_ms": ms / launches}
            if rk:
                ms = sum(v["ms_total"] for v in rk.values())
                launches = max(v["launches"] for k_, v in rk.items() if k_.startswith("k_eval") or k_ == "k_update")
                kern["replay"] = {"ms_total": ms, "launches": launches, "units": int(st_x["n_evaluations"]), "avg_ms": ms / launches,
                                  "steps": 1, "by_kernel": rk, "max_kernel_ms": max(v["ms_total"] for v in rk.values()),
                                  "note": "one extra untimed step with PGX_REPLAY_TIMING=1; launches = evaluate/update rounds"}
        cands = {}     # (--full: the roofline takes the replay-timing step and the committed counter passes)
        if a.full and "sketch" in kern:
            k = kern["sketch"]
            gbs = SKETCH_BYTES_PER_BASE * k["units"] / (k["ms_total"] * 1e-3) / 1e9
            cands["sketch"] = {"kernel": "k_sketch_blk (+ k_sketch_wave for the reads it flags)", "bound": "valu_issue", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": gbs / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": k["avg_ms"],
                               "bytes_per_unit": SKETCH_BYTES_PER_BASE, "unit_name": "base",
                               "gbases_per_s": k["units"] / (k["ms_total"] * 1e-3) / 1e9}
        if a.full and "align" in kern:
            k = kern["align"]
            gbs = ALIGN_BYTES_PER_PAIR * k["units"] / (k["ms_total"] * 1e-3) / 1e9
            cands["align"] = {"kernel": "k_align_ph<8, u16, packed> (per-group phase machine over the 2-bit packs; + k_pack2 once per stage, k_align1_list for the candidates it hands on)", "bound": "valu_issue", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": gbs / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": k["avg_ms"],
                              "bytes_per_unit": ALIGN_BYTES_PER_PAIR, "unit_name": "alignment",
                              "alignments_per_s": k["units"] / (k["ms_total"] * 1e-3),
                              "bound_note": "instruction issue AND the wavefront's own dependent chain per d-step, at the hardware's 8 wavefronts per SIMD (DESIGN 4.4 round 4 (c): "
                                            "+10 % VALU = +16 % time, +46 % SALU = +8.5 %, 28 instead of 32 wavefronts per CU = +6 %); through round 4 the work counter's "
                                            "same-address atomic (12 ns per candidate) was the floor, not the instructions"}
        if a.full and "align1" in kern:   # the one-candidate-per-wavefront form used for launches of at most 13 k alignments (tail rounds)
            k = kern["align1"]
            gbs = ALIGN_BYTES_PER_PAIR * k["units"] / (k["ms_total"] * 1e-3) / 1e9
            cands["align1"] = {"kernel": "k_align1", "bound": "latency", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": gbs / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": k["avg_ms"],
                               "bytes_per_unit": ALIGN_BYTES_PER_PAIR, "unit_name": "alignment",
                               "alignments_per_s": k["units"] / (k["ms_total"] * 1e-3)}
        if a.full and "replay" in kern:   # the greedy walk on the GPU: dependent random probes of the pair / memo tables, latency-bound
            k = kern["replay"]
            walk = 13 * st["n_pair_records"] + 16 * (st["n_seen_skip"] + st["n_align_needed"]) + 48 * st["n_align_needed"] + 16 * st["n_records"]
            per_eval = walk / max(1, st["n_buckets"])   # algorithmic bytes of one bucket evaluation
            gbs = per_eval * k["units"] / (k["ms_total"] * 1e-3) / 1e9
            cands["replay"] = {"kernel": "k_eval + k_eval_rows + k_eval_big + k_update (+ counts / k_file / k_settle / k_emit: the device replay as a stage)", "bound": "latency", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": gbs / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": k["avg_ms"],
                               "bytes_per_unit": per_eval, "unit_name": "bucket evaluation",
                               "evaluations_per_s": k["units"] / (k["ms_total"] * 1e-3)}
        attach_counters(cands, kern, a.workload)
        for nm in cands:
            cands[nm]["algorithmic_bytes_per_launch"] = cands[nm]["bytes_per_unit"] * kern[nm]["units"] / kern[nm]["launches"]
            cands[nm]["algorithmic_bytes_per_step"] = cands[nm]["bytes_per_unit"] * kern[nm]["units"] / kern[nm]["steps"]
            cands[nm]["launches_per_step"] = kern[nm]["launches"] / kern[nm]["steps"]
            cands[nm]["kernel_ms_per_step"] = cands[nm]["stage_ms_per_step"] = kern[nm]["ms_total"] / kern[nm]["steps"]
        roof = None
        if cands:
            # the STAGE with the most device time per step (the device replay counts as a whole, not by its heaviest kernel)
            stage_ms = {n: kern[n]["ms_total"] / kern[n]["steps"] for n in cands}
            if "align" in stage_ms and "align1" in stage_ms:
                stage_ms["align"] += stage_ms["align1"]
            roof = cands[max(stage_ms, key=stage_ms.get)]
        wl = WORKLOAD_TEXT.get(a.workload, a.workload)
        if strong:
            gm = a.genome_mb or simreads.WORKLOADS[a.workload]["genome_len"] / 1e6
            if a.genome_mb:
                wl = f"the {a.workload} recipe on a {gm:g} Mb genome (repeat content scaled with the size) x 30x"
            workload = (f"{a.workload}: {wl}, ONE read set held by every rank, 15 kb +-1.5 kb reads, 1 % errors, k=16 w=80 r=6 l={LEVELS}, "
                        f"index_nchunk=ovlp_nchunk={CH} dealt round-robin to {world} GPU(s) ({len(my_chunks)} index + {len(my_chunks)} overlap chunks per GPU per step), "
                        f"bestn 4, mc 2..{sp['mc_upper']}, aln_bw 100")
            comm = "rccl" if backend == "nccl" else backend
            par = f"chunks{CH}/gpus{world}" + (f"+alltoall({comm})" if world > 1 and len(my_chunks) == 1 else f"+allgather({comm})" if world > 1 else "")
        else:
            workload = (f"{a.workload}: {wl} per rank, 15 kb +-1.5 kb reads, 1 % errors, "
                        f"k=16 w=80 r=6 l={LEVELS}, index_nchunk=ovlp_nchunk={world}, bestn 4, mc 2..240, aln_bw 100"
                        + (f", {a.ambiguous_frac:g} of the reads with 1-3 ambiguous bases" if a.ambiguous_frac > 0 else ""))
            par = f"chunks{world}" + ("+forced-exchange(rccl)" if multi and world == 1 else "")
        out = {
            "metric": "confirmed overlaps/sec (ovlp_t records, index+overlap stages, seqdb resident in HBM)",
            "value": records * a.steps / elapsed, "unit": "overlaps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "u8/u32 integer", "data": "synthetic",
            "config": {"workload": workload, "reads": int(db.n_reads), "bases": int(db.n_bases), "parallelism": par},
            "bases_per_sec_indexed": bases * a.steps / t_index if t_index else None,
            "overlap_records_per_sec": records * a.steps / t_ovlp if t_ovlp else None,
            "records_per_step": records, "index_ms_per_step": t_index / a.steps * 1e3, "overlap_ms_per_step": t_ovlp / a.steps * 1e3,
            "overlap_stats_rank0": st, "reads_literal_rank0": ix.reads_literal,
            "kernels": kern,
        }
        if a.full:
            out["roofline"], out["roofline_all"] = roof, cands
        out["world_size"] = int(dist.get_world_size()) if multi else 1     # as the process group sees it
        out["per_rank"] = [{"rank": r, "hbm_bytes_in_use": row[0], "sent_records": row[1], "received_records": row[2], "records_last_step": row[3],
                            "chunks": row[4]} for r, row in enumerate(rank_rows)]
        if strong:
            out["hbm_bytes_in_use"] = int(rank_rows[0][0])
        if strong and a.full:
            out["read_set_hash"] = read_set_hash
            out["read_set_hash_equal_on_all_ranks"] = True if world == 1 else read_set_hash_equal
        if stream_report is not None:
            out["streams"] = stream_report
            out["stream_sha256"] = [r["masked_sha256"] for r in stream_report]
            out["stream_checksums_equal_in_every_timed_step"] = all(r["checksum_equal_in_every_timed_step"] is not False for r in stream_report)
            out["stream_hash_note"] = ("masked_sha256: SHA-256 of the chunk's ovlp_t stream with the padding bytes 27 and 60..63 of every record zeroed, of ONE MORE "
                                       "step run after the timed region; stream_checksum: the 64-bit checksum k_emit adds up while it writes the records, reported "
                                       "by every timed step for every chunk and equal to the hashed step's -- the hashed streams are the timed ones")
        # the HBM ledger (VERDICT r4 task 5): the library's device memory by owner at the moment its live total peaked, what its block cache
        # holds beside that, and torch's side (the adopted seqdb, the lists held between the stages)
        led = _lib.mem_ledger()
        led["torch_allocated_bytes"] = int(torch.cuda.memory_allocated())
        led["torch_reserved_bytes"] = int(torch.cuda.memory_reserved())
        if seq_dev is not None:
            led["seqdb_bytes_adopted_from_torch"] = int(seq_dev.numel())
        led["seqdb_bytes_released_after_warmup"] = bytes_released
        out["hbm_ledger"] = led
        if ref_check is not None:
            out["check_vs_reference"] = ref_check
        # device time per step by the library's own timers (HIP events; the replay's from the extra step) against the wall clock
        ksum = sum(v["ms_total"] / v["steps"] for v in kern.values())
        out["kernel_sum_ms_per_step"] = ksum
        out["kernel_sum_over_step"] = ksum / (elapsed / a.steps * 1e3) if elapsed else None
        out["kernel_sum_note"] = ("sum of the `kernels` entries per step (sketch .. visit, alignment launches, every replay kernel incl. clears, "
                                  "k_file / k_settle / counts, k_emit + the records' copy to the host); not in it: the join tables' small "
                                  "copies, RCCL; the replay's kernels are timed in an extra step WITHOUT their second stream and the record copy of a multi-chunk "
                                  "step overlaps the next chunk, so the sum can exceed the step; tools/timeline.py / chunk_timeline.py on a rocprofv3 "
                                  "kernel trace give the busy / idle split kernel by kernel")
        # (the legs below run the reference on the host and shell out: whatever goes wrong there, the line of the timed steps still goes out)
        try:
            if a.full and world == 1 and not a.no_cpu_baseline:
                if strong:
                    def gpu_index_files(prefix):     # the job's index chunk files, as bin/shmr_index writes them
                        for c in range(1, CH + 1):
                            p = rdb.index(total_chunk=CH, mychunk=c, levels=sp["levels"])
                            formats.write_mmlist("%s-L%d-%02d-of-%02d.dat" % (prefix, sp["levels"], c, CH), p.top)
                            formats.write_mm_count("%s-L%d-MC-%02d-of-%02d.dat" % (prefix, sp["levels"], c, CH), p.top_mc)
                    # The honest leg is the WHOLE workload (24 processes over 24 + 24 chunks: ~12-14 min at full size); it is the default where the
                    # command's time budget allows (PGX_BENCH_BUDGET_S, default BUDGET_S), else the bounded sample -- and the line says which
                    mode = a.cpu_baseline
                    fallback_reason = None
                    if mode is None:
                        whole = "whole_chunks" if sp["levels"] == 1 else "full"
                        need = (1300.0 if whole == "whole_chunks" else 900.0) * (db.n_bases / 93.3e9) + 60
                        left = budget_s() - (time.perf_counter() - _T0) - 150
                        mode = whole if left >= need else "sample"
                        log(f"cpu baseline: {mode} (estimated {need:.0f} s for the {whole} leg, {left:.0f} s of the budget left)")
                        if mode == "sample":
                            fallback_reason = (f"the {whole} reference leg needs ~{need:.0f} s and {left:.0f} s of the command's budget (PGX_BENCH_BUDGET_S) were left: "
                                               f"bounded sample instead; gpu_over_cpu.vs_n_cores_raw_records is null for a sample")
                            sys.stderr.write("[bench] WARNING: cpu_baseline falls back to mode 'sample': " + fallback_reason + "\n")
                    # the end-to-end leg (default where the budget allows; it runs LAST -- this process gives its HBM to the server) reads the same seqdb files
                    # as the reference: written once, shared
                    cpu_est = {"full": 900.0, "whole_chunks": 1300.0, "sample": 330.0}[mode] * (db.n_bases / 93.3e9) + 60
                    left_after = budget_s() - (time.perf_counter() - _T0) - cpu_est
                    if a.end_to_end is None:
                        a.end_to_end = bool(not a.genome_mb and a.workload == "c4" and left_after >= 200)
                        log(f"end to end leg: {'on' if a.end_to_end else 'off'} ({left_after:.0f} s of the budget expected to be left after the CPU leg)")
                    if a.end_to_end:
                        need = int(total * 1.02) + int(db.n_bases * 0.5) + (8 << 30)
                        base = _scratch_dir(need)
                        if base is not None:
                            sdir = tempfile.mkdtemp(prefix="pgx_bench_", dir=base)
                            tw = time.perf_counter()
                            simreads.write_seqdb_from_device(os.path.join(sdir, "sd"), seq_bytes(), total, db.rid, db.rlen, db.roff)
                            shared_files = {"dir": sdir, "prefix": os.path.join(sdir, "sd"), "seconds": time.perf_counter() - tw}
                    sha_thread = None
                    if not a.genome_mb and not os.environ.get("PGX_BENCH_NO_STREAM_HASH"):     # the seqdb's SHA-256, beside the CPU leg's (untimed) file writing
                        import threading
                        sha_box = {}
                        sha_src = seq_bytes()
                        sha_thread = threading.Thread(target=lambda: sha_box.update(v=seqdb_sha256_of_device(sha_src, total)))
                        sha_thread.start()
                    out["cpu_baseline"] = cpu_baseline_chunked(seq_bytes(), total, db, rdb, eng, a.workload, mode, sp["levels"], sp["mc_upper"], CH, gpu_index_files, held,
                                                               stream_report=stream_report, before_timing=(sha_thread.join if sha_thread is not None else None),
                                                               files=shared_files)
                    if sha_thread is not None:
                        sha_thread.join()
                        out["seqdb_sha256"] = sha_box.get("v")
                        sha_src = sha_thread = None     # (the thread's hold on the regenerated 93 GB: the end-to-end leg needs that HBM for its server)
                    if fallback_reason:
                        out["cpu_baseline"]["fallback_reason"] = fallback_reason
                elif a.cpu_baseline == "sample":
                    sample = simreads.simulate_reads_torch(10_000_000, 1003, 30.0, seed=42)
                    out["cpu_baseline"] = cpu_baseline_sample(sample)
                else:
                    out["cpu_baseline"] = cpu_baseline(db, keep_streams[1], a.workload, sp["levels"], sp["mc_upper"])
                cb = out["cpu_baseline"]
                if strong and cb.get("mode") == "sample" and not a.genome_mb:
                    # the bounded sample UNDERSTATES the reference: each of its processes still loads every shimmer / count file and scans the whole
                    # list (a fixed cost per process) for 1/8 of the first keys.  The whole-workload leg of the same tree family is committed:
                    try:
                        full = json.load(open(os.path.join(ROOT, "profiles", "r04e_bench_c4_full.json")))["cpu_baseline"]
                        if a.workload == "c4" and full.get("mode") == "full":
                            cb["whole_workload_leg"] = {"value": full["value"], "unit": "overlaps/s", "cores": full["cores"], "index_s": full["index_s"], "overlap_s": full["overlap_s"],
                                                        "records": full["records"], "unique_pairs_per_s": full.get("unique_pairs_per_s"),
                                                        "source": "profiles/r04e_bench_c4_full.json (python bench.py --cpu-baseline full: 24 processes over 24 + 24 chunks of the whole 93 Gbases, "
                                                                  "13 min 43 s of the box; not re-run in the default command)"}
                            cb["sample_note"] = ("the sample's rate is lower than the whole-workload leg's (fixed per-process cost over 1/8 of the work): compare `value` with "
                                                 "whole_workload_leg.value")
                    except Exception:
                        pass
                if cb.get("value"):
                    out["gpu_over_cpu"] = {"vs_n_cores_raw_records": out["value"] / cb["value"] if cb.get("mode") != "sample" else None,
                                           "vs_n_cores_unique_pairs": out["value"] / cb["unique_pairs_per_s"] if cb.get("unique_pairs_per_s") and cb.get("mode") != "sample" else None,
                                           "vs_one_core": out["value"] / cb["one_core"]["value"] if cb.get("one_core") else None, "cpu_cores": cb["cores"],
                                           "vs_whole_workload_leg_raw_records": out["value"] / cb["whole_workload_leg"]["value"] if cb.get("whole_workload_leg") else None,
                                           "note": "the N-chunk CPU run reports most pairs once per chunk, so both of its rates are given; one-chunk "
                                                   "workloads: GPU value = records of ONE overlap chunk (every read pair once)"}
                    if cb.get("mode") == "whole_chunks" and out.get("overlap_ms_per_step"):
                        k = cb["chunks_run"]
                        out["gpu_over_cpu"]["same_chunks"] = {
                            "what": "overlap stage of the SAME %d chunks of the job's own chunking (T = %d): reference wall time, %d processes side by side, vs the GPU's overlap "
                                    "time per step x %d/%d; equal streams (cpu_baseline.records_match_gpu)" % (k, CH, cb["overlap_processes"], k, CH),
                            "cpu_overlap_s": cb["overlap_s"], "cpu_processes": cb["overlap_processes"], "gpu_overlap_s": out["overlap_ms_per_step"] * 1e-3 * k / CH,
                            "ratio": cb["overlap_s"] / (out["overlap_ms_per_step"] * 1e-3 * k / CH)}
        except Exception as e:
            import traceback
            sys.stderr.write("[bench] WARNING: the reference CPU leg failed: %s\n%s" % (e, traceback.format_exc()))
            cb = out.get("cpu_baseline") or {}
            cb.update({"error": repr(e)})
            cb.setdefault("value", None), cb.setdefault("unit", "overlaps/s"), cb.setdefault("cores", 0), cb.setdefault("kind", "none"), cb.setdefault("sample", "the leg failed: see `error`")
            out["cpu_baseline"] = cb
        # ---- the pins: hashes of the REFERENCE's streams for this configuration (tests/golden/make_c4_stream_pins.py ran oracle/_ref/shmr_overlap
        # -t 8 -c 1..8 on the same seqdb bytes; SURVEY 8c/d, VERDICT r4 task 3)
        if stream_report is not None and strong and not a.genome_mb and os.path.exists(PINS_FILE):
            try:
                pins = json.load(open(PINS_FILE)).get(a.workload)
            except Exception:
                pins = None
            if pins and pins.get("chunks") == CH:
                want = {c["chunk"]: c for c in pins["streams"]}
                # (every pinned chunk must be there and equal; configs[4] pins a subset of its 24 chunks -- `chunks_pinned` says how many)
                rows_ok = [want[r["chunk"]]["records"] == r["records"] and want[r["chunk"]]["masked_sha256"] == r["masked_sha256"]
                           for r in stream_report if r["chunk"] in want]
                same_input = pins.get("read_set_hash") == read_set_hash and (out.get("seqdb_sha256") is None or out["seqdb_sha256"] == pins.get("seqdb_sha256"))
                out["streams_match_pins"] = bool(same_input and len(stream_report) == CH and len(rows_ok) == len(want) and len(want) > 0 and all(rows_ok))
                if pins.get("reference_overlap_leg_s") and out.get("overlap_ms_per_step"):
                    # the SAME job on both sides (VERDICT r5 task 6a): the reference ran exactly these CH overlap chunks (the pinned streams are its output)
                    # as `reference_overlap_processes` processes side by side on the GPU box's host cores when the pins were made
                    procs = pins.get("reference_overlap_processes", pins["chunks"])
                    out.setdefault("gpu_over_cpu", {})["same_job"] = {
                        "what": "overlap stage of this very job (T = %d, chunks %s): the reference's wall time when the pins were made vs the GPU's overlap time per step; "
                                "equal streams by the pins" % (CH, "1..%d" % CH if len(want) == CH else sorted(want)),
                        "cpu_overlap_s": pins["reference_overlap_leg_s"], "cpu_processes": procs, "cpu_chunks": len(want),
                        "gpu_overlap_s": out["overlap_ms_per_step"] * 1e-3 * len(want) / CH,
                        "ratio": pins["reference_overlap_leg_s"] / (out["overlap_ms_per_step"] * 1e-3 * len(want) / CH),
                        "cpu_overlaps_per_s": sum(c["records"] for c in pins["streams"]) / pins["reference_overlap_leg_s"],
                        "source": "tests/golden/c4_stream_pins.json (reference_overlap_leg_s; tests/golden/make_c4_stream_pins.py)"}
                out["pins"] = {"file": "tests/golden/c4_stream_pins.json", "same_input_bytes": bool(same_input), "chunks_pinned": len(want),
                               "chunks_equal": int(sum(rows_ok)), "pinned_seqdb_sha256": pins.get("seqdb_sha256"),
                               "what": "SHA-256 of oracle/_ref/shmr_overlap's stream (padding bytes zeroed) for the pinned overlap chunks of this configuration (configs[3]: all 8; configs[4]: 8 of 24), "
                                       "made on the GPU box's host cores from the same seqdb bytes (the generator is seeded; read_set_hash and seqdb_sha256 tie the inputs)"}
        if a.end_to_end is None:     # (no CPU leg in this run)
            a.end_to_end = False
        if a.end_to_end and strong and world == 1:
            try:
                seq_box = [seq_bytes() if shared_files is None else seq_dev]     # (the files exist already: nothing to write)
            except Exception as e:
                seq_box = [None]
                out["gpu_end_to_end"] = {"error": "the seqdb bytes could not be generated again: " + repr(e)}
                a.end_to_end = False
            seq_dev = None
        if a.end_to_end and strong and world == 1:

            def release_all():
                seq_box.clear()
                held.clear()
                keep_streams.clear()
            out["gpu_end_to_end"] = end_to_end_served(seq_box, total, db, rdb, CH, sp["levels"], sp["mc_upper"], stream_report, release_all, files=shared_files)
            e2e = out["gpu_end_to_end"]
            if e2e.get("overlaps_per_s"):
                e2e["over_resident"] = (e2e["index_s"] + e2e["overlap_s"]) / (out["ms_per_step"] * 1e-3)
        if shared_files is not None:
            import shutil
            shutil.rmtree(shared_files["dir"], ignore_errors=True)
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
