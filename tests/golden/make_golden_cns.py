"""Generator of tests/golden/cns_cases.npz: seeded pieces of alignments and what the REAL reference makes of them.

The reference's falcon/falcon.c, DW_banded.c and kalloc.c are compiled in place with -DNDEBUG (as its cffi build compiles them) into a
temporary directory, and align, get_align_tags and get_cns_from_align_tags are called through ctypes.  Stored: the inputs in compact form
(template, read bases, run-length operations: tests/cns_util.py expands them to strings), the reference's tags of every alignment and its
consensus of every piece.  Before the reference sees a case the restatement of cns_util runs on it and must find an end node and none of
the refusal conditions, so that no stored answer rests on undefined behaviour; afterwards the two must agree.

  real_*      falcon.align output of reads mutated at 0, 1, 5 and 15 %: templates of 60 .. 3,000 bases, 1 .. 20 reads, two-letter and
              homopolymer-rich templates, t_offset = 0 mixed with t_offset > 0 (the '.' predecessor sorts last / in place)
  backbone    the template against itself alone: the template in lower case at min_cov = 1
  hand_*      alignment strings as data: a tie of two bases, insertions of 254 / 255 / 300 bases (the cut), a long deletion, an insertion
              column of one read among many, coverage 1 and 2 at min_cov 0, 1, 2, reads that end mid-template, and one template position
              with more nodes than the scoring kernel's LDS ring holds
  batch64     64 pieces of 60 .. 2,000 bases in one case
  big8192     one piece of 8,400 bases with 12 reads
  edge_*      (a generator of their own, seed + 1, so that the cases above never move) two nodes 1023, 1024, 1025 and 2047, 2048, 2049
              apart in key order (the scoring ring holds 1024, the back-track window 2048); every pair of the ten letters tied at one
              column, every letter against a gap, every letter inserted; the cut on the last and the first lane of a chunk of columns;
              empty alignments, insertions only, rows of zero tags, insertion runs that end a chunk, one column on the last base, negative
              s2; min_cov 3, 65535 and 2^31 - 1, a lower-case and an all-N template; one piece of 65,535 identical alignments (stored
              once with its repeat count); the same distances of 2047, 2048 and 2049 between the END node and its predecessor, where
              the back-track's first window begins

    python tests/golden/make_golden_cns.py [path/to/reference/falcon]
"""
import ctypes as C
import hashlib
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import cns_util as CU  # noqa: E402

FALCON = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/falcon"
SOURCES = ("falcon.c", "DW_banded.c", "kalloc.c")
CFLAGS = ["-O2", "-DNDEBUG", "-fPIC", "-shared"]
SEED = 20261020
BENCH = dict(seed=7, pieces=2, t_len=50_000, reads=30)      # the first pieces of tools/cns_bench.py's batch, timed on the reference


class Alignment(C.Structure):
    _fields_ = [("aln_str_size", C.c_int), ("dist", C.c_int), ("aln_q_s", C.c_int), ("aln_q_e", C.c_int), ("aln_t_s", C.c_int),
                ("aln_t_e", C.c_int), ("q_aln_str", C.c_void_p), ("t_aln_str", C.c_void_p)]


class AlnRange(C.Structure):
    _fields_ = [("s1", C.c_int), ("e1", C.c_int), ("s2", C.c_int), ("e2", C.c_int), ("score", C.c_long)]


class AlignTags(C.Structure):
    _fields_ = [("len", C.c_int), ("align_tags", C.c_void_p)]


class ConsensusData(C.Structure):
    _fields_ = [("sequence", C.c_char_p), ("eqv", C.c_void_p)]


REF_TAG = np.dtype([("t_pos", "<i4"), ("delta", "u1"), ("q_base", "u1"), ("pad0", "u1", 2), ("p_t_pos", "<i4"), ("p_delta", "u1"),
                    ("p_q_base", "u1"), ("pad1", "u1", 2), ("q_id", "<u4")])


def compile_reference(tmp):
    so = os.path.join(tmp, "libfalcon_ref.so")
    subprocess.check_call(["gcc", *CFLAGS, "-I", FALCON, *[os.path.join(FALCON, s) for s in SOURCES], "-o", so])
    lib = C.CDLL(so)
    lib.align.restype = C.POINTER(Alignment)
    lib.align.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int]
    lib.free_alignment.argtypes = [C.POINTER(Alignment)]
    lib.get_align_tags.restype = C.POINTER(AlignTags)
    lib.get_align_tags.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(AlnRange), C.c_uint, C.c_int]
    lib.free_align_tags.argtypes = [C.POINTER(AlignTags)]
    lib.get_cns_from_align_tags.restype = C.POINTER(ConsensusData)
    lib.get_cns_from_align_tags.argtypes = [C.POINTER(C.POINTER(AlignTags)), C.c_uint, C.c_uint, C.c_uint]
    lib.free_consensus_data.argtypes = [C.POINTER(ConsensusData)]
    return lib


def ref_align(lib, read, template, t_offset, band=150):
    """falcon.align(read, template[t_offset:]) as an alignment of cns_util, or None where nothing aligned"""
    target = template[t_offset:]
    a = lib.align(read, len(read), target, len(target), band, 1)
    try:
        n = a.contents.aln_str_size
        if n <= 0:
            return None
        return (C.string_at(a.contents.q_aln_str, n), C.string_at(a.contents.t_aln_str, n), a.contents.aln_q_s, a.contents.aln_t_s, t_offset)
    finally:
        lib.free_alignment(a)


def ref_piece(lib, t_len, alns, min_cov):
    """the reference's tags of every alignment and its consensus of the piece; the seconds both took"""
    t0 = time.perf_counter()
    arr = (C.POINTER(AlignTags) * (len(alns) + 1))()
    tags = []
    for i, (q, t, s1, s2, off) in enumerate(alns):
        rng = AlnRange(s1, 0, s2, 0, 0)
        arr[i] = lib.get_align_tags(q, t, len(q), C.byref(rng), i, off)
    cns = lib.get_cns_from_align_tags(arr, len(alns), t_len, min_cov)
    dt = time.perf_counter() - t0
    seq = cns.contents.sequence
    lib.free_consensus_data(cns)
    for i in range(len(alns)):
        n = arr[i].contents.len
        raw = np.frombuffer(C.string_at(arr[i].contents.align_tags, n * REF_TAG.itemsize), REF_TAG) if n else np.zeros(0, REF_TAG)
        t = np.zeros(n, CU.TAG_DTYPE)
        for f in CU.TAG_FIELDS:
            t[f] = raw[f]
        tags.append(t)
        lib.free_align_tags(arr[i])
    return seq, tags, dt


def real_piece(lib, rng, template, n_reads, rate, offsets):
    """the back-bone (as pg_asm_cns.py adds it) and n_reads mutated reads of random spans, aligned by the reference"""
    alns = [ref_align(lib, template, template, 0, 50)]
    n = len(template)
    for i in range(8 * n_reads):
        if len(alns) == n_reads + 1:
            break
        # falcon.align extends from the start of both sequences: a read from the template's start at t_offset = 0, or one from
        # further in whose t_offset lies a few bases before it (pg_asm_cns.py's read_shift)
        span = int(rng.integers(max(40, n // 3), n + 1))
        a = int(rng.integers(0, n - span + 1)) if offsets and i % 2 else 0
        read = CU.mutate(rng, template[a:a + span], rate)
        t_offset = max(0, a - int(rng.integers(0, 6)))
        aln = ref_align(lib, read, template, t_offset)
        if aln is not None:
            alns.append(aln)
    assert len(alns) == n_reads + 1, (n, rate, len(alns))
    return template, alns


def hand_cases(rng):
    T = CU.random_template(rng, 120)
    full = lambda: CU.build(T, 0, 0, [("=", 120)])
    other = lambda b: bytes([next(x for x in b"ACGT" if x != b)])
    cases = []
    cases.append(("hand_tie", 1, [(T, [full(), CU.build(T, 0, 0, [("=", 50), ("X", other(T[50])), ("=", 69)])])]))
    cases.append(("hand_tie3", 1, [(T, [full(), full(), CU.build(T, 0, 0, [("=", 50), ("X", other(T[50])), ("=", 69)]),
                                       CU.build(T, 0, 0, [("=", 50), ("X", other(T[50])), ("=", 69)])])]))
    for n in (254, 255, 300):
        ins = rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
        cases.append((f"hand_ins{n}", 1, [(T, [full(), full(), CU.build(T, 0, 0, [("=", 40), ("I", ins), ("=", 80)]),
                                              CU.build(T, 10, 5, [("=", 25), ("I", ins), ("=", 60)]),
                                              CU.build(T, 0, 0, [("=", 40), ("I", ins), ("=", 80)])])]))
    cases.append(("hand_long_deletion", 1, [(T, [full(), CU.build(T, 0, 0, [("=", 30), ("D", 60), ("=", 30)]),
                                                 CU.build(T, 0, 0, [("=", 30), ("D", 60), ("=", 30)]),
                                                 CU.build(T, 0, 0, [("=", 30), ("D", 60), ("=", 30)])])]))
    cases.append(("hand_rare_insertion", 1, [(T, [full()] + [CU.build(T, 0, 0, [("=", 120)]) for _ in range(8)] +
                                              [CU.build(T, 0, 0, [("=", 70), ("I", b"GA"), ("=", 50)])])]))
    cov12 = [(T, [full(), CU.build(T, 0, 30, [("=", 40)]), CU.build(T, 20, 40, [("=", 30)])])]      # coverage 1, 2, 3 along the template
    for mc in (0, 1, 2):
        cases.append((f"hand_min_cov{mc}", mc, cov12))
    cases.append(("hand_ends_mid_template", 1, [(T, [full(), CU.build(T, 0, 0, [("=", 61)]), CU.build(T, 0, 0, [("=", 33), ("X", b"N"), ("=", 9)]),
                                                    CU.build(T, 5, 0, [("=", 47)]), CU.build(T, 0, 7, [("=", 20), ("D", 2), ("=", 30)])])]))
    cases.append(("hand_lower_case_reads", 1, [(T, [full(), CU.build(T, 0, 0, [("=", 20), ("X", b"acgtn"), ("=", 95)]),
                                                   CU.build(T, 0, 0, [("=", 20), ("X", b"acgtn"), ("=", 95)])])]))
    # 2,540 nodes at one template position: every delta 1 .. 254 with all ten letters
    letters = b"ACGTNacgtn"
    wide = [full(), full()] + [CU.build(T, 0, 0, [("=", 60), ("I", bytes(letters[(d + r) % 10] for d in range(254))), ("=", 60)]) for r in range(10)]
    cases.append(("hand_wide_position", 1, [(T, wide)]))
    return cases


def edge_cases(rng, cov12):
    """the edges of the kernels' windows at their exact values, the order of ties, rows that yield no tags: alignment strings as data"""
    T = CU.random_template(rng, 120)
    full = lambda t=T: CU.build(t, 0, 0, [("=", len(t))])
    acgt = lambda n: rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()
    cases = []
    # the nodes (59, 0) and (60, 0) exactly this far apart in key order: the scoring ring holds 1024, the back-track window 2048
    for what, dist in (("ring", 1023), ("ring", 1024), ("ring", 1025), ("back", 2047), ("back", 2048), ("back", 2049)):
        cases.append((f"edge_{what}_{dist}", 1, [CU.wide_position(T, 60, dist - 1, 12)]))
    # ties, settled by the ASCII order of the letters: every pair of letters at one column, every letter against a gap, every letter inserted
    T100 = CU.random_template(rng, 100)
    L = CU.LETTERS
    at = lambda x: CU.build(T100, 0, 0, [("=", 50), ("X", bytes([x])), ("=", 49)])
    ties = [(T100, [at(L[i]), at(L[j])]) for i in range(10) for j in range(i + 1, 10)]
    ties += [(T100, [at(x), CU.build(T100, 0, 0, [("=", 50), ("D", 1), ("=", 49)])]) for x in L]
    ties += [(T100, [CU.build(T100, 0, 0, [("=", 50), ("I", bytes([x])), ("=", 50)]), CU.build(T100, 0, 0, [("=", 100)])]) for x in L]
    cases.append(("edge_ties", 0, ties))
    # the cut at delta 255 on columns 255, 256, 319 and 320: the last and the first lane of a chunk of 64 columns
    cut = []
    for c in (1, 2, 65, 66):
        ins = [acgt(255), acgt(255)]
        cut.append((T, [full(), full()] + [CU.build(T, 0, 0, [("=", c), ("I", i), ("=", 120 - c)]) for i in ins]))
    cases.append(("edge_cut_lanes", 1, cut))
    # rows of no or few tags, insertion runs that end a chunk, starts before and at the ends of the template
    n = len(T)
    strings = [full(), full(), (b"", b"", 0, 0, 0), (b"", b"", 0, 0, 3), (b"ACGT", b"----", 0, 10, 0),
               CU.build(T, 0, 0, [("=", 63), ("I", acgt(70))]), CU.build(T, 0, 0, [("=", 64), ("I", acgt(64))]),
               CU.build(T, 0, 0, [("I", b"AC"), ("=", 30)])]
    strings += [CU.build(T, off, s2, [("I", b"AC"), ("=", 30)]) for off, s2 in ((7, 3), (7, 0), (0, 9))]
    strings += [CU.build(T, 0, 0, [("D", 3), ("=", 30)]), CU.build(T, n - 1, 0, [("=", 1)]), CU.build(T, 0, n - 1, [("=", 1)]),
                CU.build(T, 10, -3, [("=", 40)]), (T[n - 3:], T[n - 3:], 0, -3, 0)]
    cases.append(("edge_strings", 1, [(T, strings)]))
    # min_cov beyond 2, at the reference's 16 bits and at the largest the fixture stores; lower-case and all-N templates
    for mc in (3, 65535, 2**31 - 1):                                                  # cov12: hand_min_cov*'s piece
        cases.append((f"edge_min_cov_max_{mc}", mc, cov12))
    low = T.lower()
    cases.append(("edge_min_cov_max_lower", 0, [(low, [full(low), full(low), CU.build(low, 0, 0, [("=", 40), ("X", b"n"), ("=", 79)])])]))
    allN = b"N" * 200
    cases.append(("edge_min_cov_max_allN", 1, [(allN, [full(allN), full(allN), CU.build(allN, 0, 0, [("=", 80), ("D", 2), ("=", 118)])])]))
    # as many alignments as the reference's 16-bit counters hold, stored once
    T8 = CU.random_template(rng, 8)
    cases.append(("edge_full_count", 1, [(T8, [full(T8)], CU.MAX_ALNS)]))
    # the back-track's window hangs from the node the walk stands on, first the end node: the wide position before the template's LAST
    # base makes the end node (119, 0) the one that jumps, its predecessor (118, 0) the window's lowest slot at 2047 and outside from 2048
    for dist in (2047, 2048, 2049):
        cases.append((f"edge_back_end_{dist}", 1, [CU.wide_position(T, len(T) - 1, dist - 1, 12)]))
    return cases


def all_cases(lib):
    rng = np.random.default_rng(SEED)
    cases = []
    shapes = [(60, 1, b"ACGT", False), (200, 3, b"ACGT", False), (333, 7, b"AC", False), (1000, 12, b"ACGT", True), (3000, 20, b"ACGT", False)]
    for rate in (0.0, 0.01, 0.05, 0.15):
        for n, reads, letters, hp in shapes:
            if n == 3000 and rate not in (0.05, 0.15):
                continue
            T = CU.random_template(rng, n, letters, hp)
            cases.append((f"real_e{int(rate * 100):02d}_t{n}_r{reads}", 1, [real_piece(lib, rng, T, reads, rate, offsets=True)]))
    T = CU.random_template(rng, 500)
    cases.append(("backbone", 1, [(T, [ref_align(lib, T, T, 0, 50)])]))
    cases += hand_cases(rng)
    sizes = np.concatenate([[60, 2000], rng.integers(60, 2001, 62)])
    cases.append(("batch64", 1, [real_piece(lib, rng, CU.random_template(rng, int(n)), int(rng.integers(1, 5)), 0.08, offsets=True) for n in sizes]))
    cases.append(("big8192", 1, [real_piece(lib, rng, CU.random_template(rng, 8400), 12, 0.10, offsets=True)]))
    # a generator of its own: the cases above keep their inputs whatever is added here
    cases += edge_cases(np.random.default_rng(SEED + 1), next(pieces for name, _, pieces in cases if name == "hand_min_cov0"))
    return cases


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = compile_reference(tmp)
        cases = all_cases(lib)
        cns, tags, seconds = [], [], {}
        for name, mc, pieces in cases:
            seconds[name] = 0.0
            for pi, (template, unit, *rep) in enumerate(pieces):
                alns = unit * (rep[0] if rep else 1)                               # (template, alignments, repeat): stored once
                mine = CU.consensus(len(template), alns, mc, f"{name}[{pi}]")      # raises Refused: no such case is stored
                mine_tags = [CU.align_tags(*a) for a in alns]
                seq, ref_tags, dt = ref_piece(lib, len(template), alns, mc)
                assert seq == mine, (name, pi, seq[:80], mine[:80])
                assert all(np.array_equal(a, b) for a, b in zip(ref_tags, mine_tags)), (name, pi)
                assert all(np.array_equal(a, b) for a, b in zip(ref_tags, ref_tags[:len(unit)] * (len(alns) // len(unit)))), (name, pi)
                cns.append(seq); tags += ref_tags[:len(unit)]; seconds[name] = round(seconds[name] + dt, 6)
            print(f"{name}: {len(pieces)} piece(s), {sum(len(p[1]) for p in pieces)} alignments, {seconds[name]:.4f} s", flush=True)
        bench_rng = np.random.default_rng(BENCH["seed"])
        bench_s, bench_tags = [], []
        for _ in range(BENCH["pieces"]):
            t_len, alns = CU.synthetic_piece(bench_rng, BENCH["t_len"], BENCH["reads"])
            seq, rt, dt = ref_piece(lib, t_len, alns, 1)
            bench_s.append(round(dt, 4)); bench_tags.append(int(sum(len(t) for t in rt)))
            print(f"bench piece: {dt:.3f} s, {bench_tags[-1]} tags, consensus of {len(seq)}", flush=True)
    arrays = CU.pack_cases(cases)
    arrays.update(CU.pack_tags(tags))
    arrays["cns"] = np.frombuffer(b"".join(cns), np.uint8)
    arrays["cns_off"] = np.concatenate([[0], np.cumsum([len(c) for c in cns])]).astype(np.int64)
    np.savez_compressed(CU.GOLDEN, **arrays)
    prov = dict(generator="tests/golden/make_golden_cns.py", seed=SEED,
                sources={s: hashlib.sha256(open(os.path.join(FALCON, s), "rb").read()).hexdigest() for s in SOURCES + ("falcon.h", "common.h")},
                compiler=subprocess.check_output(["gcc", "--version"], text=True).splitlines()[0], cflags=CFLAGS,
                glibc=" ".join(platform.libc_ver()), cases=len(cases), pieces=len(cns), alignments=len(tags),
                tags=int(arrays["tag_off"][-1]), reference_seconds_one_thread=seconds,
                bench=dict(BENCH, generator="cns_util.synthetic_piece", reference_seconds_per_piece=bench_s, tags_per_piece=bench_tags,
                           machine="the machine that wrote the fixture (one CPU thread)"))
    with open(CU.PROVENANCE, "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(f"wrote {CU.GOLDEN}: {os.path.getsize(CU.GOLDEN)} bytes, {len(cases)} cases, {len(cns)} pieces, {len(tags)} alignments")


if __name__ == "__main__":
    main()
