"""Generator of tests/golden/aln_cases.npz: seeded pairs of sequences and pieces of reads, and what the REAL reference makes of them.

The reference's falcon/falcon.c, DW_banded.c and kalloc.c are compiled exactly as make_golden_cns.py compiles them (its compile_reference)
into a temporary directory; align, get_align_tags and get_cns_from_align_tags are called through ctypes.  Every case first runs through the
restatement of tests/aln_util.py, which must agree with the reference field by field and string by string; the pieces also run
pg_asm_cns.py:143-244 both ways (the reference's aligner, tags and consensus against aln_util.consensus_reads).  Stored: every sequence
once, per alignment the six fields, the exit that ended the front and the strings as run-length operations, per piece the consensus and
the accepted flags.  Guards: each of the exits (a), (b), (c) and max_d == 0 occurs; no stored piece is one cns_util.consensus refuses; a
case that would make the reference read outside its arrays is not built (band <= 4096 and 0.3 * (q_len + t_len) * (2 * band + 1) path
records stay far below what calloc gives it, and the restatement never reads a diagonal outside the previous row).

  self_*, empty_*, q1_t3, case_*, allN   the smallest shapes, the byte compare
  e??_t3000, nostr, two_letter, homopolymer   reads of a template mutated with cns_util.mutate, band 150
  unrelated_*                            random pairs picked by seed for each exit
  band_*                                 one read at bands 0, 1, 50, 150, 400, 4096
  stitch_*                               pg_asm_cns.py:255: 1,000 against 1,050 of a 2 % continuation, band 400, with and without strings
  inside, off_end, long_15k, backbone_60k   target tail unused; y >= t_len ends it; the shapes of a real piece
  dist_*, snake_*, nk_*, ring_*          the kernels' windows: steps per emission chunk, the snake probe / copy / extension granules, the
                                         diagonals per round, the LDS ring at bands whose 2 * band + 4 meets a power of two
  pieces_*                               templates of 300 .. 3,000 with reads of negative, zero and positive shift, accepted by either test
                                         alone, rejected, clipped to nothing; aln_base one below and at 3 * t_len; back-bone only; 32 pieces

    python tests/golden/make_golden_aln.py [path/to/reference/falcon]
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
sys.path[:0] = [os.path.join(ROOT, "tests"), HERE]
import aln_util as AU  # noqa: E402
import cns_util as CU  # noqa: E402
import make_golden_cns as MG  # noqa: E402  (compile_reference, ref_piece: the same build of the same sources)

SEED = 20261021
BENCH = dict(seed=11, pieces=2, t_len=50_000, cov=30, read_len=15_000, rate=0.01)   # the first pieces of tools/cns_align_bench.py's batch


def ref_align(lib, q, t, band, want_str=True):
    """the reference's answer and the seconds it took"""
    t0 = time.perf_counter()
    a = lib.align(q, len(q), t, len(t), band, 1 if want_str else 0)
    dt = time.perf_counter() - t0
    try:
        c = a.contents
        n = c.aln_str_size if want_str else 0
        return (c.aln_str_size, c.dist, c.aln_q_s, c.aln_q_e, c.aln_t_s, c.aln_t_e, C.string_at(c.q_aln_str, n), C.string_at(c.t_aln_str, n)), dt
    finally:
        lib.free_alignment(a)


def alignment_cases(rng):
    """[(name, q, t, band, want_str)]"""
    mut = lambda s, rate: CU.mutate(rng, s, rate)
    rt = lambda n, letters=b"ACGT", hp=False: CU.random_template(rng, n, letters, hp)
    cases = []
    add = lambda name, q, t, band=150, want=True: cases.append((name, bytes(q), bytes(t), band, want))
    for n in (1, 2, 3, 4, 10):
        T = rt(n)
        add(f"self_{n}", T, T)
    add("empty_q", b"", rt(5)); add("empty_t", rt(5), b""); add("empty_both", b"", b"")
    add("q1_t3", b"A", b"ACG")
    T = rt(200)
    add("case_lower_upper", T.lower(), T); add("case_lower_lower", T.lower(), T.lower())
    TN = bytearray(rt(300)); TN[50:60] = b"N" * 10; TN[200] = ord("N")
    add("allN_runs", TN, TN)
    T3 = rt(3000)
    reads = {}
    for pct in (0, 1, 5, 15, 30):
        reads[pct] = mut(T3, pct / 100)
        add(f"e{pct:02d}_t3000", reads[pct], T3)
    add("nostr_e05_t3000", reads[5], T3, 150, False)
    T2 = rt(1200, b"AC")
    add("two_letter_e10", mut(T2, 0.10), T2)
    TH = rt(1500, b"ACGT", True)
    add("homopolymer_e08", mut(TH, 0.08), TH)
    for band in (0, 1, 50, 150, 400, 4096):
        add(f"band_{band}", reads[5], T3, band)
    add("band_0_first_snake", T3[:500], T3, 0)
    S = rt(3000)
    s0, s1 = S[:2000], mut(S[1000:], 0.02)
    add("stitch_str", s0[-1000:], s1[:1050], 400, True); add("stitch_nostr", s0[-1000:], s1[:1050], 400, False)
    add("inside", mut(T3[:800], 0.03), T3)
    add("off_end", mut(T3[2500:], 0.03) + rt(300), T3[2500:])
    T60 = rt(60_000)
    add("backbone_60k", T60, T60, 50)
    add("long_15k", mut(T60[15_000:30_000], 0.01), T60[15_000:])
    # the windows
    TW = rt(66 * 24 + 60)
    for n in (63, 64, 65):
        add(f"dist_{n}", AU.with_insertions(rng, TW, n, 24), TW)
    for L in list(range(6, 11)) + [15, 16, 17] + list(range(62, 67)) + list(range(510, 523)):
        n = 70 if L < 20 else 6 if L < 100 else 3
        TS = rt(L * (n + 1) + 7)
        add(f"snake_{L}", AU.with_insertions(rng, TS, n, L), TS)
    TR = rt(1500)
    noisy = mut(TR, 0.15)
    for band in (29, 30, 31, 61, 62, 63, 125, 126, 127):
        add(f"ring_band_{band}", noisy, TR, band)
    return cases, (TR, noisy)


def pick_by_restatement(rng, cases, noisy_pair):
    """cases whose shape only the rule itself can aim: an exit per unrelated pair, a widest row of exactly 63, 64, 65 diagonals"""
    add = lambda name, q, t, band, want=True: cases.append((name, bytes(q), bytes(t), band, want))
    want = {("unrelated_400_band50", AU.EXIT_BAND): 2, ("unrelated_short_band400", AU.EXIT_STEPS): 2, ("unrelated_short_band400", AU.EXIT_END): 2}
    for seed in range(200):
        r = np.random.default_rng(SEED + 100 + seed)
        for (name, ex), left in list(want.items()):
            n = 400 if "400_" in name else int(r.integers(20, 101))
            q, t = CU.random_template(r, n), CU.random_template(r, n)
            if left and AU.align(q, t, 50 if "400_" in name else 400)[1] == ex:
                add(f"{name}_exit_{ex}_{left}", q, t, 50 if "400_" in name else 400)
                want[(name, ex)] = left - 1
    assert not any(want.values()), want
    # unrelated pairs at a band that prunes nothing: row d holds d + 1 diagonals, so an end reached at d = 62, 63, 64 is a widest row of 63, 64, 65
    found = {}
    for seed in range(4000):
        r = np.random.default_rng(SEED + 1000 + seed)
        n = int(r.integers(104, 126))
        q, t = CU.random_template(r, n), CU.random_template(r, n)
        info = {}
        if AU.align(q, t, 400, True, info)[1] == AU.EXIT_END and info["max_nk"] in (63, 64, 65) and info["max_nk"] not in found:
            found[info["max_nk"]] = (q, t)
        if len(found) == 3:
            break
    assert sorted(found) == [63, 64, 65], sorted(found)
    for nk, (q, t) in sorted(found.items()):
        add(f"nk_{nk}", q, t, 400)
        for band in (nk - 3, nk - 2, nk - 1):     # ... and at bands whose ring (2 * band + 4 slots, a power of two for band 62) these rows fill
            add(f"nk_{nk}_band_{band}", q, t, band)


def piece_cases(rng):
    """[(name, min_cov, [(template, [(read, shift), ...]), ...])]"""
    mut = lambda s, rate: CU.mutate(rng, s, rate)
    rt = lambda n: CU.random_template(rng, n)
    cases = []
    T = rt(1500)
    full = lambda rate=0.05: (mut(T, rate), 0)
    shapes = [full(), full(), full(), full(),
              (rt(200) + mut(T[:900], 0.05), -200),           # negative shift: the read begins before the piece
              (rt(5) + mut(T[:1200], 0.04), -5),
              (mut(T[300:], 0.05), 300), (mut(T[297:1400], 0.05), 300),      # positive shift, a few bases off
              (mut(T[400:1000], 0.04), 400),                  # ends inside the template: the first test alone accepts it
              (mut(T[1000:], 0.04) + rt(400), 1000),          # runs off the template's end: the second test alone accepts it
              (rt(700), 100), (rt(600), -50),                 # unrelated: rejected by both
              (rt(40), -40), (rt(40), -70), (rt(100), 1500), (rt(100), 1600), (b"", 0)]          # clipped to nothing
    cases.append(("pieces_shifts", 1, [(T, shapes)]))
    cases.append(("pieces_shifts_min_cov2", 2, [(T, shapes)]))
    T6 = rt(600)
    cases.append(("pieces_cov_edge", 1, [(T6, [(T6, 0), (T6, 0), (T6[:599], 0)]),            # aln_base = 1,799: one below 3 * t_len
                                         (T6, [(T6, 0), (T6, 0), (T6, 0)]),                  # 1,800: not below, the call answers
                                         (T6, []),                                           # the back-bone only
                                         (T6, [(rt(300), 0)])]))                             # ... and with a rejected read
    batch = []
    for n in np.concatenate([[300, 3000], rng.integers(300, 3001, 30)]).tolist():
        Tb = rt(int(n))
        reads = []
        for _ in range(int(rng.integers(3, 8))):
            a = int(rng.integers(0, n // 2)) if rng.random() < 0.5 else 0
            shift = a + int(rng.integers(-3, 4)) if a else int(rng.integers(-30, 1))
            reads.append((rt(-shift) + mut(Tb, 0.08), shift) if shift < 0 else (mut(Tb[a:], 0.08), max(shift, 0)))
        batch.append((Tb, reads))
    cases.append(("pieces_batch32", 1, batch))
    return cases


def ref_consensus_reads(lib, template, reads, min_cov):
    """pg_asm_cns.py:143-244 on the reference's functions: (consensus, accepted flags, answered by the low-coverage rule, seconds)"""
    t0 = time.perf_counter()
    alns, aln_base, used = AU.piece_alignments(template, reads, lambda q, t, band: ref_align(lib, q, t, band)[0])
    if aln_base / len(template) < 3:
        return bytes(template).lower(), used, True, time.perf_counter() - t0
    CU.consensus(len(template), alns, min_cov)          # raises Refused: no such piece is stored
    seq, _, _ = MG.ref_piece(lib, len(template), alns, min_cov)
    return seq, used, False, time.perf_counter() - t0


def bench_seconds(lib):
    rng = np.random.default_rng(BENCH["seed"])
    out = dict(BENCH, generator="aln_util.bench_piece", machine="the machine that wrote the fixture (one CPU thread)", with_strings=[], without_strings=[],
               alignments_per_piece=[], mean_dist=[])
    for _ in range(BENCH["pieces"]):
        T, reads = AU.bench_piece(rng, BENCH["t_len"], BENCH["cov"], BENCH["read_len"], BENCH["rate"])
        pairs = [(T, T, 50)] + [((r[-s:], T, 150) if s < 0 else (r, T[s:], 150)) for r, s in reads]
        for key, want in (("with_strings", True), ("without_strings", False)):
            res = [ref_align(lib, q, t, band, want) for q, t, band in pairs]
            out[key].append(round(sum(dt for _, dt in res), 4))
        out["alignments_per_piece"].append(len(pairs))
        out["mean_dist"].append(round(float(np.mean([a[1] for a, _ in res[1:]])), 1))
        print(f"bench piece: {len(pairs)} alignments, {out['with_strings'][-1]} s with strings, {out['without_strings'][-1]} s without", flush=True)
    return out


def main():
    rng = np.random.default_rng(SEED)
    with tempfile.TemporaryDirectory() as tmp:
        lib = MG.compile_reference(tmp)
        cases, noisy_pair = alignment_cases(rng)
        pick_by_restatement(rng, cases, noisy_pair)
        pool = AU.Pool()
        fields, exits, ops, ops_off, seconds = [], [], [], [0], {}
        aq, at = [], []
        for name, q, t, band, want in cases:
            assert band <= 4096 and len(q) + len(t) < 2**31
            info = {}
            mine, ex = AU.align(q, t, band, want, info)
            ref, dt = ref_align(lib, q, t, band, want)
            assert ref == mine, (name, ref[:6], mine[:6])
            seconds[name] = round(dt, 6)
            fields.append(ref[:6]); exits.append(ex)
            o = CU.ops_of(ref[6], ref[7]) if want else np.zeros(0, np.uint32)
            assert not want or AU.expand_strings(q, t, o) == (ref[6], ref[7]), name
            ops.append(o); ops_off.append(ops_off[-1] + len(o))
            # a sequence that is a part of a longer stored one is stored as that part
            for seq, dst in ((q, aq), (t, at)):
                host = next((h for h in pool.seqs if len(h) > len(seq) and len(seq) >= 500 and seq in h), None)
                dst.append((pool.index[host], host.index(seq), len(seq)) if host is not None else (pool.add(seq), 0, len(seq)))
            print(f"{name}: exit {ex}, size {ref[0]}, dist {ref[1]}, q_e {ref[3]}, t_e {ref[5]}, widest row {info['max_nk']}, cells {info['cells']}, {dt:.5f} s",
                  flush=True)
        kinds = {e: sum(1 for x in exits if x == e) for e in (AU.EXIT_END, AU.EXIT_BAND, AU.EXIT_STEPS)}
        assert all(kinds.values()), kinds
        assert any(int(0.3 * (len(q) + len(t))) == 0 and len(q) and len(t) for _, q, t, _, _ in cases), "no case with max_d == 0"
        pcs = piece_cases(rng)
        cns, used, by_rule, tmpl, read_seq, read_shift, piece_read_off, pc_piece_off = [], [], [], [], [], [], [0], [0]
        for name, mc, pieces in pcs:
            seconds[name] = 0.0
            for pi, (T, reads) in enumerate(pieces):
                mine = AU.consensus_reads(T, reads, mc)
                seq, u, rule, dt = ref_consensus_reads(lib, T, reads, mc)
                assert (seq, u, rule) == mine, (name, pi)
                cns.append(seq); used += u; by_rule.append(rule); tmpl.append(pool.add(T))
                for r, s in reads:
                    read_seq.append(pool.add(r)); read_shift.append(s)
                piece_read_off.append(len(read_seq))
                seconds[name] = round(seconds[name] + dt, 6)
            pc_piece_off.append(len(tmpl))
            p0 = pc_piece_off[-2]
            print(f"{name}: {len(pieces)} piece(s), {piece_read_off[-1] - piece_read_off[p0]} reads, {sum(used[piece_read_off[p0]:])} accepted, "
                  f"{sum(by_rule[p0:])} by the low-coverage rule, {seconds[name]:.4f} s", flush=True)
        u0 = pcs[0][2][0][1]
        flags0 = used[:len(u0)]
        assert True in flags0 and False in flags0 and any(by_rule) and not all(by_rule)
        bench = bench_seconds(lib)
    arrays = pool.arrays()
    arrays.update(aln_names=np.array([c[0] for c in cases]), aln_q=np.array(aq, np.int64), aln_t=np.array(at, np.int64),
                  aln_band=np.array([c[3] for c in cases], np.int32), aln_want=np.array([c[4] for c in cases], np.uint8),
                  aln_fields=np.array(fields, np.int32), aln_exit=np.array(exits), aln_ops=np.concatenate(ops).astype(np.uint32),
                  aln_ops_off=np.array(ops_off, np.int64),
                  pc_names=np.array([c[0] for c in pcs]), pc_min_cov=np.array([c[1] for c in pcs], np.int32), pc_piece_off=np.array(pc_piece_off, np.int64),
                  piece_tmpl=np.array(tmpl, np.int64), piece_read_off=np.array(piece_read_off, np.int64), piece_by_rule=np.array(by_rule, np.uint8),
                  read_seq=np.array(read_seq, np.int64), read_shift=np.array(read_shift, np.int32), read_used=np.array(used, np.uint8),
                  cns=np.frombuffer(b"".join(cns), np.uint8), cns_off=np.concatenate([[0], np.cumsum([len(c) for c in cns])]).astype(np.int64))
    np.savez_compressed(AU.GOLDEN, **arrays)
    falcon = MG.FALCON
    prov = dict(generator="tests/golden/make_golden_aln.py", seed=SEED,
                sources={s: hashlib.sha256(open(os.path.join(falcon, s), "rb").read()).hexdigest() for s in MG.SOURCES + ("falcon.h", "common.h")},
                compiler=subprocess.check_output(["gcc", "--version"], text=True).splitlines()[0], cflags=MG.CFLAGS, glibc=" ".join(platform.libc_ver()),
                alignments=len(cases), exits=kinds, piece_cases=len(pcs), pieces=len(tmpl), reads=len(read_seq),
                reference_seconds_one_thread=seconds, bench=bench)
    with open(AU.PROVENANCE, "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(f"wrote {AU.GOLDEN}: {os.path.getsize(AU.GOLDEN)} bytes, {len(cases)} alignments ({kinds}), {len(tmpl)} pieces")


if __name__ == "__main__":
    main()
