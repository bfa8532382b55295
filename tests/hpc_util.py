"""What the homopolymer-compressed (hpc) shimmer tests share: the directed and random strings, the fixture they are recorded in
(tests/golden/hpc_cases.npz, written by tests/golden/make_golden_hpc.py from the compiled reference), the seqdb encoding of ASCII
strings, and the reference calls with is_hpc = 1 where oracle/_ref is present."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import oracle_util as U
from peregrine_amd.formats import MM_DTYPE, SeqDB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpc_cases.npz")
W, K, R = 80, 16, 6   # the parameters at which the fixture also holds L1 and L2


# ---- strings ---------------------------------------------------------------------------------------------------------------------
def runs_string(rng, nruns, lens=(1, 4), first=None) -> bytes:
    """nruns runs: neighbouring codes differ, run lengths uniform in [lens[0], lens[1])"""
    out, prev = bytearray(), first
    for _ in range(nruns):
        c = int(rng.integers(0, 4))
        while c == prev:
            c = int(rng.integers(0, 4))
        out += bytes([b"ACGT"[c]]) * int(rng.integers(lens[0], lens[1]))
        prev = c
    return bytes(out)


def flat(rng, nruns) -> bytes:
    """nruns runs of one base each: every k-run span is k"""
    return runs_string(rng, nruns, (1, 2))


def with_run(rng, before, length, after) -> bytes:
    """a run of `length` bases between `before` and `after` runs of one base, its neighbours of other codes"""
    a, b = flat(rng, before), flat(rng, after)
    c = next(x for x in b"ACGT" if (not a or x != a[-1]) and (not b or x != b[0]))
    return a + bytes([c]) * length + b


def tandem(rng, period, copies, lens=(1, 4)) -> bytes:
    """copies of one unit of `period` runs whose run lengths differ from copy to copy: equal hashes with different spans"""
    unit = runs_string(rng, period, (1, 2))   # (a unit whose ends are equal merges them across copies: one run fewer per copy)
    return b"".join(bytes([ch]) * int(rng.integers(lens[0], lens[1])) for _ in range(copies) for ch in unit)


def directed_cases():
    """[(name, seq, w, k)]: the smallest shapes at which the hpc sketch can go wrong"""
    rng = np.random.default_rng(2024)
    cs = [("one_base", b"A", W, K), ("one_run_500", b"C" * 500, W, K), ("AAANAAA", b"AAANAAA", W, K), ("NN", b"NN", W, K),
          ("AAANAAA_small", b"AAANAAA", 3, 4), ("NN_small", b"NN", 3, 4)]
    for w, k in ((W, K), (5, 6), (3, 4)):   # the machine's l gates
        for nr in (k - 1, k, k + w - 2, k + w - 1, k + w, k + 2 * w + 3):
            cs.append((f"runs_{nr}_w{w}k{k}", runs_string(rng, nr), w, k))
    # k - 1 runs of one base + a run of 256 - k: a k-run span of exactly 255; one base more in that run: exactly 256
    for suffix, around, w, k in (("", 300, W, K), ("_k6", 60, 5, 6)):
        s = with_run(rng, around, 256 - k, around)
        cs.append(("span255" + suffix, s, w, k))
        cs.append(("span256" + suffix, s[:around] + s[around:around + 1] + s[around:], w, k))
    for length in (241, 300):
        cs.append((f"run{length}_middle", with_run(rng, 400, length, 400), W, K))
        cs.append((f"run{length}_start", with_run(rng, 0, length, 500), W, K))
        cs.append((f"run{length}_end", with_run(rng, 500, length, 0), W, K))
    cs.append(("ends_inside_a_run", runs_string(rng, 300) + b"TTTTT", W, K))
    body = runs_string(rng, 400)
    cs += [("N_first", b"N" + body, W, K), ("N_last", body + b"N", W, K),
           ("N_within_k_runs_of_N", body[:300] + b"N" + runs_string(rng, K - 6) + b"N" + body[300:], W, K),
           ("N_within_k_runs_small", runs_string(rng, 40) + b"N" + runs_string(rng, 2) + b"N" + runs_string(rng, 40), 3, 4),
           ("N_many", b"NNN".join(runs_string(rng, int(n)) for n in (3, 120, 15, 16, 17, 200, 1)), W, K),
           ("N_between_long_runs", b"A" * 250 + b"N" + b"A" * 250 + runs_string(rng, 200, first=0), W, K)]
    for period in range(2, 9):
        cs.append((f"tandem{period}", tandem(rng, period, 400 // period), W, K))
        cs.append((f"tandem{period}_small", tandem(rng, period, 40), int(rng.choice([3, 5])), int(rng.choice([4, 6]))))
    cs.append(("mixed_case", bytes(ch | 0x20 if rng.random() < 0.5 else ch for ch in runs_string(rng, 500)), W, K))
    for w, k in ((3, 4), (5, 4), (3, 6), (5, 6)):   # strand-ambiguous k-mers are frequent
        cs.append((f"dense_w{w}k{k}", runs_string(rng, 300), w, k))
        cs.append((f"two_letter_w{w}k{k}", bytes(b"AT"[i & 1] for i in range(200) for _ in range(int(rng.integers(1, 3)))), w, k))
    # a run across a 16-byte lane boundary (bytes 14..18) and one across a 1 KiB tile boundary (bytes 1020..1029) of a read at offset 0
    s = bytearray(flat(rng, 1400))
    for lo, hi in ((14, 19), (1020, 1030)):
        c = next(x for x in b"ACGT" if x != s[lo - 1] and x != s[hi])
        s[lo:hi] = bytes([c]) * (hi - lo)
    cs.append(("straddles_lane_and_tile", bytes(s), W, K))
    cs.append(("odd_length_17", runs_string(rng, 9, (1, 3))[:17].ljust(17, b"G"), W, K))   # the read after it starts off a 16-byte boundary
    cs.append(("after_odd_length", runs_string(rng, 500), W, K))
    cs.append(("low_complexity_AC", b"AC" * 1000, W, K))          # ~ every other run a minimizer: outgrows a slab of len / 8 + 64
    cs.append(("low_complexity_AAC", b"AAC" * 700 + b"A", W, K))
    cs.append(("low_complexity_small", b"ACG" * 400, 3, 4))
    # a read that outgrows its slab and ends in w or more ambiguous bases: no end element, so the last segment's pending element, written
    # and then stepped back over, is the highest place the first pass wrote -- one past the count the exact slab is sized by
    cs.append(("low_complexity_then_w_N", b"AC" * 1000 + b"N" * W, W, K))
    cs.append(("low_complexity_then_N_w1", b"ACG" * 400 + b"N", 1, 4))
    cs.append(("low_complexity_N_inside_then_w_N", b"AAC" * 400 + b"N" + b"AC" * 600 + b"N" * (W + 5), W, K))
    cs.append(("dense_w1k6", bytes(b"ACGT"[(i * 7 + i // 5) & 3] for i in range(700)), 1, 6))
    return cs


def random_case(rng):
    """the generator of tools/hpc_sketch_model.py with the lengths kept short: (seq, w, k)"""
    k, w = int(rng.choice([4, 6, 12, 16])), int(rng.choice([3, 5, 24, 80]))
    n = int(rng.integers(1, 900))
    s = bytearray()
    while len(s) < n:
        u = rng.random()
        if u < 0.02:
            s += bytes([b"ACGT"[rng.integers(0, 4)]]) * int(rng.integers(120, 300))
        elif u < 0.04:
            s += b"N" * int(rng.integers(1, 4))
        elif u < 0.1:
            unit = bytes(b"ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(2, 9))))
            s += unit * int(rng.integers(3, 30))
        else:
            s += bytes([b"ACGTacgt"[rng.integers(0, 8)]]) * int(rng.geometric(0.6))
    return bytes(s[:n]), w, k


def all_cases(n_random=200):
    cs = directed_cases()
    rng = np.random.default_rng(77)
    for i in range(n_random):
        seq, w, k = random_case(rng)
        if i % 4 == 0:
            w, k = W, K   # a good share at the index stage's parameters
        cs.append((f"random{i:03d}", seq, w, k))
    return cs


# ---- encoding ----------------------------------------------------------------------------------------------------------------------
_FWD = np.zeros(256, np.uint8)
_REV = np.zeros(256, np.uint8)
for _ch, _f, _r in ((b"Aa", 1, 8), (b"Cc", 2, 4), (b"Gg", 4, 2), (b"Tt", 8, 1)):
    for _b in _ch:
        _FWD[_b], _REV[_b] = _f, _r


def encode(seq: bytes) -> np.ndarray:
    """the seqdb bytes of an ASCII string (src/shmr_utils.c:18-42: forward strand in the low nibble, reverse complement in the high one)"""
    a = np.frombuffer(seq, np.uint8)
    return (_REV[a[::-1]] << 4 | _FWD[a]).astype(np.uint8)


def seqdb_of(seqs, rids=None) -> SeqDB:
    """the strings as a read database, back to back in the given order (offsets are whatever the lengths make them)"""
    rlen = np.array([len(s) for s in seqs], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    rid = np.arange(len(seqs), dtype=np.uint32) if rids is None else np.asarray(rids, np.uint32)
    return SeqDB(np.concatenate([encode(s) for s in seqs]), rid, rlen, roff, [f"c{i}" for i in range(len(seqs))])


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def ref_sketch_hpc(seq: bytes, w, k, rid) -> np.ndarray:
    v = U.RefV()
    U.ref().mm_sketch(None, C.c_char_p(seq), C.c_int(len(seq)), C.c_int(w), C.c_int(k), C.c_uint32(rid), C.c_int(1), C.byref(v))
    return U._take_ref(v, MM_DTYPE)


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, seq, w, k, l0, l1=None, l2=None):
        self.name, self.seq, self.w, self.k, self.l0, self.l1, self.l2 = name, seq, w, k, l0, l1, l2

    def with_rid(self, arr, rid):
        """the recorded list (rid 0) as read `rid`'s"""
        out = arr.copy()
        out["y"] += np.uint64(rid << 32)
        return out


_cases = None


def golden_cases():
    """the fixture's cases, loaded once: lists recorded with rid 0"""
    global _cases
    if _cases is None:
        z = np.load(GOLDEN)
        seq_off, l0_off, l1_off, l2_off = z["seq_off"], z["l0_off"], z["l1_off"], z["l2_off"]
        names = bytes(z["names"]).decode().split("\n")
        out = []
        for i, name in enumerate(names):
            seq = bytes(z["seq"][seq_off[i]:seq_off[i + 1]])
            w, k = int(z["w"][i]), int(z["k"][i])
            l0 = z["l0"][l0_off[i]:l0_off[i + 1]].view(MM_DTYPE).reshape(-1)
            l1 = l2 = None
            if (w, k) == (W, K):
                l1 = z["l1"][l1_off[i]:l1_off[i + 1]].view(MM_DTYPE).reshape(-1)
                l2 = z["l2"][l2_off[i]:l2_off[i + 1]].view(MM_DTYPE).reshape(-1)
            out.append(Case(name, seq, w, k, l0, l1, l2))
        _cases = out
    return _cases


def expected_l0(case, rid) -> np.ndarray:
    """the reference's list of the case as read `rid`: from the compiled reference where it is present, else the fixture's record"""
    if U.have_ref():
        return ref_sketch_hpc(case.seq, case.w, case.k, rid)
    return case.with_rid(case.l0, rid)
