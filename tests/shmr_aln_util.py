"""The rule of shmr_aln (src/shmr_align.c:21-160, direction 0) in plain Python / numpy, the fixture tests/golden/shmr_aln_cases.npz and
the helpers the tests of pgx_shmr_aln_batch share.  TEST INFRASTRUCTURE: imported only from tests/ and tools/shmr_aln_bench.py.

The rule, for a pair (mmers0, mmers1):
  index     mmers0 by x >> 8 (the span byte is ignored); a hash's occurrences in ascending place of the list.
  walk      mmers1 in order s = 0 .. n1 - 1.  A hash mmers0 lacks, or holds more than max_repeat times, is skipped.
  candidate each occurrence i0, in order, whose strand bit y & 1 equals the shimmer's own; delta0 = |pos0 - pos1|, pos = (y & 0xFFFFFFFF) >> 1.
  scan      every chain opened so far, in creation order; a chain qualifies if i0 >= its last idx0, |pos0 - its last pos0| < max_dist and
            diff = |delta0 - its last delta| < max_diff.  The qualifying chain with the smallest diff takes (i0, s), the first among
            equals; with none, (i0, s) opens a chain.
  stop      small = the chains of fewer than 3 elements the LAST scan saw (counted before its append); the walk ends after a shimmer
            (one that was not skipped) with small > 4,800.
"""
import os

import numpy as np

from peregrine_amd.formats import MM_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shmr_aln_cases.npz")
PROVENANCE = os.path.join(ROOT, "tests", "golden", "shmr_aln_cases.provenance.json")
MAX_SMALL_ALNS = 4800
REAL = dict(seed=20261021, t_len=20_000, shift=137, rate=0.01, w=80, k=16, r=3)   # the pairs of real shimmers (make_golden_shmr_aln.py)


def mm_list(hashes, pos, strand=0, span=16, rid=0) -> np.ndarray:
    """a shimmer list from hashes (x >> 8), positions ((y & 0xFFFFFFFF) >> 1) and strand bits"""
    h = np.asarray(hashes, np.uint64)
    out = np.zeros(len(h), MM_DTYPE)
    out["x"] = (h << np.uint64(8)) | (np.zeros(len(h), np.uint64) + np.asarray(span, np.uint64))
    out["y"] = (np.uint64(rid) << np.uint64(32)) | (np.asarray(pos, np.uint64) << np.uint64(1)) | (np.zeros(len(h), np.uint64) + np.asarray(strand, np.uint64))
    return out


def positions(mm) -> np.ndarray:
    return ((mm["y"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.int64)


def shmr_aln(mm0, mm1, max_diff=100, max_dist=1200, max_repeat=1):
    """the chains, [(idx0 list, idx1 list)] in creation order, and how the walk ended: (shimmers of list 1 it took, stopped by the count)"""
    mm0, mm1 = np.ascontiguousarray(mm0, MM_DTYPE), np.ascontiguousarray(mm1, MM_DTYPE)
    index = {}
    for i, h in enumerate((mm0["x"] >> np.uint64(8)).tolist()):
        index.setdefault(h, []).append(i)
    pos0, pos1 = positions(mm0).tolist(), positions(mm1).tolist()
    str0, str1 = (mm0["y"] & np.uint64(1)).tolist(), (mm1["y"] & np.uint64(1)).tolist()
    cap = 16
    li0, lp0, ld, ln = (np.zeros(cap, np.int64) for _ in range(4))
    chains = []
    small = 0
    s = -1
    for s, h in enumerate((mm1["x"] >> np.uint64(8)).tolist()):
        occ = index.get(h)
        if occ is None or len(occ) > max_repeat:
            continue
        for i0 in occ:
            if str0[i0] != str1[s]:
                continue
            delta0 = abs(pos0[i0] - pos1[s])
            n = len(chains)
            small = int(np.count_nonzero(ln[:n] < 3))
            diff = np.abs(delta0 - ld[:n])
            ok = (i0 >= li0[:n]) & (np.abs(pos0[i0] - lp0[:n]) < max_dist) & (diff < max_diff)
            if ok.any():
                c = int(np.argmin(np.where(ok, diff, np.iinfo(np.int64).max)))   # (argmin: the first among equals)
                chains[c][0].append(i0), chains[c][1].append(s)
            else:
                c = n
                chains.append(([i0], [s]))
                if c == cap:
                    cap *= 2
                    li0, lp0, ld, ln = (np.concatenate([a, np.zeros(len(a), np.int64)]) for a in (li0, lp0, ld, ln))
            li0[c], lp0[c], ld[c] = i0, pos0[i0], delta0
            ln[c] += 1
        if small > MAX_SMALL_ALNS:
            return chains, (s + 1, True)
    return chains, (s + 1, False)


def csr_of(chains):
    """(chain_off, idx0, idx1) of one pair's chains"""
    off = np.concatenate([[0], np.cumsum([len(c[0]) for c in chains])]).astype(np.uint64)
    cat = lambda k: np.concatenate([np.asarray(c[k], np.uint32) for c in chains]) if chains else np.zeros(0, np.uint32)
    return off, cat(0), cat(1)


def chains_of(chain_off, idx0, idx1):
    """[(idx0 list, idx1 list)] from CSR"""
    o = np.asarray(chain_off).astype(np.int64).tolist()
    return [(np.asarray(idx0[a:b]).tolist(), np.asarray(idx1[a:b]).tolist()) for a, b in zip(o[:-1], o[1:])]


class Case:
    def __init__(self, name, mm0, mm1, max_diff, max_dist, max_repeat, chains):
        self.name, self.mm0, self.mm1, self.chains = name, mm0, mm1, chains
        self.params = dict(max_diff=int(max_diff), max_dist=int(max_dist), max_repeat=int(max_repeat))


_cases = None


def load_cases():
    """the fixture's cases, read once"""
    global _cases
    if _cases is None:
        z = np.load(GOLDEN)
        mm = np.zeros(len(z["mm"]), MM_DTYPE)
        mm["x"], mm["y"] = z["mm"][:, 0], z["mm"][:, 1]
        lo, co, eo = z["list_off"].tolist(), z["case_chain_off"].tolist(), z["chain_off"]
        out = []
        for k, name in enumerate(z["names"].tolist()):
            l0, l1 = z["case_lists"][k].tolist()
            a, b = co[k], co[k + 1]
            off = eo[a:b + 1]
            chains = [(z["idx0"][int(x):int(y)].tolist(), z["idx1"][int(x):int(y)].tolist()) for x, y in zip(off[:-1], off[1:])]
            md, mx, mr = z["case_params"][k].tolist()
            out.append(Case(name, mm[lo[l0]:lo[l0 + 1]], mm[lo[l1]:lo[l1 + 1]], md, mx, mr, chains))
        _cases = out
    return _cases


def random_pairs(seed, n_pairs=300, max_len=400):
    """seeded lists with small hash alphabets (repeats and ties are common) and pairs of them, several sharing a list 0:
    (lists0, lists1, pairs as an (n, 2) array)"""
    rng = np.random.default_rng(seed)

    def one(n):
        alpha = int(rng.choice([8, 40, 150, 400]))
        step = int(rng.choice([5, 60, 700]))
        pos = np.cumsum(rng.integers(0, 2 * step + 1, n)) + int(rng.integers(0, 3000))
        if rng.random() < 0.3:
            pos = rng.permutation(pos)
        strand = rng.integers(0, 2, n) if rng.random() < 0.5 else np.zeros(n, np.int64)
        return mm_list(rng.integers(0, alpha, n), pos, strand, span=rng.integers(10, 60, n))

    special = [0, 0, 1, 1, 2, max_len, max_len]
    sizes = lambda n: rng.permutation(np.concatenate([special, rng.integers(0, max_len + 1, n - len(special))])).tolist()
    lists0 = [one(n) for n in sizes(n_pairs // 3)]
    lists1 = [one(n) for n in sizes(n_pairs)]
    pairs = np.stack([rng.integers(0, len(lists0), n_pairs), rng.permutation(n_pairs)], axis=1).astype(np.uint32)
    return lists0, lists1, pairs


_batch = None


def seeded_batch():
    """about 300 seeded pairs, sizes 0 .. 400, several pairs to a list 0, and the restatement's chains of each pair alone per max_repeat:
    (lists0, lists1, pairs, {max_repeat: [chains of pair p]}), made once and left alone"""
    global _batch
    if _batch is None:
        lists0, lists1, pairs = random_pairs(20261121)
        want = {mr: [shmr_aln(lists0[a], lists1[b], max_repeat=mr)[0] for a, b in pairs.tolist()] for mr in (1, 2, 5)}
        shared = np.bincount(pairs[:, 0])
        assert len(pairs) == 300 and shared.max() >= 3 and min(len(l) for l in lists1) == 0 and max(len(l) for l in lists1) == 400
        for mr in (1, 2, 5):   # repeats and ties are common: chains longer than one element, several chains to a pair, in many pairs
            assert sum(len(ch) > 1 for ch in want[mr]) > 50 and sum(any(len(a) > 1 for a, _ in ch) for ch in want[mr]) > 50, mr
        _batch = (lists0, lists1, pairs, want)
    return _batch


RC = bytes.maketrans(b"ACGT", b"TGCA")


def real_sequences():
    """the template, its copy with substitutions behind REAL['shift'] unrelated bases, and the copy's reverse complement"""
    rng = np.random.default_rng(REAL["seed"])
    acgt = np.frombuffer(b"ACGT", np.uint8)
    t = rng.integers(0, 4, REAL["t_len"])
    c = t.copy()
    hit = rng.random(len(c)) < REAL["rate"]
    c[hit] = (c[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    copy = np.concatenate([rng.integers(0, 4, REAL["shift"]), c])
    T, Cp = acgt[t].tobytes(), acgt[copy].tobytes()
    return T, Cp, Cp.translate(RC)[::-1]


def script_numbers(chain_pairs):
    """utils.py:57-71 on one chain's (mmer2tuple, mmer2tuple) pairs at direction 0: np.max(d), np.mean(d), np.min(d) of the LAST pair's d"""
    d = None
    for m0, m1 in chain_pairs:
        d = m0[3] - m1[3]
    return np.max(d), np.mean(d), np.min(d)


def mmer2tuple(x, y):
    """utils.py:17-25"""
    x, y = int(x), int(y)
    return (x >> 8, x & 0xFF, y >> 32, ((y & 0xFFFFFFFF) >> 1) + 1, y & 1)
