"""k_align_ph on d-steps whose band holds more than 8 diagonals (pgx_align.hip, END / BAND).

Such a step takes several rounds of 8 diagonals.  The kernel records, round by round, the lowest and the highest diagonal with
U >= best_m - band at that round's best_m; after the last round it re-checks the two against the final threshold and, when both still
pass, has the new band without scanning the step's diagonals again.  When a later round raised best_m past one of them it falls back to
the full scan.  The read pairs below are built so that both outcomes occur many times, in matched and in unmatched alignments, at three
band widths; `count_wide_steps` -- a port of the reference's d-loop that follows the kernel's bookkeeping -- proves that on the CPU, and
every form of the alignment kernels is then compared field by field with the oracle's ovlp_match on these pairs."""
import os

import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import _lib, formats
from peregrine_amd.shimmer import ResidentDB

BANDS = (30, 100, 130)
GL = 8   # diagonals per round of the grouped kernel
_COMP = np.array([3, 2, 1, 0], np.uint8)


# ---- the read pairs ---------------------------------------------------------------------------------------------------------------
def _mutate(rng, s, err):
    """substitutions, deletions and insertions in equal parts, `err` per base"""
    out = []
    for c in s:
        if rng.random() < err:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                out.append((int(c) + int(rng.integers(1, 4))) & 3)
            elif kind == 2:
                out.append(int(c)), out.append(int(rng.integers(0, 4)))
        else:
            out.append(int(c))
    return np.array(out, np.uint8)


def _pair(rng, shape):
    """(query, target) as 2-bit codes, about 1.2 kb each"""
    rnd = lambda n: rng.integers(0, 4, n, dtype=np.uint8)
    if shape == "diverging":    # 600 bases at 2 % error, then unrelated sequence: the band widens until the d-loop gives up
        s = rnd(600)
        return np.concatenate([_mutate(rng, s, 0.02), rnd(600)]), np.concatenate([s, rnd(600)])
    if shape == "noisy":        # the same sequence at 8 % error: matched, wide steps on the way
        s = rnd(1200)
        return _mutate(rng, s, 0.08), s
    if shape == "jumps":        # insertions of 12 to 40 bases every 300: the front spreads until a diagonal beyond the insertion runs far
        s, parts = rnd(1200), []      # ahead of the others, and the threshold of the step's last rounds leaves its first rounds behind
        for i in range(0, 1200, 150):
            parts.append(s[i:i + 150])
            if i % 300 == 0:
                parts.append(rnd(int(rng.integers(12, 40))))
        return _mutate(rng, np.concatenate(parts), 0.02), s
    # "lowcomplexity": a 200-base homopolymer and a period-5 tandem array inside an overlap at 2-3 % error
    s = np.concatenate([rnd(250), np.full(200, rng.integers(0, 4), np.uint8), rnd(250), np.resize(rnd(5), 200), rnd(300)])
    return _mutate(rng, s, 0.02 + 0.01 * rng.random()), s


def _encode(codes):
    """seqdb bytes of a read: low nibble = one-hot base of the forward strand, high nibble = of the reverse complement"""
    return ((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4))).astype(np.uint8)


SHAPES = ["diverging"] * 18 + ["noisy"] * 8 + ["lowcomplexity"] * 6 + ["jumps"] * 16


def _build(seed=20240611, long_read=False, ambiguous=False):
    """reads 2 i / 2 i + 1 = query / target of pair i; the query starts at q_off (never a multiple of 16) of its read, and either read may
    be stored as the reverse complement of what the alignment sees (dir = 1)"""
    rng = np.random.default_rng(seed)
    reads, keys, pairs = [], np.zeros(len(SHAPES), _lib.ALIGN_KEY_DTYPE), []
    for i, shape in enumerate(SHAPES):
        q, t = _pair(rng, shape)
        q_off = int(rng.integers(0, 8)) * 16 + int(rng.integers(1, 16))
        d0, d1 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        qs = np.concatenate([rng.integers(0, 4, q_off, dtype=np.uint8), q])     # the strand the alignment reads
        reads.append(_COMP[qs[::-1]] if d0 else qs)
        reads.append(_COMP[t[::-1]] if d1 else t)
        keys[i] = (2 * i, 2 * i + 1, q_off, d0, d1, 0)
        pairs.append((q, t))
    if long_read:   # one read beyond 65,535 bases switches every launch on this database to the 32-bit V rings
        reads.append(rng.integers(0, 4, 70_000, dtype=np.uint8))
    enc = [_encode(r) for r in reads]
    if ambiguous:   # a base without a 2-bit code in every third target: those pairs go to the byte-wise launch
        for i in range(0, len(SHAPES), 3):
            enc[2 * i + 1][len(enc[2 * i + 1]) // 2] = 0
    rlen = np.array([len(e) for e in enc], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return formats.SeqDB(np.concatenate(enc), np.arange(len(enc), dtype=np.uint32), rlen, roff, None), keys, pairs


# ---- the d-loop of the reference, with the kernel's bookkeeping of a wide step -------------------------------------------------------
def _runs(q, t):
    """run[x, y] = matching codes from (x, y) on (0 at either end)"""
    ql, tl = len(q), len(t)
    run = np.zeros((ql + 1, tl + 1), np.int32)
    eq = q[:, None] == t[None, :]
    for x in range(ql - 1, -1, -1):
        run[x, :tl] = np.where(eq[x], run[x + 1, 1:] + 1, 0)
    return run


def count_wide_steps(run, band):
    """ovlp_match's d-loop on a pair's table of runs.  Returns (matched, d of the last step, wide steps whose recorded extremes give the
    new band, wide steps that need the full scan); a wide step = more than GL diagonals, no end reached in it."""
    ql, tl = run.shape[0] - 1, run.shape[1] - 1
    max_d = int(0.3 * (ql + tl))
    off = max_d + 2
    V = np.zeros(2 * max_d + 5, np.int64)
    best_m, min_k, max_k, settled, fallback = -1, 0, 0, 0, 0
    for d in range(max_d):
        if max_k - min_k > 2 * band:
            break
        ks = np.arange(min_k, max_k + 1, 2)
        if len(ks) == 0:
            min_k, max_k = max_k - 1, min_k + 1
            continue
        va, vb = V[ks - 1 + off], V[ks + 1 + off]
        x = np.where((ks == min_k) | ((ks != max_k) & (va < vb)), vb, va + 1)
        y = x - ks
        ext = run[x, y]
        x, y = x + ext, y + ext
        hit = np.flatnonzero((x >= ql) | (y >= tl))
        if len(hit):
            return True, d, settled, fallback
        V[ks + off] = x
        u = x + y
        if len(ks) <= GL:
            best_m = max(best_m, int(u.max()))
        else:   # round by round, as the kernel: each round judged at the best_m it has seen so far
            lo, hi = None, None
            for b in range(0, len(ks), GL):
                ur = u[b:b + GL]
                best_m = max(best_m, int(ur.max()))
                ok = np.flatnonzero(ur >= best_m - band)
                if len(ok):
                    lo = b + int(ok[0]) if lo is None else lo
                    hi = b + int(ok[-1])
            if lo is None or (u[lo] >= best_m - band and u[hi] >= best_m - band):
                settled += 1
            else:
                fallback += 1
        ok = np.flatnonzero(u >= best_m - band)
        new_min, new_max = (ks[ok[0]], ks[ok[-1]]) if len(ok) else (max_k, min_k)
        if len(ks) > GL and lo is not None and u[lo] >= best_m - band and u[hi] >= best_m - band:
            assert (new_min, new_max) == (ks[lo], ks[hi])     # the claim the kernel rests on
        min_k, max_k = int(new_min) - 1, int(new_max) + 1
    return False, d, settled, fallback


def test_seeds_reach_both_outcomes_of_a_wide_step():
    """the committed seed gives, at every band, at least 50 wide steps settled from the recorded extremes and at least 50 that fall back to
    the full scan, and wide steps in matched as well as in unmatched alignments; the port's verdicts agree with the oracle's"""
    db, keys, pairs = _build()
    runs = [_runs(q, t) for q, t in pairs]
    for band in BANDS:
        settled = fallback = 0
        wide_matched = wide_unmatched = 0
        for i, (q, t) in enumerate(pairs):
            matched, d, s, f = count_wide_steps(runs[i], band)
            want = U.orc_ovlp_match(_encode(q), 0, _encode(t), 0, band)
            assert matched == (want[0] > 0) and (not matched or d == want[1]), (band, i, matched, d, want)
            settled, fallback = settled + s, fallback + f
            if s + f:
                wide_matched += matched
                wide_unmatched += not matched
        print(f"band {band}: {settled + fallback} wide steps, {settled} settled in END, {fallback} full scans; "
              f"alignments with wide steps: {wide_matched} matched, {wide_unmatched} unmatched")
        assert settled >= 50 and fallback >= 50, (band, settled, fallback)
        assert wide_matched >= 1 and wide_unmatched >= 1, (band, wide_matched, wide_unmatched)


# ---- every form of the alignment kernels on these pairs ------------------------------------------------------------------------------
def _oracle_matches(db, keys, band):
    out = np.zeros(len(keys), _lib.MATCH_DTYPE)
    for i in range(len(keys)):
        a, b = int(keys["rid0"][i]), int(keys["rid1"][i])
        q = db.seqdb[int(db.roff[a]) + int(keys["q_off"][i]):int(db.roff[a]) + int(db.rlen[a])]
        t = db.seqdb[int(db.roff[b]):int(db.roff[b]) + int(db.rlen[b])]
        out[i] = U.orc_ovlp_match(q, int(keys["dir0"][i]), t, int(keys["dir1"][i]), band)
    return out


VARIANTS = [   # (id, environment, database): the forms tests/test_gpu_parity.py::test_align_variants_vs_oracle reaches
    ("ph8-packed", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0"), "plain"),
    ("ph8-packed-ambiguous", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0"), "withN"),
    ("ph8-packed-stragglers", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ITER_LIMIT="150"), "plain"),
    ("ph8-packed-ordered", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ORDER_MIN="0"), "plain"),
    ("ph8-packed-ordered-nw4", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ORDER_MIN="0", PGX_ALIGN_NW="4", PGX_ALIGN_SEG="24"), "plain"),
    ("ph8-packed-nw1", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_NW="1", PGX_ALIGN_SEG="8"), "plain"),
    ("ph8-packed-file-order", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ORDER_MIN="0"), "plain3"),
    ("ph8-bytes", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="-1"), "plain2"),
    ("one-per-wave", dict(PGX_ALIGN_SMALL="1000000000"), "plain"),
    ("one-per-wave-bytes", dict(PGX_ALIGN_SMALL="1000000000", PGX_ALIGN1_PACKED="0"), "plain"),
    ("one-per-wave-ambiguous", dict(PGX_ALIGN_SMALL="1000000000"), "withN"),
    ("ph8-packed-stragglers-bytes", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ITER_LIMIT="150", PGX_ALIGN1_PACKED="0"), "plain"),
    ("long-reads-int32", dict(PGX_ALIGN_SMALL="0"), "long"),   # a 70 kb read in the set: k_align_ph<int32> on the bytes
]


@pytest.fixture(scope="module")
def wide_sets():
    """database name -> (db, ResidentDB, keys of one launch, {band: the oracle's matches}); computed once, never changed afterwards"""
    sets = {}
    plain_want = None
    for name, kw in (("plain", {}), ("plain2", {}), ("plain3", {}), ("withN", dict(ambiguous=True)), ("long", dict(long_read=True))):
        db, keys, _ = _build(**kw)
        rdb = ResidentDB(db, 0)
        if name == "plain":   # its overlap stage lays the packs out by locus key: the ordered forms take the requests through an order list
            ix = rdb.index()
            rdb.overlap(ix.top, ix.top_mc)
        # 48 pairs three times over, shuffled: the 8 groups of a wavefront hold different shapes in different phases
        order = np.random.default_rng(5).permutation(np.tile(np.arange(len(keys)), 3))
        if name == "withN" or plain_want is None:
            want = {band: _oracle_matches(db, keys, band) for band in BANDS}
            plain_want = want if name == "plain" else plain_want
        else:
            want = plain_want   # (the same reads)
        sets[name] = (db, rdb, keys[order], {band: w[order] for band, w in want.items()})
    yield sets
    for _, rdb, _, _ in sets.values():
        rdb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vid,env,which", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_wide_steps_vs_oracle(wide_sets, vid, env, which):
    db, rdb, keys, want = wide_sets[which]
    assert len(keys) >= 64
    if which == "long":
        assert int(db.rlen.max()) > 65535
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        for band in BANDS:
            got = rdb.align(keys, band)
            for f in _lib.MATCH_DTYPE.names:
                bad = np.flatnonzero(got[f] != want[band][f])
                assert len(bad) == 0, (vid, band, f, len(bad), keys[bad[:3]], got[bad[:3]], want[band][bad[:3]])
            assert (want[band]["m_size"] > 0).any() and (want[band]["m_size"] == 0).any()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
