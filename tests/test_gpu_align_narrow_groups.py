"""k_align_ph with groups of 4 and of 8 lanes on the in-place half ring (pgx_align.hip).

The grouped alignment kernel keeps V of a step in a ring indexed by s(k, d) = (k - d) >> 1 and updates it in place: the lane of diagonal
k reads V_old[k-1] from slot s and V_old[k+1] from slot s + 1 and writes V_new[k] to slot s.  A step of more than GL diagonals takes
several rounds, going up in k; the slot a lane overwrites held V_old[k-1], whose only other reader -- the lane of k - 2 -- ran a round
earlier at the latest, so no round finds a slot of its own overwritten.  With s = (k + d) >> 1 instead the write lands on V_old[k+1],
which the first lane of the NEXT round still needs: that form needs the value carried from round to round.  `model_match` below is a
port of the reference's d-loop (DWmatch.c:119-183) that follows the kernel round by round on such a ring, in all three forms
("minus", "plus" with the carry, "plus" without); the CPU tests show that the first two equal the oracle's ovlp_match on every pair and
that the third does not, that the kernel's form never reads a slot the step before did not write, and that the committed seeds reach
the cases listed in `test_seeds_reach_the_cases`.  Every grouped form of the kernel is then compared field by field with the oracle
on these pairs, at both group widths.

A degenerate band (max_k < min_k, an empty k-loop) cannot be reached from ovlp_match's own start state: U of a diagonal is at least one
more than U of the neighbour it starts from, so the step's largest U never falls and its diagonal always passes the band test; the
kernel and the model both keep the branch, and the model asserts that no pair takes it.  What the tests reach instead is the narrowest
band the library takes: band 1, where one or two diagonals survive a step (ring 32, a few slots in use)."""
import os

import numpy as np
import pytest

import oracle_util as U
import test_gpu_align_wide_steps as W
from peregrine_amd import _lib, formats
from peregrine_amd.shimmer import ResidentDB

BANDS = (30, 100, 130)
NARROW = 1     # the narrowest band the library takes
PROBE = 16     # bases of a probe of the packed form
FIELDS = _lib.MATCH_DTYPE.names   # m_size, dist, q_bgn, q_end, t_bgn, t_end, t_m_end, q_m_end: the order of the oracle's tuple


def ring_of(band):
    """slots of the grouped kernel's ring (dev_align): the next power of two >= band + 2, at least 32"""
    ring = 32
    while ring < band + 2:
        ring <<= 1
    return ring


# ---- the read pairs ---------------------------------------------------------------------------------------------------------------
def _drift(rng, n_t, every):
    """the target, and the target with one base in `every` deleted: k falls by one per step, the slot index by one per step"""
    t = rng.integers(0, 4, n_t, dtype=np.uint8)
    return t[np.arange(n_t) % every != every - 1], t


def _prefix(rng, run):
    """query and target of 1.2 kb that share exactly `run` bases from (0, 0) on, then one substitution, then 2 % error"""
    t = rng.integers(0, 4, 1200, dtype=np.uint8)
    q = np.concatenate([t[:run], [(t[run] + 1) & 3], W._mutate(rng, t[run + 1:], 0.02)]).astype(np.uint8)
    return q, t


def _ending(rng, run):
    """a query of `run` bases equal to the target's first `run`: the first diagonal runs to the end of the query"""
    t = rng.integers(0, 4, 1200, dtype=np.uint8)
    return t[:run].copy(), t


RANDOM_SHAPES = ["diverging"] * 8 + ["noisy"] * 6 + ["lowcomplexity"] * 4 + ["jumps"] * 8
RUNS_BEYOND_PROBE = (127, 128, 129, 255, 256, 257)
PROBES = (15, 16, 17)
ENDINGS = (PROBE + 100, PROBE + 128, PROBE + 256, PROBE + 3 * 128)   # inside the window / on the edge of 4 x 32, of 8 x 32, after three windows


def _pairs(seed=20241020):
    rng = np.random.default_rng(seed)
    pairs = [W._pair(rng, s) for s in RANDOM_SHAPES]
    pairs += [_prefix(rng, PROBE + r) for r in RUNS_BEYOND_PROBE]
    pairs += [_prefix(rng, p) for p in PROBES]
    pairs += [_ending(rng, n) for n in ENDINGS]
    pairs.append(_drift(rng, 1200, 3))    # 400 steps down the diagonals: three turns of the ring of 128
    pairs.append(_drift(rng, 2700, 3))    # 900 steps: three turns of the ring of 256
    return pairs


def _build(pairs, seed=7, long_read=False, ambiguous=False):
    """reads 2 i / 2 i + 1 = query / target of pair i, as test_gpu_align_wide_steps builds them; a short query sits at the end of a read
    of about 1.2 kb (q_off never a multiple of 16)"""
    rng = np.random.default_rng(seed)
    reads, keys = [], np.zeros(len(pairs), _lib.ALIGN_KEY_DTYPE)
    for i, (q, t) in enumerate(pairs):
        q_off = (int(rng.integers(0, 8)) if len(q) >= 1000 else (1200 - len(q)) // 16) * 16 + int(rng.integers(1, 16))
        d0, d1 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        qs = np.concatenate([rng.integers(0, 4, q_off, dtype=np.uint8), q])
        reads.append(W._COMP[qs[::-1]] if d0 else qs)
        reads.append(W._COMP[t[::-1]] if d1 else t)
        keys[i] = (2 * i, 2 * i + 1, q_off, d0, d1, 0)
    if long_read:
        reads.append(rng.integers(0, 4, 70_000, dtype=np.uint8))
    enc = [W._encode(r) for r in reads]
    if ambiguous:   # a base without a 2-bit code in every third target, beyond the shortest alignment of the set
        for i in range(0, len(pairs), 3):
            enc[2 * i + 1][len(enc[2 * i + 1]) - 7] = 0
    rlen = np.array([len(e) for e in enc], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    return formats.SeqDB(np.concatenate(enc), np.arange(len(enc), dtype=np.uint32), rlen, roff, None), keys


# ---- the d-loop on the half ring, round by round as the kernel goes ------------------------------------------------------------------
def model_match(run, band, gl, scheme="minus", carry=True, ring=None):
    """ovlp_match on a pair's table of runs (W._runs), in rounds of `gl` diagonals on a ring of `ring` slots updated in place.
    scheme "minus": slot (k - d) >> 1, the kernel's; "plus": slot (k + d) >> 1, with or without the value carried between rounds.
    Returns (the eight fields of the match in FIELDS' order, what the alignment passed through)."""
    ql, tl = run.shape[0] - 1, run.shape[1] - 1
    max_d = int(0.3 * (ql + tl))
    ring = ring or ring_of(band)
    val, tag = [0] * ring, [None] * ring           # a slot's value, and the step that wrote it
    sgn = -1 if scheme == "minus" else 1
    tag[(1 if scheme == "minus" else 0) % ring] = -1   # V[1] = 0 of the start state
    st = dict(nk=set(), hits=[], runs=set(), probes=set(), end_inside=0, end_on_edge=0, settled=0, fallback=0, turns=0, wide_across_wrap=0,
              carry_decides=0, stale_reads=0, degenerate=0, steps=0, iters=1)   # (iters: the group's wavefront iterations, FETCH's included)
    best_m, min_k, max_k, longest, started = -1, 0, 0, 0, False
    q_bgn = t_bgn = q_m_end = t_m_end = 0
    s_lo = s_hi = 0
    res = None
    d = 0
    for d in range(max_d):
        if max_k - min_k > 2 * band:
            break
        if max_k < min_k:
            st["degenerate"] += 1
            min_k, max_k = max_k - 1, min_k + 1
            continue
        nk = (max_k - min_k) // 2 + 1
        assert nk + 1 <= ring
        st["nk"].add(nk), st.__setitem__("steps", st["steps"] + 1)
        s_first = (min_k + sgn * d) >> 1
        s_lo, s_hi = min(s_lo, s_first), max(s_hi, s_first + nk)
        if nk > gl and s_first // ring != (s_first + nk) // ring:
            st["wide_across_wrap"] += 1
        us, lo, hi, carried, hit_at = [], None, None, None, None
        for base in range(0, nk, gl):
            lanes = range(base, min(base + gl, nk))
            starts = []
            for j in lanes:                                    # ROUND: every read of the round ...
                k = min_k + 2 * j
                sw = (k + sgn * d) >> 1
                sa, sb = (sw, sw + 1) if scheme == "minus" else (sw - 1, sw)
                va, vb = val[sa % ring], val[sb % ring]
                if scheme == "plus" and j == base and base > 0:
                    if k != min_k and k != max_k and (va < vb) != (carried < vb):
                        st["carry_decides"] += 1
                    if carry:
                        va = carried
                    elif k != min_k:
                        st["stale_reads"] += tag[sa % ring] != d - 1
                elif k != min_k:
                    st["stale_reads"] += tag[sa % ring] != d - 1
                if k != max_k or k == min_k:
                    st["stale_reads"] += tag[sb % ring] != d - 1
                carried = vb
                starts.append((k, sw, vb if (k == min_k or (k != max_k and va < vb)) else va + 1))
            snakes = 0
            for j, (k, sw, x1) in zip(lanes, starts):          # ... precedes its writes (END), lowest k first
                y1 = x1 - k
                ext = int(run[x1, y1])
                rem = min(ql - x1, tl - y1)
                st["probes"].add(min(ext, PROBE + 1))
                if rem > PROBE and ext >= PROBE:               # SNAKE: windows of gl x 32 bases beyond the probe
                    beyond = ext - PROBE
                    st["runs"].add(beyond)
                    snakes += beyond // (gl * 32) + (0 if ext == rem and beyond and beyond % (gl * 32) == 0 else 1)
                    if ext == rem:
                        st["end_inside" if beyond % (gl * 32) else "end_on_edge"] += 1
                x, y = x1 + ext, y1 + ext
                if not started and ext > 16:
                    q_bgn, t_bgn, started = x1, y1, True
                if ext > longest:
                    longest, q_m_end, t_m_end = ext, x, y
                val[sw % ring], tag[sw % ring] = x, d
                best_m = max(best_m, x + y)
                us.append(x + y)
                if x >= ql or y >= tl:
                    hit_at = (base // gl, j - base)
                    res = ((x - q_bgn + y - t_bgn + 2 * d) // 2, d, q_bgn, x, t_bgn, y, t_m_end, q_m_end)
                    break
            st["iters"] += max(1, snakes)   # ROUND, the first SNAKE and END share an iteration
            if hit_at:
                break
            ok = [j for j in lanes if us[j] >= best_m - band]   # the round's own mask, at the best_m it has seen
            if ok:
                lo, hi = ok[0] if lo is None else lo, ok[-1]
        if hit_at:
            st["hits"].append(hit_at)
            break
        ok = [j for j in range(nk) if us[j] >= best_m - band]
        if nk > gl:
            if lo is None or (us[lo] >= best_m - band and us[hi] >= best_m - band):
                st["settled"] += 1
                assert (lo is None and not ok) or (lo, hi) == (ok[0], ok[-1])   # END's answer is the scan's
            else:
                st["fallback"] += 1
                st["iters"] += (nk + gl - 1) // gl - 1   # BAND, a round per iteration, the first in END's
        new_min, new_max = (min_k + 2 * ok[0], min_k + 2 * ok[-1]) if ok else (max_k, min_k)
        min_k, max_k = new_min - 1, new_max + 1
    st["turns"] = s_hi // ring - s_lo // ring
    if res is None:
        res = (0, 0, 0, 0, 0, 0, t_m_end, q_m_end)
    return res, st


_cache = {}


def _cpu():
    """pairs, their run tables and the oracle's matches at every band: computed once, never changed"""
    if not _cache:
        pairs = _pairs()
        _cache["pairs"] = pairs
        _cache["runs"] = [W._runs(q, t) for q, t in pairs]
        _cache["want"] = {band: [U.orc_ovlp_match(W._encode(q), 0, W._encode(t), 0, band) for q, t in pairs] for band in BANDS + (NARROW,)}
    return _cache["pairs"], _cache["runs"], _cache["want"]


@pytest.mark.parametrize("gl", [4, 8])
def test_half_ring_model_equals_the_oracle(gl):
    """the kernel's form of the ring, in rounds of 4 and of 8, gives the oracle's eight fields on every pair at every band, and every
    value it uses was written by the step before"""
    pairs, runs, want = _cpu()
    for band in BANDS + (NARROW,):
        for i, run in enumerate(runs):
            got, st = model_match(run, band, gl)
            assert got == tuple(want[band][i]), (band, gl, i, got, want[band][i])
            assert st["stale_reads"] == 0 and st["degenerate"] == 0, (band, gl, i, st)


def test_plus_ring_needs_the_carry():
    """slot (k + d) >> 1: with the value carried from round to round the oracle's result on every pair; without it the first lane of a
    later round reads what the round before wrote, the `va < vb` choice changes, and results differ"""
    pairs, runs, want = _cpu()
    band, decided, differing = 100, 0, 0
    for i, run in enumerate(runs):
        got, st = model_match(run, band, 4, scheme="plus")
        assert got == tuple(want[band][i]) and st["stale_reads"] == 0, (i, got, want[band][i], st)
        decided += st["carry_decides"] > 0
        bad, st2 = model_match(run, band, 4, scheme="plus", carry=False)
        assert max(st["nk"]) <= 4 or st2["stale_reads"] > 0   # (every later round's first lane)
        differing += bad != tuple(want[band][i])
    print(f"pairs in which the carried value decides va < vb: {decided}; pairs the form without the carry gets wrong: {differing}")
    assert decided >= 1 and differing >= 1


def test_seeds_reach_the_cases():
    """the cases the GPU tests below rest on, shown on the CPU for the committed seed"""
    pairs, runs, want = _cpu()
    for gl in (4, 8):
        nks, hits, beyond, probes = set(), [], set(), set()
        inside = edge = 0
        for band in BANDS:
            ring = ring_of(band)
            wide = dict(settled=[0, 0], fallback=[0, 0])   # [in unmatched, in matched alignments]
            turns = across = 0
            for i, run in enumerate(runs):
                got, st = model_match(run, band, gl)
                m = got[0] > 0
                nks |= st["nk"]; hits += st["hits"]; beyond |= st["runs"]; probes |= st["probes"]
                inside += st["end_inside"]; edge += st["end_on_edge"]
                wide["settled"][m] += st["settled"]; wide["fallback"][m] += st["fallback"]
                turns = max(turns, st["turns"]); across += st["wide_across_wrap"]
            print(f"GL {gl} band {band} ring {ring}: wide steps settled in END {wide['settled']}, to BAND {wide['fallback']} (unmatched, matched); "
                  f"most turns of the ring {turns}; wide steps across the wrap {across}")
            assert min(wide["settled"]) >= 1 and min(wide["fallback"]) >= 1, (gl, band, wide)
            assert turns >= 3 and across >= 1, (gl, band, turns, across)
        assert {4, 5, 8, 9} <= nks, sorted(nks)
        rounds, lanes = {r for r, _ in hits}, {l for _, l in hits}
        print(f"GL {gl}: hits in rounds {sorted(rounds)}, lanes {sorted(lanes)}; runs that end at a sequence's end inside a window {inside}, on its edge {edge}")
        assert 0 in rounds and max(rounds) >= 1 and {0, gl - 1} <= lanes, (gl, sorted(rounds), sorted(lanes))
        assert set(RUNS_BEYOND_PROBE) <= beyond, sorted(beyond)
        assert {15, 16, 17} <= probes       # (17 = a probe that matched throughout and a base beyond)
        assert 0 in beyond and 1 in beyond  # probes of exactly 16 and 17 bases
        assert inside >= 1 and edge >= 1
    assert len({ring_of(b) for b in BANDS}) == 3 and ring_of(NARROW) == 32
    for band in BANDS:   # matched and unmatched alignments at every band
        ms = [w[0] > 0 for w in want[band]]
        assert any(ms) and not all(ms)


# ---- every grouped form of the kernel on these pairs ---------------------------------------------------------------------------------
GROUPED = dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0")
FORMS = [   # (id, environment on top of PGX_ALIGN_GL, database)
    ("packed", dict(GROUPED), "plain"),
    ("packed-ordered", dict(GROUPED, PGX_ALIGN_ORDER_MIN="0"), "plain"),
    ("packed-ordered-nw4", dict(GROUPED, PGX_ALIGN_ORDER_MIN="0", PGX_ALIGN_NW="4", PGX_ALIGN_SEG="24"), "plain"),
    ("packed-nw1", dict(GROUPED, PGX_ALIGN_NW="1", PGX_ALIGN_SEG="8"), "plain"),
    ("packed-stragglers", dict(GROUPED, PGX_ALIGN_ITER_LIMIT="150"), "plain"),
    ("packed-ambiguous", dict(GROUPED), "withN"),
    ("bytes", dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="-1"), "plain2"),
    ("compacted", dict(GROUPED), "compacted"),
    ("compacted-stragglers", dict(GROUPED, PGX_ALIGN_ITER_LIMIT="150"), "compacted"),
]


def _oracle_matches(db, keys, bands):
    return {band: W._oracle_matches(db, keys, band) for band in bands}


@pytest.fixture(scope="module")
def sets():
    """database name -> (db, ResidentDB, keys of one launch, {band: the oracle's matches}); computed once, never changed afterwards"""
    pairs = _pairs()
    out, plain_want = {}, None
    for name, kw in (("plain", {}), ("plain2", {}), ("withN", dict(ambiguous=True)), ("compacted", dict(ambiguous=True)), ("long", dict(long_read=True))):
        db, keys = _build(pairs, **kw)
        rdb = ResidentDB(db, 0)
        if name == "plain":   # its overlap stage lays the packs out by locus key: the ordered forms take the requests through an order list
            ix = rdb.index()
            rdb.overlap(ix.top, ix.top_mc)
        if kw.get("ambiguous"):
            want = out["withN"][3] if name == "compacted" else _oracle_matches(db, keys, BANDS + (NARROW,))
        else:
            want = plain_want = plain_want or _oracle_matches(db, keys, BANDS + (NARROW,))
        if name == "compacted":
            rdb.align(keys, 100)   # (a first launch builds the packs)
            assert rdb.compact_bytes() is True and not rdb.has_bytes and rdb.side_bytes > 0
        out[name] = (db, rdb, keys, want)
    yield out
    for _, rdb, _, _ in out.values():
        rdb.close()


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _check(rdb, keys, want, band, what):
    got = rdb.align(keys, band)
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, (what, band, f, len(bad), keys[bad[:3]], got[bad[:3]], want[bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("gl", [4, 8])
@pytest.mark.parametrize("fid,env,which", FORMS, ids=[f[0] for f in FORMS])
def test_grouped_forms_vs_oracle(sets, gl, fid, env, which):
    """the pairs three times over, shuffled (the groups of a wavefront hold different shapes in different phases), at three ring sizes
    and at the narrowest band"""
    db, rdb, keys, want = sets[which]
    order = np.random.default_rng(5).permutation(np.tile(np.arange(len(keys)), 3))
    assert len(order) >= 64
    with _env(PGX_ALIGN_GL=str(gl), **env):
        for band in BANDS + (NARROW,):
            _check(rdb, keys[order], want[band][order], band, (fid, gl))
            assert (want[band]["m_size"] > 0).any() and (want[band]["m_size"] == 0).any()


@pytest.mark.gpu
def test_long_reads_keep_eight_lanes(sets):
    """a 70 kb read in the set: k_align_ph<int32> on the bytes, 8 lanes whatever PGX_ALIGN_GL says, on the half ring"""
    db, rdb, keys, want = sets["long"]
    assert int(db.rlen.max()) > 65535
    order = np.random.default_rng(6).permutation(np.tile(np.arange(len(keys)), 3))
    for gl in ("4", "8"):
        with _env(PGX_ALIGN_GL=gl, PGX_ALIGN_SMALL="0"):
            for band in BANDS:
                _check(rdb, keys[order], want[band][order], band, ("long", gl))


@pytest.mark.gpu
def test_default_dispatch_vs_oracle(sets):
    """no PGX_ALIGN_GL: the main launch of a stage at 4 lanes, a tail batch at 8"""
    db, rdb, keys, want = sets["plain"]
    order = np.random.default_rng(8).permutation(np.tile(np.arange(len(keys)), 3))
    assert "PGX_ALIGN_GL" not in os.environ
    with _env(**GROUPED):
        _check(rdb, keys[order], want[100][order], 100, "default")


SHAPES = [   # (id, environment, database) of the launch-shape test
    ("plain", dict(GROUPED, PGX_ALIGN_ORDER_MIN="-1"), "plain"),
    ("ordered", dict(GROUPED, PGX_ALIGN_ORDER_MIN="0"), "plain"),
    ("stragglers", dict(GROUPED, PGX_ALIGN_ORDER_MIN="-1", PGX_ALIGN_ITER_LIMIT="100"), "plain"),
    ("stragglers-ordered", dict(GROUPED, PGX_ALIGN_ORDER_MIN="0", PGX_ALIGN_ITER_LIMIT="100"), "plain"),
    ("ambiguous", dict(GROUPED), "withN"),
    ("compacted", dict(GROUPED), "compacted"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("gl", [4, 8])
@pytest.mark.parametrize("sid,env,which", SHAPES, ids=[s[0] for s in SHAPES])
def test_launch_shapes(sets, gl, sid, env, which):
    """1, 15, 16, 17, 33 and 1,000 candidates through the grouped kernel: fewer than a wavefront's groups, exactly as many, one more,
    two wavefronts and one, and several workgroups"""
    db, rdb, keys, want = sets[which]
    rng = np.random.default_rng(11)
    with _env(PGX_ALIGN_GL=str(gl), **env):
        for n in (1, 15, 16, 17, 33, 1000):
            pick = rng.integers(0, len(keys), n)
            _check(rdb, keys[pick], want[100][pick], 100, (sid, gl, n))
