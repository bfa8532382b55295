"""The inputs of tests/test_gpu_contigs_random.py, held to what they are for.  These are conditions on the generated read set, the random
tiling path and the engineered rows, checked on the CPU from contig_util.segments over the oracle's ovlp_match: each names a path of the
layout kernels (pgx_contigs.hip) that the GPU comparison can only see if the input reaches it, so none of them may be relaxed -- a
condition that fails is a reason to change the generator.  Every count asserted on is printed (pytest -s)."""
import os

import numpy as np
import pytest

import contig_util as CU
import oracle_util as U

TILE = 4096   # k_stitch's tile of the concatenated output
GROUP = 256   # rows per workgroup of k_tile_geom / k_tile_place


@pytest.fixture(scope="module", params=(True, False), ids=("ambiguous", "plain"))
def case(request):
    return CU.case(request.param)


@pytest.fixture(scope="module")
def flat(case):
    """dst, src, length, contig of every segment in the device's numbering, and the non-empty ones' mask"""
    dst, src, n, ctg = case.flat.T
    return dst, src, n, ctg, n > 0


def test_read_set(case):
    db = case.db
    n500, near, mod16 = int((db.rlen == 500).sum()), int(((db.rlen > 500) & (db.rlen <= 520)).sum()), sorted({int(o) % 16 for o in db.roff})
    print("reads %d, bases %d, of 500 bases: %d, of 501 .. 520: %d, offsets mod 16: %s, with planted N: %d" % (db.n_reads, db.n_bases, n500, near, mod16,
                                                                                                              len(case.rs.n_rids)))
    assert db.n_reads == 3000 and db.rlen.min() == 500 and db.rlen.max() <= 1500
    assert n500 >= 50 and near >= 50 and mod16 == list(range(16))
    assert len(case.rs.n_rids) in (0, 60)
    for r in case.rs.n_rids:   # a planted read has a nibble that is no base
        b = db.seqdb[int(db.roff[r]):int(db.roff[r]) + int(db.rlen[r])]
        assert ((b & 15) == 0).any()
    assert case.rs.n_rids or not ((db.seqdb & 15) == 0).any()


def test_path_size_kinds_and_validity(case):
    rows, names = case.rows, case.names
    kinds = [ln.split()[9] for ln in case.text.splitlines()]
    by_line = {r[7]: i for i, r in enumerate(rows)}
    kind_of_row = [None] * len(rows)
    for line, k in enumerate(kinds):
        kind_of_row[by_line[line]] = k
    count = {k: kinds.count(k) for k in sorted(set(kinds))}
    file_ctg = [ln.split()[0] for ln in case.text.splitlines()]
    switches = sum(a != b for a, b in zip(file_ctg, file_ctg[1:]))
    single500 = sum(1 for sg, _ in case.segs if len(sg) == 2 and sg[0][4] == 500)
    print("rows %d, contigs %d, segments %d, output bytes %d, kinds %s, lines whose contig differs from the line before: %d, one-row contigs on a 500-base read: %d"
          % (len(rows), len(names), len(case.flat), case.ctg_off[-1], count, switches, single500))
    assert len(rows) >= 20_000 and len(names) >= 2_000 and single500 >= 300
    assert switches >= len(rows) // 2 and [r[0] for r in rows] == sorted(r[0] for r in rows) and [r[7] for r in rows] != sorted(r[7] for r in rows)
    rec = iter(case.matches)
    assert CU.offences(case.db, case.text, lambda *a: next(rec)) == []                # no invalid row by the statement
    # the dovetails: overhangs 1 .. 40 all there, and longer ones; alignments with errors in them; unmatched rows
    m = np.array(case.matches)
    dove = np.array([k.split("+")[0] in ("short", "long") for k in kind_of_row])
    spans = np.array([abs(r[6] - r[5]) for r in rows])
    share = float((m[dove, 1] >= 5).mean())
    unmatched = int((m[:, 0] == 0).sum())
    print("dovetail rows %d, with dist >= 5: %.1f %%, median dist %d; unmatched rows %d; rows with seg == 0 against themselves: %d"
          % (dove.sum(), 100 * share, np.median(m[dove, 1]), unmatched, sum(k.startswith("self") for k in kinds)))
    assert set(range(1, 41)) <= set(spans[dove].tolist()) and (spans[dove] > 200).sum() >= 1000
    assert share >= 0.30 and unmatched >= 100
    assert sum(k.startswith("self") for k in kinds) >= 200 and sum(k.startswith("arb") for k in kinds) >= 2000
    if case.rs.n_rids:
        touching = sum(1 for r in rows if r[1] in case.rs.n_rids or r[3] in case.rs.n_rids)
        print("rows whose v or w has planted N: %d" % touching)
        assert touching >= 500 and any(k.endswith("+amb") for k in kinds)
    else:
        assert not any(k.endswith("+amb") for k in kinds)


def test_copy_paths_of_the_stitch_kernel(case, flat):
    dst, src, n, ctg, full = flat
    phases = {(int(d) % 8, int(s) % 8) for d, s in zip(dst[full], src[full])}
    lengths = set(n[full].tolist())
    print("(dst mod 8, src mod 8) combinations: %d of 64; lengths 1 .. 24 present: %s" % (len(phases), sorted(lengths & set(range(1, 25)))))
    assert len(phases) == 64
    assert set(range(1, 25)) <= lengths
    # a segment split by a tile boundary: the boundary B with dst < B < dst + n (a segment is shorter than a tile: at most one)
    assert n.max() < TILE
    b = (dst // TILE + 1) * TILE
    split = full & (b < dst + n)
    cut_dst, cut_src = sorted(set(((b - dst)[split] % 8).tolist())), sorted(set(((src + b - dst)[split] % 8).tolist()))
    split_len = sorted(set(n[split].tolist()) & set(range(1, 8)))
    one = n == 1
    print("segments split by a tile boundary: %d; bytes in front of the cut mod 8: %s; source byte at the cut mod 8: %s; split lengths below 8: %s; "
          "1-byte segments as a tile's last byte: %d, as its first: %d" % (split.sum(), cut_dst, cut_src, split_len, (one & (dst % TILE == TILE - 1)).sum(),
                                                                              (one & (dst % TILE == 0)).sum()))
    assert cut_dst == list(range(8)) and cut_src == list(range(8))
    # lengths 2 .. 7 are split; one byte cannot be, so "crosses" means for it: it is the byte on either side of a boundary
    assert split_len == list(range(2, 8))
    assert (one & (dst % TILE == TILE - 1)).any() and (one & (dst % TILE == 0) & (dst > 0)).any()


def test_dense_tiles_and_the_searched_range(case, flat):
    dst, src, n, ctg, full = flat
    total = int(case.ctg_off[-1])
    tiles = -(-total // TILE)
    touch = np.zeros(tiles, np.int64)
    t0, t1 = dst[full] // TILE, (dst[full] + n[full] - 1) // TILE
    np.add.at(touch, t0, 1)
    np.add.at(touch, t1[t1 != t0], 1)
    o = case.ctg_off
    whole = np.zeros(tiles, np.int64)
    inside = o[:-1] // TILE == (o[1:] - 1) // TILE                       # a whole contig inside one tile
    np.add.at(whole, (o[:-1] // TILE)[inside], 1)
    back = sum(1 for c, (sg, _) in enumerate(case.segs) for a, b in zip(sg, sg[1:]) if b[1] < a[1])
    empty = int((~full).sum())
    # the range k_stitch searches for tile [a, b): k0 = the first k whose running furthest end passes a, k1 = the first k >= k0 from which on
    # every start is at b or beyond; an empty segment is the neutral element of both
    end_max = np.maximum.accumulate(np.where(full, dst + n, 0))
    start_min = np.minimum.accumulate(np.where(full, dst, np.iinfo(np.int64).max)[::-1])[::-1]
    a = np.arange(tiles, dtype=np.int64) * TILE
    k0 = np.searchsorted(end_max, a, side="right")
    k1 = np.maximum(np.searchsorted(start_min, np.minimum(a + TILE, total), side="left"), k0)
    before = int(((k0 > 0) & ~full[np.maximum(k0 - 1, 0)]).sum())
    after = int(((k1 < len(n)) & ~full[np.minimum(k1, len(n) - 1)]).sum())
    print("tiles %d; most segments touching one tile: %d; most in one searched range: %d; most whole contigs in one tile: %d; rows that start before the "
          "segment before them: %d; empty segments: %d; tiles with an empty segment directly before their range: %d, directly after: %d; negative steps: %d"
          % (tiles, touch.max(), (k1 - k0).max(), whole.max(), back, empty, before, after,
             sum(1 for sg, _ in case.segs for a_, b_ in zip(sg, sg[1:]) if b_[1] + b_[4] < a_[1] + a_[4])))
    assert touch.max() >= 16 and whole.max() >= 3
    assert back >= 200
    assert empty >= 200 and before >= 1 and after >= 1


def test_rows_span_the_workgroups(case):
    fr = np.array(case.first_row)
    straddle = int((fr[:-1] // GROUP != fr[1:] // GROUP).sum())
    at_edge = [int(c) for c in np.flatnonzero(fr[:-1] % GROUP == 0) if c > 0]
    print("contigs whose rows reach into the next group of %d rows: %d; contigs (not the first) whose first row opens a group: %d" % (GROUP, straddle,
                                                                                                                                    len(at_edge)))
    assert straddle >= 1 and len(at_edge) >= 1


@pytest.fixture(scope="module")
def engineered():
    c = CU.case(True)
    db, ids = CU.engineered_reads(c.db)
    return c, db, ids


def test_pull_back_row_steps_by_minus_48(engineered):
    _, db, ids = engineered
    assert int(db.rlen[ids["v500"]]) == 500 and int(db.rlen[ids["w"]]) == 801
    tail = lambda r: db.seqdb[int(db.roff[r]) + int(db.rlen[r]) - 500:int(db.roff[r]) + int(db.rlen[r])]
    assert np.array_equal(tail(ids["v"]) & 15, db.seqdb[int(db.roff[ids["v500"]]):int(db.roff[ids["v500"]]) + 500] & 15)   # strand 0 of both: X
    for v in ("v", "v500"):
        rec = CU.Recording(U.orc_ovlp_match)
        (sg, ctg_len), = CU.segments(db, "c " + CU.pull_back(ids, v) + "\n", rec, strict=False)
        m = rec.calls[0]
        print("pull-back row on %s: ovlp_match %s, seg %d, step %d" % (v, m, sg[1][4], ctg_len - sg[0][4]))
        assert (m[3], m[5], m[7], m[6]) == (452, 501, 452, 501)      # q_end, t_end, q_m_end, t_m_end
        assert sg[1][4] == 0 and ctg_len - sg[0][4] == -48


def test_error_paths_offend_where_designed(engineered):
    c, db, ids = engineered
    cases = CU.error_paths(db, ids, CU.filler_contigs(c), U.orc_ovlp_match)
    kinds_first, n_far = set(), 0
    for name, text, want, line in cases:
        got = CU.offences(db, text, U.orc_ovlp_match)
        print("%-62s rows %4d, offences %s, the line to name: %d" % (name, text.count("\n"), got, line))
        assert got and got[0] == want, name
        assert len(got) == (1 if "alone" in name else 2), name
        lines = [CU.parse_path(text)[0][i][7] for i, _ in got]
        assert lines[0] == line
        if "far apart" in name:     # the same kind twice; the smallest offending row is the LATER line where its contig's rows end the file
            assert got[1][0] - got[0][0] > GROUP and got[1][1] == got[0][1] and (lines[0] > lines[1]) == ("line last" in name)
            n_far += 1
        with pytest.raises(ValueError):
            CU.layout(db, text, U.orc_ovlp_match)
        kinds_first.add(want[1])
    assert kinds_first == set(CU.KINDS) and n_far == 6
    assert sum(1 for _, _, want, line in cases if want[0] != line) >= len(cases) - 1      # the line is not the row
    # each block alone is exactly one offence, and without the offending row the path is valid
    for name, text, want, line in cases[:4]:
        ok = "".join(ln + "\n" for i, ln in enumerate(text.splitlines()) if i != line and not ln.endswith("pull"))
        assert CU.offences(db, ok, U.orc_ovlp_match) == [], name


@pytest.mark.ref
@pytest.mark.skipif(not os.path.exists(os.path.join(U.REF_DIR, "libshimmer_ref.so")), reason="the compiled reference is not there")
def test_oracle_equals_the_reference_on_these_rows(engineered):
    c, db, ids = engineered
    rl, ro = db.by_rid()
    rng = np.random.default_rng(500)
    texts = ["c " + CU.pull_back(ids) + "\n", "c " + CU.pull_back(ids, "v500") + "\n"] + [t for _, t, _, _ in CU.error_paths(db, ids, CU.filler_contigs(c), U.orc_ovlp_match)[:4]]
    rows = [r for t in texts for r in CU.parse_path(t)[0]] + [c.rows[i] for i in rng.choice(len(c.rows), 500, replace=False)]
    for _, r0, s0, r1, s1, s, e, _line in rows:
        l0, l1 = int(rl[r0]), int(rl[r1])
        q, t = db.seqdb[int(ro[r0]) + l0 - 500:int(ro[r0]) + l0], db.seqdb[int(ro[r1]) + l1 - abs(e - s) - 500:int(ro[r1]) + l1]
        assert U.ref_ovlp_match(q, s0, t, s1, 100) == U.orc_ovlp_match(q, s0, t, s1, 100), (r0, s0, r1, s1, s, e)
    print("ovlp_match of the reference == the oracle's on %d rows" % len(rows))
