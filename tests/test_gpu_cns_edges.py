"""The consensus call on the GPU (peregrine_amd/csrc/pgx_cns.hip) where tests/test_gpu_cns.py does not reach: rows in the layouts a device
aligner leaves (interleaved across pieces, strings scattered among foreign bytes, strings shared), the scoring ring and the back-track
window at their exact sizes and at a nonzero node base, the order of ties for every pair of letters, the column scan at the edges of its
chunks, batches around the block size of the per-piece kernels, a random differential, and every checked refusal of the row contract.
Expected values: the reference's own answers stored in tests/golden/cns_cases.npz (edge_*), elsewhere the restatement of tests/cns_util.py
that the fixture's generator holds against the reference.  edge_full_count (65,535 alignments in one piece) runs alone, in
test_gpu_cns.py's case-by-case test.  Nothing here runs the reference."""
import numpy as np
import pytest

import cns_util as CU
from peregrine_amd import _lib, shimmer

pytestmark = pytest.mark.gpu

ENTRIES = ("pgx_cns_call", "pgx_cns_call_dev")
WINDOWS = ["edge_ring_1023", "edge_ring_1024", "edge_ring_1025", "edge_back_2047", "edge_back_2048", "edge_back_2049",
           "edge_back_end_2047", "edge_back_end_2048", "edge_back_end_2049"]


@pytest.fixture(scope="module")
def by():
    return {c.name: c for c in CU.load_cases()}


@pytest.fixture(scope="module")
def everything(by):
    """all pieces of the fixture but edge_full_count's in one batch per min_cov: (pieces, expected)"""
    return CU.batches_by_min_cov(by.values())


def no_live_cns_bytes():
    _lib.mem_ledger(reset_peak=True)                      # the peak becomes what is live now
    return "cns" not in _lib.mem_ledger()["peak_by_tag"]


# ---- 1. the windows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WINDOWS)
def test_window_edges_alone_and_at_a_nonzero_node_base(by, name):
    """two nodes of the case are the named number of places apart (test_cns_rule.py asserts it).  edge_ring_*: (59, 0) and (60, 0); the
    predecessor's score comes out of the ring at <= 1024 and out of memory beyond.  edge_back_end_*: (118, 0) and the end node (119, 0),
    the top of the back-track's first window; the predecessor is the window's lowest slot at 2047 and outside it from 2048.  edge_back_*:
    (59, 0) and (60, 0) again, 59 nodes below the end node: a jump of that length from the middle of the first window, which always
    leaves it.  Alone the piece's nodes start at 0; behind three other pieces they start where `ring[cur & 1023]` and
    `lo = max(first, ..)` see other values."""
    c = by[name]
    for entry in ENTRIES:
        st = {}
        assert CU.call_rows(*CU.rows_of(c.pieces), c.min_cov, entry, stats=st) == c.cns, entry
        assert st["n_nodes"] == len(CU.distinct_keys(c.pieces[0][1]))
    lead = [by["real_e05_t200_r3"], by["hand_tie"], by["backbone"]]
    assert all(x.min_cov == c.min_cov == 1 for x in lead)
    base = sum(len(CU.distinct_keys(x.pieces[0][1])) for x in lead)
    assert base % 1024 != 0
    for entry in ENTRIES:
        st = {}
        got = CU.call_rows(*CU.rows_of([x.pieces[0] for x in lead] + c.pieces), 1, entry, stats=st)
        assert got == [x.cns[0] for x in lead] + c.cns, entry
        assert st["n_nodes"] == base + len(CU.distinct_keys(c.pieces[0][1]))


# ---- 2. row layouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("layout", ["interleaved", "scattered", "shared"])
def test_rows_in_any_layout_give_the_fixtures_answers(everything, layout, entry):
    rng = np.random.default_rng(17)
    assert set(everything) >= {0, 1, 2, 3, 65535, 2**31 - 1}
    for min_cov, (pieces, want) in everything.items():
        rows, q_str, t_str, tlen = CU.rows_of(pieces, layout, rng)
        n_bytes = sum(len(a[0]) for _, alns in pieces for a in alns)
        if layout == "scattered":
            assert len(q_str) > n_bytes and (len(rows) < 10 or (np.diff(rows["str_off"].astype(np.int64)) < 0).any())
        else:
            assert len(rows) < 10 or (np.diff(rows["piece"].astype(np.int64)) < 0).any()      # the pieces do interleave
            assert len(q_str) == n_bytes or (layout == "shared" and len(q_str) < n_bytes)
            assert min_cov != 1 or (len(q_str) < n_bytes) == (layout == "shared")
        assert CU.call_rows(rows, q_str, t_str, tlen, min_cov, entry) == want, min_cov


# ---- 3. the column scan at the edges of its chunks ---------------------------------------------------------------------------------------
def assert_tags_equal(alns):
    got = shimmer.align_tags(alns)
    assert len(got) == len(alns)
    for i, (g, a) in enumerate(zip(got, alns)):
        w = CU.align_tags(*a)
        assert len(g) == len(w), (i, len(g), len(w))
        for f in CU.TAG_FIELDS:
            assert np.array_equal(g[f], w[f]), (i, f)


def test_tags_of_insertions_at_every_chunk_edge():
    """an insertion of m bases after c matched columns, then 70 matches: the run starts and ends on either side of a chunk of 64 columns,
    the cut at delta 255 (m >= 255) falls wherever c puts it; t_offset = 5 and s2 = 2, so that c = 0 -- a leading insertion -- has tags"""
    rng = np.random.default_rng(3)
    T = CU.random_template(rng, 300)
    alns = [CU.build(T, 5, 2, [("=", c), ("I", CU.random_template(rng, m, CU.LETTERS)), ("=", 70)])
            for c in (0, 1, 62, 63, 64, 65, 127, 128) for m in (1, 63, 64, 65, 128, 254, 255, 256)]
    assert len(alns) == 64 and len(CU.align_tags(*alns[0])) == 71 and len(CU.align_tags(*alns[6])) == 254
    assert_tags_equal(alns)


def test_tags_of_every_length_without_gaps():
    T = CU.random_template(np.random.default_rng(4), 140)
    assert_tags_equal([CU.build(T, 3, 1, [("=", n)]) for n in range(131)])


# ---- 4. random differential -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_pieces():
    """seeds 1000 .. 1599 -> per min_cov = seed % 3: (pieces, the restatement's consensus); the number the restatement refused"""
    out, refused = {0: ([], []), 1: ([], []), 2: ([], [])}, 0
    for s in range(1000, 1600):
        rng = np.random.default_rng(s)
        t_len = int(rng.integers(40, 401))
        n_reads = int(rng.integers(1, 7))
        rate = float(rng.choice([0.02, 0.12, 0.3]))
        piece = CU.synthetic_piece(rng, t_len, n_reads, rate=rate)
        try:
            want = CU.consensus(*piece, min_cov=s % 3)
        except CU.Refused:
            refused += 1
            continue
        out[s % 3][0].append(piece)
        out[s % 3][1].append(want)
    return out, refused


@pytest.mark.parametrize("min_cov", [0, 1, 2])
def test_random_pieces_equal_the_restatement(random_pieces, min_cov):
    """600 pieces of 40 .. 400 bases, 1 .. 6 reads, 2, 12 and 30 % difference: the restatement refuses none of them (and the reference
    agreed with it on all 600 when this test was written)"""
    batches, refused = random_pieces
    assert refused == 0
    pieces, want = batches[min_cov]
    assert len(pieces) == 200
    assert CU.call_rows(*CU.rows_of(pieces, "packed"), min_cov, "pgx_cns_call") == want
    assert CU.call_rows(*CU.rows_of(pieces, "interleaved", np.random.default_rng(min_cov)), min_cov, "pgx_cns_call_dev") == want


# ---- 5. batch shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_pieces():
    """the first 1,031 pieces in seed order (from 5000) that the restatement answers: a template of 12 .. 40 bases, its back-bone and one
    or two reads; their consensus, their node counts, the seeds tried"""
    pieces, want, nodes, tried = [], [], [], 0
    while len(pieces) < 1031:
        rng = np.random.default_rng(5000 + tried)
        tried += 1
        piece = CU.synthetic_piece(rng, int(rng.integers(12, 41)), int(rng.integers(1, 3)))
        try:
            want.append(CU.consensus(*piece, min_cov=1))
        except CU.Refused:
            continue
        pieces.append(piece)
        nodes.append(len(CU.distinct_keys(piece[1])))
    return pieces, want, nodes, tried


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1031])
def test_batches_around_the_block_size_of_the_per_piece_kernels(small_pieces, n):
    """the per-piece kernels run in blocks of 256 threads over n (k_cns_piece_check) and n + 1 (k_cns_piece_bounds) pieces, the second sort
    takes 1, 1, 2, 8, 8, 9 and 11 bits of the piece; synthetic_piece at its own rate of 0.12"""
    pieces, want, nodes, tried = small_pieces
    assert tried - len(pieces) <= tried // 20, (tried, len(pieces))
    for entry in ENTRIES:
        st = {}
        assert CU.call_rows(*CU.rows_of(pieces[:n]), 1, entry, stats=st) == want[:n], entry
        assert st["n_nodes"] == sum(nodes[:n]) and st["n_aln"] == sum(len(p[1]) for p in pieces[:n])


# ---- 6. refusals and argument errors ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good(by):
    """eight pieces as interleaved rows, and their answers"""
    c = by["batch64"]
    pieces = c.pieces[:8]
    return pieces, CU.rows_of(pieces, "interleaved", np.random.default_rng(23)), c.cns[:8]


def refused(good, code, pattern, rows, q_str, t_str, tlen, **kw):
    """both entries refuse with this code and message; afterwards the library answers a good batch and holds no memory of the call"""
    for entry in ENTRIES:
        with pytest.raises(_lib.PgxError, match=r"%s failed \(code %d\).*%s" % (entry, code, pattern)):
            CU.call_rows(rows, q_str, t_str, tlen, 1, entry, **kw)
        assert no_live_cns_bytes()
        assert CU.call_rows(*good[1], 1, entry) == good[2]
        assert no_live_cns_bytes()


def test_rows_that_name_no_piece_or_no_string_are_argument_errors(good):
    pieces, (rows, q_str, t_str, tlen), _ = good
    assert len(rows) > 6 and len(tlen) == 8
    bad = rows.copy()
    bad["piece"][[5, 2]] = len(tlen)
    refused(good, _lib.PGX_EARG, "alignment 2 names a piece beyond the 8 given", bad, q_str, t_str, tlen)
    bad = rows.copy()
    bad["str_off"][[5, 2]] = np.uint64(len(q_str) + 1) - bad["str_len"][[5, 2]].astype(np.uint64)      # one byte past the end
    refused(good, _lib.PGX_EARG, "the strings of alignment 2 lie outside the %d bytes given" % len(q_str), bad, q_str, t_str, tlen)
    bad = rows.copy()
    bad["str_off"][[5, 2]] = 2**64 - 1                                                         # str_off + str_len wraps
    refused(good, _lib.PGX_EARG, "the strings of alignment 2 lie outside", bad, q_str, t_str, tlen)
    more = np.concatenate([rows, rows[:1]])
    more["str_off"][-1], more["str_len"][-1] = len(q_str), 0                                   # an empty string at the very end is inside
    for entry in ENTRIES:
        assert CU.call_rows(more, q_str, t_str, tlen, 1, entry) == good[2]


def test_argument_errors_of_the_host_side(good):
    pieces, (rows, q_str, t_str, tlen), _ = good
    refused(good, _lib.PGX_EARG, "alignments without pieces", rows[:1], q_str, t_str, np.zeros(0, np.uint32))
    big = tlen.copy()
    big[3] = 2**31
    refused(good, _lib.PGX_EARG, "piece 3: a template of 2147483648 bases", rows, q_str, t_str, big)
    refused(good, _lib.PGX_EARG, "more than 1048576 pieces", rows, q_str, t_str, np.full(2**20 + 1, 100, np.uint32))
    refused(good, _lib.PGX_EARG, "null argument", rows, q_str, t_str, tlen, null_text=True)
    for entry in ENTRIES:
        assert CU.call_rows(rows[:0], q_str[:0], t_str[:0], np.zeros(0, np.uint32), 1, entry) == []


def with_bad_byte(piece, k):
    """the piece with a '.' in column k of its last alignment's read string"""
    t_len, alns = piece
    q, t, s1, s2, off = alns[-1]
    assert k < len(q)
    return t_len, alns[:-1] + [(q[:k] + b"." + q[k + 1:], t, s1, s2, off)]


def test_an_argument_error_goes_before_a_piece_the_reference_cannot_answer(good):
    pieces, _, _ = good
    rows, q_str, t_str, tlen = CU.rows_of(pieces[:6] + [with_bad_byte(pieces[6], 7)] + pieces[7:], "interleaved", np.random.default_rng(29))
    refused(good, _lib.PGX_EINVAL, "piece 6: an alignment string holds a byte outside", rows, q_str, t_str, tlen)
    i = int(np.flatnonzero(rows["piece"] != 6)[3])
    rows["piece"][i] = len(tlen)
    refused(good, _lib.PGX_EARG, "alignment %d names a piece beyond" % i, rows, q_str, t_str, tlen)


def test_columns_after_the_cut_are_checked_for_bytes_but_not_for_the_template_end(good):
    """what CU.check_piece and CU.consensus do: a foreign byte anywhere in a string refuses the piece, columns that yield no tag cannot
    run past the template"""
    pieces, _, _ = good
    rng = np.random.default_rng(31)
    T = CU.random_template(rng, 120)
    full = CU.build(T, 0, 0, [("=", 120)])
    ins = CU.random_template(rng, 300)
    long_ins = CU.build(T, 0, 0, [("=", 10), ("I", ins), ("=", 110)])
    assert len(CU.align_tags(*long_ins)) == 264
    bad = (120, [full, full, long_ins])
    piece = with_bad_byte(bad, 290)                                       # after the cut at column 264
    with pytest.raises(CU.Refused, match="outside"):
        CU.check_piece(*piece)
    refused(good, _lib.PGX_EINVAL, "piece 0: an alignment string holds a byte outside", *CU.rows_of([piece]))
    # the same refusal in pieces 7 and 4 of an interleaved batch names piece 4
    batch = pieces[:4] + [piece] + pieces[5:7] + [with_bad_byte(pieces[7], 3)]
    refused(good, _lib.PGX_EINVAL, "piece 4: an alignment string holds a byte outside", *CU.rows_of(batch, "interleaved", np.random.default_rng(37)))
    # 10 matched columns, 300 inserted bases, then 200 columns over a template that has only 110 left
    over = (T[:10] + ins + (T + T)[10:210], T[:10] + b"-" * 300 + (T + T)[10:210], 0, 0, 0)
    piece = (120, [full, full, over])
    want = CU.consensus(*piece)
    assert len(CU.align_tags(*over)) == 264 and want.upper() == T
    for entry in ENTRIES:
        assert CU.call_rows(*CU.rows_of([piece]), 1, entry) == [want]
    assert no_live_cns_bytes()
