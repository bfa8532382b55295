"""The consensus call on the GPU (pgx_cns_tags, pgx_cns_call, pgx_cns_call_dev; peregrine_amd/csrc/pgx_cns.hip) against the stored answers
of the reference's own get_align_tags and get_cns_from_align_tags (tests/golden/cns_cases.npz): tags field by field, consensus byte for
byte.  The cases cross every window of the kernels: chunks of 64 columns and of 64 edges, the cut at delta 255, a template position with
more nodes than the scoring kernel's LDS ring holds, a piece of 8,400 bases, a batch of 64 pieces.  Nothing here runs the reference."""
import numpy as np
import pytest

import cns_util as CU
from peregrine_amd import _lib, shimmer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return CU.load_cases()


@pytest.fixture(scope="module")
def everything(cases):
    """all pieces of the fixture in one batch, per min_cov: (pieces, expected); the 65,535 alignments of edge_full_count run alone (case by
    case), here they would only slow the shuffles"""
    return CU.batches_by_min_cov(cases)


def test_tags_equal_the_reference_field_by_field(cases):
    alns = [a for c in cases for _, al in c.pieces for a in al]
    want = [t for c in cases for t in c.tags]
    got = shimmer.align_tags(alns)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (i, len(g), len(w))
        for f in CU.TAG_FIELDS:
            assert np.array_equal(g[f], w[f]), (i, f)


def test_consensus_equals_the_reference_case_by_case(cases):
    for c in cases:
        st = {}
        got = shimmer.consensus(c.pieces, c.min_cov, stats=st)
        assert got == c.cns, c.name
        assert st["n_aln"] == sum(len(al) for _, al in c.pieces) and st["n_tags"] == sum(len(t) for t in c.tags)
        assert st["text_bytes"] == sum(len(x) for x in c.cns) and st["n_nodes"] <= st["n_edges"] <= st["n_tags"]


def test_a_batch_equals_its_pieces_one_by_one(cases):
    c = next(c for c in cases if c.name == "batch64")
    assert shimmer.consensus(c.pieces, c.min_cov) == [shimmer.consensus([p], c.min_cov)[0] for p in c.pieces] == c.cns


def test_order_of_alignments_and_pieces_is_immaterial(everything):
    rng = np.random.default_rng(11)
    for min_cov, (pieces, want) in everything.items():
        order = rng.permutation(len(pieces))
        shuffled = [(pieces[i][0], [pieces[i][1][j] for j in rng.permutation(len(pieces[i][1]))]) for i in order]
        assert shimmer.consensus(shuffled, min_cov) == [want[i] for i in order], min_cov


def test_device_entry_equals_the_host_entry(everything):
    for min_cov, (pieces, want) in everything.items():
        assert shimmer.consensus(pieces, min_cov, on_device=True) == want, min_cov


def test_refusals_name_the_piece_and_leave_the_library_usable(cases):
    good = next(c for c in cases if c.name == "real_e05_t200_r3")
    t_len, alns = good.pieces[0]
    q, t, s1, s2, off = alns[1]
    lone = (q[:1], t[:1], s1, s2, off)                                  # one column: a node, no edge into it
    bad = {
        "no alignment path": (t_len, [lone]),
        "past the end of the template": (t_len - 1, alns),
        "negative t_offset": (t_len, alns + [(q, t, s1, s2, -1)]),
        "outside ACGTNacgtn-": (t_len, alns + [(q[:7] + b"." + q[8:], t, s1, s2, off)]),
    }
    for msg, piece in bad.items():
        for at in (0, 2):
            batch = [good.pieces[0]] * at + [piece] + [good.pieces[0]]
            with pytest.raises(_lib.PgxError, match=r"code %d\).*piece %d: .*%s" % (_lib.PGX_EINVAL, at, msg)):
                shimmer.consensus(batch)
        assert shimmer.consensus(good.pieces) == good.cns
    with pytest.raises(_lib.PgxError, match="no alignment path"):
        shimmer.consensus([(t_len, [])])
    many = (t_len, [alns[0]] * 65536)
    with pytest.raises(_lib.PgxError, match=r"code %d\).*piece 1: more than 65535 alignments" % _lib.PGX_EINVAL):
        shimmer.consensus([good.pieces[0], many])
    assert shimmer.consensus([(t_len, [alns[0]] * 300)]) == [CU.consensus(t_len, [alns[0]] * 300)]
    assert shimmer.consensus(good.pieces) == good.cns
    assert shimmer.consensus([]) == []
