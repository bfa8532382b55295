"""pgx_cns_pieces on the GPU against the fixture the real reference wrote: the consensus of every piece byte for byte, the accepted reads
flag for flag; a batch against its pieces one by one, any read order, the counts of its stats, its refusals."""
import ctypes as C

import numpy as np
import pytest

import aln_util as AU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shimmer():
    from peregrine_amd import shimmer
    return shimmer


def test_every_piece_case_is_the_references(shimmer):
    for pc in AU.load_cases()[1]:
        used, st = [], {}
        got = shimmer.consensus_reads(pc.pieces, pc.min_cov, stats=st, used=used)
        for p in range(len(pc.pieces)):
            assert got[p] == pc.cns[p], (pc.name, p, len(got[p]), len(pc.cns[p]))
            assert used[p].tolist() == pc.used[p].tolist(), (pc.name, p)
        n_reads = sum(len(r) for _, r in pc.pieces)
        assert st["n_pieces"] == len(pc.pieces) and st["n_reads"] == n_reads
        assert st["n_accepted"] == sum(int(u.sum()) for u in pc.used) and st["n_accepted"] + st["n_rejected"] == n_reads
        assert st["n_by_rule"] == sum(pc.by_rule) and st["n_by_rule"] + st["n_called"] == len(pc.pieces)
        assert st["align"]["n_req"] == len(pc.pieces) + n_reads
        assert st["call"]["n_aln"] == sum(1 + int(u.sum()) for u, r in zip(pc.used, pc.by_rule) if not r)


def test_a_batch_equals_its_pieces_one_by_one(shimmer):
    pc = next(c for c in AU.load_cases()[1] if c.name == "pieces_cov_edge")
    both = next(c for c in AU.load_cases()[1] if c.name == "pieces_shifts")
    pieces = pc.pieces + both.pieces
    whole = shimmer.consensus_reads(pieces, 1)
    for p, piece in enumerate(pieces):
        assert shimmer.consensus_reads([piece], 1) == [whole[p]], p
    assert whole == pc.cns + both.cns


def test_read_order_is_immaterial(shimmer):
    pc = next(c for c in AU.load_cases()[1] if c.name == "pieces_shifts")
    T, reads = pc.pieces[0]
    rng = np.random.default_rng(3)
    for _ in range(2):
        order = rng.permutation(len(reads)).tolist()
        used = []
        assert shimmer.consensus_reads([(T, [reads[i] for i in order])], 1, used=used) == pc.cns
        assert used[0].tolist() == [bool(pc.used[0][i]) for i in order]


def test_no_pieces_and_a_piece_without_reads(shimmer):
    assert shimmer.consensus_reads([]) == []
    T = b"ACGTTGCATGCATCGATCGATTTAGC" * 8
    assert shimmer.consensus_reads([(T, [])]) == [T.lower()]


def test_refusals_name_the_piece_and_the_next_call_works(shimmer):
    from peregrine_amd import _lib
    _lib.init()
    lib = _lib.load()
    T = b"ACGTTGCATGCATCGATCGATTTAGC" * 8
    seq = np.frombuffer(T, np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(pieces, reads):
        pc, rd = np.array(pieces, _lib.CNS_PIECE_DTYPE), np.array(reads, _lib.CNS_READ_DTYPE).reshape(-1)
        off, text = np.zeros(len(pc) + 1, np.uint64), C.c_void_p()
        rc = lib.pgx_cns_pieces(ptr(pc), len(pc), ptr(rd), len(rd), ptr(seq), len(seq), 1, C.byref(text), ptr(off), None, None)
        msg = lib.pgx_last_error().decode()
        out = C.string_at(text.value, int(off[-1])) if rc == 0 else None
        if rc == 0:
            lib.pgx_free(text)
        return rc, msg, out

    ok_piece = (0, len(T), 0)
    for pieces, reads, code, word in (([ok_piece, (0, 0, 0)], [], _lib.PGX_EINVAL, "piece 1"),
                                      ([ok_piece], [(0, 50, 1, 0, 0)], _lib.PGX_EARG, "read 0"),
                                      ([ok_piece], [(0, 50, 0, 0, 0), (200, 50, 0, 0, 0)], _lib.PGX_EARG, "read 1"),
                                      ([(100, len(T), 0)], [], _lib.PGX_EARG, "piece 0")):
        rc, msg, _ = call(pieces, reads)
        assert rc == code and word in msg and "pgx_cns_pieces" in msg, (pieces, reads, rc, msg)
        rc, msg, out = call([ok_piece], [(0, 50, 0, 0, 0)])
        assert rc == 0 and out == T.lower(), (rc, msg)
