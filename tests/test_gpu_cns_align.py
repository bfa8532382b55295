"""pgx_falcon_align on the GPU against the fixture the real reference wrote (tests/golden/aln_cases.npz): every stored case field by field
and string by string, alone and in one batch, shuffled, with mixed want_str; its strings through the consensus call; its refusals."""
import ctypes as C

import numpy as np
import pytest

import aln_util as AU
import cns_util as CU

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shimmer():
    from peregrine_amd import shimmer
    return shimmer


def small(cases):
    return [c for c in cases if max(len(c.q), len(c.t)) <= AU.BIG]


def pairs_of(cases):
    return [(c.q, c.t, c.band) for c in cases]


def check(cases, got, what):
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g[:6] == c.answer[:6], (what, c.name, g[:6], c.answer[:6])
        assert g[6] == c.answer[6] and g[7] == c.answer[7], (what, c.name, "strings")


def test_every_case_alone(shimmer):
    cases = AU.load_cases()[0]
    for c in cases:
        check([c], shimmer.falcon_align([(c.q, c.t)], band=c.band, want_str=c.want_str), "alone")


def test_all_cases_in_one_batch(shimmer):
    cases = AU.load_cases()[0]
    st = {}
    check(cases, shimmer.falcon_align(pairs_of(cases), want_str=[c.want_str for c in cases], stats=st), "batch")
    assert st["n_req"] == len(cases) and st["n_aligned"] == sum(c.exit == AU.EXIT_END for c in cases)
    assert st["str_bytes"] == sum(len(c.answer[6]) for c in cases)
    info, cells = {}, 0
    for c in cases:
        if c.want_str and c.exit == AU.EXIT_END:
            AU.align(c.q, c.t, c.band, True, info)
            cells += info["cells"]
    assert st["n_cells"] == cells          # the trace kept is the trace used


def test_a_shuffled_batch_is_the_shuffle_of_the_answers(shimmer):
    cases = small(AU.load_cases()[0])
    rng = np.random.default_rng(5)
    for _ in range(2):
        order = rng.permutation(len(cases)).tolist()
        some = [cases[i] for i in order]
        check(some, shimmer.falcon_align(pairs_of(some), want_str=[c.want_str for c in some]), "shuffled")


def test_mixed_want_str(shimmer):
    cases = small(AU.load_cases()[0])
    rng = np.random.default_rng(6)
    want = (rng.random(len(cases)) < 0.5).tolist()
    got = shimmer.falcon_align(pairs_of(cases), want_str=want)
    for c, w, g in zip(cases, want, got):
        ref = AU.align(c.q, c.t, c.band, w)[0]
        assert g == ref, (c.name, w, g[:6], ref[:6])
    none = shimmer.falcon_align(pairs_of(cases), want_str=False)
    assert all(g[6:] == (b"", b"") and g[:6] == AU.align(c.q, c.t, c.band, False)[0][:6] for c, g in zip(cases, none))


def test_its_strings_through_the_consensus_call_are_the_stored_consensus(shimmer):
    for pc in AU.load_cases()[1]:
        todo = [p for p in range(len(pc.pieces)) if not pc.by_rule[p]]
        pieces = []
        for p in todo:
            T, reads = pc.pieces[p]
            aligner = lambda q, t, band: shimmer.falcon_align([(q, t)], band=band)[0]
            alns, _, used = AU.piece_alignments(T, reads, aligner)
            assert used == pc.used[p].tolist(), (pc.name, p)
            pieces.append((len(T), alns))
            if pc.name == "pieces_batch32" and len(pieces) == 4:      # (a few of the many are enough here: test_gpu_cns_pieces runs them all)
                break
        assert shimmer.consensus(pieces, pc.min_cov) == [pc.cns[p] for p in todo[:len(pieces)]], pc.name


def test_empty_batch_and_empty_pairs(shimmer):
    assert shimmer.falcon_align([]) == []
    assert shimmer.falcon_align([(b"", b""), (b"A", b""), (b"", b"A"), (b"A", b"A"), (b"AC", b"AC")]) == [AU.ZERO] * 4 + [(2, 0, 0, 2, 0, 2, b"AC", b"AC")]


def test_refusals_name_what_they_refuse_and_the_next_call_works(shimmer):
    from peregrine_amd import _lib
    _lib.init()
    lib = _lib.load()
    seq = np.frombuffer(b"ACGTACGTAC", np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(rows, n=None):
        reqs = np.array(rows, _lib.FALN_REQ_DTYPE)
        res = np.zeros(len(reqs), _lib.FALN_RES_DTYPE)
        q, t, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        rc = lib.pgx_falcon_align(ptr(reqs), len(reqs) if n is None else n, ptr(seq), len(seq), ptr(res), C.byref(q), C.byref(t), C.byref(nb), None)
        msg = lib.pgx_last_error().decode()
        if rc == 0:
            lib.pgx_free(q); lib.pgx_free(t)
        return rc, msg, res

    good = (0, 0, 10, 10, 150, 1)
    for rows, code, word in (([good, (5, 0, 6, 10, 150, 1)], _lib.PGX_EARG, "request 1"), ([(0, 11, 1, 0, 150, 1), good], _lib.PGX_EARG, "request 0"),
                             ([good, good, (0, 0, 10, 10, 4097, 1)], _lib.PGX_EARG, "request 2"), ([(1 << 40, 0, 1, 1, 150, 1)], _lib.PGX_EARG, "request 0")):
        rc, msg, _ = call(rows)
        assert rc == code and word in msg and "pgx_falcon_align" in msg, (rows, rc, msg)
        rc, msg, res = call([good])
        assert rc == 0 and res[0]["aln_str_size"] == 10 and res[0]["aln_q_e"] == 10
    rc, msg, _ = call([good], n=1 << 31)
    assert rc == _lib.PGX_EARG and "too many" in msg
    rc, msg, res = call([(0, 0, 10, 10, 4096, 1)])
    assert rc == 0 and res[0]["aln_t_e"] == 10
    # what cannot be asked through one pool of 10 bytes: q_len + t_len >= 2^31 is refused by its range first; the library still runs
    assert shimmer.falcon_align([(b"ACGT", b"ACGT")])[0][:2] == (4, 0)
