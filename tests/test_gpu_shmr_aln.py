"""The shimmer chain alignment on the GPU (pgx_shmr_aln_batch, shimmer.shimmer_alns / get_shimmer_alns) against the chains the real
shmr_aln wrote into tests/golden/shmr_aln_cases.npz and against the restatement of tests/shmr_aln_util.py, chain for chain: every fixture
case, seeded batches whose pairs share lists (in both pair orders), the chain state's second path, the refusals, two sequences sketched on
the device, and the script's return shape."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import cnsjob_util as J
import shmr_aln_util as A
from peregrine_amd import _lib, shimmer

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _as_lists(result):
    """shimmer_alns' answer as [[(idx0 list, idx1 list)]]"""
    return [[(a.tolist(), b.tolist()) for a, b in chains] for chains in result]


def _fixture_groups():
    """the fixture's cases grouped by their parameters (a call has one set): [(params, [case])]"""
    groups = {}
    for c in A.load_cases():
        groups.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(k), v) for k, v in groups.items()]


def _run_fixture(**env):
    n = 0
    for params, cases in _fixture_groups():
        st = {}
        with _env(**env):
            got = _as_lists(shimmer.shimmer_alns([c.mm0 for c in cases], [c.mm1 for c in cases], stats=st, **params))
        assert len(got) == len(cases)
        for c, chains in zip(cases, got):
            assert len(chains) == len(c.chains), c.name
            for k, (mine, ref) in enumerate(zip(chains, c.chains)):
                assert mine == ref, (c.name, k)
            if not env:   # ... and alone, a single array for side 0
                assert _as_lists(shimmer.shimmer_alns(c.mm0, [c.mm1], **params)) == [c.chains], c.name
        assert st["n_stopped"] == sum(c.name == "stop_4810" for c in cases)
        assert st["n_chains"] == sum(len(c.chains) for c in cases) and st["n_elems"] == sum(len(a) for c in cases for a, _ in c.chains)
        n += len(cases)
    return n


def test_every_fixture_case_equals_the_references_chains():
    assert _run_fixture() == len(A.load_cases()) >= 41


@pytest.mark.parametrize("lds", [0, 1, 64, 128])
def test_fixture_on_the_second_path(lds):
    """PGX_SHMR_ALN_LDS at its smallest value keeps every chain's state in the pair's slice; 64 and 128 put the boundary between the two
    inside the 129 live chains of best_*_of_129"""
    assert _run_fixture(PGX_SHMR_ALN_LDS=lds) == len(A.load_cases())


@pytest.fixture(scope="module")
def batch():
    """about 300 seeded pairs, sizes 0 .. 400, several pairs to a list 0, and the restatement's chains of each pair alone per max_repeat"""
    return A.seeded_batch()   # (shared with test_gpu_wave_reuse.py)


@pytest.mark.parametrize("max_repeat", [1, 2, 5])
def test_a_batch_equals_each_pair_alone(batch, max_repeat):
    lists0, lists1, pairs, want = batch
    got = _as_lists(shimmer.shimmer_alns(lists0, lists1, pairs, max_repeat=max_repeat))
    assert got == want[max_repeat]
    rev = _as_lists(shimmer.shimmer_alns(lists0, lists1, pairs[::-1], max_repeat=max_repeat))
    assert rev == want[max_repeat][::-1]
    with _env(PGX_SHMR_ALN_LDS=0):
        assert _as_lists(shimmer.shimmer_alns(lists0, lists1, pairs, max_repeat=max_repeat)) == want[max_repeat]
    with _env(PGX_SHMR_ALN_LDS=2):
        assert _as_lists(shimmer.shimmer_alns(lists0, lists1, pairs, max_repeat=max_repeat)) == want[max_repeat]


def test_the_arrays_of_both_paths_are_the_same(batch):
    """the four arrays as the C entry point hands them out, with the hook at its smallest value and without it"""
    lists0, lists1, pairs, _ = batch
    mm0, off0 = shimmer._pool_lists(lists0)
    mm1, off1 = shimmer._pool_lists(lists1)
    pr = np.zeros(len(pairs), _lib.SHMR_ALN_PAIR_DTYPE)
    pr["list0"], pr["list1"] = pairs[:, 0], pairs[:, 1]

    def arrays():
        outs = [C.c_void_p() for _ in range(4)]
        st = _lib.ShmrAlnStats()
        _lib.check(_lib.load().pgx_shmr_aln_batch(mm0.ctypes.data, off0.ctypes.data, len(lists0), mm1.ctypes.data, off1.ctypes.data, len(lists1), pr.ctypes.data, len(pr),
                                                  0, 100, 1200, 2, *[C.byref(o) for o in outs], C.byref(st)), "pgx_shmr_aln_batch")
        po = _lib.take(outs[0].value, len(pr) + 1, np.dtype("<u8")).copy()
        co = _lib.take(outs[1].value, int(po[-1]) + 1, np.dtype("<u8")).copy()
        return po, co, _lib.take(outs[2].value, int(co[-1]), np.dtype("<u4")).copy(), _lib.take(outs[3].value, int(co[-1]), np.dtype("<u4")).copy(), st

    a = arrays()
    with _env(PGX_SHMR_ALN_LDS=0):
        b = arrays()
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))
    assert a[0][0] == 0 and a[1][0] == 0 and a[4].n_pairs == 300 and a[4].n_chains == a[0][-1] and a[4].n_elems == a[1][-1] <= a[4].n_candidates


def test_refusals_and_the_empty_batch():
    c = next(c for c in A.load_cases() if c.name == "real_fwd")
    with pytest.raises(_lib.PgxError) as e:
        shimmer.shimmer_alns([c.mm0], [c.mm1], direction=1)
    assert "code -1" in str(e.value) and "direction 1" in str(e.value) and "one past the list" in str(e.value), str(e.value)
    for bad in ([(1, 0)], [(0, 1)], [(0, 0), (0, 2**32 - 1)], [(-1, 0)]):
        with pytest.raises(_lib.PgxError) as e:
            shimmer.shimmer_alns([c.mm0], [c.mm1], bad)
        assert "out of range" in str(e.value), str(e.value)
    assert shimmer.shimmer_alns([], []) == [] and shimmer.shimmer_alns([c.mm0], [c.mm1], []) == []
    assert shimmer.shimmer_alns(c.mm0, []) == []
    outs = [C.c_void_p() for _ in range(4)]
    off = np.zeros(1, np.uint64)
    _lib.check(_lib.load().pgx_shmr_aln_batch(None, off.ctypes.data, 0, None, off.ctypes.data, 0, None, 0, 0, 100, 1200, 1, *[C.byref(o) for o in outs], None),
               "pgx_shmr_aln_batch")
    po, co = _lib.take(outs[0].value, 1, np.dtype("<u8")), _lib.take(outs[1].value, 1, np.dtype("<u8"))
    assert po.tolist() == [0] and co.tolist() == [0] and all(o.value for o in outs)
    assert len(_lib.take(outs[2].value, 0, np.dtype("<u4"))) == 0 and len(_lib.take(outs[3].value, 0, np.dtype("<u4"))) == 0
    null = [C.c_void_p(5) for _ in range(4)]   # a null argument: refused, the outputs untouched
    rc = _lib.load().pgx_shmr_aln_batch(None, None, 0, None, off.ctypes.data, 0, None, 0, 0, 100, 1200, 1, *[C.byref(o) for o in null], None)
    assert rc == _lib.PGX_EARG and [o.value for o in null] == [5] * 4
    # a list of 2^31 entries, offsets that decrease, offsets that do not start at 0: refused on the offsets alone, before a byte of the lists is read
    one = np.zeros(1, A.MM_DTYPE)
    pr = np.zeros(1, _lib.SHMR_ALN_PAIR_DTYPE)
    good = np.array([0, 1], np.uint64)
    for bad_off, word in ((np.array([0, 2**31], np.uint64), "2^31"), (np.array([0, 5, 3], np.uint64), "decrease"), (np.array([1, 2], np.uint64), "start at 0")):
        for side in (0, 1):
            offs = [good, good]
            offs[side] = bad_off
            rc = _lib.load().pgx_shmr_aln_batch(one.ctypes.data, offs[0].ctypes.data, len(offs[0]) - 1, one.ctypes.data, offs[1].ctypes.data, len(offs[1]) - 1,
                                                pr.ctypes.data, 1, 0, 100, 1200, 1, *[C.byref(o) for o in null], None)
            assert rc == _lib.PGX_EARG and word in _lib.load().pgx_last_error().decode() and [o.value for o in null] == [5] * 4, (word, side)
    # ... and the library goes on
    assert _as_lists(shimmer.shimmer_alns([c.mm0], [c.mm1])) == [c.chains]


def test_from_sequences_the_planted_shift():
    """the template and its shifted, substituted copy (no indels) sketched and reduced on the device: the lists are the fixture's, and the
    first pair of the longest chain gives exactly the planted shift"""
    T, Cp, _ = A.real_sequences()
    R = A.REAL
    rdb = shimmer.ResidentDB(J.db_of([T, Cp], ["template", "copy"]), 0)
    try:
        lists = [shimmer.mm_reduce(shimmer.mm_reduce(rdb.sketch([slot], R["w"], R["k"]), R["r"]), R["r"]) for slot in (0, 1)]
    finally:
        rdb.close()
    fx = next(c for c in A.load_cases() if c.name == "real_fwd")
    low = np.uint64(0xFFFFFFFF)
    for mine, ref in zip(lists, (fx.mm0, fx.mm1)):   # (the fixture's lists carry other read ids)
        assert np.array_equal(mine["x"], ref["x"]) and np.array_equal(mine["y"] & low, ref["y"] & low)
    alns = shimmer.get_shimmer_alns(lists[0], lists[1])
    alns.sort(key=lambda x: -len(x[0]))
    first = alns[0][0][0]
    assert len(alns[0][0]) >= 20 and first[0][3] - first[1][3] == -R["shift"]   # (utils.py:149: read_offset)


def test_get_shimmer_alns_has_the_scripts_shape_and_numbers():
    for name in ("real_fwd", "rand_02_a12_r5", "tie_earlier", "no_shared"):
        c = next(c for c in A.load_cases() if c.name == name)
        got = shimmer.get_shimmer_alns(c.mm0, c.mm1, 0, **c.params)
        assert len(got) == len(c.chains), name
        for (chain, mx, mean, mn), (i0, i1) in zip(got, c.chains):
            want = [(A.mmer2tuple(c.mm0["x"][a], c.mm0["y"][a]), A.mmer2tuple(c.mm1["x"][b], c.mm1["y"][b])) for a, b in zip(i0, i1)]
            assert chain == want, name
            w = A.script_numbers(want)
            assert (mx, mean, mn) == w and [type(v) for v in (mx, mean, mn)] == [type(v) for v in w], name
            assert mx == mn == want[-1][0][3] - want[-1][1][3]
