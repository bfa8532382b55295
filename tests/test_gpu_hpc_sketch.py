"""mm_sketch with is_hpc = 1 on the GPU (pgx_sketch_hpc.hip), read by read: ResidentDB.sketch(hpc=True) / pgx_sketch_batch_hpc and the
exported mm_sketch(is_hpc=1) give the compiled reference's list element for element, on the directed and random strings of
tests/hpc_util.py (the reference itself where oracle/_ref is present, else its record in tests/golden/hpc_cases.npz).  All comparisons
are on integers and exact."""
import ctypes as C

import numpy as np
import pytest

import hpc_util as H
from peregrine_amd import _lib, formats
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu


class Work:
    """the fixture's strings as ONE database (read i = case i, offsets whatever the lengths make them) and the expected lists: made once"""

    def __init__(self):
        self.cases = H.golden_cases()
        self.db = H.seqdb_of([c.seq for c in self.cases])
        self.want = [H.expected_l0(c, i) for i, c in enumerate(self.cases)]
        self.groups = {}
        for i, c in enumerate(self.cases):
            self.groups.setdefault((c.w, c.k), []).append(i)
        self.rdb = ResidentDB(self.db, 0)


@pytest.fixture(scope="module")
def work():
    wk = Work()
    yield wk
    wk.rdb.close()


def _split(mm, slots):
    """a batch's list cut by read id, in the batch's order"""
    rid = (mm["y"] >> np.uint64(32)).astype(np.int64)
    assert np.all(np.diff(np.searchsorted(np.asarray(slots), rid)) >= 0)
    return {s: mm[rid == s] for s in slots}


def test_a_batch_of_many_reads(work):
    """every (w, k) group in one call: the lists in read order, each the reference's; the group holds reads at offsets off the 16-byte
    grid (one right after a read of 17 bases), runs across lane and tile boundaries, and reads that outgrow their slabs"""
    names = [c.name for c in work.cases]
    after = names.index("after_odd_length")
    assert names[after - 1] == "odd_length_17" and int(work.db.roff[after]) % 16 != 0 and len(work.groups) >= 10
    for (w, k), slots in work.groups.items():
        got = work.rdb.sketch(slots, w, k, hpc=True)
        want = np.concatenate([work.want[s] for s in slots])
        if not np.array_equal(got, want):
            parts = _split(got, slots)
            bad = [work.cases[s].name for s in slots if not np.array_equal(parts[s], work.want[s])]
            raise AssertionError(f"w={w} k={k}: {len(bad)} of {len(slots)} reads differ: {bad[:8]}")


def test_one_read_per_call_gives_the_same(work):
    """the output of a read does not depend on its neighbours in the launch"""
    for i, c in enumerate(work.cases):
        got = work.rdb.sketch([i], c.w, c.k, hpc=True)
        assert np.array_equal(got, work.want[i]), c.name


def test_a_permuted_batch(work):
    slots = work.groups[(H.W, H.K)][::-1]
    got = work.rdb.sketch(slots, H.W, H.K, hpc=True)
    assert np.array_equal(got, np.concatenate([work.want[s] for s in slots]))


class KV(C.Structure):
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


def test_the_exported_mm_sketch_answers_is_hpc(work):
    """the shimmer4py symbol on the ASCII strings themselves (mixed case included), appending to the vector it is given"""
    lib, libc = _lib.load(), C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    for i, c in enumerate(work.cases):
        v = KV()
        for _ in range(2 if c.name == "mixed_case" else 1):
            lib.mm_sketch(None, C.c_char_p(c.seq), C.c_int(len(c.seq)), C.c_int(c.w), C.c_int(c.k), C.c_uint32(i), C.c_int(1), C.byref(v))
        got = np.frombuffer((C.c_uint8 * (int(v.n) * 16)).from_address(v.a), dtype=formats.MM_DTYPE).copy() if v.n else np.zeros(0, formats.MM_DTYPE)
        if v.a:
            libc.free(C.c_void_p(v.a))
        want = work.want[i] if c.name != "mixed_case" else np.concatenate([work.want[i]] * 2)
        assert np.array_equal(got, want), c.name


def test_the_plain_sketch_is_what_it_was(work):
    """hpc=False in the same process, before and after hpc calls: the CPU oracle's list (strings without ambiguous bases or with)"""
    import oracle_util as U
    slots = work.groups[(H.W, H.K)][:40] + work.groups[(3, 4)][:10]
    for _ in range(2):
        for s in slots:
            c = work.cases[s]
            want = U.orc_sketch_seqdb(H.encode(c.seq), c.w, c.k, s)
            assert np.array_equal(work.rdb.sketch([s], c.w, c.k), want), c.name
        work.rdb.sketch(slots[:5], H.W, H.K, hpc=True)
