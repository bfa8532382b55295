"""The second item a workgroup takes.  The persistent kernels of the library stride over their items (`for (i = blockIdx.x; i < n;
i += gridDim.x)`) with a grid capped at a multiple of the CU count, and keep LDS tables, register carries and slices of global scratch
from one item to the next.  No other test call is larger than such a grid on a 256-CU device, so the hand-over between items runs here:
under PGX_GRID_CAP = 1 and 3 (pgx_internal.h: stride_grid / grid_cap; 1 = one workgroup takes every item, in order) on the inputs and
against the expectations of the kernels' own tests, and without the hook on inputs of more than three grids.  PGX_SKETCH_BATCH cuts
the sketch launches into batches the same way.  Every comparison is exact, on integers or bytes; the expected values are the compiled
reference's where oracle/_ref is present, else the golden fixtures', the CPU oracle's and the restatements' of tests/*_util.py.

Every capped run first shows, from a count made on the CPU, that the list its kernel walks holds at least 3 * cap items, and that
pgx_stride_grid answers the cap; every natural-size run that its call is more than twice the grid pgx_stride_grid reports.

kernel               grid (CUs x)   largest other test call                       second item reached by
k_sketch_hpc         16             1,133 reads (test_gpu_hpc_downstream)         test_hpc_*, test_batches_*
k_sketch_general     16             ~525 reads (test_gpu_shimmer_params)          test_general_*, test_batches_*
k_aln_bound/_walk/
  _lens/_unroll      8              300 pairs (test_gpu_shmr_aln)                 test_shmr_aln_*
k_sg_tr_lds          32             <= 720 nodes                                  test_string_graph, test_chimer_step
k_sg_tr_global       32             the nodes beyond PGX_SGRAPH_DEG_MAX           the same two, hooks = "global"
k_sg_chimer_lds      32             <= 842 candidates                             test_chimer_step
k_sg_chimer_global   <= 64 slices   a few listed candidates                       test_chimer_step, hooks = "global" (every candidate)
k_align1_list        32             the hand-on lists of 39 .. 123 pairs          test_align1_list
k_pack_reads         64             ~3,300 reads (test_gpu_eval_big_walk's sets)  test_pack_reads
k_eval_big           512 in all     9,434 buckets of 3 .. 128 entries in one      the tests of test_gpu_eval_big_walk.py under
                     (no CU term)   window: family8 of test_gpu_eval_big_walk.py  PGX_REPLAY_BIG=2 (18 buckets a workgroup); the count is
                                                                                  asserted, and the cap run, by
                                                                                  test_a_workgroup_walks_many_buckets there
"""
import contextlib
import os

import numpy as np
import pytest

import chimer_util as CU
import dedup_graph_util as DG
import hpc_util as H
import oracle_util as U
import sgraph_util as SG
import shmr_aln_util as A
import test_gpu_align_narrow_groups as NG
import test_gpu_align_wide_steps as W
from peregrine_amd import _lib, formats, shimmer
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu

CAPS = (1, 3)
GENERAL = (24, 12)   # a (w, k) of k_sketch_general (the wave kernel takes k = 16 with w = 64, 80, 96, 128)


# ---- the hooks -----------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(**kw):
    """environment variables for the block; None takes one out"""
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _grid(n_items, per_cu):
    _lib.init()
    return int(_lib.load().pgx_stride_grid(int(n_items), int(per_cu)))


@contextlib.contextmanager
def capped(cap, n_items, **env):
    """PGX_GRID_CAP = cap around a call of n_items items: at least three to a workgroup, and the hook holds for every kernel's factor"""
    assert n_items >= 3 * cap, (n_items, cap)
    with _env(PGX_GRID_CAP=cap, **env):
        assert [_grid(2**40, x) for x in (1, 8, 16, 32, 64)] == [cap] * 5
        yield


def test_the_grid_hook():
    """without the variable a grid is min(items, CUs * per_cu), as every launch site wrote it by hand before; with it, at most the cap;
    the variable is read at every call; what is no positive integer caps nothing"""
    import torch
    _lib.init()
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    with _env(PGX_GRID_CAP=None):
        for x in (8, 16, 32, 64):
            assert _grid(2**40, x) == cu * x and _grid(cu * x + 1, x) == cu * x and _grid(cu * x - 1, x) == cu * x - 1
        assert _grid(5, 16) == 5 and _grid(0, 16) == 0
        for c in (1, 3, 7):
            with _env(PGX_GRID_CAP=c):
                assert all(_grid(2**40, x) == c for x in (8, 16, 32, 64)) and _grid(2, 16) == min(2, c) and _grid(0, 8) == 0
            assert _grid(2**40, 16) == cu * 16
        for junk in ("0", "-3", "", "x"):
            with _env(PGX_GRID_CAP=junk):
                assert _grid(2**40, 16) == cu * 16


# ---- a. k_sketch_hpc -------------------------------------------------------------------------------------------------------------------
class Hpc:
    """the fixture's strings as one database (read i = case i) with the expected hpc lists, the w = 80, k = 16 strings as a database of
    their own (for the index stage), and the natural-size tiling: made once, never changed"""

    def __init__(self):
        self.cases = H.golden_cases()
        self.db = H.seqdb_of([c.seq for c in self.cases])
        self.want = [H.expected_l0(c, i) for i, c in enumerate(self.cases)]
        self.groups = {}
        for i, c in enumerate(self.cases):
            self.groups.setdefault((c.w, c.k), []).append(i)
        self.rdb = ResidentDB(self.db, 0)
        self.main = [self.cases[i] for i in self.groups[(H.W, H.K)]]
        self.main_db = H.seqdb_of([c.seq for c in self.main])
        self.main_want = [H.expected_l0(c, i) for i, c in enumerate(self.main)]
        self.main_rdb = ResidentDB(self.main_db, 0)
        self._plain = {}
        self._big = None

    def plain(self, slot, w, k):
        """the CPU oracle's plain list of read `slot` of the whole database at (w, k)"""
        if (slot, w, k) not in self._plain:
            self._plain[(slot, w, k)] = U.orc_sketch_seqdb(H.encode(self.cases[slot].seq), w, k, slot)
        return self._plain[(slot, w, k)]

    def big(self):
        """3 grids + 7 reads: the w = 80, k = 16 strings of at most 600 bases, tiled in a seeded permutation, rid = position"""
        if self._big is None:
            grid = _grid(2**40, 16)
            n = 3 * grid + 7
            small = [c for c in self.main if len(c.seq) <= 600]
            assert len(small) >= 50 and any(b"N" in c.seq for c in small) and any(len(c.seq) == 1 for c in small)
            pick = np.random.default_rng(20261201).permutation(np.resize(np.arange(len(small)), n))
            enc = [H.encode(c.seq) for c in small]
            rlen = np.array([len(enc[i]) for i in pick], np.uint32)
            roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
            db = formats.SeqDB(np.concatenate([enc[i] for i in pick]), np.arange(n, dtype=np.uint32), rlen, roff, None)
            self._big = (grid, n, small, pick, ResidentDB(db, 0))
        return self._big

    def close(self):
        self.rdb.close(), self.main_rdb.close()
        if self._big:
            self._big[4].close()


@pytest.fixture(scope="module")
def hpc():
    h = Hpc()
    yield h
    h.close()


def _cat(parts):
    return np.concatenate(parts) if len(parts) else np.zeros(0, formats.MM_DTYPE)


def _same(got, want_parts, names):
    """got == the lists back to back; a failure names the reads"""
    want = _cat(want_parts)
    if np.array_equal(got, want):
        return
    at, bad = 0, []
    for name, part in zip(names, want_parts):
        if not np.array_equal(got[at:at + len(part)], part):
            bad.append(name)
        at += len(part)
    raise AssertionError(f"{len(got)} elements against {len(want)}; reads that differ where the expected list puts them: {bad[:8]}")


def _at_least(slots, n):
    """the slots repeated until there are n of them (a read may be listed more than once)"""
    return list(slots) * -(-n // len(slots))


@pytest.mark.parametrize("cap", CAPS)
def test_hpc_every_group(hpc, cap):
    """every (w, k) group of the fixture through k_sketch_hpc, `cap` workgroups for the whole group (cap 1: one wavefront sketches it in
    order); a group of fewer than 3 * cap reads is listed several times over"""
    assert len(hpc.groups) >= 10
    for (w, k), slots in hpc.groups.items():
        slots = _at_least(slots, 3 * cap)
        with capped(cap, len(slots)):
            got = hpc.rdb.sketch(slots, w, k, hpc=True)
        _same(got, [hpc.want[s] for s in slots], [hpc.cases[s].name for s in slots])


def _outgrows(case):
    return len(case.l0) > len(case.seq) // 8 + 64   # (the slab of the first pass: slab_offsets(reads, 8, 64))


def _directed_order(hpc):
    """the w = 80, k = 16 group in the fixture's order with `NN` moved in front of the 1,400-base read"""
    slots = list(hpc.groups[(H.W, H.K)])
    name = {s: hpc.cases[s].name for s in slots}
    nn = next(s for s in slots if name[s] == "NN")
    slots.remove(nn)
    slots.insert(next(i for i, s in enumerate(slots) if name[s] == "straddles_lane_and_tile"), nn)
    return slots


def _adjacencies(hpc, slots):
    """what stands directly in front of what, in the order `slots`"""
    c = [hpc.cases[s] for s in slots]
    found = set()
    for a, b in zip(c[:-1], c[1:]):
        if b"N" in a.seq and b"N" not in b.seq:
            found.add("N before none")
        if len(a.seq) == 1 and len(b.seq) >= 500:
            found.add("one base before a long read")
        if a.seq == b"NN" and len(b.seq) >= 500:
            found.add("NN before a long read")
        if _outgrows(a) and not _outgrows(b):
            found.add("outgrown slab before one that holds")
        if b"N" in a.seq and a.seq.rstrip(b"N") != a.seq and b"N" not in b.seq:
            found.add("ends in N before none")
    return found


@pytest.mark.parametrize("order", ["directed", "reversed", "permuted"])
@pytest.mark.parametrize("cap", CAPS)
def test_hpc_main_group_orders(hpc, cap, order):
    """the 98 reads of w = 80, k = 16 (56.8 kb, 40 with N) in three orders.  What a wavefront carries from read to read -- nr, carry_code,
    ns, l_carry, open, carry, nout -- matters where neighbours differ; the directed order holds, and this test asserts: a read with N
    directly before one without (l_carry, the segment state); a read that ends in N before one without; a read of one base, and `NN`,
    directly before a read of 500 bases and more (nr, ns of nearly nothing before many); a read that outgrows its slab directly before
    one that does not (nout beyond the capacity, the flag)."""
    slots = _directed_order(hpc)
    if order == "directed":
        assert _adjacencies(hpc, slots) == {"N before none", "one base before a long read", "NN before a long read", "outgrown slab before one that holds",
                                            "ends in N before none"}
    elif order == "reversed":
        slots = slots[::-1]
    else:
        slots = [slots[i] for i in np.random.default_rng(98).permutation(len(slots))]
    assert len(slots) == 98 and sum(b"N" in hpc.cases[s].seq for s in slots) == 40
    with capped(cap, len(slots)):
        got = hpc.rdb.sketch(slots, H.W, H.K, hpc=True)
    _same(got, [hpc.want[s] for s in slots], [hpc.cases[s].name for s in slots])


LOW = ("low_complexity_AC", "low_complexity_AAC", "low_complexity_then_w_N", "low_complexity_N_inside_then_w_N")


def test_hpc_redo_pass_on_one_wavefront(hpc):
    """the index stage on the w = 80, k = 16 strings: four reads outgrow len / 8 + 64 and are sketched again from a list into slabs of
    exactly their size; under cap 1 one wavefront takes all four, one after the other"""
    redo = [c.name for c in hpc.main if _outgrows(c)]
    assert redo == list(LOW)
    with capped(1, len(redo)):
        a = hpc.main_rdb.index(levels=1, want_l0=True, hpc=True)
    assert a.reads_literal >= 4 and a.reads == len(hpc.main)
    _same(a.l0, hpc.main_want, [c.name for c in hpc.main])


def test_hpc_more_reads_than_three_grids(hpc):
    """no hook: 3 * (16 workgroups a CU) + 7 reads, so every workgroup takes three and some a fourth"""
    grid, n, small, pick, rdb = hpc.big()
    assert n > 2 * grid and "PGX_GRID_CAP" not in os.environ and _grid(n, 16) == grid
    got = rdb.sketch(np.arange(n), H.W, H.K, hpc=True)
    want = [H.expected_l0(small[i], rid) for rid, i in enumerate(pick.tolist())]
    _same(got, want, [f"{rid}:{small[i].name}" for rid, i in enumerate(pick.tolist())])


# ---- b. k_sketch_general, and the run-by-run path behind it ----------------------------------------------------------------------------
@pytest.mark.parametrize("cap", CAPS)
def test_general_every_group(hpc, cap):
    """the same strings through the plain sketch at the fixture's (w, k) other than (80, 16): k_sketch_general, and for the reads it flags
    (an ambiguous base, a slab outgrown) dev_sketch_nreads, whose sketch launches obey the cap too; against the CPU oracle"""
    n_amb = 0
    for (w, k), slots in hpc.groups.items():
        if (w, k) == (H.W, H.K):
            continue
        n_amb += sum(b"N" in hpc.cases[s].seq for s in slots)
        slots = _at_least(slots, 3 * cap)
        with capped(cap, len(slots)):
            got = hpc.rdb.sketch(slots, w, k)
        _same(got, [hpc.plain(s, w, k) for s in slots], [hpc.cases[s].name for s in slots])
    assert n_amb >= 30


def test_general_more_reads_than_three_grids(hpc):
    """no hook: the natural-size tiling through k_sketch_general at w = 24, k = 12"""
    grid, n, small, pick, rdb = hpc.big()
    assert n > 2 * grid and "PGX_GRID_CAP" not in os.environ and _grid(n, 16) == grid
    w, k = GENERAL
    got = rdb.sketch(np.arange(n), w, k)
    base = [U.orc_sketch_seqdb(H.encode(c.seq), w, k, 0) for c in small]
    want = [small[i].with_rid(base[i], rid) for rid, i in enumerate(pick.tolist())]
    assert sum(len(b) for b in base) > 500
    _same(got, want, [f"{rid}:{small[i].name}" for rid, i in enumerate(pick.tolist())])


# ---- c. batches ------------------------------------------------------------------------------------------------------------------------
BATCH_CASES = [(2000, None), (2000, 1), (1, None)]   # (bases per batch, grid cap; with a read per batch a cap has nothing to cap)


def _hpc_batches(lens, batch):
    """launch_sketch_hpc's cut: a read opens a batch when the batch's scratch (len + 1 a read) and the read pass `batch`"""
    first, acc = [0], 0
    for i, n in enumerate(lens):
        if i > first[-1] and acc + n > batch:
            first.append(i)
            acc = 0
        acc += n + 1
    return first


def _general_batches(lens, batch):
    """launch_sketch_general's cut: reads join a batch while its bases stay within `batch`; a longer read is a batch of its own"""
    first, i = [], 0
    while i < len(lens):
        first.append(i)
        acc, j = 0, i
        while j < len(lens) and (j == i or acc + lens[j] <= batch):
            acc += lens[j]
            j += 1
        i = j
    return first


@pytest.mark.parametrize("batch,cap", BATCH_CASES)
def test_batches_hpc(hpc, batch, cap):
    """PGX_SKETCH_BATCH = 2000 bases on the w = 80, k = 16 strings: the first pass takes its reads in batches (slot0 = b0, the scratch offsets
    from d_so + b0), and the four low-complexity reads, each a batch of its own, make the redo launch run its list form with
    b0 = 1, 2, 3 (d_list + b0, d_slab_off + b0).  1: every read is a batch."""
    lens = [len(c.seq) for c in hpc.main]
    redo = [len(c.seq) for c in hpc.main if _outgrows(c)]
    first, again = _hpc_batches(lens, batch), _hpc_batches(redo, batch)
    assert len(redo) == 4 and min(redo) >= 2000 and again == [0, 1, 2, 3]   # (2,000 bases and their scratch do not leave room for a second read)
    assert len(first) >= 10 and len(again) >= 3
    if batch == 1:
        assert len(first) == len(lens)
    with _env(PGX_SKETCH_BATCH=batch), (capped(cap, len(redo)) if cap else contextlib.nullcontext()):
        a = hpc.main_rdb.index(levels=1, want_l0=True, hpc=True)
    assert a.reads_literal >= 4
    _same(a.l0, hpc.main_want, [c.name for c in hpc.main])


@pytest.mark.parametrize("batch,cap", BATCH_CASES)
def test_batches_general(hpc, batch, cap):
    """the same strings in batches through k_sketch_general (w = 24, k = 12): the list form with b0 > 0 (d_list + b0 of the identity list),
    and dev_sketch_nreads' own batches of the runs between ambiguous bases"""
    slots = hpc.groups[(H.W, H.K)]
    w, k = GENERAL
    assert len(_general_batches([len(hpc.cases[s].seq) for s in slots], batch)) >= 10
    with _env(PGX_SKETCH_BATCH=batch), (capped(cap, len(slots)) if cap else contextlib.nullcontext()):
        got = hpc.rdb.sketch(slots, w, k)
    _same(got, [hpc.plain(s, w, k) for s in slots], [hpc.cases[s].name for s in slots])


# ---- d. pgx_shmr_aln_batch ---------------------------------------------------------------------------------------------------------------
def _as_lists(result):
    return [[(a.tolist(), b.tolist()) for a, b in chains] for chains in result]


def _aln_groups():
    """the fixture's cases by their parameters (a call has one set), each a list of (name, mm0, mm1, expected chains).  The group of
    stop_4810 (max_diff 100, max_repeat 1) is ordered so that stop_4810 has pairs on both sides, and best_65_of_129 -- 129 live chains,
    here under this group's parameters, its chains the restatement's -- stands directly behind it."""
    groups = {}
    for c in A.load_cases():
        groups.setdefault(tuple(sorted(c.params.items())), []).append((c.name, c.mm0, c.mm1, c.chains))
    out = []
    for key, cases in groups.items():
        params = dict(key)
        names = [c[0] for c in cases]
        if "stop_4810" in names:
            b = next(c for c in A.load_cases() if c.name == "best_65_of_129")
            chains = A.shmr_aln(b.mm0, b.mm1, **params)[0]
            assert len(chains) > 64
            cases.insert(names.index("stop_4810") + 1, ("best_65_of_129", b.mm0, b.mm1, chains))
        out.append((params, cases))
    return out


ALN_LDS = [None, 0, 2, 64]


@pytest.mark.parametrize("lds", ALN_LDS, ids=lambda v: f"lds{v}")
@pytest.mark.parametrize("cap", CAPS)
def test_shmr_aln_fixture(cap, lds):
    """the 41 fixture cases, a call per parameter set, in both pair orders.  Under cap 1 one wavefront walks stop_4810 -- 4,802 chains:
    the LDS head of 1,024 full, the rest in the pair's slice, the walk stopped by the count -- between two other pairs, and then
    best_65_of_129; small, last_small, the chain count and the LDS head of the pair before must not reach the pair behind."""
    n = 0
    for params, cases in _aln_groups():
        names = [c[0] for c in cases]
        if "stop_4810" in names:
            at = names.index("stop_4810")
            assert 0 < at and names[at + 1] == "best_65_of_129" and at + 2 < len(names) and len(cases[at][3]) == 4802
        order = _at_least(range(len(cases)), 3 * cap)
        for pairs in (order, order[::-1]):
            st = {}
            with capped(cap, len(pairs), PGX_SHMR_ALN_LDS=lds):
                got = _as_lists(shimmer.shimmer_alns([c[1] for c in cases], [c[2] for c in cases], [(i, i) for i in pairs], stats=st, **params))
            for i, chains in zip(pairs, got):
                assert chains == cases[i][3], (names[i], params, len(chains), len(cases[i][3]))
            assert st["n_stopped"] == sum(names[i] == "stop_4810" for i in pairs)
        if "stop_4810" in names:
            assert st["n_stopped"] == 1
        n += len(cases)
    assert n == len(A.load_cases()) + 1 >= 42


@pytest.mark.parametrize("lds", ALN_LDS, ids=lambda v: f"lds{v}")
@pytest.mark.parametrize("cap", CAPS)
def test_shmr_aln_seeded_batch(cap, lds):
    """the 300 seeded pairs of test_gpu_shmr_aln.py (sizes 0 .. 400, several pairs to a list) at max_repeat 1, 2, 5, in both orders"""
    lists0, lists1, pairs, want = A.seeded_batch()
    for mr in (1, 2, 5):
        for rev in (False, True):
            pr = pairs[::-1] if rev else pairs
            with capped(cap, len(pr), PGX_SHMR_ALN_LDS=lds):
                got = _as_lists(shimmer.shimmer_alns(lists0, lists1, pr, max_repeat=mr))
            assert got == (want[mr][::-1] if rev else want[mr]), (mr, rev)


@pytest.mark.parametrize("lds", [None, 2], ids=lambda v: f"lds{v}")
def test_shmr_aln_more_pairs_than_three_grids(lds):
    """no grid hook: the 300 pairs repeated and permuted to 3 * (8 workgroups a CU) + 5 pairs over the same lists"""
    lists0, lists1, pairs, want = A.seeded_batch()
    grid = _grid(2**40, 8)
    n = 3 * grid + 5
    pick = np.random.default_rng(20261202).permutation(np.resize(np.arange(len(pairs)), n))
    assert n > 2 * grid and "PGX_GRID_CAP" not in os.environ and _grid(n, 8) == grid
    with _env(PGX_SHMR_ALN_LDS=lds):
        got = _as_lists(shimmer.shimmer_alns(lists0, lists1, pairs[pick], max_repeat=2))
    bad = [int(p) for p, g in zip(pick.tolist(), got) if g != want[2][p]]
    assert not bad, (len(bad), bad[:8])


# ---- e. string graph -------------------------------------------------------------------------------------------------------------------
SG_HOOKS = {"lds": {}, "global": dict(PGX_SGRAPH_DEG_MAX=3, PGX_SGRAPH_CHIMER_LDS=0)}
_graphs = {}


def _out_degrees(edges):
    """out-edges per node that has any, from the expected edge records"""
    return np.unique(edges["v_rid"].astype(np.int64) * 2 + edges["v_end"], return_counts=True)[1]


def _plain_graph():
    if "plain" not in _graphs:
        recs = DG.make_records(seed=11, n_reads=120, genome=3000, contained_share=0.2)
        _graphs["plain"] = (recs,) + SG.string_graph_of_full_text(U.orc_dedup(recs)[0], 2000, 96.0)
    return _graphs["plain"]


def _chimer_graph():
    if "chimer" not in _graphs:
        recs = CU.chimeric_sim(seed=23, n_reads=360, genome=120_000, n_chimers=100)
        _graphs["chimer"] = (recs,) + CU.string_graph_of_full_text(U.orc_dedup(recs)[0], 2000, 96.0)
    return _graphs["chimer"]


@pytest.mark.parametrize("hooks", list(SG_HOOKS))
@pytest.mark.parametrize("cap", CAPS)
def test_string_graph(cap, hooks):
    """the transitive reduction on the records of test_gpu_sgraph.py against the restatement: k_sg_tr_lds over every node, and with
    PGX_SGRAPH_DEG_MAX = 3 k_sg_tr_global over the listed nodes of more than 3 out-edges, several to a workgroup: the tables of the
    node before (LDS; the marks in HBM) are the next node's"""
    recs, want, edges, stats = _plain_graph()
    deg = _out_degrees(edges)
    n_items = int((deg > 3).sum()) if hooks == "global" else len(deg)
    with capped(cap, n_items, **SG_HOOKS[hooks]):
        with shimmer.string_graph(recs, 2000, 96.0, piece=777) as g:
            assert g.stats == stats
            assert b"".join(g.text(1 << 20)) == want and np.array_equal(g.edges(), edges)


@pytest.mark.parametrize("hooks", list(SG_HOOKS))
@pytest.mark.parametrize("cap", CAPS)
def test_chimer_step(cap, hooks):
    """the chimer bridge step on the simulated chimeric reads of test_gpu_sgraph_chimer.py: 842 candidates through k_sg_chimer_lds; with
    PGX_SGRAPH_CHIMER_LDS = 0 every one of them is handed on to k_sg_chimer_global, and under cap 1 they all share one ChGlobal slice: a tag
    that an earlier candidate left valid, or an LDS table that was not reset, changes chimers_nodes"""
    recs, want, edges, stats, ch, nodes = _chimer_graph()
    assert ch["chosen"] >= 20 and ch["past_test1"] > ch["chosen"]
    n_items = min(ch["candidates"], int((_out_degrees(edges) > 3).sum())) if hooks == "global" else ch["candidates"]
    with capped(cap, n_items, **SG_HOOKS[hooks]):
        with shimmer.string_graph(recs, 2000, 96.0, piece=777, chimer_ordered=True) as g:
            assert g.stats == stats and g.chimer_stats == ch
            assert g.chimers_nodes() == nodes
            assert b"".join(g.text(1 << 20)) == want and np.array_equal(g.edges(), edges)


# ---- f. k_align1_list, k_pack_reads ----------------------------------------------------------------------------------------------------
BAND, ITER_LIMIT = 100, 100
ALIGN_FORMS = {   # id -> (environment, database, whose hand-on list is counted)
    "handon": (dict(PGX_ALIGN_SMALL="1000000000"), "compacted", "flagged"),
    "stragglers": (dict(NG.GROUPED, PGX_ALIGN_GL="4", PGX_ALIGN_ITER_LIMIT=str(ITER_LIMIT)), "plain", "slow"),
    "compacted-stragglers": (dict(NG.GROUPED, PGX_ALIGN_GL="4", PGX_ALIGN_ITER_LIMIT=str(ITER_LIMIT)), "compacted", "slow of each kind"),
}


@pytest.fixture(scope="module")
def align_sets():
    """the pairs of test_gpu_align_narrow_groups.py as a plain and as a compacted database (every third target holds a base without a
    2-bit code), the oracle's matches, and per pair whether the packed kernel's model needs more than twice the iteration budget"""
    pairs, runs, _ = NG._cpu()
    slow = np.array([NG.model_match(r, BAND, 4)[1]["iters"] >= 2 * ITER_LIMIT for r in runs])
    out = {}
    for name, amb in (("plain", False), ("compacted", True)):
        db, keys = NG._build(pairs, ambiguous=amb)
        rdb = ResidentDB(db, 0)
        want = W._oracle_matches(db, keys, BAND)
        if amb:
            rdb.align(keys, BAND)   # (a first launch builds the packs)
            assert rdb.compact_bytes() is True and not rdb.has_bytes and rdb.side_bytes > 0
        out[name] = (rdb, keys, want)
    yield out, slow
    for rdb, _, _ in out.values():
        rdb.close()


@pytest.mark.parametrize("form", list(ALIGN_FORMS))
@pytest.mark.parametrize("cap", CAPS)
def test_align1_list(align_sets, cap, form):
    """k_align1_list from its three launch sites, the hand-on forced as test_gpu_align_* force it: the candidates on reads with ambiguous
    bases of a small launch on a compacted database (the list: every key that names a flagged read); the stragglers of the packed grouped
    launch past PGX_ALIGN_ITER_LIMIT (the list: at least the pairs whose model run, which test_gpu_align_narrow_groups.py holds to the
    oracle, takes twice the budget); both kinds on a compacted database, where the flagged pairs run the byte-wise form first (half
    the codes an iteration of the packed form's, so no fewer iterations).  The V ring in LDS is the candidate's before.
    The length of the "handon" list is exact.  The lengths of the straggler lists are a SUPPOSITION: the library reports no count of
    the candidates it hands on, the model's results are held to the oracle but its iteration count is held to nothing, and the
    byte-wise form's count is an argument, not a measurement; the factor 2 is the margin for both.  Were fewer pairs handed on, these
    two forms would pass without a second candidate on a wavefront; the "handon" form would not."""
    sets, slow = align_sets
    env, which, kind = ALIGN_FORMS[form]
    rdb, keys, want = sets[which]
    order = np.random.default_rng(5).permutation(np.tile(np.arange(len(keys)), 3))
    flagged = (order % 3 == 0) if which == "compacted" else np.zeros(len(order), bool)
    if kind == "flagged":
        n_list = int(flagged.sum())
    else:
        n_list = min(int((slow[order] & f).sum()) for f in ((flagged, ~flagged) if which == "compacted" else (~flagged,)))
    with capped(cap, n_list, **env):
        got = rdb.align(keys[order], BAND)
    for f in NG.FIELDS:
        bad = np.flatnonzero(got[f] != want[order][f])
        assert len(bad) == 0, (form, f, len(bad), keys[order][bad[:3]], got[bad[:3]], want[order][bad[:3]])
    assert (want["m_size"] > 0).any() and (want["m_size"] == 0).any()


@pytest.mark.parametrize("cap", CAPS)
def test_pack_reads(cap):
    """k_pack_reads on the reads of test_unpacked_reads_equal_the_file_at_every_length_and_phase (1 .. 70 bases and around the 1,024-base
    step, every offset mod 16, one read with ambiguous bases): the packs are built under the cap, the database compacted, and every read
    unpacked is byte for byte the file's; only the flagged read went to the side store"""
    rng = np.random.default_rng(77)
    lens = list(range(1, 71)) + [1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 16385, 65535]
    seqs = [bytes(b"ACGT"[x] for x in rng.integers(0, 4, n)) for n in lens]
    amb = bytearray(bytes(b"ACGT"[x] for x in rng.integers(0, 4, 500)))
    amb[0] = amb[250] = ord("N")
    seqs.insert(3, bytes(amb))
    db = H.seqdb_of(seqs)
    assert len(set(int(o) % 16 for o in db.roff)) == 16
    rdb = ResidentDB(db, 0)
    try:
        with capped(cap, len(seqs)):
            assert rdb.compact_bytes() is True   # (builds the packs)
        assert not rdb.has_bytes and 0 < rdb.side_bytes <= 500 + 64 + 4096
        for r, s in enumerate(seqs):
            got = rdb.read_bytes(r, len(s))
            assert np.array_equal(got, H.encode(s)), (r, len(s), int(db.roff[r]) % 16, np.flatnonzero(got != H.encode(s))[:5])
    finally:
        rdb.close()
