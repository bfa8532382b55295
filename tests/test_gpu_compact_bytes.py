"""A read database with ambiguous bases, COMPACTED (pgx_seqdb_compact_bytes, pgx_side.hip): the whole-seqdb bytes leave HBM, the 2-bit packs
serve what they can, the flagged reads' bytes stay in a side store and the byte-wise kernels read a byte view (side store + partners rebuilt
from the packs by k_unpack_reads).  Every list, stream and alignment equals the oracle's, bit for bit, as in test_gpu_parity.py."""
import contextlib
import os

import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    saved = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _enc(codes):
    codes = np.asarray(codes, np.uint8)
    return ((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4))).astype(np.uint8)


def _with_ambiguous(codes, positions, both=True):
    e = _enc(codes).copy()
    _make_ambiguous(e, positions, both)
    return e


def _make_ambiguous(e, positions, both=True):
    """in place, on the biseq bytes of ONE read: both nibbles of a base zero (its forward nibble and its mirror image on the reverse strand), or
    -- both=False -- the forward nibble only"""
    n = len(e)
    for p in positions:
        e[p] &= 0xF0 if not both else 0x00
        if both:
            e[n - 1 - p] &= 0x0F


def _read(db, r):
    return db.seqdb[int(db.roff[r]):int(db.roff[r]) + int(db.rlen[r])]


N_FLAGGED = 200   # of ~2,000 reads: ~18 % of the overlap records then touch exactly one flagged read and ~1 % two


def stage_set():
    """the read set of test_index_and_overlap_from_the_packs_and_with_the_bytes_released (500 kb genome, 24x, seed 47) with N_FLAGGED reads
    given ambiguous bases: at the read start, the read end, mid-read as a run of 40, and on the forward strand only, in turn.
    Returns (db, flagged idx-file slots)."""
    g = simreads.make_genome(500_000, 19, repeat_families=2, repeat_len=4000, repeat_copies=6, tandem=60)
    db = simreads.simulate_reads(g, seed=47, coverage=24, mean_len=6000, sd_len=3000, min_len=200)
    sd = db.seqdb.copy()
    rng = np.random.default_rng(4711)
    long_enough = np.flatnonzero(db.rlen >= 400)
    slots = np.sort(rng.choice(long_enough, N_FLAGGED, replace=False))
    for j, s in enumerate(slots):
        o, n = int(db.roff[s]), int(db.rlen[s])
        e = sd[o:o + n]
        kind = j % 4
        if kind == 0:
            _make_ambiguous(e, [0, 1, 2])
        elif kind == 1:
            _make_ambiguous(e, [n // 2 + 7])      # (its mirror image lands near the middle too; the read END is flagged on the forward strand:)
            _make_ambiguous(e, [n - 1], both=False)
        elif kind == 2:
            _make_ambiguous(e, range(n // 3, n // 3 + 40))
        else:
            _make_ambiguous(e, [int(rng.integers(0, n))], both=False)
    return formats.SeqDB(sd, db.rid, db.rlen, db.roff, None), slots


def oracle_lists(db, T, levels):
    out = {}
    for c in range(1, T + 1):
        l = np.concatenate([U.orc_sketch_seqdb(_read(db, r), 80, 16, int(db.rid[r])) for r in np.flatnonzero(db.rid % T == c % T)])
        for _ in range(levels):
            l = U.orc_reduce(l, 6)
        out[c] = l
    return out


def flagged_record_counts(ov, flagged_rids):
    f = np.zeros(int(max(flagged_rids.max(), (ov["y0"] >> np.uint64(32)).max(), (ov["y1"] >> np.uint64(32)).max())) + 1, bool)
    f[flagged_rids] = True
    k = f[(ov["y0"] >> np.uint64(32)).astype(np.int64)].astype(int) + f[(ov["y1"] >> np.uint64(32)).astype(np.int64)].astype(int)
    return int((k == 1).sum()), int((k == 2).sum())


def _ledger_now():
    _lib.mem_ledger(reset_peak=True)   # (the peak starts again from now: peak_by_tag is the live bytes by owner)
    return _lib.mem_ledger()["peak_by_tag"]


def test_stage_parity_on_a_compacted_database():
    """Index lists and overlap streams of a database with 200 flagged reads, before and after compaction, against the oracle; the streams under
    the device and the host replay, with grouped launches + stragglers and with everything on k_align1.  The whole-seqdb bytes leave the
    ledger, the side store stays within length + 64 per flagged read + 4 KiB, and what needs the whole bytes says so."""
    db, slots = stage_set()
    flagged_rids = db.rid[slots]
    T = 2
    want_l2, want_l1 = oracle_lists(db, T, 2), oracle_lists(db, T, 1)
    mm = np.concatenate([want_l2[c] for c in (1, 2)])
    mc = U.orc_count(mm)
    want_ov = {c: U.orc_overlap(db, mm, mc, mychunk=c, total=3)[0] for c in (1, 3)}
    one = two = 0
    for c in (1, 3):
        a, b = flagged_record_counts(want_ov[c], flagged_rids)
        one, two = one + a, two + b
    print(f"oracle streams of chunks 1 and 3: {sum(len(v) for v in want_ov.values())} records, {one} with exactly one flagged read, {two} with two")
    assert one >= 50 and two >= 5          # (a condition on the input)

    rdb = ResidentDB(db, 0)

    def check_lists(tag):
        for c in (1, 2):
            assert np.array_equal(rdb.index(total_chunk=T, mychunk=c).top, want_l2[c]), (tag, c)
            assert np.array_equal(rdb.index(total_chunk=T, mychunk=c, levels=1).top, want_l1[c]), (tag, c, "levels=1")

    def check_streams(tag):
        for env in (dict(PGX_GPU_REPLAY="1"), dict(PGX_GPU_REPLAY="0"),
                    dict(PGX_GPU_REPLAY="1", PGX_ALIGN_SMALL="0", PGX_ALIGN_PACKED_MIN="0", PGX_ALIGN_ITER_LIMIT="300"),   # grouped launches + stragglers
                    dict(PGX_GPU_REPLAY="1", PGX_ALIGN_SMALL="1000000000")):                                             # everything through k_align1
            with _env(**env):
                for c in (1, 3):
                    got, _ = rdb.overlap(mm, mc, total_chunk=3, mychunk=c)
                    assert formats.ovlp_fields_equal(got, want_ov[c]), (tag, env, c)

    check_lists("bytes")
    check_streams("bytes")
    assert rdb.release_bytes() is False and rdb.has_bytes and rdb.side_bytes == 0
    assert _ledger_now().get("seqdb.bytes", 0) >= len(db.seqdb)
    assert rdb.compact_bytes() is True and not rdb.has_bytes
    bound = int(db.rlen[slots].sum()) + 64 * len(slots) + 4096
    print(f"side store: {rdb.side_bytes} bytes for {len(slots)} flagged reads of {int(db.rlen[slots].sum())} bases (bound {bound}); seqdb {len(db.seqdb)} bytes")
    assert 0 < rdb.side_bytes <= bound
    led = _ledger_now()
    assert led.get("seqdb.bytes", 0) == 0 and 0 < led.get("seqdb.side", 0), led
    check_lists("compacted")
    check_streams("compacted")
    assert rdb.compact_bytes() is True and not rdb.has_bytes      # (idempotent)
    assert rdb.release_bytes() is True                            # (released already: nothing to refuse)
    for call in (lambda: rdb.index(want_l0=True), lambda: rdb.index(window=64), lambda: rdb.sketch(np.arange(4, dtype=np.uint32), 80, 16)):
        with pytest.raises(_lib.PgxError):
            call()
    check_lists("compacted, after the refused calls")
    rdb.close()


def _oracle_matches(db, keys, band):
    out = np.zeros(len(keys), _lib.MATCH_DTYPE)
    for i in range(len(keys)):
        a, b = int(keys["rid0"][i]), int(keys["rid1"][i])
        q = db.seqdb[int(db.roff[a]) + int(keys["q_off"][i]):int(db.roff[a]) + int(db.rlen[a])]
        t = db.seqdb[int(db.roff[b]):int(db.roff[b]) + int(db.rlen[b])]
        out[i] = U.orc_ovlp_match(q, int(keys["dir0"][i]), t, int(keys["dir1"][i]), band)
    return out


def _small_set_with_flagged_reads():
    db = simreads.make_workload("small")
    sd = db.seqdb.copy()
    rng = np.random.default_rng(23)
    flagged = np.sort(rng.choice(db.n_reads, 40, replace=False))
    for j, r in enumerate(flagged):
        o, n = int(db.roff[r]), int(db.rlen[r])
        _make_ambiguous(sd[o:o + n], [0, n - 1] if j % 3 == 0 else rng.integers(0, n, 3), both=j % 3 != 1)
    db.seqdb = sd
    assert np.array_equal(db.rid, np.arange(db.n_reads))
    return db, flagged


def _hand_made_keys(db, flagged, seed):
    """true overlaps of the set (query x target flagged or not, as they come) + hand-made ones: {flagged, unflagged} query x {flagged, unflagged}
    target x both strands of either x q_off 0 and mid-read"""
    rng = np.random.default_rng(seed)
    plain = np.setdiff1d(np.arange(db.n_reads), flagged)
    rows = []
    for qs, ts in ((flagged, flagged), (flagged, plain), (plain, flagged), (plain, plain)):
        for d0 in (0, 1):
            for d1 in (0, 1):
                for mid in (False, True):
                    for _ in range(6):
                        a, b = int(rng.choice(qs)), int(rng.choice(ts))
                        rows.append((a, b, int(rng.integers(1, int(db.rlen[a]))) if mid else 0, d0, d1))
    for a in flagged[:10]:          # a read against itself: a long match straight through the ambiguous bases (zero nibbles compare equal)
        rows.append((int(a), int(a), 0, 0, 0)), rows.append((int(a), int(a), 0, 1, 1))
    keys = np.zeros(len(rows), _lib.ALIGN_KEY_DTYPE)
    for i, (a, b, q, d0, d1) in enumerate(rows):
        keys["rid0"][i], keys["rid1"][i], keys["q_off"][i], keys["dir0"][i], keys["dir1"][i] = a, b, q, d0, d1
    return keys


def test_alignment_keys_on_a_compacted_database():
    """ResidentDB.align with keys that pair flagged and unflagged reads every way, and the true overlaps of the set, against the oracle's
    ovlp_match: below the k_align1 threshold (k_align1_handon -> k_align1_list on the byte view) and above it (k_align_ph on the packs -> the
    byte-wise k_align_ph on the byte view -> both straggler lists)."""
    db, flagged = _small_set_with_flagged_reads()
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    ov, _ = rdb.overlap(ix.top, ix.top_mc)
    true = np.zeros(len(ov), _lib.ALIGN_KEY_DTYPE)
    true["rid0"] = ov["y0"] >> np.uint64(32); true["rid1"] = ov["y1"] >> np.uint64(32)
    true["q_off"] = (((ov["y0"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1)) - ((ov["y1"] & np.uint64(0xFFFFFFFF)) >> np.uint64(1))).astype(np.uint32)
    true["dir0"] = ov["strand0"]; true["dir1"] = ov["strand1"]
    isf = np.zeros(db.n_reads, bool); isf[flagged] = True
    touching = true[isf[true["rid0"]] | isf[true["rid1"]]]
    assert len(touching) >= 20
    keys = np.concatenate([_hand_made_keys(db, flagged, 5), touching[:300], true[:300]])
    want = {band: _oracle_matches(db, keys, band) for band in (100, 20)}
    assert rdb.compact_bytes() is True and not rdb.has_bytes and rdb.side_bytes > 0
    for env in (dict(PGX_ALIGN_SMALL="1000000000"), dict(PGX_ALIGN_SMALL="0"), dict(PGX_ALIGN_SMALL="0", PGX_ALIGN_ITER_LIMIT="150"), dict()):
        with _env(**env):
            for band in (100, 20):
                got = rdb.align(keys, band)
                bad = np.flatnonzero(got != want[band])
                assert len(bad) == 0, (env, band, len(bad), keys[bad[:3]], got[bad[:3]], want[band][bad[:3]])
    # ---- k_unpack_reads, directly: the rebuilt bytes of unflagged reads (and the side store's of flagged ones) are the file's
    for r in list(flagged[:5]) + list(np.setdiff1d(np.arange(db.n_reads), flagged)[:40]):
        got = rdb.read_bytes(int(r), int(db.rlen[r]))
        assert np.array_equal(got, _read(db, r)), (int(r), int(db.rlen[r]), np.flatnonzero(got != _read(db, r))[:5])
    rdb.close()


def test_unpacked_reads_equal_the_file_at_every_length_and_phase():
    """k_unpack_reads on reads of 1 .. 70 bases and around the 1,024-base step, at every seqdb offset mod 16 (the slot rule keeps that phase),
    next to one flagged read: byte for byte the seqdb's."""
    rng = np.random.default_rng(77)
    lens = list(range(1, 71)) + [1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4100, 16385, 65535]
    enc = [_enc(rng.integers(0, 4, n).astype(np.uint8)) for n in lens]
    enc.insert(3, _with_ambiguous(rng.integers(0, 4, 500).astype(np.uint8), [0, 250]))
    rlen = np.array([len(e) for e in enc], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    db = formats.SeqDB(np.concatenate(enc), np.arange(len(enc), dtype=np.uint32), rlen, roff, None)
    assert len(set(int(o) % 16 for o in roff)) == 16
    rdb = ResidentDB(db, 0)
    before = [rdb.read_bytes(r, int(rlen[r])) for r in range(len(enc))]
    assert rdb.compact_bytes() is True and not rdb.has_bytes and 0 < rdb.side_bytes <= 500 + 64 + 4096
    for r in range(len(enc)):
        got = rdb.read_bytes(r, int(rlen[r]))
        assert np.array_equal(before[r], enc[r]) and np.array_equal(got, enc[r]), (r, int(rlen[r]), int(roff[r]) % 16, np.flatnonzero(got != enc[r])[:5])
    rdb.close()


def test_sketch_patterns_on_a_compacted_database():
    """the read list of test_reads_with_ambiguous_bases_run_by_run (single / many / clustered ambiguous bases, at the read ends, after
    strand-ambiguous and low-complexity stretches, runs shorter than a window / a k-mer, a read of nothing else, forward strand only), compacted:
    the run-by-run sketch on the side store, every list level and a chunk selection, against the oracle"""
    rng = np.random.default_rng(2024)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    at = lambda n: np.resize(np.array([0, 3], np.uint8), n)
    enc = [
        _with_ambiguous(rnd(7000), [10, 3000, 6990]),
        _with_ambiguous(rnd(15000), [0]), _with_ambiguous(rnd(15000), [14999]), _with_ambiguous(rnd(15000), [14999 - 40]),
        _with_ambiguous(rnd(12000), list(range(5000, 5040))),
        _with_ambiguous(rnd(9000), sorted(rng.choice(9000, 60, replace=False))),
        _with_ambiguous(rnd(9000), sorted(rng.choice(9000, 400, replace=False))),
        _with_ambiguous(np.concatenate([rnd(3000), at(500), rnd(3000)]), [3499, 3500, 3520]),
        _with_ambiguous(np.concatenate([rnd(2000), np.zeros(700, np.uint8), rnd(2000)]), [2300, 2350, 2699]),
        _with_ambiguous(np.resize(rnd(5), 8000), [4000]),
        _with_ambiguous(rnd(40), [20]), _with_ambiguous(rnd(16), [15]), _with_ambiguous(rnd(17), [0]), _with_ambiguous(rnd(200), [100]),
        _with_ambiguous(rnd(300), list(range(300))),
        _with_ambiguous(rnd(15000), [7000], both=False),
        _with_ambiguous(rnd(6000), [5999 - 90, 5999 - 30]),
        _with_ambiguous(rnd(6000), [5999 - 17]), _with_ambiguous(rnd(6000), [5999 - 16]), _with_ambiguous(rnd(6000), [5999 - 15]),
    ]
    n_amb = len(enc)
    enc += [_enc(rnd(int(n))) for n in rng.integers(3000, 20000, 30)]
    order = rng.permutation(len(enc))
    enc = [enc[i] for i in order]
    rlen = np.array([len(e) for e in enc], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    db = formats.SeqDB(np.concatenate(enc), np.arange(len(enc), dtype=np.uint32), rlen, roff, None)
    rdb = ResidentDB(db, 0)
    l0 = np.concatenate([U.orc_sketch_seqdb(e, 80, 16, i) for i, e in enumerate(enc)])
    l1 = U.orc_reduce(l0, 6)
    l2 = U.orc_reduce(l1, 6)
    assert np.array_equal(rdb.index().top, l2)                      # (bytes)
    assert rdb.compact_bytes() is True and not rdb.has_bytes and rdb.side_bytes > 0
    f2 = rdb.index()
    assert np.array_equal(f2.top, l2) and f2.reads_literal >= n_amb - 1
    assert np.array_equal(rdb.index(levels=1).top, l1)
    sel = [i for i in range(len(enc)) if i % 3 == 2]
    assert np.array_equal(rdb.index(total_chunk=3, mychunk=2).top,
                          U.orc_reduce(U.orc_reduce(np.concatenate([U.orc_sketch_seqdb(enc[i], 80, 16, i) for i in sel]), 6), 6))
    rdb.close()


def test_degenerate_cases():
    """no flagged read: compaction is the release; a read beyond 65,535 bases: refused, bytes kept; an adopted device buffer: the caller may
    free it after compaction"""
    import torch
    db = simreads.make_workload("small")
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    want, _ = rdb.overlap(ix.top, ix.top_mc)
    assert rdb.compact_bytes() is True and not rdb.has_bytes and rdb.side_bytes == 0
    assert rdb.release_bytes() is True and rdb.compact_bytes() is True
    got, _ = rdb.overlap(ix.top, ix.top_mc)
    assert formats.ovlp_fields_equal(got, want) and np.array_equal(rdb.index().top, ix.top)
    with pytest.raises(_lib.PgxError, match="released"):
        rdb.index(want_l0=True)
    rdb.close()
    # ---- a 70,000-base read
    rng = np.random.default_rng(5)
    enc = [_enc(rng.integers(0, 4, n).astype(np.uint8)) for n in (70_000, 5000, 6000)] + [_with_ambiguous(rng.integers(0, 4, 4000).astype(np.uint8), [17])]
    rlen = np.array([len(e) for e in enc], np.uint32)
    roff = np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64)
    rl = ResidentDB(formats.SeqDB(np.concatenate(enc), np.arange(len(enc), dtype=np.uint32), rlen, roff, None), 0)
    assert rl.compact_bytes() is False and rl.has_bytes and rl.side_bytes == 0
    assert np.array_equal(rl.index(want_l0=True).l0, np.concatenate([U.orc_sketch_seqdb(e, 80, 16, i) for i, e in enumerate(enc)]))
    rl.close()
    # ---- an adopted device buffer
    dbn, flagged = _small_set_with_flagged_reads()
    oix = ResidentDB(dbn, 0)
    ix = oix.index()
    want, _ = oix.overlap(ix.top, ix.top_mc)     # (bit-exact against the oracle on this set: test_alignment_keys_..., test_gpu_parity.py)
    oix.close()
    want_orc, _ = U.orc_overlap(dbn, ix.top, ix.top_mc)
    assert formats.ovlp_fields_equal(want, want_orc)
    buf = torch.zeros(len(dbn.seqdb) + 1024, dtype=torch.uint8, device="cuda:0")
    buf[:len(dbn.seqdb)] = torch.from_numpy(dbn.seqdb).to("cuda:0")
    torch.cuda.synchronize()
    ra = ResidentDB.adopt_device(buf, len(dbn.seqdb), dbn.rid, dbn.rlen, dbn.roff, 0)
    assert ra.compact_bytes() is True and not ra.has_bytes and ra.side_bytes > 0
    buf.fill_(0xFF)                               # the caller's buffer is the caller's again: overwritten, then freed
    torch.cuda.synchronize()
    del buf
    torch.cuda.empty_cache()
    with _env(PGX_GPU_REPLAY="1"):
        got, _ = ra.overlap(ix.top, ix.top_mc)
    assert formats.ovlp_fields_equal(got, want_orc) and np.array_equal(ra.index().top, ix.top)
    ra.close()
