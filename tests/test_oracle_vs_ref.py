"""Randomised checks of the oracle against the REAL reference compiled in place (oracle/_ref).
Skipped where oracle/_ref is absent."""
import os
import subprocess

import numpy as np
import pytest

import oracle_util as U
from peregrine_amd import formats, simreads

pytestmark = [pytest.mark.ref, pytest.mark.skipif(not U.have_ref(), reason="oracle/_ref not built")]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def test_codec_roundtrip_matches_reference():
    rng = np.random.default_rng(1)
    for n in (1, 2, 17, 1000):
        s = np.frombuffer(b"ACGTNacgtnX", np.uint8)[rng.integers(0, 11, n)].tobytes()
        enc = U.ref_encode(s)
        import ctypes as C
        mine = np.zeros(n, np.uint8)
        U.oracle().orc_encode_biseq(C.c_void_p(mine.ctypes.data), C.c_char_p(s), C.c_size_t(n))
        assert np.array_equal(enc, mine)
        for strand in (0, 1):
            buf = C.create_string_buffer(n)
            U.oracle().orc_decode_biseq(C.c_void_p(mine.ctypes.data), buf, C.c_size_t(n), C.c_uint8(strand))
            assert buf.raw == U.ref_decode(enc, strand)


def test_sketch_random_and_adversarial():
    rng = np.random.default_rng(2)
    for it in range(1500):
        kind = it % 5
        n = int(rng.integers(1, 700))
        if kind == 0:
            s = ACGT[rng.integers(0, 4, n)].tobytes()
        elif kind == 1:
            p = int(rng.integers(1, 30))
            s = (ACGT[rng.integers(0, 4, p)].tobytes() * (n // p + 1))[:n]
        elif kind == 2:
            s = ACGT[rng.integers(0, 2, n) * 3].tobytes()  # A/T only: many palindromes
        elif kind == 3:
            a = bytearray(ACGT[rng.integers(0, 4, n)].tobytes())
            for p in rng.integers(0, n, 3):
                a[int(p)] = ord("N")
            s = bytes(a)
        else:
            s = ACGT[rng.integers(0, 4, n)].tobytes()
            s = s + s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
        w, k = [(80, 16), (24, 12), (5, 15), (11, 13)][it % 4]
        assert np.array_equal(U.orc_sketch_ascii(s, w, k, it), U.ref_sketch_ascii(s, w, k, it)), (it, w, k)


def test_reduce_random():
    rng = np.random.default_rng(3)
    for it in range(500):
        n = int(rng.integers(0, 300))
        mm = np.zeros(n, formats.MM_DTYPE)
        mm["x"] = (rng.integers(0, 9, n).astype(np.uint64) << np.uint64(8)) | np.uint64(16)
        mm["y"] = (np.sort(rng.integers(0, 4, n)).astype(np.uint64) << np.uint64(32)) | (np.arange(n, dtype=np.uint64) << np.uint64(1))
        rs = int(rng.choice([2, 3, 6, 24]))
        assert np.array_equal(U.orc_reduce(mm, rs), U.ref_reduce(mm, rs))
        rs = int(rng.choice([1, 4, 5, 7, 16, 17, 18, 255]))   # the factors tests/test_gpu_parity.py runs across the switch of the reduce kernels
        assert np.array_equal(U.orc_reduce(mm, rs), U.ref_reduce(mm, rs)), rs


def test_ovlp_match_random_pairs():
    db = simreads.make_workload("tiny")
    rng = np.random.default_rng(4)
    for it in range(150):
        a, b = rng.integers(0, db.n_reads, 2)
        q = db.seqdb[int(db.roff[a]):int(db.roff[a]) + int(db.rlen[a])][int(rng.integers(0, 500)):]
        t = db.seqdb[int(db.roff[b]):int(db.roff[b]) + int(db.rlen[b])]
        args = (q, int(rng.integers(0, 2)), t, int(rng.integers(0, 2)), int(rng.choice([100, 20])))
        assert U.orc_ovlp_match(*args) == U.ref_ovlp_match(*args)


def _small_set():
    g = simreads.make_genome(300_000, 11, repeat_families=2, repeat_len=3000, repeat_copies=6, tandem=4)
    return g, simreads.simulate_reads(g, coverage=14.0, seed=5, mean_len=8000, sd_len=900)


# (w, k, r, levels, index chunks, overlap chunks, records of the reference's stream per overlap chunk in this very run): the three
# rows at the reference's defaults, then the shimmer sets everything after the index stage is run on (tests/test_gpu_shimmer_params.py)
STAGE_ROWS = [
    (80, 16, 6, 2, 1, 1, (5672,)),
    (80, 16, 6, 2, 3, 2, (4960, 4663)),
    (80, 16, 6, 1, 2, 1, (6937,)),
    (80, 20, 6, 2, 1, 1, (5674,)),
    (80, 28, 6, 2, 2, 2, (4349, 4082)),
    (48, 12, 4, 2, 1, 1, (6891,)),
    (64, 24, 3, 2, 1, 1, (7374,)),
    (80, 16, 2, 1, 1, 1, (6390,)),
    (40, 15, 2, 1, 3, 2, (111, 109)),
    (128, 16, 3, 1, 1, 1, (6897,)),
    (32, 14, 12, 1, 1, 1, (6878,)),
    (255, 28, 2, 1, 1, 1, (6672,)),
    (100, 17, 5, 2, 1, 1, (5862,)),
]


@pytest.mark.parametrize("w,k,r,lv,IT,OT,n_ref", STAGE_ROWS, ids=["w%d-k%d-r%d-l%d-t%d-%d" % row[:6] for row in STAGE_ROWS])
def test_stages_on_small_dataset(tmp_path, w, k, r, lv, IT, OT, n_ref):
    """shmr_index -w -k -r -l and shmr_overlap on its lists, reference against oracle: files byte for byte, streams field for field.
    An empty or short stream cannot pass: every chunk's stream holds at least half (rounded down) of what the reference wrote."""
    g, db = _small_set()
    pre = str(tmp_path / "sd")
    formats.write_seqdb(pre, db)
    for c in range(1, IT + 1):
        U.ref_run("shmr_index", "-p", pre, "-t", IT, "-c", c, "-l", lv, "-m", 1, "-w", w, "-k", k, "-r", r, "-o", tmp_path / "ref")
        U.orc_index_chunk(pre, str(tmp_path / "orc"), IT, c, lv, r, 1, w, k)
        tag = f"{c:02d}-of-{IT:02d}"
        for L in ("L0", f"L{lv}"):
            assert open(tmp_path / f"ref-{L}-{tag}.dat", "rb").read() == open(tmp_path / f"orc-{L}-{tag}.dat", "rb").read()
            a = formats.read_mm_count(str(tmp_path / f"ref-{L}-MC-{tag}.dat"))
            b = formats.read_mm_count(str(tmp_path / f"orc-{L}-MC-{tag}.dat"))
            assert np.array_equal(a["mer"], b["mer"]) and np.array_equal(a["count"], b["count"])  # same khash slot order
    for c in range(1, OT + 1):
        U.ref_run("shmr_overlap", "-p", pre, "-l", tmp_path / f"ref-L{lv}", "-t", OT, "-c", c, "-o", tmp_path / f"r.{c}")
        U.orc_overlap_chunk(pre, str(tmp_path / f"ref-L{lv}"), str(tmp_path / f"o.{c}"), OT, c)
        a, b = formats.read_ovlp(str(tmp_path / f"r.{c}")), formats.read_ovlp(str(tmp_path / f"o.{c}"))
        print(f"w {w} k {k} r {r} l {lv}: overlap chunk {c} of {OT} (index chunks {IT}): {len(a)} records")
        assert len(a) >= n_ref[c - 1] // 2 >= 50, (c, len(a))
        assert formats.ovlp_fields_equal(a, b), c


MAP_ROWS = [(80, 16, 6, 2), (80, 28, 6, 2), (48, 12, 4, 2), (64, 24, 3, 2), (80, 16, 2, 1), (255, 28, 2, 1)]


@pytest.mark.parametrize("w,k,r,lv", MAP_ROWS, ids=["w%d-k%d-r%d-l%d" % row for row in MAP_ROWS])
def test_map_on_small_dataset(tmp_path, w, k, r, lv):
    """shmr_map's text, reference against oracle, on lists of other shimmer parameters: the reads against two exact 120 kb pieces of
    their genome as contigs; the whole map with the default bounds, and chunk 2 of 3 with -M 30"""
    g, db = _small_set()
    ctg = simreads.simulate_reads(g[20_000:280_000], n_reads=2, seed=6, mean_len=120_000, sd_len=0, wrap=0, err=0.0)
    pre, cpre = str(tmp_path / "sd"), str(tmp_path / "ctg")
    formats.write_seqdb(pre, db)
    formats.write_seqdb(cpre, ctg)
    flags = ("-t", 1, "-c", 1, "-l", lv, "-m", 0, "-w", w, "-k", k, "-r", r)
    U.ref_run("shmr_index", "-p", pre, *flags, "-o", tmp_path / "rd")
    U.ref_run("shmr_index", "-p", cpre, *flags, "-o", tmp_path / "ctg")
    rf = formats.read_mmlist(str(tmp_path / f"ctg-L{lv}-01-of-01.dat"))
    mm = formats.read_mmlist(str(tmp_path / f"rd-L{lv}-01-of-01.dat"))
    mc = formats.read_mm_count(str(tmp_path / f"rd-L{lv}-MC-01-of-01.dat"))
    rl, _ = db.by_rid()
    for c, T, hi in ((1, 1, 240), (2, 3, 30)):
        want = subprocess.run([os.path.join(U.REF_DIR, "shmr_map"), "-r", cpre, "-m", str(tmp_path / f"ctg-L{lv}"), "-p", pre, "-l",
                               str(tmp_path / f"rd-L{lv}"), "-t", str(T), "-c", str(c), "-M", str(hi)], check=True,
                              stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
        got, n = U.orc_map_reads_to_ref(rf, mm, mc, rl, c, T, 1, hi)   # (shmr_map's own lower bound is 1)
        print(f"w {w} k {k} r {r} l {lv}: map chunk {c} of {T}, -M {hi}: {want.count(10)} lines")
        assert want.count(b"\n") >= 250, (c, T, hi)
        assert got == want and n == want.count(b"\n"), (c, T, hi)
