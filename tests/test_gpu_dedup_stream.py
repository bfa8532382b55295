"""The streaming shmr_dedup on the GPU (pgx_dedup_open / _feed / _feed_dev / _close, DedupStream, the two drop-ins): whatever the
cut of the stream into feeds, the concatenated text is the one-shot call's, the reference's and the oracle's, byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import oracle_util as U
from peregrine_amd import _lib, formats, simreads
from peregrine_amd.formats import OVLP_DTYPE
from peregrine_amd.shimmer import DedupStream, ResidentDB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DEDUP = os.path.join(U.REF_DIR, "shmr_dedup")


def one_shot(recs):
    """pgx_dedup itself (shimmer.shmr_dedup goes through the stream)"""
    _lib.init()
    recs = np.ascontiguousarray(recs, OVLP_DTYPE)
    text, tl, nu = C.c_void_p(), C.c_size_t(0), C.c_uint64(0)
    _lib.check(_lib.load().pgx_dedup(recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(text), C.byref(tl), C.byref(nu)), "pgx_dedup")
    data = C.string_at(text.value, tl.value)
    _lib.load().pgx_free(text)
    return data, int(nu.value)


def streamed(recs, cuts, **kw):
    """text of the feeds recs[cuts[i]:cuts[i + 1]], each feed's text, and close()'s counts"""
    texts = []
    with DedupStream(**kw) as ds:
        for a, b in zip(cuts[:-1], cuts[1:]):
            texts.append(ds.feed(recs[a:b]))
        counts = ds.close()
    return b"".join(texts), texts, counts


def expected_text(recs):
    """the real reference's stdout where its binary travels with the tree, else the oracle's restatement"""
    if len(recs) and os.path.exists(REF_DEDUP):
        return subprocess.run([REF_DEDUP], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout
    return U.orc_dedup(recs)[0]


def golden_streams():
    z, d = G.load("tiny_stage.npz"), G.load("dedup_cases.npz")
    for name in ("dd_t1", "dd_t2", "dd_t3", "dd_l1"):
        yield name, np.concatenate([z[str(k)] for k in d[name + "_keys"]]), d[name].tobytes()
    t = G.load("dedup_format_cases.npz")
    yield "format", t["recs"], t["text"].tobytes()


@pytest.mark.parametrize("piece", [1, 7, 64, 1000, 0])
def test_pieces_equal_the_one_shot_call_and_the_reference(piece):
    for name, recs, ref in golden_streams():
        n = len(recs)
        cuts = list(range(0, n, piece)) + [n] if piece else [0, n]
        text, texts, counts = streamed(recs, cuts)
        assert text == ref, (name, piece)
        assert text == one_shot(recs)[0], (name, piece)
        assert counts == (n, ref.count(b"\n")), (name, piece)
        assert sum(t.count(b"\n") for t in texts) == counts[1]


def test_empty_feeds_and_empty_streams():
    with DedupStream() as ds:
        assert ds.close() == (0, 0)
    recs = G.load("dedup_format_cases.npz")["recs"]
    with DedupStream() as ds:
        assert ds.feed(recs[:0]) == b""
        first = ds.feed(recs[:50])
        assert ds.feed(np.zeros(0, OVLP_DTYPE)) == b"" and ds.feed_dev(0, 0) == b""
        assert ds.feed(recs[:50]) == b""                       # only pairs seen before: nothing to add
        assert first == U.orc_dedup(recs[:50])[0]
        assert ds.close() == (100, first.count(b"\n"))
        with pytest.raises(_lib.PgxError):                     # a closed stream takes nothing more
            ds.feed(recs[:1])
        with pytest.raises(_lib.PgxError):
            ds.close()
    # null arguments on an open stream: an error, after which the stream accepts only close
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.pgx_dedup_open(0, C.byref(h)), "pgx_dedup_open")
    text, tl = C.c_void_p(), C.c_size_t(0)
    assert lib.pgx_dedup_feed(h, None, 5, C.byref(text), C.byref(tl)) == -1 and not text.value
    r1 = np.ascontiguousarray(recs[:1])
    assert lib.pgx_dedup_feed(h, r1.ctypes.data_as(C.c_void_p), 1, C.byref(text), C.byref(tl)) == _lib.PGX_ESTATE and not text.value
    nr, nu = C.c_uint64(9), C.c_uint64(9)
    assert lib.pgx_dedup_close(h, C.byref(nr), C.byref(nu)) == 0 and (nr.value, nu.value) == (0, 0)


def test_first_wins_across_pieces():
    z = G.load("tiny_stage.npz")
    rng = np.random.default_rng(77)
    base = np.concatenate([z[k] for k in ("ov_i2_t3_1", "ov_i2_t3_2", "ov_i2_t3_3", "ov_i2_t2_1", "ov_i2_t2_2", "ov_l1_t1_1")])
    rep = np.concatenate([base, base, base])
    recs = np.concatenate([rep, rep[rng.permutation(len(rep))]])
    want, nu = U.orc_dedup(recs)
    for _ in range(3):
        inner = np.sort(rng.choice(np.arange(1, len(recs)), 40, replace=False))
        cuts = [0, *inner.tolist(), len(recs)]
        text, texts, counts = streamed(recs, cuts)
        assert text == want and counts == (len(recs), nu)
        assert any(t == b"" for t in texts[len(texts) // 2:])   # feeds that consist only of pairs seen before
    # the first and a later record of a pair in different feeds: the EARLIER one's line is printed
    half = len(base)
    text, texts, _ = streamed(recs, [0, half, len(recs)])
    assert texts[0] == U.orc_dedup(recs[:half])[0] and texts[1] == b"" and text == want


def synthetic(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, OVLP_DTYPE)
    i = np.arange(n, dtype=np.uint64)
    a, b = i, i + np.uint64(3_000_000)
    swap = rng.random(n) < 0.5
    rid0, rid1 = np.where(swap, b, a), np.where(swap, a, b)
    r["y0"] = (rid0 << np.uint64(32)) | (rng.integers(0, 20000, n, dtype=np.uint64) << np.uint64(1))
    r["y1"] = (rid1 << np.uint64(32)) | (rng.integers(0, 20000, n, dtype=np.uint64) << np.uint64(1))
    r["rl0"], r["rl1"] = rng.integers(5000, 30000, n), rng.integers(5000, 30000, n)
    r["strand0"], r["strand1"], r["ovlp_type"] = rng.integers(0, 2, n), rng.integers(0, 2, n), rng.integers(0, 3, n)
    r["m_size"] = rng.integers(1, 20000, n)
    r["dist"] = (r["m_size"] * rng.random(n) * 0.05).astype(np.int32)
    r["q_bgn"], r["t_bgn"] = rng.integers(0, 3000, n), rng.integers(0, 3000, n)
    r["q_end"], r["t_end"] = r["q_bgn"] + r["m_size"], r["t_bgn"] + r["m_size"]
    return r


def test_the_pair_set_grows():
    recs = synthetic(2_000_000, 5)
    rng = np.random.default_rng(6)
    recs = np.concatenate([recs, recs[rng.choice(len(recs), 100_000, replace=False)]])   # recurrences at the end of the stream
    want, nu = U.orc_dedup(recs)
    assert nu == 2_000_000
    cuts = list(range(0, len(recs), 300_000)) + [len(recs)]

    def tag_bytes():
        _lib.mem_ledger(reset_peak=True)   # the peak starts again from now: peak_by_tag is the live bytes by owner
        return _lib.mem_ledger()["peak_by_tag"].get("dedup", 0)

    for expected in (0, 2_000_000):
        parts = []
        ds = DedupStream(expected_pairs=expected)
        at_open = tag_bytes()
        assert at_open >= (8 << 16)
        for a, b in zip(cuts[:-1], cuts[1:]):
            parts.append(ds.feed(recs[a:b]))
        held = tag_bytes()
        assert held >= 2 * nu * 8                                   # load <= 1/2, one 64-bit word per slot
        # sized up front for EXACTLY the stream's pairs (2 * 2,000,000 <= 2^22 slots): it never grows, although the late feeds bring
        # 100,000 records of pairs seen before -- the table is grown by the pairs a feed really adds, not by its record count
        assert (held > at_open) == (expected == 0)
        assert ds.close() == (len(recs), nu)
        assert tag_bytes() == 0                                     # back in the block cache
        assert b"".join(parts) == want, expected


def small_job(tmp_path):
    g = simreads.make_genome(300_000, 21, repeat_families=2, repeat_len=3000, repeat_copies=4, divergence=0.02, tandem=2)
    return simreads.simulate_reads(g, coverage=14.0, seed=3, mean_len=7000, sd_len=1500, err=0.01, n_files=1)


def test_feed_dev_and_a_two_chunk_job(tmp_path):
    import torch
    db = small_job(tmp_path)
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    chunks = [np.array(rdb.overlap(ix.top, ix.top_mc, total_chunk=2, mychunk=c)[0]) for c in (1, 2)]
    rdb.close()
    assert min(len(c) for c in chunks) > 500
    allrecs = np.concatenate(chunks)
    if U.have_ref() and os.path.exists(REF_DEDUP):   # the reference's own two streams, concatenated
        pre = str(tmp_path / "sd")
        formats.write_seqdb(pre, db)
        U.ref_run("shmr_index", "-p", pre, "-t", 1, "-c", 1, "-o", tmp_path / "ix")
        for c in (1, 2):
            U.ref_run("shmr_overlap", "-p", pre, "-l", tmp_path / "ix-L2", "-t", 2, "-c", c, "-o", tmp_path / f"ov.{c}")
        cat = b"".join((tmp_path / f"ov.{c}").read_bytes() for c in (1, 2))
        want = subprocess.run([REF_DEDUP], input=cat, stdout=subprocess.PIPE, check=True).stdout
    else:
        want = U.orc_dedup(allrecs)[0]
    dev = [torch.from_numpy(np.ascontiguousarray(c).view(np.uint8).copy()).to("cuda:0") for c in chunks]
    with DedupStream() as ds:       # chunk by chunk, by device pointer
        got = b"".join(ds.feed_dev(t.data_ptr(), t.numel() // 64) for t in dev)
        assert ds.close() == (len(allrecs), want.count(b"\n"))
    assert got == want
    with DedupStream() as ds:       # the same records from the host
        assert b"".join(ds.feed(c) for c in chunks) == want
    # host and device feeds alternating within one stream
    cuts = np.linspace(0, len(allrecs), 8).astype(int)
    d_all = torch.from_numpy(allrecs.view(np.uint8).copy()).to("cuda:0")
    with DedupStream() as ds:
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(ds.feed_dev(d_all.data_ptr() + int(a) * 64, int(b - a)) if k % 2 else ds.feed(allrecs[a:b]))
        assert b"".join(parts) == want


@pytest.fixture(scope="module")
def big_job_records():
    """the pipeline test's recipe at a larger coverage: >= 50,000 overlap records of a two-chunk job"""
    g = simreads.make_genome(1_500_000, 21, repeat_families=2, repeat_len=3000, repeat_copies=4, divergence=0.02, tandem=2)
    db = simreads.simulate_reads(g, coverage=50.0, seed=3, mean_len=7000, sd_len=1500, err=0.01, n_files=1)
    rdb = ResidentDB(db, 0)
    ix = rdb.index()
    recs = np.concatenate([np.array(rdb.overlap(ix.top, ix.top_mc, total_chunk=2, mychunk=c)[0]) for c in (1, 2)])
    rdb.close()
    assert len(recs) >= 50_000, len(recs)
    return recs


def _native_cmd():
    exe = os.path.join(ROOT, "bin", "native", "shmr_dedup")
    return [exe] if os.path.exists(exe) else [os.path.join(ROOT, "bin", "native", "pgx_cli"), "shmr_dedup"]


def test_drop_ins_stream_in_pieces(big_job_records, tmp_path):
    recs = big_job_records
    want = expected_text(recs)
    raw = recs.tobytes() + b"\x01" * 17   # a trailing partial record is dropped
    env = dict(os.environ, PGX_DEDUP_PIECE="1000")
    for cmd in (_native_cmd(), [sys.executable, os.path.join(ROOT, "bin", "shmr_dedup")]):
        r = subprocess.run(cmd, input=raw, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, cmd
    assert subprocess.run(_native_cmd(), input=b"", stdout=subprocess.PIPE, check=True, timeout=120).stdout == b""


def _run_rss(cmd, path, env):
    """stdout and the peak resident size (bytes) of that one child"""
    with open(path, "rb") as f:
        p = subprocess.Popen(cmd, stdin=f, stdout=subprocess.PIPE, env=env)
        out = p.stdout.read()
        _, status, ru = os.wait4(p.pid, 0)
        p.returncode = os.waitstatus_to_exitcode(status)
    assert p.returncode == 0
    return out, ru.ru_maxrss * 1024


def test_native_drop_in_runs_in_bounded_memory(big_job_records, tmp_path):
    """peak resident size on the stream repeated 8 times exceeds the peak on the stream once by at most ONE copy of the stream (a tool
    that buffers its input grows by seven)"""
    base = big_job_records
    parts, k = [], 0
    while sum(len(p) for p in parts) < 1_000_000:   # the job again under shifted read ids
        s = base.copy()
        s["y0"] += np.uint64((k * 50_000) << 32)
        s["y1"] += np.uint64((k * 50_000) << 32)
        parts.append(s)
        k += 1
    stream = np.concatenate(parts)
    want = U.orc_dedup(stream)[0]
    one, eight = tmp_path / "one.dat", tmp_path / "eight.dat"
    stream.tofile(one)
    with open(eight, "wb") as f:
        for _ in range(8):
            f.write(stream.tobytes())
    env = dict(os.environ, PGX_DEDUP_PIECE="65536")
    out1, rss1 = _run_rss(_native_cmd(), one, env)
    out8, rss8 = _run_rss(_native_cmd(), eight, env)
    print(f"peak resident size: stream once {rss1 >> 20} MiB, eight times {rss8 >> 20} MiB; one copy is {stream.nbytes >> 20} MiB")
    assert out1 == want and out8 == want
    assert rss8 - rss1 <= stream.nbytes, (rss1, rss8, stream.nbytes)
