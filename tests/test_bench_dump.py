"""bench.py --dump-outputs (CPU): the sampled records come out as exact float64 columns, the sample is the same from run to run, and a job's
dump stays within its size bound."""
import numpy as np

from peregrine_amd import formats
from test_hashes import _records


def test_dump_columns_are_the_record_fields():
    import bench
    assert bench.DUMP_COLUMNS[5:] == tuple(f for f in formats.OVLP_FIELDS if f not in ("y0", "y1"))


def test_dump_is_exact_and_repeatable(tmp_path):
    import bench
    chunks = 8
    ov = _records(100_000, 5)
    ov["y0"][:3] = [0, (1 << 64) - 1, (123 << 32) | 4567]
    idx, rec = bench.dump_sample(ov, 3, chunks)
    idx2, rec2 = bench.dump_sample(ov.copy(), 3, chunks)
    assert np.array_equal(idx, idx2) and formats.ovlp_fields_equal(rec, rec2)
    assert 0 < len(idx) <= bench.DUMP_RECORDS // chunks and np.all(np.diff(idx) > 0)
    assert not np.array_equal(idx, bench.dump_sample(ov, 4, chunks)[0])     # another chunk, another sample
    small = ov[:1000]
    assert np.array_equal(bench.dump_sample(small, 3, chunks)[0], np.arange(1000))   # a stream shorter than the sample: all of it
    bench.write_dump(str(tmp_path), {3: (idx, rec)}, {3: (len(ov), (0xDEADBEEF << 32) | 0x12345678)}, chunks)
    got = np.load(tmp_path / "records_chunk03_of_08.npy")
    assert got.dtype == np.float64 and got.shape == (len(idx), len(bench.DUMP_COLUMNS))
    col = {n: got[:, i] for i, n in enumerate(bench.DUMP_COLUMNS)}
    assert np.array_equal(col["index"].astype(np.int64), idx)
    for y in ("y0", "y1"):
        back = (col[y + "_hi"].astype(np.uint64) << np.uint64(32)) | col[y + "_lo"].astype(np.uint64)
        assert np.array_equal(back, rec[y])
    for f in bench.DUMP_COLUMNS[5:]:
        assert np.array_equal(col[f].astype(rec[f].dtype), rec[f])
    st = np.load(tmp_path / "stream_chunk03_of_08.npy")
    assert st.dtype == np.float64 and st.tolist() == [len(ov), 0xDEADBEEF, 0x12345678]


def test_dump_of_a_job_stays_within_64_mb():
    import bench
    for chunks in (1, 8, 24):
        assert max(1, bench.DUMP_RECORDS // chunks) * chunks * len(bench.DUMP_COLUMNS) * 8 <= 64 << 20
