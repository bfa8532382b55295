"""The FASTA/FASTQ grammar of the read-database builder, on the CPU: its plain restatement and the byte-at-a-time reader
(tests/fastq_util.py) against the reference binary's files for every golden case, against each other on the generators' texts, and --
where oracle/_ref/shmr_mkseqdb exists -- against that binary live."""
import os
import subprocess

import numpy as np
import pytest

import fastq_util as Q

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fastq_cases.npz")
REF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "shmr_mkseqdb")


def golden_cases():
    z = np.load(GOLDEN)
    return [(str(k), [z["text_%s_%d" % (k, i)].tobytes() for i in range(int(z["files_" + str(k)]))], z["seqdb_" + str(k)].tobytes(),
             z["idx_" + str(k)].tobytes()) for k in z["order"]]


CASES = golden_cases()
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("name,texts,seqdb,idx", CASES, ids=IDS)
def test_restatement_equals_reference_files(name, texts, seqdb, idx):
    got_db, got_idx = Q.files_of(*Q.reads_of_files(texts, Q.parse_reads))
    assert got_idx == idx
    assert got_db == seqdb


@pytest.mark.parametrize("name,texts,seqdb,idx", CASES, ids=IDS)
def test_byte_reader_equals_reference_files(name, texts, seqdb, idx):
    assert Q.files_of(*Q.reads_of_files(texts, Q.kseq_loop_q)) == (seqdb, idx)


def test_golden_file_is_small_and_holds_the_cases():
    assert os.path.getsize(GOLDEN) < 64 << 10
    want = {"four_line", "quality_starts_with_at", "quality_lines_start_with_markers", "multi_line", "crlf", "lone_cr_first_sequence_line",
            "lone_cr_first_quality_line_behind_empty", "empty_sequence_plus_at_end", "empty_sequence_nonempty_quality", "truncated_quality",
            "quality_longer", "plus_without_newline", "record_behind_bad_one", "header_mid_line_behind_quality", "fasta_fastq_mixed",
            "mixed_at_16384", "mixed_at_16385", "two_files_first_stops_early", "file_without_record_between"}
    assert want <= set(IDS)
    by = {c[0]: c for c in CASES}
    # the cases say what their names say: the reference dropped the record behind the bad one, and read on in the next file
    assert by["record_behind_bad_one"][3].count(b"\n") == 1
    assert [ln.split(b" ")[1] for ln in by["two_files_first_stops_early"][3].split(b"\n")[:-1]] == [b"a1", b"b1", b"b2"]
    assert [ln.split(b" ")[1] for ln in by["file_without_record_between"][3].split(b"\n")[:-1]] == [b"a1", b"c1", b"c2"]
    assert [ln.split(b" ")[1] for ln in by["header_mid_line_behind_quality"][3].split(b"\n")[:-1]] == [b"r1", b"r2", b"r3"]


def test_restatement_equals_byte_reader_on_the_generators_texts():
    texts = Q.random_texts() + Q.padded_texts()
    assert len(texts) == 345
    refused = several = with_quality = 0
    for t in texts:
        a, b = Q.answer(Q.parse_reads, t), Q.answer(Q.kseq_loop_q, t)
        if isinstance(a[0], str):
            assert a[0] == "cr" and len(t) > a[1] >= 0 and t[a[1]] == 0x0A and t[a[1] - 1] == 0x0A   # an empty line
            refused += 1
            continue
        assert a == b, t
        several += len(a[0]) >= 2
        with_quality += len(a[0]) >= 1 and b"\n+" in t
    print("refused", refused, "of", len(texts))
    assert refused <= 0.02 * len(texts)
    assert several > len(texts) // 3 and with_quality > len(texts) // 4


def test_the_refusal_class():
    """an empty quality line at which the reader's strip takes a '\\r' of an earlier line: refused by the restatement; the reader's own
    answer is what the reference gives (next test); the same lines without the deviation are read"""
    bad = b"@r1\nACGTA\n+\nII\r\r\r\n\nI\n@r2\nA\n+\nI\n"
    with pytest.raises(Q.Refused) as e:
        Q.parse_reads(bad)
    assert (e.value.kind, e.value.offset) == ("cr", bad.index(b"\n\n") + 1)
    for ok in (b"@r1\nAC\n+\nI\r\n\nI\n", b"@r1\nAC\n+\n\r\n\nI\n", b"@r1\nAC\n+\n\n\nII\n", b"@r1\nACG\n+\nI\r\r\nII\n"):
        assert Q.parse_reads(ok) == Q.kseq_loop_q(ok)


@pytest.mark.skipif(not os.path.exists(REF), reason="the reference binary is not built here")
def test_both_statements_equal_the_reference_binary_live(tmp_path):
    texts = Q.random_texts(120, seed=7) + Q.padded_texts()[::3] + [b"@r1\nACGTA\n+\nII\r\r\r\n\nI\n@r2\nA\n+\nI\n"]
    fn, lst, pre = str(tmp_path / "t.fq"), str(tmp_path / "t.lst"), str(tmp_path / "o")
    open(lst, "w").write(fn + "\n")
    for t in texts:
        open(fn, "wb").write(t)
        subprocess.run([REF, "-p", pre, "-d", lst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        want = (open(pre + ".seqdb", "rb").read(), open(pre + ".idx", "rb").read())
        assert Q.files_of(*Q.kseq_loop_q(t)) == want, t
        a = Q.answer(Q.parse_reads, t)
        assert isinstance(a[0], str) or Q.files_of(*a) == want, t
