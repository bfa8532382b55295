"""The FASTA grammar of pgx_seqdb_from_fasta, on the CPU: its plain restatement (tests/fasta_util.py) against the reference binary's files
for every golden case, and against a byte-at-a-time reader written from the kseq loop over seeded random texts."""
import os

import numpy as np
import pytest

import fasta_util as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fasta_cases.npz")


def golden_cases():
    z = np.load(GOLDEN)
    return [(str(k), z["text_" + str(k)].tobytes(), z["seqdb_" + str(k)].tobytes(), z["idx_" + str(k)].tobytes()) for k in z["order"]]


CASES = golden_cases()


@pytest.mark.parametrize("name,text,seqdb,idx", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_reference_files(name, text, seqdb, idx):
    names, seqs = F.parse_fasta(text)
    got_db, got_idx = F.files_of(names, seqs)
    assert got_idx == idx
    assert got_db == seqdb


@pytest.mark.parametrize("name,text,seqdb,idx", CASES, ids=[c[0] for c in CASES])
def test_byte_reader_equals_reference_files(name, text, seqdb, idx):
    assert F.files_of(*F.kseq_loop(text)) == (seqdb, idx)


def test_golden_file_is_small():
    assert os.path.getsize(GOLDEN) < 32 << 10
    assert len(CASES) >= 20


def _answer(fn, text):
    try:
        return fn(text)
    except F.Refused as r:
        return (r.kind, r.offset)


def test_restatement_equals_byte_reader_on_random_texts():
    texts = F.random_texts()
    assert len(texts) == 300 and max(map(len, texts)) <= 400 and min(map(len, texts)) >= 0
    several = 0
    for t in texts:
        assert not any(t[i] == 0x2B and (i == 0 or t[i - 1] == 0x0A) for i in range(len(t)))
        a, b = _answer(F.parse_fasta, t), _answer(F.kseq_loop, t)
        assert a == b, t
        several += isinstance(a[0], list) and len(a[0]) >= 2
    assert several > len(texts) // 2


def test_refusals_of_both_statements():
    for fn in (F.parse_fasta, F.kseq_loop):
        with pytest.raises(F.Refused) as e:
            fn(b">r1\nACGT\n+\nIIII\n>r2\nAC\n+\nII\n")
        assert (e.value.kind, e.value.offset) == ("fastq", 9)
        for t in (b"", b"no header here\n", b"junk\n>", b"@"):
            with pytest.raises(F.Refused) as e:
                fn(t)
            assert e.value.kind == "no record"
        assert fn(b"+junk\n+\n>r1\nAC+\n") == ([b"r1"], [b"AC+"])   # a '+' before the first header, or not at a line start, is no record
