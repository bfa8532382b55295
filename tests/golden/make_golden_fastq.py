#!/usr/bin/env python3
"""Golden vectors for the read-database builder (pgx_reads.hip): small FASTQ / FASTA texts, and lists of texts for the multi-file cases,
with the REAL reference binary's .seqdb and .idx for each, one list a run.
Run in the build container, after `make -C oracle ref`: python tests/golden/make_golden_fastq.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_util as U  # noqa: E402


def cases():
    """name -> list of texts (one file each)"""
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qv = np.frombuffer(b"I5F:,~!9", np.uint8)

    def rnd(n):
        return acgt[rng.integers(0, 4, n)].tobytes()

    def q(n):
        return qv[rng.integers(0, len(qv), n)].tobytes()

    def fq(name, n):
        return b"@" + name + b"\n" + rnd(n) + b"\n+\n" + q(n) + b"\n"

    c = {}
    c["four_line"] = [fq(b"r1 c", 40) + fq(b"r2", 7) + fq(b"r3\tx", 23)]
    c["quality_starts_with_at"] = [b"@r1\nACGT\n+\n@III\n@r2\nAC\n+r2\n@@\n@r3\nA\n+\n@\n"]
    c["quality_lines_start_with_markers"] = [b"@r1\nACGTACGTACGT\n+\nIIII\n>III\n+III\n@r2\nACG\n+\n+II\n"]
    c["multi_line"] = [b"@r1 x\n" + rnd(30) + b"\n" + rnd(30) + b"\n" + rnd(11) + b"\n+r1\n" + q(25) + b"\n" + q(25) + b"\n" + q(21) + b"\n" + fq(b"r2", 9)]
    c["crlf"] = [b"@r1 c\r\n" + rnd(20) + b"\r\n+\r\n" + q(20) + b"\r\n@r2\r\nAC\r\nGT\r\n+r2\r\nII\r\nII\r\n"]
    c["lone_cr_first_sequence_line"] = [b"@r1\n\r\n+\nI\n@r2\n\r\nAC\n+\nIII\n@r3\nA\n\r\n+\nI\n"]
    c["lone_cr_first_quality_line_behind_empty"] = [b"@r1\nACG\n+\n\n\r\nII\n@r2\nA\n+\n\n\r\n@r3\nAC\n+\nI\n\r\nI\n@r4\nC\n+\nI\n"]
    c["empty_sequence_plus_at_end"] = [fq(b"r1", 5) + b"@r2\n+\n"]
    c["empty_sequence_plus_no_newline"] = [fq(b"r1", 5) + b"@r2\n+"]
    c["empty_sequence_nonempty_quality"] = [b"@r1\n+\nIII\n@r2\nAC\n+\nII\n"]
    c["empty_sequence_empty_quality_line"] = [b"@r1\n+\n\n@r2\nAC\n+\nII\n"]
    c["truncated_quality"] = [fq(b"r1", 8) + b"@r2\nACGTACGT\n+\nIIII\n"]
    c["truncated_quality_then_record"] = [fq(b"r1", 8) + b"@r2\nACGTACGT\n+\nIIII\n@r3\nAC\n+\nII\n"]
    c["quality_longer"] = [fq(b"r1", 8) + b"@r2\nACGT\n+\nIIIIII\n" + fq(b"r3", 4)]
    c["plus_without_newline"] = [fq(b"r1", 8) + b"@r2\nACGT\n+r2"]
    c["record_behind_bad_one"] = [fq(b"r1", 6) + b"@r2\nACGT\n+\nII\nI\n@r3\nAC\n+\nII\n"]
    c["header_mid_line_behind_quality"] = [b"@r1\nACGT\n+\nIIII\nxx yy@r2 c\nAC\n+\nII\njunk\nmore>r3\nACG\n"]
    c["fasta_fastq_mixed"] = [b">f1\n" + rnd(30) + b"\n" + rnd(4) + b"\n" + fq(b"q1", 12) + b">f2 c\n" + rnd(9) + b"\n@q2\nAC\n+\nII\n>f3\n"]
    c["junk_before"] = [b"junk\n+\n+x\n\n" + fq(b"r1", 5)]
    c["no_final_newline"] = [fq(b"r1", 5) + b"@r2\nACGT\n+\nIIII"]
    c["last_quality_line_lone_cr"] = [b"@r1\nAC\n+\nI\n\r"]
    c["last_marker_byte"] = [fq(b"r1", 5) + b"@"]
    body = fq(b"r", 30) * 300
    for size in (16384, 16385):
        for tag, tail in (("mixed", b">f\nACGT\n@q\nACGT\n+\nIIII\nxx@z\nAC"), ("trunc", b"@q\nACGT\n+\nII\n"), ("marker_last", b"@q\nACGT\n+\nIIII\n@"),
                          ("lone_cr", b"@q\nAC\n+\nI\n\r")):
            cut = ((size - len(tail)) // 67) * 67   # (whole records of body)
            pad = size - len(tail) - cut
            t = body[:cut] + (b">p\n" + b"A" * (pad - 4) + b"\n" if pad >= 4 else b"\n" * pad) + tail
            assert len(t) == size and len(body) == 300 * 67
            c["%s_at_%d" % (tag, size)] = [t]
    c["two_files_first_stops_early"] = [fq(b"a1", 6) + b"@a2\nACGT\n+\nII\n" + fq(b"a3", 4), fq(b"b1", 5) + b">b2\nAC\n"]
    c["file_without_record_between"] = [fq(b"a1", 6), b"no marker in this one\n+\n\n", fq(b"c1", 3) + fq(b"c2", 2)]
    c["three_files_mixed"] = [b">f\n" + rnd(20), fq(b"q", 9), b"@x\nAC\n+\nI"]
    return c


def main():
    store = {}
    tmp = tempfile.mkdtemp()
    cs = cases()
    for k, texts in cs.items():
        fns = []
        for i, text in enumerate(texts):
            fns.append(os.path.join(tmp, "%s.%d.fq" % (k, i)))
            open(fns[-1], "wb").write(text)
            store["text_%s_%d" % (k, i)] = np.frombuffer(text, np.uint8)
        lst, pre = os.path.join(tmp, k + ".lst"), os.path.join(tmp, k)
        open(lst, "w").write("\n".join(fns) + "\n")
        U.ref_run("shmr_mkseqdb", "-p", pre, "-d", lst)
        store["files_" + k] = np.array(len(texts))
        store["seqdb_" + k] = np.fromfile(pre + ".seqdb", np.uint8)
        store["idx_" + k] = np.frombuffer(open(pre + ".idx", "rb").read(), np.uint8)
        print(k, repr(open(pre + ".idx").read()[-200:]))
    store["order"] = np.array(list(cs))
    np.savez_compressed(os.path.join(HERE, "fastq_cases.npz"), **store)


if __name__ == "__main__":
    main()
