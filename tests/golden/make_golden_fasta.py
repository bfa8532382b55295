#!/usr/bin/env python3
"""Golden vectors for pgx_seqdb_from_fasta: small FASTA texts and the REAL reference binary's .seqdb and .idx for each, one text a run.
Run in the build container: python tests/golden/make_golden_fasta.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_util as U  # noqa: E402


def cases():
    rng = np.random.default_rng(29)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def rnd(n):
        return acgt[rng.integers(0, 4, n)].tobytes()

    c = {}
    c["junk_before"] = b"junk line\nmore junk\n\n>r1 c\n" + rnd(70) + b"\n" + rnd(33) + b"\n>r2\n" + rnd(10) + b"\n"
    c["first_marker_midline"] = b"xx yy>r1 rest of it\n" + rnd(40) + b"\n>r2\n" + rnd(9) + b"\n"
    c["first_marker_midline_at"] = b"ACGT@r1\n" + rnd(12) + b"\n"
    c["at_header"] = b"@r1\n" + rnd(21) + b"\n@r2 x\n" + rnd(22) + b"\n>r3\n" + rnd(5) + b"\n"
    c["gt_in_comment_and_sequence"] = b">r1 a>b >c\nAC>GT\nA@C\n>r2\t>x\nGG>\n"
    c["crlf"] = b">r1 c\r\n" + rnd(30) + b"\r\n" + rnd(7) + b"\r\n>r2\r\nA\r\n>r3\r\n\r\n" + rnd(4) + b"\r\n"
    c["cr_first_line"] = b">r1\n\r\nACGT\n>r2\n\r\n"
    c["cr_later_line"] = b">r1\nACGT\n\r\nAC\n\r\n>r2\nA\n\r\n"
    c["a_cr_cr"] = b">r1\nA\r\r\n>r2\nACG\r\r\nT\r\r\r\n"
    c["blank_lines"] = b">r1\n\n\nACGT\n\n\nAC\n\n>r2\n\nG\n\n"
    c["two_headers"] = b">r1\n>r2\n>r3 x\nACGT\n>r4\n>r5\n"
    c["header_last_nl"] = b">r1\nACGT\n>r2\n"
    c["header_last_no_nl"] = b">r1\nACGT\n>r2"
    c["header_last_no_nl_comment"] = b">r1\nACGT\n>r2 comment"
    c["marker_last_after_nl"] = b">r1\nACGT\n>"
    c["marker_last_after_nl_at"] = b">r1\nACGT\n@"
    c["marker_last_midline"] = b">r1\nACGT\nAC>"
    c["marker_last_in_header"] = b">r1\nACGT\n>r2>"
    c["empty_name"] = b">\nACGT\n> c\nAC\n>\tx\nG\n"
    c["tab_name"] = b">r1\tcomment here\nACGT\n>r2\vx\nAC\n>r3\rx\nA\n"
    c["lower_iupac"] = b">r1\nacgtnACGTNRYKMSWBDHVryu*-.\n>r2\nNNNNacgtNNNN\n"
    c["no_final_nl"] = b">r1\n" + rnd(50) + b"\n" + rnd(13)
    c["no_final_nl_cr"] = b">r1\nACGT\r"
    c["blanks_in_sequence"] = b">r1\nAC GT\n \nA\tC\n"
    # the reader's end of input: a last line of one byte without '\n' (short text: its '\r' stays; a text of one buffer: it goes), and a
    # marker as the very last byte of a text of exactly one buffer (a record with an empty name)
    c["last_line_lone_cr"] = b">r1\nACGT\n\r"
    c["last_line_lone_base"] = b">r1\nACGT\nC"
    body = b">r1\n" + b"\n".join([rnd(60)] * 300)   # (one line repeated: the file stays a few KB)
    c["one_buffer_lone_cr"] = body[:16384 - 2] + b"\n\r"
    c["one_buffer_marker_last"] = body[:16384 - 2] + b"\n>"
    assert len(c["one_buffer_lone_cr"]) == 16384 and len(c["one_buffer_marker_last"]) == 16384
    return c


def main():
    store = {}
    tmp = tempfile.mkdtemp()
    cs = cases()
    for k, text in cs.items():
        fa, lst, pre = (os.path.join(tmp, k + e) for e in (".fa", ".lst", ""))
        open(fa, "wb").write(text)
        open(lst, "w").write(fa + "\n")
        U.ref_run("shmr_mkseqdb", "-p", pre, "-d", lst)
        store["text_" + k] = np.frombuffer(text, np.uint8)
        store["seqdb_" + k] = np.fromfile(pre + ".seqdb", np.uint8)
        store["idx_" + k] = np.frombuffer(open(pre + ".idx", "rb").read(), np.uint8)
        print(k, repr(open(pre + ".idx").read()))
    store["order"] = np.array(list(cs))
    np.savez_compressed(os.path.join(HERE, "fasta_cases.npz"), **store)


if __name__ == "__main__":
    main()
