"""The restatement of the tiling-path rule (tests/tiling_util.tiling_rule) against tests/golden/tiling_cases.npz: on every case the two
files are, byte for byte, what the real graph_to_path.py wrote from the same inputs, and the counts are the fixture's.  No GPU."""
import pytest

import tiling_util as TU

Z, CASES = TU.load_fixture()


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_rule_reproduces_the_script(case):
    sg, utg, ctg, p, a = TU.case_files(Z, case)
    got_p, got_a, st = TU.tiling_rule(sg, utg, ctg)
    assert (got_p, got_a) == (p, a)
    assert st == {k: CASES[case][k] for k in st} and st["compound_tie_rounds"] == 0
    assert st["p_rows"] == p.count(b"\n") and st["a_rows"] == a.count(b"\n")


def test_the_fixture_covers_the_ground():
    compound = [c for c, s in CASES.items() if s["rounds"]]
    assert len(compound) >= 6 and CASES["bubble3"]["rounds"] == 3 and CASES["long"]["p_rows"] == 5000
    assert CASES["duals"]["ctg_skipped"] == 3 and CASES["contained_only"]["ctg_empty"] == 1 and CASES["empty_ctg"]["p_rows"] == 0
    assert b"-002-02 " in Z["two_compounds_a"].tobytes() and Z["ring_p"].tobytes().startswith(b"3 ")
    assert not Z["no_newline_sg"].tobytes().endswith(b"\n")
    assert b"000000F 000000003:E 000000005:E 000000005 1000 1710 7100 99.60 1100 710\n" in Z["bubble2_p"].tobytes()
    assert CASES["real_dense"]["p_rows"] > 50 and CASES["real_quant"]["p_rows"] > 10


def test_rows_of_text_numbers_names_by_first_appearance():
    rows, names = TU.rows_of_text(Z["duals_p"].tobytes())
    assert names == ["000000F", "000001F", "000002F", "000003R"] and [r[0] for r in rows] == sorted(r[0] for r in rows)
    assert rows[0][1:] == (1, 2) + rows[0][3:5] + (0, 0)


def test_a_tie_is_counted():
    b = TU.Builder(99)
    s, t, x, a, bb, c = (TU.key(r, TU.E) for r in (1, 2, 3, 5, 6, 7))
    for v, w, sc in ((s, x, 1), (x, a, 4), (x, bb, 4), (a, t, 10), (bb, t, 10), (s, c, 20), (c, t, 30)):
        b.edge(v, w, 100, sc)
    b.contig("000000F", [b.compound(s, t, [b.simple([s, x]), b.simple([x, a, t]), b.simple([x, bb, t]), b.simple([s, c, t])])], t)
    p, a_text, st = TU.tiling_rule(*b.files())
    assert st["compound_tie_rounds"] == 1 and st["alternates"] == 1
    assert b"000000005:E" in a_text and b"000000006:E" not in a_text and b"000000007:E" in p
