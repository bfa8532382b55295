"""The restatement of falcon.align and of pg_asm_cns.py's inner loop (tests/aln_util.py) against the fixture the real reference wrote
(tests/golden/aln_cases.npz, make_golden_aln.py): every stored answer, the exits, the provenance.  No GPU."""
import json

import aln_util as AU


def test_the_restatement_equals_every_stored_alignment():
    alns, _ = AU.load_cases()
    assert len(alns) >= 80
    for c in alns:
        got, ex = AU.align(c.q, c.t, c.band, c.want_str)
        assert got == c.answer, (c.name, got[:6], c.answer[:6])
        assert ex == c.exit, c.name
        if not c.want_str and ex == AU.EXIT_END:
            assert got[0] == (got[3] + got[5] + got[1]) // 2 and got[6:] == (b"", b""), c.name
        if ex != AU.EXIT_END:
            assert got == AU.ZERO, c.name


def test_the_strings_are_a_path_from_the_origin_without_mismatch_columns():
    for c in AU.load_cases()[0]:
        if not c.want_str or c.exit != AU.EXIT_END:
            continue
        size, dist, q_s, q_e, t_s, t_e, qs, ts = c.answer
        assert (q_s, t_s) == (0, 0) and len(qs) == len(ts) == size, c.name
        assert qs.replace(b"-", b"") == c.q[:q_e] and ts.replace(b"-", b"") == c.t[:t_e], c.name
        indel = sum(1 for a, b in zip(qs, ts) if a == 45 or b == 45)
        assert indel == dist and all(a == b or a == 45 or b == 45 for a, b in zip(qs, ts)), c.name


def test_every_exit_and_every_window_is_in_the_fixture():
    alns, pieces = AU.load_cases()
    by_name = {c.name: c for c in alns}
    assert {c.exit for c in alns} == {AU.EXIT_END, AU.EXIT_BAND, AU.EXIT_STEPS}
    assert any(len(c.q) and len(c.t) and int(0.3 * (len(c.q) + len(c.t))) == 0 for c in alns)          # max_d == 0
    assert by_name["self_1"].answer == AU.ZERO and by_name["self_2"].answer[0] == 2 and by_name["q1_t3"].answer[0] == 1
    assert by_name["case_lower_upper"].exit != AU.EXIT_END and by_name["case_lower_lower"].exit == AU.EXIT_END
    assert [by_name[f"dist_{n}"].answer[1] for n in (63, 64, 65)] == [63, 64, 65]
    for nk in (63, 64, 65):
        info = {}
        c = by_name[f"nk_{nk}"]
        AU.align(c.q, c.t, c.band, True, info)
        assert info["max_nk"] == nk
    info = {}
    c = by_name["backbone_60k"]
    AU.align(c.q, c.t, c.band, True, info)
    assert info["snakes"] == [60_000] and c.answer[0] == 60_000
    for L in (8, 9, 64, 65, 512, 513, 520, 521):
        info = {}
        c = by_name[f"snake_{L}"]
        AU.align(c.q, c.t, c.band, True, info)
        assert L in info["snakes"], (L, info["snakes"][:5])
    assert {c.band for c in alns} >= {0, 1, 50, 150, 400, 4096}
    assert sum(len(p) for pc in pieces for p in pc.pieces) >= 38 and any(len(pc.pieces) == 32 for pc in pieces)


def test_the_restatement_equals_every_stored_piece():
    for pc in AU.load_cases()[1]:
        for p, (T, reads) in enumerate(pc.pieces):
            cns, used, rule = AU.consensus_reads(T, reads, pc.min_cov)
            assert cns == pc.cns[p] and used == pc.used[p].tolist() and rule == pc.by_rule[p], (pc.name, p)
            if rule:
                assert cns == T.lower()


def test_the_pieces_hold_every_kind_of_read():
    pc = next(c for c in AU.load_cases()[1] if c.name == "pieces_shifts")
    T, reads = pc.pieces[0]
    kinds = set()
    for (read, shift), u in zip(reads, pc.used[0].tolist()):
        q, t = (read[-shift:], T) if shift < 0 else (read, T[shift:])
        if not q or not t:
            kinds.add("clipped"); assert not u
            continue
        a = AU.align(q, t, 150)[0]
        first, second = abs(a[3] - len(q)) < 48, shift >= 0 and abs(len(T) - shift - a[3]) < 48
        assert u == (first or second)
        kinds.add(("neg" if shift < 0 else "zero" if shift == 0 else "pos") if u else "rejected")
        if first != second:
            kinds.add("first only" if first else "second only")
    assert kinds == {"clipped", "neg", "zero", "pos", "rejected", "first only", "second only"}
    edge = next(c for c in AU.load_cases()[1] if c.name == "pieces_cov_edge")
    assert edge.by_rule == [True, False, True, True]


def test_provenance_lists_the_sources_and_the_reference_times():
    prov = json.load(open(AU.PROVENANCE))
    assert {"falcon.c", "DW_banded.c", "kalloc.c"} <= set(prov["sources"]) and all(len(h) == 64 for h in prov["sources"].values())
    assert "-DNDEBUG" in prov["cflags"] and prov["compiler"]
    alns, pieces = AU.load_cases()
    assert set(prov["reference_seconds_one_thread"]) == {c.name for c in alns} | {c.name for c in pieces}
    assert all(prov["exits"][e] > 0 for e in "abc")
    b = prov["bench"]
    assert b["pieces"] == 2 and len(b["with_strings"]) == len(b["without_strings"]) == 2 and "one CPU thread" in b["machine"]
