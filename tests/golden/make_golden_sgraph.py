"""Generator of tests/golden/sgraph_cases.npz and sgraph_cases_quant.npz (the `quant` case's arrays, to keep either file small): record sets built with tests/dedup_graph_util (make_records / rec), the REAL reference
shmr_dedup's text of each (oracle/_ref/shmr_dedup, built by `make -C oracle ref`), and the sg_edges_list that the reference's own
generate_string_graph (py/scripts/ovlp_to_graph.py, imported in place from the reference tree, nothing of it copied) writes for that
text with disable_chimer_bridge_removal=True and lfc=False.

Every case runs in two child processes with different PYTHONHASHSEEDs; the fixture is written only if the two outputs are equal.
networkx 3.4.2.

    python tests/golden/make_golden_sgraph.py [path/to/reference/py/scripts]

Cases (npz keys <name>_recs -- the records as a (64, n) matrix of byte columns, sgraph_util.fixture_recs undoes it -- and <name>_sg; thresholds in the provenance JSON and in `cases`):
  dense        make_records(seed=7, n_reads=260, genome=5000, contained_share=0.0), min_len 2000: a node with more than 64 out-edges
  dense_idt    the same records under min_idt 99.5            dense_len   ... under min_len 6000
  quant        make_records(seed=8, n_reads=150, genome=3000, contained_share=0.1) with q_bgn, q_end, t_end, m_size floored to multiples
               of 100, min_len 0: ties of length and of score
  spur_a/_b    three lines A-U, A-W, C-U in two orders: the spur pass depends on the order of the nodes
  directed     records that sit on every threshold of the rule (the generator asserts each)
  none         a stream whose every row is filtered: an empty file         single   one surviving row
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dedup_graph_util as DG  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
SCRIPTS = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "--child" else "/root/reference/py/scripts"
rec = DG.rec


def child(scripts, text_path, min_len, min_idt, out_path):
    """one run of the reference's function in this process (whose hash seed the parent chose)"""
    sys.path.insert(0, scripts)
    import ovlp_to_graph
    text = open(text_path, "rb").read()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        with open("preads.ovl", "wb") as f:
            f.write(text + b"-\n")
        ovlp_to_graph.generate_string_graph(types.SimpleNamespace(overlap_file="preads.ovl", min_len=int(min_len), min_idt=float(min_idt), lfc=False,
                                                                  disable_chimer_bridge_removal=True))
        sg = open("sg_edges_list", "rb").read()
    with open(out_path, "wb") as f:
        f.write(sg)


def sg_edges(text: bytes, min_len, min_idt) -> bytes:
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        tp = os.path.join(tmp, "text")
        with open(tp, "wb") as f:
            f.write(text)
        for seed in ("1", "4242"):
            op = os.path.join(tmp, "sg" + seed)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", SCRIPTS, tp, str(min_len), str(min_idt), op], check=True,
                           env=dict(os.environ, PYTHONHASHSEED=seed))
            outs.append(open(op, "rb").read())
    if outs[0] != outs[1]:
        sys.exit("two hash seeds give two sg_edges_list files: the fixture is NOT written")
    return outs[0]


def ref_text(recs) -> bytes:
    if len(recs) == 0:
        return b""
    return subprocess.run([REF], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout


def dv(f, g, oh_f, oh_g=None, rl=9000, **kw):
    """f to the left of g on the same strand: the edges g:B -> f:B of length oh_f and f:E -> g:E of length oh_g"""
    oh_g = oh_f if oh_g is None else oh_g
    args = dict(q_bgn=oh_f, q_end=rl, t_end=rl - oh_g, rl0=rl, rl1=rl)
    args.update(kw)
    return rec(f, g, **args)


def spur_lines():
    A, U, W, C_ = 1, 2, 3, 4
    au, aw, cu = dv(A, U, 1000), dv(A, W, 3000), dv(C_, U, 2000)
    return np.concatenate([au, aw, cu]), np.concatenate([aw, au, cu])


def fields(text):
    return [ln.split() for ln in text.split(b"\n")[:-1]]


def type_of(sg, v, w):
    for ln in sg.split(b"\n")[:-1]:
        f = ln.split()
        if f[0] == v and f[1] == w:
            return f[7]
    raise KeyError((v, w))


def nm(rid, end):
    return b"%09d:%s" % (rid, end)


MIN_LEN, MIN_IDT = 4000, 96.0
BIG = 1 << 24


def directed_records():
    """records on the rule's thresholds; returns (records, checks) where checks(text, sg) asserts that each condition is met"""
    r = []
    # --- the four geometry cases, each taken both ways (ids 100 ..)
    r.append(dv(100, 101, 1000))                                                                   # case 1 passes
    r.append(dv(102, 103, 1000, 0))                                                                # case 1: g_e == g_l, skipped
    r.append(rec(104, 105, s1=1, q_bgn=1000, q_end=9000, t_end=6000, rl0=9000, rl1=9000))          # case 2 passes (g_e = 3000)
    r.append(rec(106, 107, s1=1, q_bgn=1000, q_end=9000, t_end=9000, rl0=9000, rl1=9000))          # case 2: g_e == 0, skipped
    r.append(rec(108, 109, s1=1, q_bgn=0, q_end=7000, t_end=-500, rl0=9000, rl1=9000))             # case 3 passes (g_b = 9000 < g_e = 9500)
    r.append(rec(110, 111, s1=0, q_bgn=0, q_end=7000, t_end=7000, rl0=9000, rl1=9000))             # case 3: g_b == 0, skipped
    r.append(rec(112, 113, s0=1, s1=0, q_bgn=1000, q_end=9000, t_end=5000, rl0=9000, rl1=9000))    # case 4 passes (f: 0 .. 8000, g_b = 5000, g_e = 0)
    r.append(rec(114, 115, s0=0, s1=1, q_bgn=0, q_end=7000, t_end=7000, rl0=9000, rl1=9000))       # case 4: g_b == g_l, skipped
    # --- a negative a_bgn (case 4 again, passes)
    r.append(rec(116, 117, s0=1, s1=0, pos0=300, pos1=100, q_bgn=1000, q_end=9000, t_end=5000, rl0=9000, rl1=9000))
    # --- identity at and one tenth below min_idt
    r.append(dv(120, 121, 1000, m_size=5000, dist=200))     # 96.0
    r.append(dv(122, 123, 1000, m_size=5000, dist=205))     # 95.9
    # --- lengths min_len and min_len - 1
    r.append(rec(124, 125, q_bgn=1000, q_end=9000, t_end=3000, rl0=9000, rl1=MIN_LEN))
    r.append(rec(126, 127, q_bgn=1000, q_end=9000, t_end=3000, rl0=9000, rl1=MIN_LEN - 1))
    r.append(rec(128, 129, q_bgn=1000, q_end=MIN_LEN, t_end=3000, rl0=MIN_LEN, rl1=9000))
    r.append(rec(130, 131, q_bgn=1000, q_end=MIN_LEN - 1, t_end=2999, rl0=MIN_LEN - 1, rl1=9000))
    # --- a length sum equal to, and one below, max_len (ids 200 .. / 210 ..): A:E -> U:E 1000, A:E -> X:E 3000 (max_len 3500), U:E -> X:E
    # 2500 / 2499; U:E and U:B each have a shorter first out-edge to a node outside, so that only the sum decides
    for base, ux in ((200, 2500), (210, 2499)):
        A, U, X, Y, Z = base, base + 1, base + 2, base + 3, base + 4
        r += [dv(A, U, 1000), dv(A, X, 3000), dv(U, X, ux), dv(U, Y, 300), dv(Z, U, 300)]
    # --- e2 lengths 499 and 500 (ids 300 .. / 310 ..): at A:E the neighbour P:E (500) eliminates W:E (1000) in the first loop, so only the
    # second loop reads W:E's list: Y:E (100) first, then X:E with 499 / 500.  The reverse edges get lengths that reduce nothing.
    for base, wx in ((300, 499), (310, 500)):
        A, P, W, X, Y = base, base + 1, base + 2, base + 3, base + 4
        r += [dv(A, P, 3300, 500), dv(A, W, 3200, 1000), dv(A, X, 3400, 3000), dv(P, W, 3100, 400), dv(W, Y, 3000, 100), dv(W, X, 3050, wx)]
    # --- read ids above 2^24, with gaps
    r += [dv(BIG + 5, BIG + 900, 1000), dv(BIG + 900, 3 * BIG + 77, 1200), dv(BIG + 5, 3 * BIG + 77, 2500), dv(BIG + 5, 2**31 + 9, 700)]   # (as rid1: a line that starts with "-" ends the loader's file)
    recs = np.concatenate(r)

    def checks(text, sg):
        by = {(int(f[0]), int(f[1])): f for f in fields(text)}
        out_pairs = {tuple(sorted((int(ln.split()[0][:-2]), int(ln.split()[1][:-2])))) for ln in sg.split(b"\n")[:-1]}
        has = lambda a, b: tuple(sorted((a, b))) in out_pairs   # noqa: E731
        assert [has(a, a + 1) for a in range(100, 116, 2)] == [True, False] * 4, [has(a, a + 1) for a in range(100, 116, 2)]
        # which branch each took, from the line's own fields
        for a, f_pos, g_fwd in ((100, 1, 1), (102, 1, 1), (104, 1, 0), (106, 1, 0), (108, 0, 1), (110, 0, 1), (112, 0, 0), (114, 0, 0)):
            f = by[(a, a + 1)]
            g_b, g_e = (int(f[10]), int(f[9])) if f[8] == b"1" else (int(f[9]), int(f[10]))
            assert (int(f[5]) > 0) == bool(f_pos) and (g_b < g_e) == bool(g_fwd), f
        assert int(by[(116, 117)][5]) < 0 and has(116, 117)
        assert by[(120, 121)][3] == b"96.0" and has(120, 121) and by[(122, 123)][3] == b"95.9" and not has(122, 123)
        assert has(124, 125) and not has(126, 127) and has(128, 129) and not has(130, 131)
        assert int(by[(124, 125)][11]) == MIN_LEN and int(by[(126, 127)][11]) == MIN_LEN - 1
        assert int(by[(128, 129)][7]) == MIN_LEN and int(by[(130, 131)][7]) == MIN_LEN - 1
        assert type_of(sg, nm(200, b"E"), nm(202, b"E")) != b"TR" and type_of(sg, nm(210, b"E"), nm(212, b"E")) == b"TR"
        assert type_of(sg, nm(300, b"E"), nm(303, b"E")) == b"TR" and type_of(sg, nm(310, b"E"), nm(313, b"E")) != b"TR"
        assert any(b"-2147483639:" in ln for ln in sg.split(b"\n")) and has(BIG + 5, 3 * BIG + 77)
    return recs, checks


def quantised():
    recs = DG.make_records(seed=8, n_reads=150, genome=3000, contained_share=0.1).copy()
    for k in ("q_bgn", "q_end", "t_end", "m_size"):
        recs[k] = recs[k] // 100 * 100
    return recs


def out_degrees(sg):
    deg = {}
    for ln in sg.split(b"\n")[:-1]:
        v = ln.split()[0]
        deg[v] = deg.get(v, 0) + 1
    return deg


def main():
    import networkx
    sys.path.insert(0, SCRIPTS)
    import ovlp_to_graph
    arrays, cases, summary = {}, {}, {}

    def case(name, recs, min_len=MIN_LEN, min_idt=MIN_IDT, store_recs=True):
        text = ref_text(recs)
        sg = sg_edges(text, min_len, min_idt)
        if store_recs:
            arrays[name + "_recs"] = np.ascontiguousarray(recs.view(np.uint8).reshape(len(recs), -1).T)   # byte columns: they compress far better
        arrays[name + "_sg"] = np.frombuffer(sg, np.uint8)
        cases[name] = dict(min_len=min_len, min_idt=min_idt, recs=name if store_recs else "dense")
        types_ = [ln.split()[-1].decode() for ln in sg.split(b"\n")[:-1]]
        summary[name] = dict(records=len(recs), lines=text.count(b"\n"), edges=len(types_), **{t: types_.count(t) for t in ("G", "TR", "S", "R")},
                             max_out_degree=max(out_degrees(sg).values(), default=0), sha256=hashlib.sha256(sg).hexdigest())
        return text, sg

    dense = DG.make_records(seed=7, n_reads=260, genome=5000, contained_share=0.0)
    _, sg = case("dense", dense, min_len=2000)
    assert summary["dense"]["max_out_degree"] > 64 and all(summary["dense"][t] > 0 for t in ("G", "TR", "S", "R")), summary["dense"]
    case("dense_idt", dense, min_len=2000, min_idt=99.5, store_recs=False)
    case("dense_len", dense, min_len=6000, store_recs=False)
    assert len({summary[k]["sha256"] for k in ("dense", "dense_idt", "dense_len")}) == 3
    case("quant", quantised(), min_len=0)
    a, b = spur_lines()
    _, sg_a = case("spur_a", a)
    _, sg_b = case("spur_b", b)
    assert sorted(sg_a.split(b"\n")) != sorted(sg_b.split(b"\n")), "the two line orders give the same types"
    assert type_of(sg_a, nm(1, b"E"), nm(3, b"E")) == b"G" and type_of(sg_b, nm(1, b"E"), nm(3, b"E")) == b"S"
    recs, checks = directed_records()
    text, sg = case("directed", recs)
    checks(text, sg)
    _, sg = case("none", np.concatenate([dv(1, 2, 1000, dist=400), dv(2, 3, 1000, rl=3000), dv(3, 4, 1000, 0)]))
    assert sg == b""
    _, sg = case("single", np.concatenate([dv(1, 2, 1000, dist=400), dv(5, 6, 1500), dv(2, 3, 1000, rl=3000)]))
    assert sg.count(b"\n") == 2

    prov = dict(generator="tests/golden/make_golden_sgraph.py", reference="oracle/_ref/shmr_dedup",
                reference_sha256=hashlib.sha256(open(REF, "rb").read()).hexdigest(), reference_script="py/scripts/ovlp_to_graph.py",
                reference_script_sha256=hashlib.sha256(open(ovlp_to_graph.__file__, "rb").read()).hexdigest(), networkx=networkx.__version__,
                disable_chimer_bridge_removal=True, lfc=False, hash_seeds=[1, 4242], cases=cases, summary=summary)
    # two files, each below the size of the largest fixture committed before (the quantised case's arrays go to the second)
    second = {k: arrays.pop(k) for k in list(arrays) if k.startswith("quant_")}
    dst = os.path.join(HERE, "sgraph_cases.npz")
    np.savez_compressed(dst, cases=np.array(json.dumps(cases)), **arrays)
    np.savez_compressed(os.path.join(HERE, "sgraph_cases_quant.npz"), **second)
    with open(os.path.join(HERE, "sgraph_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    for name in ("sgraph_cases.npz", "sgraph_cases_quant.npz"):
        assert os.path.getsize(os.path.join(HERE, name)) < 1_000_000, (name, os.path.getsize(os.path.join(HERE, name)))
    print(dst, os.path.getsize(dst), "bytes;", json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6])
    else:
        main()
