"""Generator of tests/golden/tiling_cases.npz: the three inputs of py/scripts/graph_to_path.py (sg_edges_list, utg_data, ctg_paths) and the
two files the REAL script writes from them -- run in place with runpy from the reference tree, in a temporary working directory, nothing
of it copied.  networkx 3.4.2.

    python tests/golden/make_golden_tiling.py [path/to/reference/py/scripts]

Real graphs (`real_*`): the reference's own ovlp_to_graph.py --disable_chimer_bridge_removal, run in place the same way, on the text the
real shmr_dedup (oracle/_ref/shmr_dedup) makes of the record sets of sgraph_cases.npz.  Its later phases pop from sets, so its output
varies with the hash seed; any one output of it is a valid input, and the one used is stored.
Hand-made cases: built with tests/tiling_util.Builder (see CASES below).

Ties: in every round of every compound unitig the generator enumerates all simple s -> t paths (nx.all_simple_paths) of the graph as it
stands; a case in which two share the minimum weight is DROPPED (the script's choice there depends on networkx), and the rule's own
count (tiling_util.tiling_rule: compound_tie_rounds) must agree with the enumeration.  At least 6 compound cases must remain.
The rule's restatement must reproduce every stored case, or nothing is written.

npz keys: <case>_sg, _utg, _ctg, _p, _a as bytes; `cases`: a JSON object, case -> summary."""
import hashlib
import json
import os
import runpy
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sgraph_util as SG  # noqa: E402
import tiling_util as TU  # noqa: E402
from tiling_util import B, E, Builder, bubble, key, name, rev  # noqa: E402

SCRIPTS = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/py/scripts"
REF_DEDUP = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")


def run_script(script, argv, files):
    """the reference script run in place in a temporary directory holding `files`; returns the directory's files afterwards"""
    with tempfile.TemporaryDirectory() as tmp:
        for fn, data in files.items():
            with open(os.path.join(tmp, fn), "wb") as f:
                f.write(data)
        code = ("import os, runpy, sys\nos.chdir(%r)\nsys.argv = %r\nrunpy.run_path(%r, run_name='__main__')\n" % (tmp, [script] + argv, os.path.join(SCRIPTS, script)))
        subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, PYTHONHASHSEED="1"), stderr=subprocess.DEVNULL)
        return {fn: open(os.path.join(tmp, fn), "rb").read() for fn in os.listdir(tmp) if os.path.isfile(os.path.join(tmp, fn))}


def real_script(sg, utg, ctg):
    out = run_script("graph_to_path.py", [], {"sg_edges_list": sg, "utg_data": utg, "ctg_paths": ctg})
    return out["p_ctg_tiling_path"], out["a_ctg_tiling_path"]


def tie_census(sg, utg, ctg):
    """(rounds, rounds with more than one minimum-weight simple path by enumeration, the rule's outputs)"""
    import networkx as nx
    seen = [0, 0]

    def on_round(adj, gone, s, t, weight):
        g = nx.DiGraph()
        for u, outs in adj.items():
            for v, w in outs:
                if (u, v) not in gone:
                    g.add_edge(u, v, w=w)
        weights = [sum(g[a][b]["w"] for a, b in zip(p[:-1], p[1:])) for p in nx.all_simple_paths(g, s, t)]
        assert min(weights) == weight
        seen[0] += 1
        seen[1] += weights.count(weight) > 1

    p, a, st = TU.tiling_rule(sg, utg, ctg, on_round)
    assert st["compound_tie_rounds"] == seen[1], (st, seen)
    return seen[0], seen[1], p, a, st


# ---- hand-made cases --------------------------------------------------------------------------------------------------------------------
def chain_nodes(first, n, end=E):
    return [key(first + i, end) for i in range(n + 1)]


def case_one_edge():
    b = Builder(1)
    b.contig("000000F", [b.simple(chain_nodes(1, 1))], key(2, E))
    return b


def case_joins():
    b = Builder(2)
    u = [b.simple(chain_nodes(1, 3)), b.simple([key(4, E), key(9, B), key(10, B), key(11, E)]), b.simple(chain_nodes(11, 2))]
    b.contig("000000F", u, key(13, E))
    return b


def case_s_gt_t():
    b = Builder(3)
    b.contig("000000F", [b.simple(chain_nodes(1, 5, B))], key(6, B))
    return b


def case_ring():
    b = Builder(4)
    nodes = chain_nodes(1, 4) + [key(1, E)]
    u = b.simple(nodes)
    b.ctg.append("%6d %s %s %s %d %d %s\n" % (3, "ctg_circular", u, name(key(1, E)), 0, 0, u))
    return b


def case_duals():
    b = Builder(5)
    f = chain_nodes(1, 3)
    r = [rev(x) for x in reversed(f)]
    uf, ur = b.simple(f), b.simple(r)
    b.contig("000000F", [uf], f[-1])
    b.contig("000000R", [ur], r[-1])                       # the dual of the first row: skipped
    b.contig("000001F", [uf], f[-1])                       # the kept key again: kept
    pal = [key(20, E), key(21, E), key(20, B)]             # a self-dual key: (rev t0, rev s0) == (s0, t0)
    up = b.simple(pal)
    b.contig("000002F", [up], pal[-1])
    b.contig("000002R", [up], pal[-1])                     # ... only the first is kept
    g = chain_nodes(30, 2)
    ug, ugr = b.simple(g), b.simple([rev(x) for x in reversed(g)])
    b.contig("000003R", [ugr], rev(g[0]))                  # here the reverse comes first and wins
    b.contig("000003F", [ug], g[-1])
    return b


def case_contained_only():
    b = Builder(6)
    b.contig("000000F", [b.simple(chain_nodes(1, 2), kind="contained")], key(3, E))
    b.contig("000001F", [b.simple(chain_nodes(5, 2))], key(7, E))
    b.utg.append("%s %s %s spur:2 10 10 %s\n" % (name(key(90, E)), name(key(91, E)), name(key(92, E)), "x~y"))   # a dropped type: never parsed further
    return b


def case_bubble2():
    """a two-way bubble of weights 15,000 and 16,100: the heavier branch (through read 5) goes into the primary path"""
    b = Builder(7)
    s, t = key(3, E), key(9, E)
    b.edge(key(1, E), key(2, E), 500), b.edge(key(2, E), s, 600)
    pre = b.simple([key(1, E), key(2, E), s])
    b.edge(s, key(5, E), 710, 7100, "99.60", s=1000), b.edge(key(5, E), t, 800, 9000, "99.50")
    b.edge(s, key(6, E), 900, 7000, "99.40"), b.edge(key(6, E), t, 650, 8000, "99.30")
    c = b.compound(s, t, [b.simple([s, key(5, E), t]), b.simple([s, key(6, E), t])])
    post = b.simple([t, key(10, E), key(11, B)])
    b.contig("000000F", [pre, c, post], key(11, B))
    return b


def case_bubble3():
    b = Builder(8)
    s, t = key(1, E), key(2, E)
    c, _ = bubble(b, s, t, 10, 3, [1, 2, 3])
    b.contig("000000F", [b.simple([key(5, E), s]), c], t)
    return b


def case_compound_first():
    b = Builder(9)
    s, t = key(1, E), key(2, E)
    c, nxt = bubble(b, s, t, 10, 2, [2, 1])
    b.contig("000000F", [c, b.simple([t, key(nxt, B), key(nxt + 1, E)])], key(nxt + 1, E))
    return b


def case_two_compounds():
    b = Builder(10)
    s, m, t = key(1, E), key(2, E), key(3, B)
    c1, nxt = bubble(b, s, m, 10, 2, [1, 3])
    c2, nxt = bubble(b, m, t, nxt, 3, [2, 1, 1])
    b.contig("000000F", [c1, c2], t)
    return b


def case_shared_subs():
    """a bundle whose sub-unitigs share an inner node and an edge: the expanded graph is not the contracted one"""
    b = Builder(11)
    s, t, x = key(1, E), key(2, E), key(3, E)
    subs = [b.simple([s, x]), b.simple([x, key(4, E), t]), b.simple([x, key(5, E), key(6, E), t]), b.simple([s, key(7, E), t]), b.simple([s, x, key(8, E), t], kind="contained")]
    b.contig("000000F", [b.compound(s, t, subs)], t)
    return b


def case_fork_bundle():
    """a bundle that forks again inside a branch, used by two contigs"""
    b = Builder(17)
    s, t, x, y = key(1, E), key(2, E), key(3, B), key(4, E)
    subs = [b.simple([s, key(5, E), x]), b.simple([x, key(6, E), y]), b.simple([x, key(7, B), key(8, B), y]), b.simple([y, t]), b.simple([s, key(9, E), key(10, E), t])]
    c = b.compound(s, t, subs)
    b.contig("000000F", [b.simple([key(20, E), key(21, E), s]), c], t)
    b.contig("000001F", [c, b.simple([t, key(22, E)])], key(22, E))
    return b


def case_long():
    b = Builder(12)
    nodes = [key(1 + i, int(b.rng.integers(0, 2))) for i in range(5001)]
    b.contig("000000F", [b.simple(nodes)], nodes[-1])
    return b


def case_wide():
    b = Builder(13)
    n = [key(1234567, E), key(2147483647, E), key(1000000000, B)]
    b.edge(n[0], n[1], 1234567, 98765432101, "100.00", s=7654321)
    b.edge(n[1], n[2], 99999, 123456, " 7.05", s=100000)
    b.contig("ctg.with-a_longer.name/7", [b.simple(n)], n[-1])
    return b


def case_no_newline():
    b = Builder(14)
    b.contig("000000F", [b.simple(chain_nodes(1, 3))], key(4, E))
    return b


def case_empty_ctg():
    b = Builder(15)
    b.simple(chain_nodes(1, 3))
    return b


def case_blanks():
    """blank lines, runs of blanks and tabs between the fields, other edge types among the G lines"""
    b = Builder(16)
    b.contig("000000F", [b.simple(chain_nodes(1, 6))], key(7, E))
    b.edge(key(50, E), key(51, B), 100, 5, kind="TR"), b.edge(key(52, E), key(53, E), 100, 5, kind="C")
    b.sg = [ln.replace(" ", "\t  ", 1) for ln in b.sg]
    b.sg.insert(2, "\n"), b.sg.insert(4, "   \n")
    b.utg.insert(0, "\n"), b.ctg.append("\n")
    return b


CASES = dict(one_edge=case_one_edge, joins=case_joins, s_gt_t=case_s_gt_t, ring=case_ring, duals=case_duals, contained_only=case_contained_only, bubble2=case_bubble2,
             bubble3=case_bubble3, compound_first=case_compound_first, two_compounds=case_two_compounds, shared_subs=case_shared_subs, fork_bundle=case_fork_bundle, long=case_long, wide=case_wide,
             no_newline=case_no_newline, empty_ctg=case_empty_ctg)


def real_graph(recs, min_len, min_idt):
    text = subprocess.run([REF_DEDUP], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout
    out = run_script("ovlp_to_graph.py", ["--min_len", str(min_len), "--min_idt", str(min_idt), "--disable_chimer_bridge_removal"], {"preads.ovl": text + b"-\n"})
    return out["sg_edges_list"], out["utg_data"], out["ctg_paths"]


def main():
    import networkx
    arrays, cases, dropped = {}, {}, []

    def add(case, sg, utg, ctg):
        rounds, ties, rp, ra, st = tie_census(sg, utg, ctg)
        if ties:
            dropped.append(case)
            return
        p, a = real_script(sg, utg, ctg)
        assert (rp, ra) == (p, a), "%s: the rule's restatement and the real script differ" % case
        for part, data in zip(("sg", "utg", "ctg", "p", "a"), (sg, utg, ctg, p, a)):
            arrays["%s_%s" % (case, part)] = np.frombuffer(data, np.uint8)
        cases[case] = dict(st, rounds=rounds, sha256_p=hashlib.sha256(p).hexdigest(), sha256_a=hashlib.sha256(a).hexdigest())

    for case, make in CASES.items():
        sg, utg, ctg = make().files()
        if case == "no_newline":
            sg, utg, ctg = sg[:-1], utg[:-1], ctg[:-1]
        add(case, sg, utg, ctg)
    # blank lines end the script (it unpacks every line): that case is held to the rule alone, which skips them
    sg, utg, ctg = case_blanks().files()
    p, a, st = TU.tiling_rule(sg, utg, ctg)
    strip = lambda t: b"".join(ln + b"\n" for ln in t.split(b"\n") if ln.strip())   # noqa: E731
    assert real_script(strip(sg), strip(utg), strip(ctg)) == (p, a)
    for part, data in zip(("sg", "utg", "ctg", "p", "a"), (sg, utg, ctg, p, a)):
        arrays["blanks_%s" % part] = np.frombuffer(data, np.uint8)
    cases["blanks"] = dict(st, rounds=0, note="expected output: the real script on the files without their blank lines")
    zs, sc = SG.load_fixture()
    for nm in ("dense", "quant"):
        add("real_" + nm, *real_graph(SG.fixture_recs(zs, sc[nm]["recs"]), sc[nm]["min_len"], sc[nm]["min_idt"]))
    b2 = arrays["bubble2_p"].tobytes()
    assert b"000000F 000000003:E 000000005:E 000000005 1000 1710 7100 99.60 1100 710\n" in b2 and arrays["bubble2_a"].tobytes().startswith(b"000000F-001-01 "), b2
    compound = [c for c, s in cases.items() if s["rounds"]]
    assert len(compound) >= 6, (compound, dropped)
    assert cases["bubble3"]["rounds"] == 3 and cases["two_compounds"]["alternates"] == 3 and b"-002-02 " in arrays["two_compounds_a"].tobytes()
    assert cases["duals"]["ctg_kept"] == 4 and cases["duals"]["ctg_skipped"] == 3 and cases["contained_only"]["ctg_empty"] == 1
    assert cases["long"]["p_rows"] == 5000 and cases["ring"]["p_rows"] == 5 and arrays["ring_p"].tobytes().startswith(b"3 ")
    sha = lambda fn: hashlib.sha256(open(os.path.join(SCRIPTS, fn), "rb").read()).hexdigest()   # noqa: E731
    prov = dict(generator="tests/golden/make_golden_tiling.py", reference_script="py/scripts/graph_to_path.py", reference_script_sha256=sha("graph_to_path.py"),
                graph_script="py/scripts/ovlp_to_graph.py", graph_script_sha256=sha("ovlp_to_graph.py"), graph_options="--disable_chimer_bridge_removal", hash_seed=1,
                reference_dedup_sha256=hashlib.sha256(open(REF_DEDUP, "rb").read()).hexdigest(), networkx=networkx.__version__, dropped_for_ties=dropped,
                compound_cases=compound, cases=cases)
    dst = os.path.join(HERE, "tiling_cases.npz")
    np.savez_compressed(dst, cases=np.array(json.dumps(cases)), **arrays)
    with open(os.path.join(HERE, "tiling_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    assert os.path.getsize(dst) < 1_000_000, os.path.getsize(dst)
    print(dst, os.path.getsize(dst), "bytes; dropped:", dropped, "; compound:", compound)


if __name__ == "__main__":
    main()
