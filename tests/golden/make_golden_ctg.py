"""Generator of tests/golden/ctg_cases.npz: hand-made string graphs (their G edge records) and the utg_data and ctg_paths the REAL
py/scripts/ovlp_to_graph.py makes of them -- its function ovlp_to_graph() run in place with runpy from the reference tree, in a temporary
working directory, nothing of it copied.  In the function's globals generate_string_graph is replaced by LOADER below: it reads the
hand-made sg_edges_list into the DiGraph of its G lines, with `best_in` set per G line as the script's own :890-891 set it.  networkx 3.4.2.

    python tests/golden/make_golden_ctg.py [path/to/reference/py/scripts]

The script's later phases pop from sets of strings, so its output varies with the hash seed.  Every case is run under SEEDS; it is STORED
ONLY IF the normal forms (tests/ctg_util.normalise: what the project's rule states as its own is taken out, nothing else) of all runs
agree; the stored files are those of the first seed.  The restatement of the rule (ctg_util.contig_paths) must reproduce every stored
case in normal form, the stored cases must between them show every type and every kind of contig listed in REQUIRED, or nothing is written.
Cases the script has no single answer on are kept as edges only (`stored`: false) and are held to the restatement alone.

The loader is checked against the whole script: on the `quant` records of sgraph_cases.npz, under one seed, the script run from preads.ovl
(the text of oracle/_ref/shmr_dedup) and the loader run from the sg_edges_list that run wrote give byte-equal utg_data and ctg_paths.

The end-to-end expectation: for the stored cases the REAL graph_to_path.py, run in place the same way on (our sg_edges_list text, the
restatement's utg_data, the restatement's ctg_paths), gives <case>_p / <case>_a (only for cases without a compound tie round).

npz keys: <case>_edges (pgx_sgraph_edge records as bytes), <case>_sg (the sg_edges_list text), <case>_utg, <case>_ctg (the script's), <case>_p,
<case>_a; `cases`: a JSON object, case -> summary."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import ctg_util as CU  # noqa: E402
import sgraph_util as SG  # noqa: E402
import tiling_util as TU  # noqa: E402

SCRIPTS = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/py/scripts"
REF_DEDUP = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
SEEDS = (1, 2, 3, 4, 5)
REQUIRED = ("spur:2", "simple_dup", "compound", "contained", "repeat_bridge", "passes_best_in", "stops_at_best_in", "through_compound", "circular_ring",
            "circular_cycle", "long_spur_stays", "second_pass_spur")

LOADER = '''
def _load(args):
    import networkx as nx
    g, edge_data = nx.DiGraph(), {}
    for ln in open("sg_edges_list"):
        v, w, rid, sp, tp, score, idt, ty = ln.split()
        if ty != "G":
            continue
        sp, tp, score = int(sp), int(tp), int(score)
        g.add_edge(v, w, label="%s:%d-%d" % (rid, sp, tp), length=abs(sp - tp), score=score)
        edge_data[(v, w)] = (rid, sp, tp, abs(sp - tp), score, float(idt), ty)
        g.nodes[w]["best_in"] = v
    return g, g.reverse(), edge_data
'''


def run_ovlp_to_graph(files, seed, loader=True, argv=()):
    """utg_data, ctg_paths (and sg_edges_list) after the reference's ovlp_to_graph() ran in a temporary directory holding `files`"""
    with tempfile.TemporaryDirectory() as tmp:
        for fn, data in files.items():
            with open(os.path.join(tmp, fn), "wb") as f:
                f.write(data)
        script = os.path.join(SCRIPTS, "ovlp_to_graph.py")
        if loader:
            code = ("import os, runpy, sys\nos.chdir(%r)\ng = runpy.run_path(%r, run_name='ref')\nfn = g['ovlp_to_graph']\n%s\nfn.__globals__['generate_string_graph'] = _load\nfn(None)\n"
                    % (tmp, script, LOADER))
        else:
            code = "import os, runpy, sys\nos.chdir(%r)\nsys.argv = %r\nrunpy.run_path(%r, run_name='__main__')\n" % (tmp, ["ovlp_to_graph.py"] + list(argv), script)
        p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONHASHSEED=str(seed)), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if p.returncode:
            return None
        return {fn: open(os.path.join(tmp, fn), "rb").read() for fn in ("sg_edges_list", "utg_data", "ctg_paths")}


def run_graph_to_path(sg, utg, ctg):
    with tempfile.TemporaryDirectory() as tmp:
        for fn, data in (("sg_edges_list", sg), ("utg_data", utg), ("ctg_paths", ctg)):
            with open(os.path.join(tmp, fn), "wb") as f:
                f.write(data)
        code = "import os, runpy, sys\nos.chdir(%r)\nsys.argv = ['graph_to_path.py']\nrunpy.run_path(%r, run_name='__main__')\n" % (tmp, os.path.join(SCRIPTS, "graph_to_path.py"))
        subprocess.run([sys.executable, "-c", code], check=True, env=dict(os.environ, PYTHONHASHSEED="1"), stderr=subprocess.DEVNULL)
        return open(os.path.join(tmp, "p_ctg_tiling_path"), "rb").read(), open(os.path.join(tmp, "a_ctg_tiling_path"), "rb").read()


from ctg_util import MOTIFS, Graph  # noqa: E402  (the hand-made graphs: shared with the tests)


def sg_text(lines) -> bytes:
    nm = lambda k: CU.node_name(k).decode()   # noqa: E731
    return "".join("%s %s %s %5d %5d %5d %5.2f %s\n" % (nm(v), nm(w), nm(w)[:9], sp, tp, score, 99.9, "G") for v, w, sp, tp, score in lines).encode()


def features(utg, ctg, edges):
    """which of REQUIRED a stored case shows (from the script's files and the restatement's trace)"""
    f = set()
    ulines = [ln.split(b" ") for ln in utg.split(b"\n")[:-1]]
    for x in ulines:
        f.add(x[3].decode())
    clines = [[y for y in ln.split(b" ") if y] for ln in ctg.split(b"\n")[:-1]]
    for c in clines:
        subs = c[6].split(b"|")
        if b"~NA~" in c[6]:
            f.add("through_compound")
        if c[1] == b"ctg_circular":
            f.add("circular_ring" if not c[0][-1:] in (b"F", b"R") else ("circular_cycle" if len(subs) > 1 else "circular_other"))
    return f


def main():
    import networkx
    arrays, cases, unstable = {}, {}, []
    graphs = {}
    for name, make in MOTIFS.items():
        g = Graph()
        make(g)
        graphs[name] = g.lines
    g = Graph()
    for k, make in enumerate(MOTIFS.values()):
        g.base = 1000 * (k + 1)
        make(g)
    graphs["all"] = g.lines
    g = Graph()
    for k, name in enumerate(("ring", "spur", "compound")):
        g.base = 500 * (k + 1)
        MOTIFS[name](g)
    graphs["ring_chain_bubble"] = g.lines
    shown = set()
    for name, lines in graphs.items():
        sg = sg_text(lines)
        edges = CU.edges_of_g_lines(lines)
        runs = [run_ovlp_to_graph({"sg_edges_list": sg}, seed) for seed in SEEDS]
        arrays[name + "_edges"] = np.frombuffer(edges.tobytes(), np.uint8)
        arrays[name + "_sg"] = np.frombuffer(sg, np.uint8)
        ours = CU.contig_paths(edges)
        forms = [CU.normalise(r["utg_data"], r["ctg_paths"]) if r else None for r in runs]
        stable = all(f is not None and f == forms[0] for f in forms)
        summary = dict(CU.stats_of(ours), g_edges=len(lines), stored=bool(stable))
        if stable:
            assert CU.normalise(ours.utg_text, ours.ctg_text) == forms[0], "%s: the restatement and the script differ" % name
            arrays[name + "_utg"] = np.frombuffer(runs[0]["utg_data"], np.uint8)
            arrays[name + "_ctg"] = np.frombuffer(runs[0]["ctg_paths"], np.uint8)
            feats = features(runs[0]["utg_data"], runs[0]["ctg_paths"], edges)
            summary["features"] = sorted(feats)
            shown |= feats
            _, _, st = TU.tiling_rule(sg, ours.utg_text, ours.ctg_text)
            if st["compound_tie_rounds"] == 0:
                p, a = run_graph_to_path(sg, ours.utg_text, ours.ctg_text)
                arrays[name + "_p"], arrays[name + "_a"] = np.frombuffer(p, np.uint8), np.frombuffer(a, np.uint8)
                summary["tiling"] = True
        else:
            unstable.append(name)
        cases[name] = summary
    # what the files alone cannot show is read off the motifs that are stored: their doc strings say what they are made to show
    for name, feat in (("yjoin", ("passes_best_in", "stops_at_best_in")), ("spur", ("long_spur_stays",)), ("spur2", ("second_pass_spur",))):
        if cases[name]["stored"]:
            shown.update(feat)
    y = CU.contig_paths(CU.fixture_edges(arrays, "yjoin")) if cases["yjoin"]["stored"] else None
    assert y is not None and sorted(len(r) for r in y.rows) == [1, 1, 2, 2], "yjoin: one chain must pass the best_in test and one stop at it"
    assert cases["spur"]["spur2"] == 2 and cases["spur"]["spur_rounds"] == 1 and cases["spur2"]["spur2"] == 2 and cases["spur2"]["spur_rounds"] == 1
    s2 = CU.contig_paths(CU.fixture_edges(arrays, "spur2"))
    assert b" spur:2 60000 " in s2.utg_text
    missing = [r for r in REQUIRED if r not in shown]
    assert not missing, ("the stored cases do not show", missing, "unstable:", unstable)
    assert sum(c["stored"] for c in cases.values()) >= 8, unstable
    # ---- the loader against the whole script
    zs, sc = SG.load_fixture()
    recs = SG.fixture_recs(zs, sc["quant"]["recs"])
    text = subprocess.run([REF_DEDUP], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout
    whole = run_ovlp_to_graph({"preads.ovl": text + b"-\n"}, 1, loader=False,
                              argv=["--min_len", str(sc["quant"]["min_len"]), "--min_idt", str(sc["quant"]["min_idt"]), "--disable_chimer_bridge_removal"])
    via_loader = run_ovlp_to_graph({"sg_edges_list": whole["sg_edges_list"]}, 1)
    assert whole is not None and via_loader is not None
    assert (whole["utg_data"], whole["ctg_paths"]) == (via_loader["utg_data"], via_loader["ctg_paths"]), "the loader and the whole script differ"
    sha = lambda fn: hashlib.sha256(open(os.path.join(SCRIPTS, fn), "rb").read()).hexdigest()   # noqa: E731
    prov = dict(generator="tests/golden/make_golden_ctg.py", graph_script="py/scripts/ovlp_to_graph.py", graph_script_sha256=sha("ovlp_to_graph.py"),
                tiling_script="py/scripts/graph_to_path.py", tiling_script_sha256=sha("graph_to_path.py"), hash_seeds=list(SEEDS), networkx=networkx.__version__,
                loader_check="quant records of sgraph_cases.npz, seed 1: byte-equal utg_data and ctg_paths", no_single_answer=unstable, shown=sorted(shown), cases=cases)
    dst = os.path.join(HERE, "ctg_cases.npz")
    np.savez_compressed(dst, cases=np.array(json.dumps(cases)), **arrays)
    with open(os.path.join(HERE, "ctg_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    assert os.path.getsize(dst) < 1_000_000, os.path.getsize(dst)
    print(dst, os.path.getsize(dst), "bytes; no single answer:", unstable, "; shown:", sorted(shown))


if __name__ == "__main__":
    main()
