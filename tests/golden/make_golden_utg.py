"""Generator of tests/golden/utg_cases.npz: inputs -- record sets built with tests/dedup_graph_util (make_records / rec), or edge arrays --
and what the reference's own identify_simple_paths (py/scripts/ovlp_to_graph.py:1033-1144, imported in place from the reference tree,
nothing of it copied) makes of them, normalised.

Record cases: the REAL reference shmr_dedup's text of the records (oracle/_ref/shmr_dedup, built by `make -C oracle ref`), the real
generate_string_graph on it (disable_chimer_bridge_removal=True, lfc=False), the DiGraph of the G edges of the returned edge_data as
ovlp_to_graph() builds it (:1368-1380), the real identify_simple_paths.  Edge-array cases: the DiGraph and edge_data straight from the
array.  Every case runs in two child processes with PYTHONHASHSEED 1 and 4242; each child asserts via in (path[1], path[-2]) for every
unitig and then normalises what varies with the seed:
  * via is dropped;
  * a circular path (a closed path of simple nodes only) is rotated to start at the tail of its edge that comes first in the edge list;
  * the lines are sorted by the creation index of their first edge.
The fixture is written only if the two seeds agree.  A line: 's t simple length score n0~n1~...~nk'.  networkx 3.4.2.

    python tests/golden/make_golden_utg.py [path/to/reference/py/scripts]

Cases (npz keys <name>_utg; <name>_recs -- byte columns as in sgraph_cases.npz -- or <name>_edges -- pgx_sgraph_edge records as bytes):
  single   one surviving row: two unitigs of one edge each, via == t
  chains   disjoint read chains of 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256 and 257 edges, the records shuffled
  long     one chain of 4,100 reads: more than 12 doubling rounds, a line of about 49 KB
  rings    rings of 3, 64 and 1,000 reads, the records shuffled: circular unitigs, the cut rule
  dense, quant   the records of sgraph_cases.npz / sgraph_cases_quant.npz with their thresholds (not stored again)
  none     every row filtered: no unitig
  forks    (edge array) a chain with one extra edge out of an inner node and one into another; single-edge unitigs between two non-simple
           nodes; a cycle through exactly one non-simple node; an all-simple ring; every edge with its reverse
  typed    (edge array) forks with TR, S and R edges mixed in
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
import sgraph_util as SG  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
SCRIPTS = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "--child" else "/root/reference/py/scripts"
SEEDS = (1, 4242)
MIN_LEN, MIN_IDT = 4000, 96.0
rec = DG.rec


# ---- the child: one run of the reference's functions in this process (whose hash seed the parent chose) ------------------------------------
def child(scripts, kind, src, min_len, min_idt, out_path):
    sys.path.insert(0, scripts)
    import networkx as nx
    import ovlp_to_graph as O
    if kind == "recs":
        text = open(src, "rb").read()
        with tempfile.TemporaryDirectory() as tmp:
            os.chdir(tmp)
            with open("preads.ovl", "wb") as f:
                f.write(text + b"-\n")
            _, _, edge_data = O.generate_string_graph(types.SimpleNamespace(overlap_file="preads.ovl", min_len=int(min_len), min_idt=float(min_idt), lfc=False,
                                                                            disable_chimer_bridge_removal=True))
            lines = [ln.split() for ln in open("sg_edges_list")]                 # the file lists the edges in creation order
            os.chdir("/")
        order = [(f[0], f[1]) for f in lines]
        assert set(edge_data) == {(f[0], f[1]) for f in lines if f[7] == "G"}       # (the function returns the G edges only)
    else:
        edges = np.load(src)
        edge_data, order = {}, []
        for e in edges:
            v = SG.node_name(int(e["v_rid"]) << 1 | int(e["v_end"])).decode()
            w = SG.node_name(int(e["w_rid"]) << 1 | int(e["w_end"])).decode()
            edge_data[(v, w)] = ("%09d" % int(e["label_rid"]), int(e["sp"]), int(e["tp"]), abs(int(e["sp"]) - int(e["tp"])), int(e["score"]), int(e["idt_tenths"]) / 10.0,
                                 SG.TYPE_NAMES[int(e["type"])].decode())
            order.append((v, w))
    assert len(order) == len(set(order)) >= len(edge_data)
    index = {vw: k for k, vw in enumerate(order)}
    sg2 = nx.DiGraph()
    for v, w in edge_data:                                                       # ovlp_to_graph(), :1368-1380
        assert (O.reverse_end(w), O.reverse_end(v)) in edge_data
        rid, sp, tp, length, score, identity, type_ = edge_data[(v, w)]
        if type_ != "G":
            continue
        sg2.add_edge(v, w, label="%s:%d-%d" % (rid, sp, tp), length=length, score=score)
    simple_paths = O.identify_simple_paths(sg2, edge_data)
    is_simple = lambda x: sg2.in_degree(x) == 1 and sg2.out_degree(x) == 1     # noqa: E731
    rows = []
    for (s, via, t), (length, score, path) in simple_paths.items():
        assert via in (path[1], path[-2]), (s, via, t)
        assert path[0] == s and path[-1] == t
        if s == t and is_simple(s):                                              # a ring of simple nodes: open it at its first edge's tail
            assert all(is_simple(x) for x in path)
            k = min(range(len(path) - 1), key=lambda i: index[(path[i], path[i + 1])])
            nodes = path[:-1][k:] + path[:-1][:k]
            path = nodes + [nodes[0]]
        rows.append((index[(path[0], path[1])], "%s %s simple %d %d %s\n" % (path[0], path[-1], length, score, "~".join(path))))
    rows.sort()
    assert sum(ln.count("~") for _, ln in rows) == sg2.number_of_edges()         # every directed G edge in exactly one unitig
    with open(out_path, "w") as f:
        f.write("".join(ln for _, ln in rows))


# ---- the parent ------------------------------------------------------------------------------------------------------------------------------
def run_seeds(kind, src, min_len, min_idt) -> bytes:
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for seed in SEEDS:
            op = os.path.join(tmp, "utg%d" % seed)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", SCRIPTS, kind, src, str(min_len), str(min_idt), op], check=True,
                           env=dict(os.environ, PYTHONHASHSEED=str(seed)))
            outs.append(open(op, "rb").read())
    if outs[0] != outs[1]:
        sys.exit("two hash seeds give two normalised outputs: the fixture is NOT written")
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


def chain(first, n_edges):
    return [dv(i, i + 1, 1000 + (i % 7) * 10, 1200 + (i % 5) * 10, m_size=5000 + i % 13) for i in range(first, first + n_edges)]


def ring(first, n):
    return [dv(first + i, first + (i + 1) % n, 1000 + (i % 7) * 10, 1200 + (i % 5) * 10, m_size=5000 + i % 13) for i in range(n)]


def shuffled(parts, seed):
    recs = np.concatenate(parts)
    np.random.default_rng(seed).shuffle(recs)
    return recs


CHAIN_EDGES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)


def chains_records():
    parts, at = [], 0
    for k in CHAIN_EDGES:
        parts += chain(at, k)
        at += k + 10
    return shuffled(parts, 5)


def fork_edges(typed: bool) -> np.ndarray:
    E, B = 1, 0
    pairs = []

    def pair(a, b, L, sc):          # a -> b and its reverse
        pairs.append((a, E, b, E, L, sc)), pairs.append((b, B, a, B, L + 7, sc))

    for i in range(11):
        pair(i, i + 1, 1000 + i, 5000 + i)
    pair(5, 20, 900, 4000), pair(21, 8, 800, 4100)                         # one more out of 5:E, one more into 8:E
    pair(30, 31, 700, 3000), pair(30, 32, 710, 3010), pair(33, 31, 720, 3020)   # 30:E -> 31:E joins two non-simple nodes
    pair(40, 41, 600, 2000), pair(41, 42, 610, 2010), pair(42, 40, 620, 2020), pair(43, 40, 630, 2030)   # a cycle through 40:E alone
    for i in range(6):
        pair(50 + i, 50 + (i + 1) % 6, 500 + i, 1000 + i)                  # a ring of simple nodes
    rng = np.random.default_rng(9)
    rng.shuffle(pairs)
    rows = [(v, w, w, L, 0, ve, we, SG.G, 0, sc, 990) for v, ve, w, we, L, sc in pairs]
    if typed:                                                                # reduced edges, also where they would change a degree
        other = []
        for k, (a, b) in enumerate(((3, 9), (2, 7), (41, 50), (52, 55), (60, 61), (10, 30))):
            t = (SG.TR, SG.S, SG.R)[k % 3]
            other += [(a, b, b, 3000 + k, 0, E, E, t, 0, 100 + k, 970), (b, a, a, 3100 + k, 0, B, B, t, 0, 100 + k, 970)]
        for row in other:
            rows.insert(int(rng.integers(0, len(rows) + 1)), row)
    edges = np.zeros(len(rows), SG.EDGE_DTYPE)
    for k, row in enumerate(rows):
        edges[k] = row
    return edges


def main():
    import networkx
    sys.path.insert(0, SCRIPTS)
    import ovlp_to_graph
    arrays, cases, summary = {}, {}, {}
    tmpdir = tempfile.mkdtemp()

    def summarise(name, utg, n_in):
        f = [ln.split(b" ") for ln in utg.split(b"\n")[:-1]]
        n_edges = [x[5].count(b"~") for x in f]
        summary[name] = dict(input=n_in, unitigs=len(f), g_edges=sum(n_edges), longest_edges=max(n_edges, default=0), closed=sum(x[0] == x[1] for x in f),
                             longest_line=max((len(ln) + 1 for ln in utg.split(b"\n")[:-1]), default=0), sha256=hashlib.sha256(utg).hexdigest())

    def rec_case(name, recs, min_len=MIN_LEN, min_idt=MIN_IDT, stored_in=None):
        src = os.path.join(tmpdir, name + ".text")
        with open(src, "wb") as f:
            f.write(ref_text(recs))
        utg = run_seeds("recs", src, min_len, min_idt)
        if stored_in is None:
            arrays[name + "_recs"] = np.ascontiguousarray(recs.view(np.uint8).reshape(len(recs), -1).T)
        arrays[name + "_utg"] = np.frombuffer(utg, np.uint8)
        cases[name] = dict(kind="recs", recs_in=stored_in or "utg", recs_of=name, min_len=min_len, min_idt=min_idt)
        summarise(name, utg, len(recs))
        return utg

    def edge_case(name, edges):
        src = os.path.join(tmpdir, name + ".npy")
        np.save(src, edges)
        utg = run_seeds("edges", src, 0, 0)
        arrays[name + "_edges"] = np.frombuffer(edges.tobytes(), np.uint8)
        arrays[name + "_utg"] = np.frombuffer(utg, np.uint8)
        cases[name] = dict(kind="edges")
        summarise(name, utg, len(edges))
        return utg

    utg = rec_case("single", np.concatenate([dv(1, 2, 1000, dist=400), dv(5, 6, 1500), dv(2, 3, 1000, rl=3000)]))
    assert summary["single"]["unitigs"] == 2 and summary["single"]["g_edges"] == 2
    rec_case("chains", chains_records())
    assert summary["chains"]["unitigs"] == 2 * len(CHAIN_EDGES) and summary["chains"]["g_edges"] == 2 * sum(CHAIN_EDGES) and summary["chains"]["closed"] == 0
    rec_case("long", np.concatenate(chain(0, 4099)))
    assert summary["long"]["unitigs"] == 2 and summary["long"]["longest_edges"] == 4099 and summary["long"]["longest_line"] > 40000
    rec_case("rings", shuffled(ring(0, 3) + ring(100, 64) + ring(1000, 1000), 6))
    assert summary["rings"]["unitigs"] == summary["rings"]["closed"] == 6 and summary["rings"]["g_edges"] == 2 * 1067
    zs, sc = SG.load_fixture()
    for name in ("dense", "quant"):
        rec_case(name, SG.fixture_recs(zs, sc[name]["recs"]), sc[name]["min_len"], sc[name]["min_idt"], stored_in="sgraph")
        assert summary[name]["unitigs"] > 10
    utg = rec_case("none", np.concatenate([dv(1, 2, 1000, dist=400), dv(2, 3, 1000, rl=3000), dv(3, 4, 1000, 0)]))
    assert utg == b""
    edge_case("forks", fork_edges(False))
    utg_typed = edge_case("typed", fork_edges(True))
    for name in ("forks", "typed"):
        s = summary[name]
        assert s["g_edges"] == 2 * 26 and s["closed"] == 4, s          # closed: the ring and the cycle through 40:E, each with its reverse
    assert sorted(arrays["forks_utg"].tobytes().split(b"\n")) == sorted(utg_typed.split(b"\n"))   # the reduced edges change nothing but the order

    prov = dict(generator="tests/golden/make_golden_utg.py", reference="oracle/_ref/shmr_dedup", reference_sha256=hashlib.sha256(open(REF, "rb").read()).hexdigest(),
                reference_script="py/scripts/ovlp_to_graph.py", reference_script_sha256=hashlib.sha256(open(ovlp_to_graph.__file__, "rb").read()).hexdigest(),
                reference_function="identify_simple_paths", networkx=networkx.__version__, disable_chimer_bridge_removal=True, lfc=False, hash_seeds=list(SEEDS),
                normalisation=["via dropped (asserted to be path[1] or path[-2])", "circular paths rotated to the tail of their first edge in the edge list",
                               "lines sorted by the creation index of their first edge"], cases=cases, summary=summary)
    dst = os.path.join(HERE, "utg_cases.npz")
    np.savez_compressed(dst, cases=np.array(json.dumps(cases)), **arrays)
    with open(os.path.join(HERE, "utg_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    assert os.path.getsize(dst) < 1_000_000, os.path.getsize(dst)
    print(dst, os.path.getsize(dst), "bytes;", json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:8])
    else:
        main()
