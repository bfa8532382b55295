"""Phase 1 of unitig construction in plain Python over arrays: from edge records in creation order to the `simple` lines of utg_data.
TEST INFRASTRUCTURE, written from the rule as the project states it ("unitigs"; include/pgx.h), not from the script: no graph
objects and no sets -- edges are numbered in creation order, a node is the integer (rid << 1) | end, and everything else is a list or a
dictionary indexed by those.

  edges     only type G takes part
  checks    no G edge joins the two ends of one read; no (v, w) twice; every (v, w) has its reverse (w ^ 1, v ^ 1).  The first rule that
            fails raises Invalid with the smallest offending creation index (of a repeated (v, w): the later edge)
  simple    a node with exactly one G in-edge and one G out-edge
  linear    every edge that leaves a non-simple node starts a unitig, which follows the single out-edge of every simple node it reaches
  circular  what is left lies on rings of simple nodes: a ring is cut at the tail of its edge with the smallest creation index
  fields    length = sum |sp - tp|, score = sum of scores, via = the path's second node
  order     by the creation index of the first edge
"""
import json
import os

import numpy as np

from sgraph_util import EDGE_DTYPE, G, node_name

UNITIG_DTYPE = np.dtype([("s_rid", "<u4"), ("t_rid", "<u4"), ("via_rid", "<u4"), ("s_end", "u1"), ("t_end", "u1"), ("via_end", "u1"), ("circular", "u1"),
                         ("n_edges", "<u4"), ("pad", "<u4"), ("first", "<u8"), ("length", "<i8"), ("score", "<i8")])   # pgx_unitig


class Invalid(ValueError):
    def __init__(self, rule, index):
        super().__init__("%s: edge %d" % (rule, index))
        self.rule, self.index = rule, index


def unitigs(edges: np.ndarray):
    """(text, table (UNITIG_DTYPE), paths (creation indices, unitig after unitig)) of the edge records"""
    g = [int(e) for e in np.flatnonzero(edges["type"] == G)]
    v = {e: int(edges["v_rid"][e]) << 1 | int(edges["v_end"][e]) for e in g}
    w = {e: int(edges["w_rid"][e]) << 1 | int(edges["w_end"][e]) for e in g}
    length = {e: abs(int(edges["sp"][e]) - int(edges["tp"][e])) for e in g}
    score = {e: int(edges["score"][e]) for e in g}
    bad = [e for e in g if v[e] >> 1 == w[e] >> 1]
    if bad:
        raise Invalid("self", bad[0])
    seen = {}
    bad = [e for e in g if seen.setdefault((v[e], w[e]), e) != e]
    if bad:
        raise Invalid("duplicate", bad[0])
    bad = [e for e in g if (w[e] ^ 1, v[e] ^ 1) not in seen]
    if bad:
        raise Invalid("reverse", bad[0])
    out, inn = {}, {}
    for e in g:
        out.setdefault(v[e], []).append(e), inn.setdefault(w[e], []).append(e)

    def simple(x):
        return len(out.get(x, ())) == 1 and len(inn.get(x, ())) == 1

    def walk(e, stop=None):
        path = [e]
        while simple(w[path[-1]]) and out[w[path[-1]]][0] != stop:
            path.append(out[w[path[-1]]][0])
        return path

    found, used = [], set()
    for e in g:
        if not simple(v[e]):
            found.append((walk(e), 0))
            used.update(found[-1][0])
    for e in g:                                    # ascending: the first unused edge of a ring is the ring's smallest
        if e not in used:
            found.append((walk(e, stop=e), 1))
            used.update(found[-1][0])
    found.sort(key=lambda pc: pc[0][0])
    assert sorted(used) == g and sum(len(p) for p, _ in found) == len(g)
    table = np.zeros(len(found), UNITIG_DTYPE)
    paths, lines = [], []
    for u, (p, circ) in enumerate(found):
        s, via, t = v[p[0]], w[p[0]], w[p[-1]]
        ln, sc = sum(length[e] for e in p), sum(score[e] for e in p)
        table[u] = (s >> 1, t >> 1, via >> 1, s & 1, t & 1, via & 1, circ, len(p), 0, len(paths), ln, sc)
        paths += p
        lines.append(b"%s %s %s simple %d %d %s\n" % (node_name(s), node_name(via), node_name(t), ln, sc, b"~".join([node_name(s)] + [node_name(w[e]) for e in p])))
    return b"".join(lines), table, np.array(paths, np.uint32)


def drop_via(text: bytes) -> bytes:
    """the lines without their second field"""
    return b"".join(b" ".join(f[:1] + f[2:]) + b"\n" for f in (ln.split(b" ") for ln in text.split(b"\n")[:-1]))


def via_is_second_node(text: bytes) -> bool:
    return all(f[1] == f[6].split(b"~")[1] for f in (ln.split(b" ") for ln in text.split(b"\n")[:-1]))


def table_of_text(text: bytes):
    """what the lines say of the table: (s, via, t, n_edges, length, score) per line, names as text"""
    return [(f[0], f[1], f[2], f[6].count(b"~"), int(f[4]), int(f[5])) for f in (ln.split(b" ") for ln in text.split(b"\n")[:-1])]


def names_of_table(table):
    nm = lambda rid, end: node_name(int(rid) << 1 | int(end))   # noqa: E731
    return [(nm(r["s_rid"], r["s_end"]), nm(r["via_rid"], r["via_end"]), nm(r["t_rid"], r["t_end"]), int(r["n_edges"]), int(r["length"]), int(r["score"]))
            for r in table]


def check_against_edges(edges, text, table, paths):
    """the text, the table and the path array agree with each other and with the edge records; the paths partition the G edges"""
    assert names_of_table(table) == table_of_text(text)
    assert sorted(int(e) for e in paths) == [int(e) for e in np.flatnonzero(edges["type"] == G)]
    assert [int(x) for x in table["first"]] == [int(x) for x in np.concatenate([[0], np.cumsum(table["n_edges"].astype(np.int64))[:-1]])] if len(table) else len(paths) == 0
    key = lambda rid, end: node_name(int(rid) << 1 | int(end))   # noqa: E731
    for r, ln in zip(table, text.split(b"\n")[:-1]):
        p = [int(e) for e in paths[int(r["first"]):int(r["first"]) + int(r["n_edges"])]]
        nodes = [key(edges["v_rid"][p[0]], edges["v_end"][p[0]])] + [key(edges["w_rid"][e], edges["w_end"][e]) for e in p]
        assert ln.split(b" ")[6] == b"~".join(nodes)
        assert all(key(edges["v_rid"][b], edges["v_end"][b]) == key(edges["w_rid"][a], edges["w_end"][a]) for a, b in zip(p, p[1:]))
        assert not r["circular"] or (nodes[0] == nodes[-1] and p[0] == min(p))


def load_fixture():
    """(arrays, cases) of tests/golden/utg_cases.npz: per case <name>_utg (the normalised lines: via dropped), and its input -- <name>_edges
    (EDGE_DTYPE as bytes) or the records of `recs_of` (here as <name>_recs, or in sgraph_cases*.npz) with min_len / min_idt"""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(gold, "utg_cases.npz")) as f:
        z = {k: f[k] for k in f.files}
    return z, json.loads(str(z["cases"]))


def fixture_edges(z, name) -> np.ndarray:
    return z[name + "_edges"].view(EDGE_DTYPE).reshape(-1).copy()


def fixture_recs(z, case) -> np.ndarray:
    """the records of a record case"""
    import sgraph_util as SG
    if case["recs_in"] == "sgraph":
        zs, _ = SG.load_fixture()
        return SG.fixture_recs(zs, case["recs_of"])
    return SG.fixture_recs(z, case["recs_of"])


def random_symmetric_edges(seed: int, n_pairs: int, n_rings: int = 3) -> np.ndarray:
    """A random valid edge array of n_pairs edges and more, each with its reverse at a random place: chains of up to 400 reads, rings of
    simple nodes, a tenth as many random edges between the chains' read ends (forks and joins, out-degree at most 3), and a few TR / S / R
    edges that must be ignored.  Lengths and scores random."""
    rng = np.random.default_rng(seed)
    pairs, outdeg, have = [], {}, set()

    def add(a, b):   # a, b node keys
        if a >> 1 == b >> 1 or (a, b) in have or (b ^ 1, a ^ 1) in have or outdeg.get(a, 0) >= 3 or outdeg.get(b ^ 1, 0) >= 3:
            return False
        have.update([(a, b), (b ^ 1, a ^ 1)])
        outdeg[a] = outdeg.get(a, 0) + 1
        outdeg[b ^ 1] = outdeg.get(b ^ 1, 0) + 1
        pairs.append((a, b))
        return True

    r = 0
    while len(pairs) < n_pairs * 85 // 100:          # chains of reads r, r + 1, ...
        run = int(rng.integers(1, 400))
        for i in range(r, r + run):
            add(i << 1 | 1, (i + 1) << 1 | 1)
        r += run + 2
    base = ring0 = r
    for k in range(n_rings):                         # rings of simple nodes: nothing else touches their reads
        n = int(rng.integers(3, 300))
        for i in range(n):
            add((base + i) << 1 | 1, (base + (i + 1) % n) << 1 | 1)
        base += n
    pool = np.concatenate([np.arange(0, 2 * ring0), np.arange(2 * base, 2 * base + 100)])
    target = len(pairs) + max(20, n_pairs // 10)
    while len(pairs) < target:                       # random edges: forks and joins, into the chains too
        add(int(rng.choice(pool)), int(rng.choice(pool)))
    order = []
    for k, (a, b) in enumerate(pairs):
        order.append((rng.random(), a, b, k))
        order.append((rng.random(), b ^ 1, a ^ 1, k))
    order.sort()
    n_other = len(order) // 20
    edges = np.zeros(len(order) + n_other, EDGE_DTYPE)
    other_at = set(int(x) for x in rng.choice(len(edges), n_other, replace=False))
    it = iter(order)
    for e in range(len(edges)):
        if e in other_at:
            edges[e] = (int(rng.integers(0, base)), int(rng.integers(0, base)), 0, 5, 0, int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(1, 4)), 0, 77, 990)
        else:
            _, a, b, k = next(it)
            sp, tp = int(rng.integers(0, 20000)), int(rng.integers(0, 20000))
            edges[e] = (a >> 1, b >> 1, b >> 1, sp, tp, a & 1, b & 1, G, 0, int(rng.integers(-50, 20000)) + k % 7, 990)
    return edges
