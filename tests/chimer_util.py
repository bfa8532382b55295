"""The string graph with the chimer bridge step under a stated pop order, in plain Python over arrays: sgraph_util's pieces with one pass
between the transitive reduction and the first spur pass.  TEST INFRASTRUCTURE, written from the rule as the project states it
(include/pgx.h, PGX_SGRAPH_CHIMER_ORDERED), not from the script: nodes and edges are numbers in creation order.

  state read   the marks as the transitive reduction left them; the pass never reads a mark it set
  candidates   node n: some unreduced u -> n whose tail has >= 2 unreduced out-edges, and some unreduced n -> x whose head has >= 2 unreduced
               in-edges
  test 1       O = heads of all out-edges of n, T = heads of all out-edges of the tails of n's in-edges, minus n (edges in any state):
               O and T are disjoint
  flow(s, n)   A = pool = {s}; up to 4 times, while the pool is not empty, its smallest (rid as unsigned, end) leaves it as p, and every
               p -> w with w != n and w not in A puts w into A, and into the pool if w has out-edges
  test 2       the union of flow(v, n) over O and the union over T are disjoint
  marking      every edge of a chosen node that the reduction left unreduced becomes C, with its reverse; TR stays TR
"""
import numpy as np

import dedup_graph_util as DG
import sgraph_util as SG

C = 4
TYPE_NAMES = SG.TYPE_NAMES + (b"C",)
COUNTS = ("edges", "n_g", "n_tr", "n_s", "n_r")
CHIMER_STATS = ("candidates", "past_test1", "chosen", "c_edges")


def load_fixture():
    """(arrays, cases) of tests/golden/chimer_cases.npz + chimer_cases_sim.npz: <name>_recs, <name>_sg (the pinned policy's
    sg_edges_list), <name>_nodes (its chimers_nodes lines, sorted), <name>_off (the flag-off sg_edges_list of the same records)"""
    import json
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z = {}
    for name in ("chimer_cases.npz", "chimer_cases_sim.npz"):
        with np.load(os.path.join(gold, name)) as f:
            z.update({k: f[k] for k in f.files})
    return z, json.loads(str(z["cases"]))


def flow(s, n, out, w, key):
    a, pool = {s}, {s}
    for _ in range(4):
        if not pool:
            break
        p = min(pool, key=key.__getitem__)
        pool.remove(p)
        for e in out[p]:
            x = w[e]
            if x != n and x not in a:
                a.add(x)
                if out[x]:
                    pool.add(x)
    return a


def chimer_pass(n_nodes, out, inn, v, w, key, typ):
    """marks the C edges in typ; returns (chosen nodes in creation order, candidates, candidates past test 1)"""
    before = list(typ)
    live_out = [sum(before[e] == SG.G for e in out[n]) for n in range(n_nodes)]
    live_in = [sum(before[e] == SG.G for e in inn[n]) for n in range(n_nodes)]
    cands = [n for n in range(n_nodes)
             if any(before[e] == SG.G and live_out[v[e]] >= 2 for e in inn[n]) and any(before[e] == SG.G and live_in[w[e]] >= 2 for e in out[n])]
    chosen, past1 = [], 0
    for n in cands:
        o = {w[e] for e in out[n]}
        t = {w[e2] for e in inn[n] for e2 in out[v[e]]} - {n}
        if o & t:
            continue
        past1 += 1
        f1 = set().union(*(flow(s, n, out, w, key) for s in o))
        f2 = set().union(*(flow(s, n, out, w, key) for s in t))
        if f1 & f2:
            continue
        chosen.append(n)
    for n in chosen:
        for e in out[n] + inn[n]:
            if before[e] != SG.TR:
                typ[e] = typ[e ^ 1] = C
    return chosen, len(cands), past1


def string_graph(kept: bytes, min_len: int = 4000, min_idt: float = 96.0, chimer: bool = True):
    """(sg_edges_list bytes, edge records, stats, chimer stats, chimers_nodes lines in creation order) of the kept lines"""
    rows = SG.rows_of_text(kept)
    ev, ew, lab, msz, idt, n_pass = SG.build_edges(rows, min_len, min_idt)
    v, w, n_nodes = SG.number_nodes(ev, ew)
    n_e = len(ev)
    key = [0] * n_nodes
    for e in range(n_e):
        key[v[e]], key[w[e]] = ev[e], ew[e]
    length = [abs(sp - tp) for _, sp, tp in lab]
    out = [[] for _ in range(n_nodes)]
    inn = [[] for _ in range(n_nodes)]
    for e in range(n_e):
        out[v[e]].append(e), inn[w[e]].append(e)
    for lst in out:
        lst.sort(key=lambda e: (length[e], e))
    typ = [SG.G] * n_e
    SG.transitive_reduction(n_nodes, out, w, length, typ)
    chosen, n_cand, past1 = chimer_pass(n_nodes, out, inn, v, w, key, typ) if chimer else ([], 0, 0)
    cands = SG.spur_candidates(n_nodes, out, inn, v, w)
    SG.spur_pass(cands, out, inn, v, w, typ)
    SG.best_overlap(n_nodes, out, inn, msz, typ)
    SG.spur_pass(cands, out, inn, v, w, typ)
    lines = []
    recs = np.zeros(n_e, SG.EDGE_DTYPE)
    for e in range(n_e):
        rid, sp, tp = lab[e]
        srid = rid if rid < 2**31 else rid - 2**32
        t = idt[e]
        ident = b"%s%d.%d0" % (b"-" if t < 0 else b"", abs(t) // 10, abs(t) % 10)
        lines.append(b"%s %s %09d %5d %5d %5d %5s %s\n" % (SG.node_name(ev[e]), SG.node_name(ew[e]), srid, sp, tp, msz[e], ident, TYPE_NAMES[typ[e]]))
        recs[e] = (ev[e] >> 1, ew[e] >> 1, rid, sp, tp, ev[e] & 1, ew[e] & 1, typ[e], 0, msz[e], t)
    counts = [typ.count(k) for k in (SG.G, SG.TR, SG.S, SG.R)]
    stats = dict(rows_in=len(rows), rows_pass=n_pass, edges=n_e, nodes=n_nodes, n_g=counts[0], n_tr=counts[1], n_s=counts[2], n_r=counts[3],
                 max_out_degree=max((len(x) for x in out), default=0), spur_candidates=len(cands))
    ch = dict(candidates=n_cand, past_test1=past1, chosen=len(chosen), c_edges=typ.count(C))
    nodes = b"".join(SG.node_name(key[n]) + b"\n" + SG.node_name(key[n] ^ 1) + b"\n" for n in chosen)
    return b"".join(lines), recs, stats, ch, nodes


def string_graph_of_full_text(text: bytes, min_len: int = 4000, min_idt: float = 96.0, chimer: bool = True):
    return string_graph(DG.select_graph_lines(text), min_len, min_idt, chimer)


def stats_of_text(sg: bytes) -> dict:
    """the counts a sg_edges_list text shows: edges, the four types pgx_sgraph_stats_t counts, and the C lines"""
    types = [ln.split()[-1] for ln in sg.split(b"\n")[:-1]]
    return dict(edges=len(types), n_g=types.count(b"G"), n_tr=types.count(b"TR"), n_s=types.count(b"S"), n_r=types.count(b"R")), types.count(b"C")


def edges_of_text(sg: bytes) -> np.ndarray:
    """the edge records a sg_edges_list text with C lines shows (sgraph_util.edges_of_text with the fifth type)"""
    names = SG.TYPE_NAMES
    SG.TYPE_NAMES = TYPE_NAMES
    try:
        return SG.edges_of_text(sg)
    finally:
        SG.TYPE_NAMES = names


def chimeric_sim(seed: int, n_reads: int = 200, genome: int = 30_000, n_chimers: int = 30, pile: int = 70, rid_base: int = 100_000) -> np.ndarray:
    """make_records(seed, n_reads, genome, no contained reads) plus n_chimers chimeric reads: each a new read id with dovetail records from
    reads that end shortly before a junction at one locus and to reads that start shortly after a junction at another.  On top a pile:
    `pile` further new reads that each continue the first chimeric read's first successor, whose out-degree so passes 64."""
    base = DG.make_records(seed=seed, n_reads=n_reads, genome=genome, contained_share=0.0)
    rng = np.random.default_rng(seed)            # make_records' own draws again: the reads' lengths and starts
    rlen = rng.integers(2000, 16000, n_reads)
    start = rng.integers(0, genome, n_reads)
    end = start + rlen
    rng = np.random.default_rng(seed + 10_000)
    parts = [base]
    hub = None
    for c in range(n_chimers):
        x, xl = rid_base + c, 9000
        j1, j2 = (int(t) for t in rng.integers(min(4000, genome // 4), genome - min(4000, genome // 4) + 1, 2))
        # X's left half lies on the genome up to j1, its right half from j2 on
        left = [i for i in range(n_reads) if j1 - 4000 <= end[i] < j1 - 300 and rlen[i] >= 4500][: int(rng.integers(1, 4))]
        right = [i for i in range(n_reads) if j2 + 300 < start[i] <= j2 + 4000 and rlen[i] >= 4500][: int(rng.integers(1, 4))]
        for i in left:      # i to the left of X: i's last (4500 - oh) bases are X's first
            oh = int(j1 - end[i])            # X's bases past i's end ... as the length of i:E -> X:E
            ovl = 4500 - oh
            parts.append(DG.rec(i, x, m_size=ovl, dist=int(rng.integers(0, 40)), rl0=int(rlen[i]), rl1=xl, q_bgn=int(rlen[i]) - ovl, q_end=int(rlen[i]), t_end=ovl))
        if hub is None and right:
            hub = right[0]
        for i in right:     # X to the left of i
            oh = int(start[i] - j2)
            ovl = 4500 - oh
            parts.append(DG.rec(x, i, m_size=ovl, dist=int(rng.integers(0, 40)), rl0=xl, rl1=int(rlen[i]), q_bgn=xl - ovl, q_end=xl, t_end=ovl))
    for k in range(pile if hub is not None else 0):
        ovl = 1000 + 37 * k
        parts.append(DG.rec(hub, rid_base + 50_000 + k, m_size=ovl, dist=int(rng.integers(0, 30)), rl0=int(rlen[hub]), rl1=6000, q_bgn=int(rlen[hub]) - ovl,
                            q_end=int(rlen[hub]), t_end=ovl))
    tail = np.concatenate(parts[1:]) if len(parts) > 1 else base[:0]
    rng.shuffle(tail)
    cut = len(base) // 2
    return np.concatenate([base[:cut], tail, base[cut:]])
