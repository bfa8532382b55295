"""The phases of ovlp_to_graph.py after identify_simple_paths in plain Python over arrays: from edge records in creation order to the final
utg_data and ctg_paths.  TEST INFRASTRUCTURE, written from the rule as the project states it (include/pgx.h), not from
the script: no graph objects and no sets of strings -- a node is the integer (rid << 1) | end, a unitig is its index (the simple ones as
utg_util.unitigs numbers them, the compound ones behind them in order of creation), and every container has a stated order:

  sets       pop their smallest element and iterate ascending
  nodes      iterate in ascending key
  edges      a node's out-edges and in-edges iterate in ascending unitig index; u_edge_data iterates in unitig order
  dual       of a unitig with s != t (and of a linear one with s == t): the unitig (s', via') = (t ^ 1, tail of the last edge ^ 1); a ring has none
  best_in    of a node: the tail of the G edge that enters it with the largest creation index

contig_paths(edges) answers a Result; Invalid is raised where the script would assert or raise.  normalise_* bring the script's files and
ours to the form in which the fixtures of ctg_cases.npz are stored (what the rule states as ours is taken out, nothing else).
"""
import heapq
import json
import os

import numpy as np

import utg_util as UT
from sgraph_util import G, node_name

SIMPLE, SPUR2, SIMPLE_DUP, CONTAINED, REPEAT_BRIDGE, COMPOUND = range(6)
TYPE_NAMES = (b"simple", b"spur:2", b"simple_dup", b"contained", b"repeat_bridge", b"compound")
NONE = 0xFFFFFFFF
CTG_UNITIG_DTYPE = np.dtype([("type", "<u4"), ("dual", "<u4")])   # pgx_ctg_unitig
STATS = ("unitigs", "simple", "spur2", "simple_dup", "contained", "repeat_bridge", "compound", "ctg_linear", "ctg_circular", "ctg_lines", "row_entries",
         "longest_ctg", "spur_rounds", "host_us", "device_walks")   # pgx_ctg_paths_stats_t


class Invalid(ValueError):
    pass


class MinSet:
    """a set that pops its smallest element"""

    def __init__(self, items=()):
        self.h, self.s = [], set()
        for x in items:
            self.add(x)

    def add(self, x):
        if x not in self.s:
            self.s.add(x), heapq.heappush(self.h, x)

    def discard(self, x):
        self.s.discard(x)

    def __contains__(self, x):
        return x in self.s

    def __bool__(self):
        return bool(self.s)

    def pop(self):
        while True:
            x = heapq.heappop(self.h)
            if x in self.s:
                self.s.discard(x)
                return x


class Result:
    pass


def contig_paths(edges: np.ndarray) -> Result:
    try:
        _, table, paths = UT.unitigs(edges)
    except UT.Invalid as e:
        raise Invalid(str(e))
    n_u = len(table)
    key = lambda r, e: int(r) << 1 | int(e)   # noqa: E731
    S = [key(r["s_rid"], r["s_end"]) for r in table]
    T = [key(r["t_rid"], r["t_end"]) for r in table]
    VIA = [key(r["via_rid"], r["via_end"]) for r in table]
    LEN = [int(x) for x in table["length"]]
    SCORE = [int(x) for x in table["score"]]
    NE = [int(x) for x in table["n_edges"]]
    TYPE = [SIMPLE] * n_u
    SUB = [None] * n_u
    ekey = lambda e, a, b: int(edges[a][e]) << 1 | int(edges[b][e])   # noqa: E731
    LAST_TAIL = [ekey(int(paths[int(r["first"]) + int(r["n_edges"]) - 1]), "v_rid", "v_end") for r in table]
    best_in = {}
    for e in np.flatnonzero(edges["type"] == G):
        best_in[ekey(int(e), "w_rid", "w_end")] = ekey(int(e), "v_rid", "v_end")
    by_sv = {(S[u], VIA[u]): u for u in range(n_u)}
    DUAL = [NONE] * n_u
    for u in range(n_u):
        if table["circular"][u]:
            continue
        DUAL[u] = by_sv.get((T[u] ^ 1, LAST_TAIL[u] ^ 1), NONE)
        if DUAL[u] == NONE:
            raise Invalid("unitig %d has no dual" % u)
    # ---- phase 1: the unitig graph
    out, inn, alive = {}, {}, []
    circular = [u for u in range(n_u) if S[u] == T[u]]

    def add_edge(u):
        out.setdefault(S[u], []).append(u), inn.setdefault(T[u], []).append(u)
        out.setdefault(T[u], []), inn.setdefault(S[u], [])
        alive[u] = True

    alive = [False] * n_u
    for u in range(n_u):
        if S[u] != T[u]:
            add_edge(u)
    outs = lambda x: [u for u in out.get(x, ()) if alive[u]]   # noqa: E731
    ins = lambda x: [u for u in inn.get(x, ()) if alive[u]]   # noqa: E731
    r = Result()
    r.spur_rounds = 0

    def ego(n, radius):
        seen, front = {n}, [n]
        for _ in range(radius):
            nxt = []
            for x in front:
                for u in outs(x):
                    if T[u] not in seen:
                        seen.add(T[u]), nxt.append(T[u])
            front = nxt
        return seen

    def spurs(spur_len):
        cands = MinSet(x for x in sorted(out) if not ins(x))
        while cands:
            n = cands.pop()
            if ins(n):
                continue
            eg = ego(n, 10)
            for b in sorted(eg):
                b_in = ins(b)
                if len(b_in) <= 1 or all(S[u] in eg for u in b_in):
                    continue
                pred, front = {n: None}, [n]        # fewest hops, neighbours in edge order, the first discoverer is the predecessor
                while b not in pred:
                    nxt = []
                    for x in front:
                        for u in outs(x):
                            if T[u] not in pred:
                                pred[T[u]] = x
                                nxt.append(T[u])
                    front = nxt
                hops, x = [], b
                while pred[x] is not None:
                    hops.append((pred[x], x))
                    x = pred[x]
                hops.reverse()
                if sum(LEN[u] for a, c in hops for u in outs(a) if T[u] == c) >= spur_len:
                    continue
                for a, c in hops:
                    for u in [u for u in outs(a) if T[u] == c]:
                        d = DUAL[u]
                        alive[u] = False
                        if d != NONE and alive[d]:      # (otherwise the script's second remove_edge raises into its `except: pass`)
                            alive[d] = False
                            TYPE[u] = TYPE[d] = SPUR2
                    if not ins(c):
                        cands.add(c)
                r.spur_rounds += 1
                break

    spurs(50000)
    # ---- phase 3: duplicate short simple paths
    groups = {}
    for u in range(n_u):
        if NE[u] <= 2 and TYPE[u] == SIMPLE:
            groups.setdefault((S[u], T[u]), []).append(u)
    for (s, t), us in groups.items():
        us.sort(key=lambda u: VIA[u])
        for u in us[1:]:
            if not alive[u]:
                raise Invalid("unitig %d: a second short loop at one node" % u)
            alive[u] = False
            TYPE[u] = SIMPLE_DUP

    # ---- phase 4: compound paths
    def find_bundle(start):
        loc = ego(start, 48)
        o = lambda x: [u for u in outs(x) if T[u] in loc]   # noqa: E731
        i = lambda x: [u for u in ins(x) if S[u] in loc]   # noqa: E731
        tips, b_edges, b_nodes = MinSet(), set(), {start}
        length_to, score_to = {start: 0}, {start: 0}

        def best_in_edge(v, strict):
            best, mx = None, 0
            for u in i(v):
                if S[u] not in length_to:
                    if strict:
                        return False
                    continue
                if SCORE[u] > mx:
                    mx, best = SCORE[u], u
            return best

        def settle(v, best):
            if best is None:
                raise Invalid("node %d: no in-edge of a bundle has a positive score" % v)
            length_to[v], score_to[v] = length_to[S[best]] + LEN[best], score_to[S[best]] + SCORE[best]

        for u in o(start):
            if T[u] ^ 1 not in b_nodes:
                b_edges.add(u), tips.add(T[u])
        b_nodes |= tips.s
        depth = 1
        while True:
            if len(tips.s) > 4:
                return None
            if len(tips.s) == 1:
                end = tips.pop()
                if end not in length_to:
                    settle(end, best_in_edge(end, False))
                return start, end, sorted(b_edges), length_to[end], score_to[end]
            depth += 1
            if depth > 10 and len(b_edges) / depth > 16:
                return None
            if depth > 48:
                return None
            updated = loop = False
            for v in sorted(tips.s):
                if not o(v):
                    continue
                best = best_in_edge(v, True)
                if best is not False:
                    settle(v, best)
                    if length_to[v] > 500000:
                        return None
                    v_up = False
                    for u in o(v):
                        if T[u] in length_to:
                            loop = True
                            break
                        if u not in b_edges and T[u] ^ 1 not in b_nodes:
                            tips.add(T[u]), b_edges.add(u)
                            updated = v_up = True
                    if v_up:
                        tips.discard(v)
                        if len(tips.s) == 1:
                            break
                if loop:
                    break
            if loop or not updated:
                return None
            b_nodes |= tips.s

    found = []
    for p in sorted(out):
        if len(outs(p)) > 1:
            b = find_bundle(p)
            if b:
                found.append(b)
    found.sort(key=lambda b: -len(b[2]))

    def dual_of(u, what):
        if DUAL[u] == NONE:
            raise Invalid("unitig %d of %s has no dual" % (u, what))
        return DUAL[u]

    e2c, cp1 = set(), {}
    for s, t, be, ln, sc in found:
        if any(u in e2c or dual_of(u, "a bundle") in e2c for u in be):
            continue
        ber = [DUAL[u] for u in be]
        e2c.update(be), e2c.update(ber)
        cp1[(s, t)] = (ln, sc, be)
        cp1[(t ^ 1, s ^ 1)] = (ln, sc, ber)
    cp2, e2c = {}, {}
    for (s, t), val in cp1.items():
        if (t ^ 1, s ^ 1) in cp1:
            cp2[(s, t)] = val
            for u in val[2]:
                e2c.setdefault(u, set()).add((s, t))
    cp3 = {k: val for k, val in cp2.items() if not any(len(e2c.get(u, ())) > 1 for u in outs(k[0]))}
    compound = {k: val for k, val in cp3.items() if (k[1] ^ 1, k[0] ^ 1) in cp3}
    for val in compound.values():
        for u in val[2]:
            if alive[u]:
                alive[u] = False
                TYPE[u] = CONTAINED
    first_c = {}
    for (s, t), (ln, sc, be) in compound.items():
        first_c[(s, t)] = len(S)
        S.append(s), T.append(t), VIA.append(None), LEN.append(ln), SCORE.append(sc), NE.append(0), TYPE.append(COMPOUND), SUB.append(list(be)), LAST_TAIL.append(None)
        DUAL.append(NONE), alive.append(False)
    for (s, t), c in first_c.items():
        DUAL[c] = first_c[(t ^ 1, s ^ 1)]
        add_edge(c)
    # ---- phase 5: repeat bridges
    all_nodes = sorted(out)
    bridges = set()
    for x in all_nodes:
        for u in outs(x):
            s, t = S[u], T[u]
            if len(ins(s)) == 1 and len(outs(s)) == 2 and len(ins(t)) == 2 and len(outs(t)) == 1 and LEN[u] < 60000:
                bridges.update((u, dual_of(u, "a repeat bridge")))
    for u in sorted(bridges):
        if not alive[u]:
            raise Invalid("unitig %d: the dual of a repeat bridge is not in the graph" % u)
        alive[u] = False
        TYPE[u] = REPEAT_BRIDGE
    # ---- phase 6
    spurs(80000)
    # ---- phase 7: utg_data
    n_all = len(S)
    triple = lambda u: b"%s~%s~%s" % (node_name(S[u]), b"NA" if VIA[u] is None else node_name(VIA[u]), node_name(T[u]))   # noqa: E731
    simple_text, _, _ = UT.unitigs(edges)
    lines = []
    for u, ln in enumerate(simple_text.split(b"\n")[:-1]):
        f = ln.split(b" ")
        f[3] = TYPE_NAMES[TYPE[u]]
        lines.append(b" ".join(f) + b"\n")
    for u in range(n_u, n_all):
        lines.append(b"%s NA %s %s %d %d %s\n" % (node_name(S[u]), node_name(T[u]), TYPE_NAMES[TYPE[u]], LEN[u], SCORE[u], b"|".join(triple(x) for x in SUB[u])))
    r.utg_text = b"".join(lines)
    # ---- phase 8: contig walks
    starts = MinSet(x for x in all_nodes if outs(x) and not (len(ins(x)) == 1 and len(outs(x)) == 1))
    r.start_edges = sum(len(outs(x)) for x in starts.s)   # the walks that do not depend on another one's pop: a lane each on the device
    free = MinSet(u for u in range(n_all) if alive[u])
    c_path = []
    while free:
        n = starts.pop() if starts else S[free.pop()]
        for u in outs(n):
            path, plen, pscore, nodes = [], 0, 0, {S[u]}
            t = T[u]
            while len(outs(t)) == 1:
                if t in nodes or t ^ 1 in nodes:
                    break
                ln, sc = LEN[u], SCORE[u]
                if len(ins(t)) > 1:
                    b = best_in[t]
                    if TYPE[u] == SIMPLE and b != LAST_TAIL[u]:
                        break
                    if TYPE[u] == COMPOUND:
                        t_in = set()
                        for x in SUB[u]:
                            if VIA[x] != t:
                                continue
                            ln, sc = LEN[x], SCORE[x]
                            if T[x] == VIA[x]:
                                t_in.add(LAST_TAIL[x])
                        if b not in t_in:
                            break
                path.append(u), nodes.add(t)
                plen += ln
                pscore += sc
                u = outs(t)[0]
                t = T[u]
            path.append(u)
            plen += LEN[u]
            c_path.append((plen, path))
            for x in path:
                free.discard(x)
    # ---- phase 9: ctg_paths
    c_path.sort(key=lambda c: -c[0])
    free = set(u for u in range(n_all) if alive[u])
    rows, lines = [], []
    r.ctg_linear = r.ctg_circular = 0
    r.claimed_walk_lengths = []          # path_length of the walks that claimed a contig, in the order of their ids
    for walk_length, path in c_path:
        keep = []
        for u in path:
            if u in free and DUAL[u] in free:
                keep.append(u)
            else:
                break
        if not keep:
            continue
        r.claimed_walk_lengths.append(walk_length)
        rev = [DUAL[u] for u in reversed(keep)]
        circ = T[keep[-1]] == S[keep[0]]
        for tag, row in ((b"F", keep), (b"R", rev)):
            lines.append(b"%06d%s %s %s %s %d %d %s\n" % (len(rows) // 2, tag, b"ctg_circular" if circ else b"ctg_linear", triple(row[0]), node_name(T[row[-1]]),
                                                        sum(LEN[u] for u in row), sum(SCORE[u] for u in row), b"|".join(triple(u) for u in row)))
            rows.append(row)
        r.ctg_circular += circ
        r.ctg_linear += not circ
        free.difference_update(keep), free.difference_update(rev)
    ctg_id = len(rows) // 2
    for u in circular:
        lines.append(b"%6d ctg_circular %s %s %d %d %s\n" % (ctg_id, triple(u), node_name(T[u]), LEN[u], SCORE[u], triple(u)))
        rows.append([u])
        ctg_id += 1
    r.ctg_circular += len(circular)
    r.ctg_text = b"".join(lines)
    r.rows = rows
    r.table = np.zeros(n_all, CTG_UNITIG_DTYPE)
    r.table["type"], r.table["dual"] = TYPE, DUAL
    r.n_simple_unitigs, r.sub = n_u, SUB
    return r


def stats_of(r: Result) -> dict:
    """what pgx_ctg_paths_stats says, host_us apart"""
    cnt = np.bincount(r.table["type"], minlength=6)
    return {"unitigs": len(r.table), "simple": int(cnt[SIMPLE]), "spur2": int(cnt[SPUR2]), "simple_dup": int(cnt[SIMPLE_DUP]), "contained": int(cnt[CONTAINED]),
            "repeat_bridge": int(cnt[REPEAT_BRIDGE]), "compound": int(cnt[COMPOUND]), "ctg_linear": int(r.ctg_linear), "ctg_circular": int(r.ctg_circular),
            "ctg_lines": len(r.rows), "row_entries": sum(len(x) for x in r.rows), "longest_ctg": max([len(x) for x in r.rows] or [0]), "spur_rounds": r.spur_rounds}


# ---- normal forms: what the rule states as ours is taken out ------------------------------------------------------------------------------
def _rev_name(n: bytes) -> bytes:
    return n[:-1] + (b"B" if n.endswith(b"E") else b"E")


def _canon_path(p):
    """a node path as a name: a ring (first == last) rotated to its smallest node"""
    p = list(p)
    if len(p) > 1 and p[0] == p[-1] and len(set(p[:-1])) == len(p) - 1:
        k = p.index(min(p[:-1]))
        p = p[k:-1] + p[:k] + [p[k]]
    return b"~".join(p)


def normalise(utg_text: bytes, ctg_text: bytes):
    """(utg lines, contigs) in normal form.  A unitig is named by its node path (rings rotated to their smallest node), a compound one by
    the sorted names of its sub-unitigs; utg lines are sorted; a `spur:2` line is named by the smaller of its path and the reverse path and
    loses its length and score (the script writes a spur's own data over its dual's); a contig is the sorted pair of its F and R lines without
    their ids, a ring's line a 1-tuple without its end node (the ring's cut); contigs are a sorted list (the F ids must count from 0; the printed lengths need not fall along them: the
    script sorts by the length of the whole walk and prints that of the claimed prefix)."""
    name, out = {}, []
    comp = []
    for ln in utg_text.split(b"\n")[:-1]:
        s, v, t, ty, length, score, p = ln.split(b" ")
        if v == b"NA":
            comp.append((s, v, t, ty, length, score, p))
            continue
        nodes = p.split(b"~")
        nm = _canon_path(nodes)
        if ty == b"spur:2":
            nm = min(nm, _canon_path([_rev_name(x) for x in reversed(nodes)]))
            out.append((nm, ty, b"", b""))
        else:
            name.setdefault((s, v, t), nm)
            out.append((nm, ty, length, score))
    for ln in utg_text.split(b"\n")[:-1]:   # (a spur's names last: its dual's line may carry the wrong path)
        s, v, t, ty, length, score, p = ln.split(b" ")
        if v != b"NA" and ty == b"spur:2":
            name.setdefault((s, v, t), b"spur")
    for s, v, t, ty, length, score, p in comp:
        subs = sorted(name[tuple(x.split(b"~"))] for x in p.split(b"|"))
        name[(s, v, t)] = b"{" + b"|".join(subs) + b"}"
        if ty == b"spur:2":
            out.append((min(s + t, _rev_name(t) + _rev_name(s)), ty, b"", b""))
        else:
            out.append((s + b" " + t + b" " + name[(s, v, t)], ty, length, score))
    ctgs, by_id = [], {}
    for ln in ctg_text.split(b"\n")[:-1]:
        cid, ty, first, end, length, score, p = [x for x in ln.split(b" ") if x]   # (a ring's id is "%6d": blanks in front)
        row = (ty, name[tuple(first.split(b"~"))], end, int(length), int(score), tuple(name[tuple(x.split(b"~"))] for x in p.split(b"|")))
        if cid.endswith(b"F") or cid.endswith(b"R"):
            by_id.setdefault(cid[:-1], []).append(row)
            if cid.endswith(b"F"):
                assert int(cid[:-1]) == len(by_id) - 1, "the F ids do not count from 0"
        else:
            ctgs.append(((ty, row[1], row[3], row[4], row[5]),))   # (without the end node: the place where a ring is cut)
    for cid, pair in by_id.items():
        assert len(pair) == 2
        ctgs.append(tuple(sorted(pair)))
    return sorted(out), sorted(ctgs)


def edges_of_g_lines(g_lines) -> np.ndarray:
    """edge records of (v key, w key, sp, tp, score) tuples in creation order, all of type G (label rid: w's read)"""
    from sgraph_util import EDGE_DTYPE
    e = np.zeros(len(g_lines), EDGE_DTYPE)
    for k, (v, w, sp, tp, score) in enumerate(g_lines):
        e[k] = (v >> 1, w >> 1, w >> 1, sp, tp, v & 1, w & 1, G, 0, score, 999)
    return e


# ---- hand-made graphs (the cases of ctg_cases.npz are made of these; the GPU tests build larger ones) -----------------------------------
E, B = 1, 0


class Graph:
    """G edges in creation order, every edge followed by its reverse; sp / tp are made so that |sp - tp| is the wanted length"""

    def __init__(self, base=0):
        self.lines, self.base, self.k = [], base, 0

    def n(self, i, end=E):
        return (self.base + i) << 1 | end

    def edge(self, a, b, length=30000, score=None):
        self.k += 1
        score = length - 7 * self.k if score is None else score      # distinct, positive
        for v, w in ((a, b), (b ^ 1, a ^ 1)):          # the label is a stretch of w's read: forward (sp < tp) when the edge enters its E end
            self.lines.append((v, w, 1000, 1000 + length, score) if w & 1 else (v, w, 1000 + length, 1000, score))   # (1,000 bases in: room for a contig layout)

    def chain(self, ids, length=30000, end=E):
        for a, b in zip(ids[:-1], ids[1:]):
            self.edge(self.n(a, end), self.n(b, end), length)


def m_spur(g):
    """a chain with a short side branch into its middle: the branch is `spur:2`; the long way into the same node stays (over the limit)"""
    g.chain([1, 2, 3, 4, 5, 6, 7, 8])
    g.chain([20, 21, 4], 2000)


def m_spur2(g):
    """a side branch of 60,000: stays in the first spur pass, goes in the second"""
    g.chain([1, 2, 3, 4, 5, 6, 7, 8, 9])
    g.chain([30, 31, 32, 5], 20000)


def m_dup(g):
    """a bubble of two paths of three nodes: the larger via is `simple_dup`"""
    g.chain([1, 2, 3, 4])
    g.chain([4, 5, 7], 3000), g.chain([4, 6, 7], 3100)
    g.chain([7, 8, 9, 10])


def m_compound(g):
    """a bubble of two paths of four nodes: one compound unitig and its reverse, the branches `contained`; the contig runs through it"""
    g.chain([1, 2, 3, 4])
    g.chain([4, 5, 6, 9], 3000), g.chain([4, 7, 8, 9], 3300)
    g.chain([9, 10, 11, 12])


def m_yjoin(g):
    """two long chains into one node: the chain whose last edge is the later one passes the best_in test, the other stops at it"""
    g.chain([5, 6, 7, 8, 10], 31000)
    g.chain([1, 2, 3, 4, 10])
    g.chain([10, 11, 12, 13], 29000)


def m_bridge(g):
    """two chains and a short unitig from the middle of one into the middle of the other: `repeat_bridge`"""
    g.chain([1, 2, 3, 4, 5, 6, 7, 8])                       # s = 5
    g.chain([11, 12, 13, 14, 15, 16, 17, 18, 19, 20], 28000)   # t = 16
    g.chain([5, 25, 16], 9000)


def m_ring(g):
    g.chain([1, 2, 3, 1], 12000)


def m_cycle(g):
    """a cycle of two unitigs P -> Q -> P with a tail into P and one out of Q: one circular contig of two unitigs"""
    g.chain([1, 2, 3, 4, 10], 31000)          # the tail into P = 10
    g.chain([10, 11, 12, 20], 27000)          # P -> Q = 20
    g.chain([20, 21, 22, 10], 32000)          # Q -> P, its last edge the latest into P
    g.chain([20, 31, 34], 20000)              # out of Q, created last: the reverse walk of the cycle stops at rev Q, so the cycle has one start


def m_hairpin(g):
    """a chain that turns into its own reverse: the walk stops at `rev t`"""
    g.chain([1, 2, 3, 4])
    g.edge(g.n(4), g.n(40, B), 30000)
    g.edge(g.n(40, B), g.n(3, B), 29000)


MOTIFS = dict(spur=m_spur, spur2=m_spur2, dup=m_dup, compound=m_compound, yjoin=m_yjoin, bridge=m_bridge, ring=m_ring, cycle=m_cycle, hairpin=m_hairpin)


def chain_with_tips(n_unitigs: int, seg: int = 3) -> np.ndarray:
    """a chain cut into n_unitigs unitigs by short side branches into it (each `spur:2`): one contig of n_unitigs unitigs"""
    g = Graph()
    g.chain(list(range(1, seg * n_unitigs + 2)))
    for k in range(1, n_unitigs):
        g.chain([100000 + 2 * k, 100001 + 2 * k, 1 + seg * k], 2000)
    return edges_of_g_lines(g.lines)


def ladder(levels: int, rails: int = 3) -> np.ndarray:
    """a bundle of rails * rails * (levels - 1) + 2 * rails single-edge unitigs between two chains: `levels` levels of `rails` nodes, every
    node of a level joined to every node of the next"""
    g = Graph()
    g.chain([1, 2, 3, 4])
    node = lambda lv, r: 1000 + 10 * lv + r   # noqa: E731
    score = lambda: 500 + 7 * len(g.lines) % 311   # noqa: E731  (positive, and distinct among the in-edges of a node)
    for r in range(rails):
        g.edge(g.n(4), g.n(node(0, r)), 1000, score())
    for lv in range(levels - 1):
        for a in range(rails):
            for b in range(rails):
                g.edge(g.n(node(lv, a)), g.n(node(lv + 1, b)), 1000, score())
    for r in range(rails):
        g.edge(g.n(node(levels - 1, r)), g.n(5), 1000, score())
    g.chain([5, 6, 7, 8])
    return edges_of_g_lines(g.lines)


def long_spur(n_nodes: int) -> np.ndarray:
    """a side branch of n_nodes nodes and a total length under 50,000 into a chain: one unitig of n_nodes nodes typed `spur:2`"""
    g = Graph()
    g.chain([1, 2, 3, 4, 5, 6, 7, 8])
    g.chain(list(range(20000, 20000 + n_nodes - 1)) + [4], 5)
    return edges_of_g_lines(g.lines)


def load_fixture():
    """(arrays, cases) of tests/golden/ctg_cases.npz: per case <name>_edges (EDGE_DTYPE as bytes) and, for the stored cases (those on which
    the script gave one answer under every hash seed), <name>_utg / <name>_ctg: the script's two files under the first seed"""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with np.load(os.path.join(gold, "ctg_cases.npz")) as f:
        z = {k: f[k] for k in f.files}
    return z, json.loads(str(z["cases"]))


def fixture_edges(z, name) -> np.ndarray:
    from sgraph_util import EDGE_DTYPE
    return z[name + "_edges"].view(EDGE_DTYPE).reshape(-1).copy()
