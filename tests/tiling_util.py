"""The tiling-path rule ("tiling paths"; py/scripts/graph_to_path.py:134-326) restated over arrays, a builder of the three input
files, and seeded random inputs.  tests/test_tiling_rule.py holds the restatement to the fixtures the real script wrote; the GPU tests
hold the library to the fixtures and, on the random inputs, to the restatement.

Nodes are keys (rid << 1) | end with end 1 for E; a name is '%09d:E' or '%09d:B'."""
import heapq
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "tiling_cases.npz")
E, B = 1, 0


def key(rid, end):
    return rid << 1 | end


def name(k):
    return "%09d:%s" % (k >> 1, "E" if k & 1 else "B")


def key_of(text):
    rid, end = text.split(":")
    assert end in ("B", "E") and rid.isdigit() and ("%09d" % int(rid)) == rid, text
    return int(rid) << 1 | (end == "E")


def rev(k):
    return k ^ 1


def load_fixture():
    z = np.load(FIXTURE)
    cases = json.loads(str(z["cases"]))
    return z, cases


def case_files(z, case):
    return tuple(z["%s_%s" % (case, part)].tobytes() for part in ("sg", "utg", "ctg", "p", "a"))


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
class RuleError(ValueError):
    """where the script would raise (or the rule refuses): .file is 'sg', 'utg' or 'ctg', .line the 0-based line"""

    def __init__(self, file, line, why):
        ValueError.__init__(self, "%s line %d: %s" % (file, line, why))
        self.file, self.line = file, line


def hundredths(field: str) -> int:
    neg = field.startswith("-")
    body = field[1:] if neg else field
    whole, dot, frac = body.partition(".")
    if not (whole + frac).isdigit() or not (whole + frac).isascii() or len(whole) > 9 or len(frac) > 2:
        raise ValueError(field)
    v = int(whole or "0") * 100 + int((frac + "00")[:2])
    if neg and v == 0:
        raise ValueError(field)
    return -v if neg else v


def shortest(adj, gone, s, t):
    """forward Dijkstra from s, priority (distance, push sequence), a predecessor changes only on a strictly smaller distance, neighbours in
    order of first insertion, stops when t is popped.  Returns (weight, path, minimum-weight paths counted up to 2) or None."""
    dist, pred, done, order = {s: 0}, {}, set(), []
    heap, seq = [(0, 0, s)], 1
    while heap:
        d, _, u = heapq.heappop(heap)
        if u in done:
            continue
        done.add(u), order.append(u)
        if u == t:
            break
        for v, w in adj.get(u, ()):
            if (u, v) in gone:
                continue
            if v not in dist or d + w < dist[v]:
                dist[v], pred[v] = d + w, u
                heapq.heappush(heap, (d + w, seq, v))
                seq += 1
    if t not in done:
        return None
    cnt = {s: 1}
    for u in order:
        if u == t:
            break
        for v, w in adj.get(u, ()):
            if (u, v) not in gone and v in done and dist[u] + w == dist[v]:
                cnt[v] = min(2, cnt.get(v, 0) + cnt.get(u, 0))
    path = [t]
    while path[-1] != s:
        path.append(pred[path[-1]])
    return dist[t], path[::-1], cnt[t]


def tiling_rule(sg: bytes, utg: bytes, ctg: bytes, on_round=None):
    """(p file, a file, statistics) of the three files.  on_round(adj, gone, s, t, weight) is called before every successful round's path
    is removed (the generator counts the simple paths of that weight there)."""
    st = dict.fromkeys(("sg_lines", "g_edges", "utg_simple", "utg_contained", "utg_compound", "ctg_kept", "ctg_skipped", "ctg_empty", "p_rows", "a_rows", "alternates",
                        "compound_tie_rounds"), 0)
    # ---- the edge table as arrays sorted by (v, w)
    ev, ew, rid, es, et, score, hund = [], [], [], [], [], [], []
    for k, ln in enumerate(sg.decode().split("\n")):
        f = ln.split()
        if not f:
            continue
        if len(ln.encode()) > 256:
            raise RuleError("sg", k, "longer than 256 bytes")
        if len(f) != 8:
            raise RuleError("sg", k, "fields")
        st["sg_lines"] += 1
        if f[7] != "G":
            continue
        try:
            row = (key_of(f[0]), key_of(f[1]), int(f[2]), int(f[3]), int(f[4]), int(f[5]), hundredths(f[6]))
            assert "%09d" % row[2] == f[2]
        except (ValueError, AssertionError):
            raise RuleError("sg", k, "a field that does not print back") from None
        if (row[3] < row[4]) != bool(row[1] & 1):
            raise RuleError("sg", k, "the script's assertion on w's end")
        for col, x in zip((ev, ew, rid, es, et, score, hund), row):
            col.append(x)
    st["g_edges"] = len(ev)
    ev, ew, rid, es, et, score, hund = (np.array(c, np.int64) for c in (ev, ew, rid, es, et, score, hund))
    order = np.lexsort((ew, ev))
    ev, ew, rid, es, et, score, hund = (c[order] for c in (ev, ew, rid, es, et, score, hund))
    if len(ev) > 1 and np.any((ev[1:] == ev[:-1]) & (ew[1:] == ew[:-1])):
        raise RuleError("sg", -1, "a (v, w) twice")
    index = {vw: i for i, vw in enumerate(zip(ev.tolist(), ew.tolist()))}

    def edges_of(nodes, file, line):
        """indices into the sorted table of the consecutive pairs of a node array"""
        at = [index.get(vw, -1) for vw in zip(nodes[:-1], nodes[1:])]
        if -1 in at:
            raise RuleError(file, line, "an edge the table lacks")
        return np.array(at, np.int64)

    # ---- the unitig table
    table = {}
    for k, ln in enumerate(utg.decode().split("\n")):
        f = ln.split()
        if not f:
            continue
        if len(f) != 7:
            raise RuleError("utg", k, "fields")
        if f[3] not in ("simple", "contained", "compound"):
            continue
        st["utg_" + f[3]] += 1
        tkey = (key_of(f[0]), -1 if f[1] == "NA" else key_of(f[1]), key_of(f[2]))
        if tkey in table:
            raise RuleError("utg", k, "a (s, via, t) twice")
        int(f[4]), int(f[5])
        if f[3] == "compound":
            body = [tuple(-1 if x == "NA" else key_of(x) for x in e.split("~")) for e in f[6].split("|")]
        else:
            body = [key_of(x) for x in f[6].split("~")]
        table[tkey] = (f[3], k, body)

    def unitig(text, file, line):
        s, v, t = text.split("~")
        tkey = (key_of(s), -1 if v == "NA" else key_of(v), key_of(t))
        if tkey not in table:
            raise RuleError(file, line, "a unitig the table lacks")
        return tkey, table[tkey]

    def bundle(tkey, line, subs):
        adj, seen = {}, set()
        for sub in subs:
            if sub not in table:
                raise RuleError("utg", line, "a sub-unitig the table lacks")
            kind, _, nodes = table[sub]
            if kind == "compound":
                raise RuleError("utg", line, "a compound sub-unitig")
            at = edges_of(nodes, "utg", line)
            for a, b, w in zip(nodes[:-1], nodes[1:], score[at]):
                if w <= 0 or w >= 1 << 40:
                    raise RuleError("utg", line, "a weight <= 0 or >= 2^40")
                seen.update((a, b))
                if b not in [x for x, _ in adj.setdefault(a, [])]:
                    adj[a].append((b, int(w)))
        s, t = tkey[0], tkey[2]
        if s not in seen or t not in seen or s == t:
            raise RuleError("utg", line, "s or t")
        found, gone = [], set()
        while True:
            r = shortest(adj, gone, s, t)
            if r is None:
                break
            if on_round:
                on_round(adj, gone, s, t, r[0])
            st["compound_tie_rounds"] += r[2] > 1
            found.append((r[0], [name(x) for x in r[1]], r[1]))
            gone.update(zip(r[1][:-1], r[1][1:]))
        if not found:
            raise RuleError("utg", line, "no path")
        found.sort(key=lambda x: (x[0], x[1]), reverse=True)
        return [x[2] for x in found]

    def lines_of(ctg_id, nodes, file, line):
        at = edges_of(nodes, file, line)
        dl = np.abs(es[at] - et[at])
        start = np.cumsum(dl) - dl
        return ["%s %s %s %09d %d %d %d %d.%02d %d %d\n" % (ctg_id, name(nodes[i]), name(nodes[i + 1]), rid[a], es[a], et[a], score[a], hund[a] // 100, hund[a] % 100,
                                                         start[i], dl[i]) for i, a in enumerate(at)]

    # ---- the rows of ctg_paths
    bundles, layout, p_out, a_out = {}, set(), [], []
    for k, ln in enumerate(ctg.decode().split("\n")):
        f = ln.split()
        if not f:
            continue
        if len(f) != 7:
            raise RuleError("ctg", k, "fields")
        s0, t0 = key_of(f[2].split("~")[0]), key_of(f[3])
        if (rev(t0), rev(s0)) in layout:
            st["ctg_skipped"] += 1
            continue
        layout.add((s0, t0))
        int(f[4])
        path, group = [], {}
        for u in f[6].split("|"):
            tkey, (kind, uline, body) = unitig(u, "ctg", k)
            if kind == "simple":
                path += body[1:] if path else body
            elif kind == "compound":
                if tkey not in bundles:
                    bundles[tkey] = bundle(tkey, uline, body)
                best = bundles[tkey][0]
                path += best[1:] if path else best
                group[(tkey[0], tkey[2])] = bundles[tkey]
        if not path:
            st["ctg_empty"] += 1
            continue
        if len(path) < 2:
            raise RuleError("ctg", k, "a path of one node")
        st["ctg_kept"] += 1
        p_out += lines_of(f[0], path, "ctg", k)
        for a_id, alts in enumerate(group.values()):
            for sub_id in range(1, len(alts)):
                a_out += lines_of("%s-%03d-%02d" % (f[0], a_id + 1, sub_id), alts[sub_id], "ctg", k)
                st["alternates"] += 1
    st["p_rows"], st["a_rows"] = len(p_out), len(a_out)
    return "".join(p_out).encode(), "".join(a_out).encode(), st


def rows_of_text(text: bytes):
    """(rows as TILE_ROW-like tuples, names in order of first appearance) of a tiling path file"""
    names, number, rows = [], {}, []
    for ln in text.decode().split("\n")[:-1]:
        f = ln.split(" ")
        if f[0] not in number:
            number[f[0]] = len(names)
            names.append(f[0])
        v, w = key_of(f[1]), key_of(f[2])
        rows.append((number[f[0]], v >> 1, w >> 1, int(f[4]), int(f[5]), 0 if v & 1 else 1, 0 if w & 1 else 1))
    return rows, names


# ---- a builder of the three files --------------------------------------------------------------------------------------------------------
class Builder:
    """G edges along node paths, unitig lines and contig rows; the texts as the script's producers format them"""

    def __init__(self, seed=0):
        self.rng = np.random.default_rng(seed)
        self.sg, self.utg, self.ctg, self.edges, self.used = [], [], [], {}, set()

    def edge(self, v, w, length=None, score=None, idt=None, kind="G", s=None):
        if (v, w) in self.edges and kind == "G":
            return self.edges[(v, w)]
        length = int(self.rng.integers(200, 3000)) if length is None else length
        score = self.fresh_score() if score is None else score
        s = int(self.rng.integers(0, 9000)) if s is None else s
        s, t = (s, s + length) if w & 1 else (s + length, s)
        idt = "%5.2f" % (int(self.rng.integers(960, 1000)) / 10.0) if idt is None else idt
        self.sg.append("%s %s %09d %5d %5d %5d %s %s\n" % (name(v), name(w), w >> 1, s, t, score, idt, kind))
        if kind == "G":
            self.edges[(v, w)] = (length, score)
        return length, score

    def fresh_score(self):
        """a score no other edge has, of a set whose subset sums are distinct with overwhelming probability"""
        while True:
            x = int(self.rng.integers(1000, 1 << 30))
            if x not in self.used:
                self.used.add(x)
                return x

    def simple(self, nodes, kind="simple", **kw):
        tot = [self.edge(a, b, **kw) for a, b in zip(nodes[:-1], nodes[1:])]
        self.utg.append("%s %s %s %s %d %d %s\n" % (name(nodes[0]), name(nodes[1]), name(nodes[-1]), kind, sum(x[0] for x in tot), sum(x[1] for x in tot),
                                                    "~".join(name(x) for x in nodes)))
        return "%s~%s~%s" % (name(nodes[0]), name(nodes[1]), name(nodes[-1]))

    def compound(self, s, t, subs):
        self.utg.append("%s NA %s compound 0 0 %s\n" % (name(s), name(t), "|".join(subs)))
        return "%s~NA~%s" % (name(s), name(t))

    def contig(self, ctg_id, utgs, t0, kind="ctg_linear"):
        self.ctg.append("%s %s %s %s %d %d %s\n" % (ctg_id, kind, utgs[0], name(t0), 0, 0, "|".join(utgs)))

    def files(self):
        return "".join(self.sg).encode(), "".join(self.utg).encode(), "".join(self.ctg).encode()


def bubble(b, s, t, first, n_ways, lens):
    """n_ways branches from s to t through fresh reads first, first + 1, ..; returns the compound unitig and the next unused read"""
    subs = []
    for way in range(n_ways):
        inner = [key(first + i, E) for i in range(lens[way % len(lens)])]
        first += len(inner)
        subs.append(b.simple([s] + inner + [t]))
    return b.compound(s, t, subs), first


def random_case(seed):
    """chains, bubbles, dual rows and rings of a few hundred edges: (sg, utg, ctg)"""
    rng = np.random.default_rng(1000 + seed)
    b = Builder(seed)
    rid, n_ctg = 1, 0
    for _ in range(int(rng.integers(1, 6))):
        utgs, at = [], key(rid, E)
        rid += 1
        first = at
        for _ in range(int(rng.integers(1, 5))):
            if rng.random() < 0.4:
                t = key(rid, E)
                u, rid = bubble(b, at, t, rid + 1, int(rng.integers(2, 4)), [int(x) for x in rng.integers(1, 5, 3)])
            else:
                nodes = [at] + [key(rid + i, int(rng.integers(0, 2))) for i in range(int(rng.integers(1, 120)))]
                rid += len(nodes)
                t = nodes[-1]
                u = b.simple(nodes)
            utgs.append(u)
            at = t
        if rng.random() < 0.3:
            utgs.insert(int(rng.integers(1, len(utgs) + 1)), b.simple([key(rid, E), key(rid + 1, E)], kind="contained"))
            rid += 2
        b.contig("%06dF" % n_ctg, utgs, at)
        if rng.random() < 0.5:   # the dual row: skipped (its unitigs need not exist)
            b.contig("%06dR" % n_ctg, ["%s~%s~%s" % (name(rev(at)), name(rev(at)), name(rev(first)))], rev(first))
        n_ctg += 1
    for k in range(int(rng.integers(0, 30))):   # edges of other types among them
        b.sg.insert(int(rng.integers(0, len(b.sg) + 1)), "%s %s %09d %5d %5d %5d %5.2f %s\n" % (name(key(rid, E)), name(key(rid + 1, B)), rid + 1, 5, 900, 77, 98.5,
                                                                                             ("TR", "S", "R")[k % 3]))
        rid += 2
    return b.files()
