"""The GFA rule in plain Python over arrays: from the unitigs' table and path array (Unitigs.table() / .paths(), or utg_util.unitigs) and
the edge records to segments, rows, links and the file's text.  TEST INFRASTRUCTURE, written from the rule as the project states it
(include/pgx.h, "assembly graph as GFA"): lists and dictionaries indexed by integers, no graph objects.

  dual      dual(u) holds the reverse (rev w, rev v) of u's first edge
  segments  u with u < dual(u), numbered in ascending u, named utg%06u of u
  rows      per edge of the path: (j, v_rid, w_rid, sp, tp, 1 - v_end, 1 - w_end)
  links     every (a, b) with t(a) == s(b), found as the G out-edges of t(a); of (a, b) and (dual b, dual a) the smaller is written
  text      H, the S lines (with the bases passed in and LN, or '*'), the L lines with '*' for the overlap
"""
import numpy as np

from sgraph_util import G

SEGMENT_DTYPE = np.dtype([("unitig", "<u4"), ("dual", "<u4"), ("n_rows", "<u4"), ("circular", "u1"), ("pad", "u1", (3,)), ("first_row", "<u8"),
                          ("seq_off", "<u8"), ("seq_len", "<u8")])   # pgx_gfa_segment
LINK_DTYPE = np.dtype([("from_seg", "<u4"), ("to_seg", "<u4"), ("from_rev", "u1"), ("to_rev", "u1"), ("pad", "u1", (2,))])   # pgx_gfa_link
ROW_DTYPE = np.dtype([("ctg", "<u4"), ("rid0", "<u4"), ("rid1", "<u4"), ("s", "<i4"), ("e", "<i4"), ("strand0", "u1"), ("strand1", "u1"),
                      ("pad", "u1", (2,))])   # pgx_tile_row
HEADER = b"H\tVN:Z:1.0\n"


def node_keys(edges):
    v = (edges["v_rid"].astype(np.int64) << 1) | edges["v_end"]
    w = (edges["w_rid"].astype(np.int64) << 1) | edges["w_end"]
    return [int(x) for x in v], [int(x) for x in w]


def duals(edges, table, paths):
    """dual(u) for every unitig, by rule 1 (host records: the edge (rev w, rev v)); asserts what the rule says follows"""
    v, w = node_keys(edges)
    g = [int(e) for e in np.flatnonzero(edges["type"] == G)]
    edge_at = {(v[e], w[e]): e for e in g}
    unitig_of = {}
    for u, r in enumerate(table):
        for e in paths[int(r["first"]):int(r["first"]) + int(r["n_edges"])]:
            unitig_of[int(e)] = u
    dual = []
    for r in table:
        e = int(paths[int(r["first"])])
        dual.append(unitig_of[edge_at[(w[e] ^ 1, v[e] ^ 1)]])
    assert all(dual[dual[u]] == u and dual[u] != u for u in range(len(table)))
    return dual, unitig_of


def gfa(edges, table, paths, bases=None):
    """(segments, rows, links_directed (list of (a, b)), links, text) of the unitigs; bases: the segments' sequences in segment order (a
    list of bytes), or None for the topology-only file"""
    v, w = node_keys(edges)
    dual, unitig_of = duals(edges, table, paths)
    n_u = len(table)
    canon = [u for u in range(n_u) if u < dual[u]]
    seg_of = {}
    for j, u in enumerate(canon):
        seg_of[u] = seg_of[dual[u]] = j
    segments = np.zeros(len(canon), SEGMENT_DTYPE)
    rows = []
    for j, u in enumerate(canon):
        r = table[u]
        segments[j]["unitig"], segments[j]["dual"], segments[j]["n_rows"], segments[j]["circular"], segments[j]["first_row"] = u, dual[u], r["n_edges"], r["circular"], len(rows)
        for e in paths[int(r["first"]):int(r["first"]) + int(r["n_edges"])]:
            x = edges[int(e)]
            rows.append((j, int(x["v_rid"]), int(x["w_rid"]), int(x["sp"]), int(x["tp"]), 1 - int(x["v_end"]), 1 - int(x["w_end"])))
    if bases is not None:
        assert len(bases) == len(canon)
        at = 0
        for j, b in enumerate(bases):
            segments[j]["seq_off"], segments[j]["seq_len"] = at, len(b)
            at += len(b)
    cols = list(zip(*rows)) if rows else [[]] * 7
    rows = np.zeros(len(cols[0]), ROW_DTYPE)
    for field, col in zip(("ctg", "rid0", "rid1", "s", "e", "strand0", "strand1"), cols):
        rows[field] = col
    # links: the out-list of t(a); every out-edge of t(a) is the first edge of a unitig
    out = {}
    for e in (int(x) for x in np.flatnonzero(edges["type"] == G)):
        out.setdefault(v[e], []).append(e)
    first_of = {int(paths[int(r["first"])]): u for u, r in enumerate(table)}
    directed = []
    for a, r in enumerate(table):
        t = int(r["t_rid"]) << 1 | int(r["t_end"])
        directed += [(a, first_of[e]) for e in out.get(t, [])]
    directed.sort()
    kept = [(a, b) for a, b in directed if (a, b) < (dual[b], dual[a])]
    assert all((a, b) != (dual[b], dual[a]) for a, b in directed)
    links = np.zeros(len(kept), LINK_DTYPE)
    for k, (a, b) in enumerate(kept):
        links[k]["from_seg"], links[k]["to_seg"], links[k]["from_rev"], links[k]["to_rev"] = seg_of[a], seg_of[b], a > dual[a], b > dual[b]

    def name(x):
        return b"utg%06d\t%s" % (min(x, dual[x]), b"+" if x < dual[x] else b"-")

    lines = [HEADER]
    for j, u in enumerate(canon):
        if bases is None:
            lines.append(b"S\tutg%06d\t*\n" % u)
        else:
            lines.append(b"S\tutg%06d\t%s\tLN:i:%d\n" % (u, bases[j], len(bases[j])))
    lines += [b"L\t%s\t%s\t*\n" % (name(a), name(b)) for a, b in kept]
    return segments, rows, directed, links, b"".join(lines)


def parse(text: bytes):
    """(segments: name -> bases, links: list of (a, ±, b, ±)) of a GFA text, its form checked line by line"""
    lines = text.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b""
    seg, links = {}, []
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        if f[0] == b"S":
            assert not links and f[1] not in seg and (f[2:] == [b"*"] or (len(f) == 4 and f[3] == b"LN:i:%d" % len(f[2])))
            seg[f[1]] = f[2]
        else:
            assert f[0] == b"L" and len(f) == 6 and f[1] in seg and f[3] in seg and f[2] in (b"+", b"-") and f[4] in (b"+", b"-") and f[5] == b"*"
            links.append((f[1], f[2], f[3], f[4]))
    return seg, links
