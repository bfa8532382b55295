"""Generator of tests/golden/contig_cases.npz: tiling paths over a seeded read set and what the REAL reference script makes of them.

The script py/scripts/path_to_contig.py runs in place, as a child process, on a seqdb written from tests/contig_util.make_db(); its
`peregrine._shimmer4py` is the stand-in under tests/golden/shimmer4py_standin (ctypes over oracle/_ref/libshimmer_ref.so, the reference's own
ovlp_match and decode_biseq), on PYTHONPATH for that child only.  Stored: the seqdb's SHA-256, the tiling-path texts, the script's stdout.
  bio  chains over the dedup lines of the read set's own overlap stage (oracle), both strands: for a dovetail whose coordinates the line gives
       exactly, `s` / `e` name the part of w beyond the overlap.  Asserted: >= 90 % of its rows have q_m_end >= 400 in the script's own calls.
  adv  valid but arbitrary rows: unrelated reads (unmatched alignments), a query of N only (q_m_end = t_m_end = 0), true overlaps with a short
       overhang followed by an unrelated row (a segment shorter than 500 - q_m_end: the next start lies BEFORE it), a read against itself
       (seg == 0), a one-row contig, a contig id that comes back after another contig, the read that holds N on both strands.

    python tests/golden/make_golden_contigs.py [path/to/reference/py/scripts/path_to_contig.py]
"""
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
import contig_util as CU  # noqa: E402
import oracle_util as U  # noqa: E402
from peregrine_amd import formats  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libshimmer_ref.so")
SCRIPT = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/py/scripts/path_to_contig.py"


def dovetail_edges(db):
    """node (rid, strand) -> [(node, x)]: w's bases from x on lie beyond v's end; only the dovetails whose x the dedup line gives exactly"""
    l0 = np.concatenate([U.orc_sketch_seqdb(db.seqdb[int(o):int(o) + int(n)], 80, 16, int(r)) for r, n, o in zip(db.rid, db.rlen, db.roff)])
    l2 = U.orc_reduce(U.orc_reduce(l0, 6), 6)
    ov, _ = U.orc_overlap(db, l2, U.orc_count(l2))
    text, _ = U.orc_dedup(ov)
    edges = {}
    for ln in text.decode().splitlines():
        f = ln.split()
        if f[12] != "overlap":
            continue
        a, b, a_bgn, a_end, la, sb, b_bgn, b_end, lb = int(f[0]), int(f[1]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]), int(f[10]), int(f[11])
        t_end = b_end if sb == 0 else lb - b_bgn        # the overlap's end on b's strand sb
        if a_end == la and a_bgn > 0 and CU.H <= t_end < lb:            # a's end runs into b: a:E -> b
            edges.setdefault((a, 0), []).append(((b, sb), t_end))
        elif a_bgn == 0 and t_end == lb and CU.H <= a_end < la:         # b's end runs into a: b -> a:E
            edges.setdefault((b, sb), []).append(((a, 0), a_end))
    return edges


def row(ctg, v, w, x, lw):
    """the tiling-path row of the edge v -> w that appends w's bases from x on"""
    s, e = (x, lw) if w[1] == 0 else (lw - x, 0)
    return "%s %d:%s %d:%s %d %d %d %d 99.9 0 0" % (ctg, v[0], "EB"[v[1]], w[0], "EB"[w[1]], w[0], s, e, lw - x)


def bio_path(db, edges):
    used, lines, n_ctg = set(), [], 0
    for start in sorted(edges):
        if start[0] in used or n_ctg == 6:
            continue
        chain, v = [], start
        seen = {start[0]}
        while len(chain) < 12:
            nxt = [(w, x) for w, x in edges.get(v, []) if w[0] not in used and w[0] not in seen and w[0] != CU.N_READ and v[0] != CU.N_READ]
            if not nxt:
                break
            w, x = min(nxt, key=lambda t: t[1])      # the longest extension
            chain.append((v, w, x))
            seen.add(w[0])
            v = w
        if len(chain) >= 4:
            used |= seen
            lines += [row("ctg%03d" % n_ctg, v, w, x, int(db.rlen[w[0]])) for v, w, x in chain]
            n_ctg += 1
    assert n_ctg >= 4 and {ln.split()[2][-1] for ln in lines} == {"E", "B"}, (n_ctg, "both strands are needed")
    return "\n".join(lines) + "\n"


def adv_path(db, edges):
    rng = np.random.default_rng(77)
    rl = db.rlen.astype(np.int64)
    others = [int(r) for r in db.rid if r != CU.N_READ]

    def arbitrary(ctg, v=None, w=None, span=None):
        """valid, unrelated: s' >= 500 so that e - seg >= 0 whatever the match, span >= 600 so that the contig's length never steps back"""
        v = v or (int(rng.choice(others)), int(rng.integers(0, 2)))
        w = w or (int(rng.choice(others)), int(rng.integers(0, 2)))
        lw = int(rl[w[0]])
        span = span or int(rng.integers(600, lw - 2 * CU.H))
        s2 = int(rng.integers(CU.H, lw - span + 1))          # on w's strand: [s2, s2 + span)
        s, e = (s2, s2 + span) if w[1] == 0 else (lw - s2, lw - s2 - span)
        return "%s %d:%s %d:%s 0 %d %d 0 0.0 x y" % (ctg, v[0], "EB"[v[1]], w[0], "EB"[w[1]], s, e)

    short = [(v, w, x) for v in sorted(edges) for w, x in edges[v] if 20 <= rl[w[0]] - x <= 400 and CU.N_READ not in (v[0], w[0])]
    assert len(short) >= 3, len(short)
    nr = CU.N_READ
    lines = [arbitrary("advA"), arbitrary("advA"), arbitrary("advA")]
    for v, w, x in short[:3]:                                 # a short true overhang, then an unrelated row: its start lies before
        lines += [row("advA", v, w, x, int(rl[w[0]])), arbitrary("advA")]
    lines += [arbitrary("one")]
    lines += [arbitrary("advB", v=(nr, 0)), arbitrary("advB", w=(nr, 1)), arbitrary("advB", v=(nr, 0), w=(nr, 0)), arbitrary("advB", v=(nr, 1), w=(nr, 1))]
    r = others[3]
    lr = int(rl[r])
    lines += ["advB %d:E %d:E 0 %d %d 0 0.0 x y" % (r, r, lr - 40, lr),            # a read against itself: t_m_end = |e - s| + 500, seg == 0
              "advB %d:B %d:B 0 %d %d 0 0.0 x y" % (r, r, 60, 0), arbitrary("advB")]
    lines += [arbitrary("advA"), arbitrary("advA", v=(nr, 0)), arbitrary("advA")]    # advA comes back after two other contigs
    return "\n".join(lines) + "\n"


def run_reference(prefix, path_text, tmp, tag):
    tp = os.path.join(tmp, tag + ".path")
    log = os.path.join(tmp, tag + ".log")
    open(tp, "w").write(path_text)
    env = dict(os.environ, PYTHONPATH=os.path.join(HERE, "shimmer4py_standin"), SHIMMER_REF_LIB=REF_LIB, SHIMMER_MATCH_LOG=log)
    r = subprocess.run([sys.executable, SCRIPT, prefix, tp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return r.stdout, np.loadtxt(log, dtype=np.int64, ndmin=2)


def main():
    db = CU.make_db()
    edges = dovetail_edges(db)
    paths = dict(bio=bio_path(db, edges), adv=adv_path(db, edges))
    out, stats = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "reads")
        formats.write_seqdb(prefix, db)
        for tag, text in paths.items():
            fasta, ends = run_reference(prefix, text, tmp, tag)
            assert len(ends) == text.count("\n")
            out[tag] = fasta
            stats[tag] = dict(rows=len(ends), contigs=int(fasta.count(b">")), bases=len(fasta), share_q_m_end_ge_400=float((ends[:, 0] >= 400).mean()),
                              unmatched_q0=int((ends[:, 0] == 0).sum()),   # (the script's calls come contig by contig: parse_path's order)
                              seg0=int(sum(1 for r, (q, t) in zip(CU.parse_path(text)[0], ends) if abs(r[6] - r[5]) + CU.H == t)))
    assert stats["bio"]["share_q_m_end_ge_400"] >= 0.9, stats["bio"]
    assert stats["adv"]["unmatched_q0"] >= 2 and stats["adv"]["seg0"] >= 2, stats["adv"]
    assert out["bio"] == CU.layout(db, paths["bio"], U.ref_ovlp_match) and out["adv"] == CU.layout(db, paths["adv"], U.ref_ovlp_match)
    prov = dict(generator="tests/golden/make_golden_contigs.py", reference_script="py/scripts/path_to_contig.py",
                reference_script_sha256=hashlib.sha256(open(SCRIPT, "rb").read()).hexdigest(), reference_lib="oracle/_ref/libshimmer_ref.so",
                shimmer4py="tests/golden/shimmer4py_standin (ctypes)", genome=CU.GENOME, reads=CU.READS, n_read=CU.N_READ, cases=stats)
    dst = os.path.join(HERE, "contig_cases.npz")
    np.savez_compressed(dst, seqdb_sha256=np.array(CU.seqdb_sha256(db)), provenance=np.array(json.dumps(prov)),
                        **{"path_" + t: np.array(p) for t, p in paths.items()}, **{"fasta_" + t: np.frombuffer(f, np.uint8) for t, f in out.items()})
    with open(os.path.join(HERE, "contig_cases.provenance.json"), "w") as f:   # (a file of its own, next to provenance.json)
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", json.dumps(stats))


if __name__ == "__main__":
    main()
