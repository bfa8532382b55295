"""Generator of tests/golden/cnsjob_cases.npz: seeded read and contig databases, map rows, and what the REAL reference script makes of them.

The script py/scripts/pg_asm_cns.py runs in place, as a child process, on databases written from tests/cnsjob_util.py's builders.  Its
`peregrine._shimmer4py` is the stand-in under tests/golden/shimmer4py_standin (decode_biseq of oracle/_ref/libshimmer_ref.so), its
`peregrine._falcon4py` the stand-in beside it: ctypes over the reference's falcon sources, compiled as make_golden_cns.compile_reference
compiles them, into a temporary directory.  Both are on PYTHONPATH for that child only.  Stored: the seeds' databases as SHA-256, the map
text, and per chunk the script's stdout and the layout parsed from its stderr (per group `left right n_mapped`, the `(read, strand) offset`
lines in the script's order, the accepted reads in order, aln_count and aln_base).  Before anything is stored the restatement of
cnsjob_util must give the same layout and the same stdout.

  bio    two contigs of 120 kb and 60 kb, reads of 8 kb at 1 % on both strands at about 6x, map rows at the true positions with a few
         bases of jitter, the file's rows shuffled.  Asserted: at least three quarters of the pieces go through the consensus call.
  edges  hand-placed rows (cnsjob_util.build_edges), total_chunks = 3 with my_chunk 0 .. 3: contig lengths 1, 999, 1000, 1999, 2000, 2001,
         2002; p1 - left_anchor of 49,999 / 50,000 / 99,999 / 100,000; tails of 1,000 / 1,001 / 99,999 / 100,000; the tail merged into a
         group that had rows and into one that had none; equal p1 in file order; offsets 50 and 51 apart and a chain of 40 + 40; one read on
         both strands and in two groups; equal, negative and too large shifts; p1 < 1000; a lower-case segment between two called ones;
         contig ids interleaved in the file.

    python tests/golden/make_golden_cnsjob.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
import cnsjob_util as J  # noqa: E402
import make_golden_cns as G  # noqa: E402
from peregrine_amd import formats  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libshimmer_ref.so")
SCRIPT = os.path.join(os.path.dirname(G.FALCON.rstrip("/")), "py", "scripts", "pg_asm_cns.py")


def run_reference(tmp, tag, total, my):
    env = dict(os.environ, PYTHONPATH=os.path.join(HERE, "shimmer4py_standin"), SHIMMER_REF_LIB=REF_LIB, FALCON_REF_LIB=os.path.join(tmp, "libfalcon_ref.so"))
    env.pop("SHIMMER_MATCH_LOG", None)
    r = subprocess.run([sys.executable, SCRIPT, os.path.join(tmp, tag + "_reads"), os.path.join(tmp, tag + "_ref"), os.path.join(tmp, tag + ".map"),
                        str(total), str(my)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def main():
    out, stats = dict(names=np.array(list(J.BUILDERS))), {}
    with tempfile.TemporaryDirectory() as tmp:
        G.compile_reference(tmp)
        for name, build in J.BUILDERS.items():
            b, text = build()
            rdb, cdb = b.dbs()
            formats.write_seqdb(os.path.join(tmp, name + "_reads"), rdb)
            formats.write_seqdb(os.path.join(tmp, name + "_ref"), cdb)
            open(os.path.join(tmp, name + ".map"), "w").write(text)
            out[name + "_map"], out[name + "_read_sha256"], out[name + "_ref_sha256"] = np.array(text), np.array(J.db_sha256(rdb)), np.array(J.db_sha256(cdb))
            name_to_ctg = {n: int(r) for r, n in zip(cdb.rid, cdb.names)}
            rl, _ = cdb.by_rid()
            st = dict(reads=rdb.n_reads, contigs=cdb.n_reads, rows=len(b.rows), chunks={})
            for total, my in J.CHUNKS[name]:
                t0 = time.time()
                fasta, err = run_reference(tmp, name, total, my)
                t_ref = time.time() - t0
                lay, runs = J.parse_stderr(err, name_to_ctg)
                # the restatement, before anything is stored
                mine = J.layout(J.chunk_rows(J.parse_map(text), total, my), {int(r): int(rl[int(r)]) for r in cdb.rid})
                assert [c["ctg"] for c in mine] == [c["ctg"] for c in lay], (name, my)
                for a, c in zip(mine, lay):
                    assert [(g["left"], g["right"], g["n_mapped"], g["offsets"]) for g in a["groups"]] == \
                           [(g["left"], g["right"], g["n_mapped"], g["offsets"]) for g in c["groups"]], (name, my, a["ctg"])
                det = []
                t0 = time.time()
                assert J.job(rdb, cdb, text, total, my, details=det) == fasta, (name, my)
                groups = [(g, c["ctg"]) for c in mine for g in c["groups"]]
                assert len(det) == len(runs) == len(groups)
                for (ctg, seg, said, n, base), run, (g, _) in zip(det, runs, groups):
                    assert [e[0] for e, s in zip(g["entries"], said) if s] == run["accepted"] and (n, base) == (run["aln_count"], run["aln_base"]), (name, ctg, seg)
                called = sum(1 for (g, _), run in zip(groups, runs) if run["aln_base"] / (g["right"] - g["left"] + J.FLANK) >= 3)
                st["chunks"][f"{total}_{my}"] = dict(contigs=len(lay), pieces=len(runs), called=called, fasta_bytes=len(fasta), script_s=round(t_ref, 2),
                                                    restatement_s=round(time.time() - t0, 2))
                k = f"{name}_{total}_{my}"
                out[k + "_stdout"], out[k + "_layout"] = np.frombuffer(fasta, np.uint8), np.array(json.dumps([lay, runs]))
            stats[name] = st
    bio = stats["bio"]["chunks"]["1_0"]
    assert 4 * bio["called"] >= 3 * bio["pieces"], bio
    e = stats["edges"]["chunks"]["3_0"]
    assert e["called"] >= 3, e
    prov = dict(generator="tests/golden/make_golden_cnsjob.py", reference_script="py/scripts/pg_asm_cns.py",
                reference_script_sha256=hashlib.sha256(open(SCRIPT, "rb").read()).hexdigest(),
                falcon_sources={s: hashlib.sha256(open(os.path.join(G.FALCON, s), "rb").read()).hexdigest() for s in G.SOURCES}, cflags=G.CFLAGS,
                shimmer4py="tests/golden/shimmer4py_standin (ctypes; decode_biseq of oracle/_ref/libshimmer_ref.so)",
                falcon4py="tests/golden/shimmer4py_standin/peregrine/_falcon4py.py (ctypes)", cases=stats)
    dst = os.path.join(HERE, "cnsjob_cases.npz")
    np.savez_compressed(dst, provenance=np.array(json.dumps(prov)), **out)
    with open(os.path.join(HERE, "cnsjob_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", json.dumps(stats))


if __name__ == "__main__":
    main()
