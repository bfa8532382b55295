"""Generator of tests/golden/graph_filter_cases.npz: the record set of tests/dedup_graph_util.make_records(), the REAL reference
shmr_dedup's text of it (oracle/_ref/shmr_dedup, built by `make -C oracle ref`), and the sg_edges_list that the reference's own
generate_string_graph (py/scripts/ovlp_to_graph.py, imported in place from the reference tree, nothing of it copied) writes for that text.

The same function then runs on the text shmr_dedup's graph mode would write (dedup_graph_util.select_graph_lines): the fixture is written
only if the two sg_edges_list files are byte-identical.  disable_chimer_bridge_removal=True: the chimer step iterates sets of objects, the
only step of the function whose result depends on their order.  networkx 3.4.2.

    python tests/golden/make_golden_graph_filter.py [path/to/reference/py/scripts]
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

REF = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
SCRIPTS = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/py/scripts"
MIN_LEN, MIN_IDT = 4000, 96.0


def sg_edges(text: bytes, generate_string_graph) -> bytes:
    """sg_edges_list of the text (with pg_run.py's end marker appended), written where the function writes it: the working directory"""
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            with open("preads.ovl", "wb") as f:
                f.write(text + b"-\n")
            generate_string_graph(types.SimpleNamespace(overlap_file="preads.ovl", min_len=MIN_LEN, min_idt=MIN_IDT, lfc=False,
                                                        disable_chimer_bridge_removal=True))
            return open("sg_edges_list", "rb").read()
        finally:
            os.chdir(cwd)


def main():
    import networkx
    sys.path.insert(0, SCRIPTS)
    import ovlp_to_graph
    recs = DG.make_records()
    text = subprocess.run([REF], input=recs.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    kept = DG.select_graph_lines(text)
    st = DG.graph_stats(text)
    n_reads = len({f for ln in text.split(b"\n")[:-1] for f in ln.split()[:2]})
    share = st["lines_kept"] / st["lines_total"]
    assert 0.05 <= share <= 0.95, share
    full, filtered = sg_edges(text, ovlp_to_graph.generate_string_graph), sg_edges(kept, ovlp_to_graph.generate_string_graph)
    if full != filtered:
        sys.exit("the filtered text gives another sg_edges_list: the fixture is NOT written")
    assert full.count(b"\n") > 1000, full.count(b"\n")
    prov = dict(generator="tests/golden/make_golden_graph_filter.py", reference="oracle/_ref/shmr_dedup",
                reference_sha256=hashlib.sha256(open(REF, "rb").read()).hexdigest(), reference_script="py/scripts/ovlp_to_graph.py",
                reference_script_sha256=hashlib.sha256(open(ovlp_to_graph.__file__, "rb").read()).hexdigest(), networkx=networkx.__version__,
                min_len=MIN_LEN, min_idt=MIN_IDT, disable_chimer_bridge_removal=True, n_records=len(recs), n_reads=n_reads, **st,
                sg_edges=full.count(b"\n"), sg_edges_sha256=hashlib.sha256(full).hexdigest(), filtered_text_gives_the_same_sg_edges_list=True)
    dst = os.path.join(HERE, "graph_filter_cases.npz")
    np.savez_compressed(dst, recs=recs, text=np.frombuffer(text, np.uint8), sg_edges_list=np.frombuffer(full, np.uint8),
                        provenance=np.array(json.dumps(prov)))
    with open(os.path.join(HERE, "graph_filter_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", json.dumps(prov))


if __name__ == "__main__":
    main()
