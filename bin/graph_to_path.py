#!/usr/bin/env python3
"""Drop-in for the reference script `graph_to_path.py` (py/scripts/graph_to_path.py; pg_run.py runs it between ovlp_to_graph.py and
path_to_contig.py): the script's six options, p_ctg_tiling_path and a_ctg_tiling_path written into the working directory, nothing on
stdout.  The edge file is tokenised and every node, edge and line of the paths is made on the GPU (pgx_tiling_chunk); the files are
byte for byte the script's."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PGX_NO_TORCH", "1")  # a stand-alone executable: no PyTorch in this process, skip its import


def main():
    ap = argparse.ArgumentParser(description="Generate the primary and alternate tiling paths, given the string graph.")
    ap.add_argument("--improper-p-ctg", action="store_true", help="accepted; changes nothing in the tiling paths (as in the script)")
    ap.add_argument("--proper-a-ctg", action="store_true", help="accepted; changes nothing in the tiling paths (as in the script)")
    ap.add_argument("--seqdb-prefix", default="./seq_dataset", help="the reads, for --p-ctg-fa / --a-ctg-fa; the tiling paths do not read them")
    ap.add_argument("--sg-edges-list-fn", default="./sg_edges_list")
    ap.add_argument("--utg-data-fn", default="./utg_data")
    ap.add_argument("--ctg-paths-fn", default="./ctg_paths")
    ap.add_argument("--p-ctg-fa", metavar="FILE", help="extension: also lay the primary contigs out, from the rows, as FASTA")
    ap.add_argument("--a-ctg-fa", metavar="FILE", help="extension: the same for the alternate contigs")
    args = ap.parse_args()
    from peregrine_amd import _lib
    from peregrine_amd.shimmer import graph_to_path
    try:
        graph_to_path(args.sg_edges_list_fn, args.utg_data_fn, args.ctg_paths_fn, "p_ctg_tiling_path", "a_ctg_tiling_path", seqdb_prefix=args.seqdb_prefix,
                      p_ctg_fa=args.p_ctg_fa, a_ctg_fa=args.a_ctg_fa)
    except _lib.PgxError as e:
        sys.stderr.write(f"graph_to_path.py: {e}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
