#!/usr/bin/env python3
"""Drop-in for the reference script `path_to_contig.py` (py/scripts/path_to_contig.py; pg_run.py:356-362 runs it for the primary and
for the alternate contigs): `path_to_contig.py seqdb_prefix tiling_path > contigs.fa`.  The stitching alignments and the layout run
on the GPU (pgx_contigs_chunk); the FASTA on stdout is byte for byte the script's."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PGX_NO_TORCH", "1")  # a stand-alone executable: no PyTorch in this process, skip its import


def main():
    if len(sys.argv) != 3:
        sys.stderr.write("Usage: path_to_contig.py seqdb_prefix tiling_path > contigs.fa\n")
        return 1
    from peregrine_amd import _lib
    from peregrine_amd.shimmer import path_to_contig
    try:
        path_to_contig(sys.argv[1], sys.argv[2])
    except _lib.PgxError as e:
        sys.stderr.write(f"path_to_contig.py: {e}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
