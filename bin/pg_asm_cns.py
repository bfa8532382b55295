#!/usr/bin/env python3
"""Drop-in for the reference script `pg_asm_cns.py` (py/scripts/pg_asm_cns.py, the last stage of pg_run.py):
`pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk > cns.fa`.  Chunk filter, read grouping, the
alignments, the consensus call and the stitching run on the GPU (pgx_cns_job); the FASTA on stdout is byte for byte the script's.  The
script's chatter on stderr is not reproduced."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("PGX_NO_TORCH", "1")  # a stand-alone executable: no PyTorch in this process, skip its import


def main():
    try:
        if len(sys.argv) != 6:
            raise ValueError
        total, my = int(sys.argv[4]), int(sys.argv[5])
        if total < 0 or my < 0:
            raise ValueError
    except ValueError:
        sys.stderr.write("Usage: pg_asm_cns.py read_db_prefix ref_db_prefix read_to_contig_map total_chunks my_chunk > cns.fa\n")
        return 1
    from peregrine_amd import _lib
    from peregrine_amd.shimmer import pg_asm_cns
    try:
        pg_asm_cns(sys.argv[1], sys.argv[2], sys.argv[3], total, my)
    except _lib.PgxError as e:
        sys.stderr.write(f"pg_asm_cns.py: {e}\n")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
