"""Stand-in package for the golden generators only: `peregrine._shimmer4py` bound to oracle/_ref/libshimmer_ref.so (see _shimmer4py.py)."""
