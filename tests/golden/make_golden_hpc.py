#!/usr/bin/env python3
"""Writes tests/golden/hpc_cases.npz and hpc_cases.provenance.json: the strings of tests/hpc_util.py (directed + seeded random) with
the list mm_sketch(is_hpc = 1) of the compiled reference (oracle/_ref/libshimmer_ref.so) gives for each as read 0, and -- at w = 80,
k = 16 -- that list reduced once and twice by its mm_reduce with r = 6.  Data only.   usage: python tests/golden/make_golden_hpc.py"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import hpc_util as H   # noqa: E402
import oracle_util as U   # noqa: E402


def pool(arrs, dtype):
    off = np.zeros(len(arrs) + 1, np.uint64)
    np.cumsum([len(a) for a in arrs], out=off[1:])
    return (np.concatenate(arrs) if arrs else np.zeros(0, dtype)), off


def main():
    cases = H.all_cases()
    names, seqs, ws, ks, l0s, l1s, l2s = [], [], [], [], [], [], []
    empty = np.zeros((0, 2), np.uint64)
    for name, seq, w, k in cases:
        l0 = H.ref_sketch_hpc(seq, w, k, 0)
        l1 = l2 = None
        if (w, k) == (H.W, H.K):
            l1 = U.ref_reduce(l0, H.R)
            l2 = U.ref_reduce(l1, H.R)
        as2 = lambda a: empty if a is None else np.stack([a["x"], a["y"]], axis=1).astype(np.uint64).reshape(-1, 2)
        names.append(name), seqs.append(np.frombuffer(seq, np.uint8)), ws.append(w), ks.append(k)
        l0s.append(as2(l0)), l1s.append(as2(l1)), l2s.append(as2(l2))
    seq, seq_off = pool(seqs, np.uint8)
    l0, l0_off = pool(l0s, np.uint64)
    l1, l1_off = pool(l1s, np.uint64)
    l2, l2_off = pool(l2s, np.uint64)
    out = os.path.join(HERE, "hpc_cases.npz")
    np.savez_compressed(out, names=np.frombuffer("\n".join(names).encode(), np.uint8), seq=seq, seq_off=seq_off, w=np.array(ws, np.int32),
                        k=np.array(ks, np.int32), l0=l0, l0_off=l0_off, l1=l1, l1_off=l1_off, l2=l2, l2_off=l2_off)
    prov = dict(what="mm_sketch(is_hpc = 1) / mm_reduce(r = 6) of the compiled reference on the strings of tests/hpc_util.all_cases()",
                made_by="tests/golden/make_golden_hpc.py", cases=len(cases), directed=len(H.directed_cases()), bases=int(len(seq)),
                l0_elements=int(len(l0)), l1_elements=int(len(l1)), l2_elements=int(len(l2)), nonempty_l0=int(sum(len(a) > 0 for a in l0s)),
                cases_with_a_run_of_241_or_more=int(sum(bool(re.search(rb"A{241}|C{241}|G{241}|T{241}", c[1].upper())) for c in cases)),
                sha256=hashlib.sha256(open(out, "rb").read()).hexdigest(), bytes=os.path.getsize(out))
    with open(os.path.join(HERE, "hpc_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(json.dumps(prov))


if __name__ == "__main__":
    main()
