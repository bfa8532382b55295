#!/usr/bin/env python3
"""Golden vectors for the map merge: the REAL reference's shmr_map (oracle/_ref) on the tiny set of tiny_stage.npz against three contigs
cut from the reads' genome, in 3 chunks (inputs built the way make_golden_query.py builds its own), and GNU sort's merge of the three
outputs, `cat map_1 map_2 map_3 | LC_ALL=C sort -k 1 -g -k 2 -g` (pg_run.py:491-496).  The versions of sort and of the C library are
recorded beside the data.  Run in the build container: python tests/golden/make_golden_mapmerge.py"""
import json
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_util as U  # noqa: E402
from peregrine_amd import formats, simreads  # noqa: E402


def main():
    assert U.have_ref()
    tiny = np.load(os.path.join(HERE, "tiny_stage.npz"))
    tmp = tempfile.mkdtemp(prefix="goldenmm_")
    pre = os.path.join(tmp, "sd")
    open(pre + ".seqdb", "wb").write(tiny["seqdb"].tobytes())
    open(pre + ".idx", "wb").write(tiny["idx_text"].tobytes())
    sp = os.path.join(tmp, "ix-L2")
    for c in (1, 2):
        formats.write_mmlist(f"{sp}-{c:02d}-of-02.dat", tiny[f"ix2l2_L2_{c}"])
        mc = np.zeros(len(tiny[f"ix2l2_L2MC_{c}"]), formats.MC_DTYPE)
        mc["mer"], mc["count"] = tiny[f"ix2l2_L2MC_{c}"][:, 0], tiny[f"ix2l2_L2MC_{c}"][:, 1]
        formats.write_mm_count(f"{sp}-MC-{c:02d}-of-02.dat", mc)
    cfg = dict(simreads.WORKLOADS["tiny"])
    g = simreads.make_genome(cfg["genome_len"], cfg["genome_seed"])
    contigs = [g[:30000], (3 - g[24000:])[::-1], g[10000:10900]]

    def enc(codes):
        codes = np.asarray(codes, np.uint8)
        return ((np.uint8(1) << codes) | ((np.uint8(8) >> codes[::-1]) << np.uint8(4))).astype(np.uint8)

    rlen = np.array([len(c) for c in contigs], np.uint32)
    ref_db = formats.SeqDB(np.concatenate([enc(c) for c in contigs]), np.arange(len(contigs), dtype=np.uint32), rlen,
                           np.concatenate([[0], np.cumsum(rlen.astype(np.uint64))[:-1]]).astype(np.uint64), [f"ctg{i}" for i in range(len(contigs))])
    rpre = os.path.join(tmp, "ref")
    formats.write_seqdb(rpre, ref_db)
    U.ref_run("shmr_index", "-p", rpre, "-t", 1, "-c", 1, "-l", 2, "-r", 6, "-o", os.path.join(tmp, "ref"))
    store, paths = {}, []
    for c in (1, 2, 3):
        out = subprocess.run([os.path.join(U.REF_DIR, "shmr_map"), "-r", rpre, "-m", os.path.join(tmp, "ref-L2"), "-p", pre, "-l", sp, "-t", "3", "-c", str(c)],
                             check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
        store[f"map_{c}"] = np.frombuffer(out, np.uint8)
        paths.append(os.path.join(tmp, f"map_{c}.dat"))
        open(paths[-1], "wb").write(out)
        print("shmr_map chunk", c, out.count(b"\n"), "lines")
    env = {"LC_ALL": "C", "PATH": os.environ["PATH"]}
    cat = b"".join(open(p, "rb").read() for p in paths)
    merged = subprocess.run(["sort", "-k", "1", "-g", "-k", "2", "-g"], input=cat, check=True, stdout=subprocess.PIPE, env=env).stdout
    store["sorted"] = np.frombuffer(merged, np.uint8)
    np.savez_compressed(os.path.join(HERE, "mapmerge_cases.npz"), **store)
    prov = {"made_by": "tests/golden/make_golden_mapmerge.py",
            "what": "shmr_map (the reference's, compiled in place) on tiny_stage.npz's reads against three contigs of their genome, -t 3 -c 1..3; "
                    "GNU sort's `LC_ALL=C sort -k 1 -g -k 2 -g` of the three outputs concatenated",
            "sort_version": subprocess.check_output(["sort", "--version"], text=True).splitlines()[0],
            "libc": " ".join(platform.libc_ver()),
            "lines": int(merged.count(b"\n"))}
    json.dump(prov, open(os.path.join(HERE, "mapmerge_cases.provenance.json"), "w"), indent=1)
    print(prov, os.path.getsize(os.path.join(HERE, "mapmerge_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
