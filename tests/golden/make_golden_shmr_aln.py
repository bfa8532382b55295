"""Generator of tests/golden/shmr_aln_cases.npz: pairs of shimmer lists and the chains the REAL shmr_aln makes of them.

The reference's shmr_align.c, shmr_utils.c and kalloc.c are compiled into a temporary directory at generation time and shmr_aln is called
through ctypes with mm128_v structs; no reference text or binary is kept.  Every case also runs through the restatement of
tests/shmr_aln_util.py, which must agree chain by chain.  Stored: every list once (x, y), per case its two lists, the three parameters and
the chains as CSR.  Direction is 0 throughout (the reference's reversed walk reads one entry past list 1).

  empty_0, empty_1, empty_both, no_shared        nothing to chain
  one_shared, one_shared_opposite                one hash, taken; the same with opposite strand bits, skipped
  rep{1,3}_at, rep{1,3}_over                     a hash that list 0 holds exactly max_repeat times (every occurrence, in order) / once more (skipped)
  twice_in_list1                                 the same hash twice in list 1: equal idx0 appended again, mm_dist 0
  before_last                                    a candidate whose idx0 lies before the chain's last opens a chain
  diff_{below,at}, dist_{below,at}               diff == max_diff - 1 / max_diff, mm_dist == max_dist - 1 / max_dist
  tie_earlier, later_smaller                     two chains at the same smallest diff: the earlier; a later chain with a smaller diff: that one
  best_{1,64,65,128,129}_of_129                  the best chain at the lane boundaries of 129 live chains (max_diff 1000)
  near_2_31                                      positions up to 2^31 - 1
  stop_4810, no_stop_4810                        4,810 hashes spaced by more than max_dist: the walk stops once a scan sees more than 4,800 small
                                                 chains; the twin grows 20 chains to 3 elements first and does not stop
  rand_*                                         small seeded lists over few hashes, max_repeat 1, 2, 5
  real_fwd, real_rc, real_self                   a 20 kb template against its substituted, shifted copy, against the copy's reverse
                                                 complement and against itself: w = 80, k = 16, reduced twice by 3 through the oracle

    python tests/golden/make_golden_shmr_aln.py [path/to/reference/src]
"""
import ctypes as C
import hashlib
import json
import os
import platform
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_util as U  # noqa: E402
import shmr_aln_util as A  # noqa: E402

SRC = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src"
SOURCES = ("shmr_align.c", "shmr_utils.c", "kalloc.c")
HEADERS = ("shimmer.h", "kvec.h", "khash.h", "kalloc.h")
CFLAGS = ["-O2", "-w", "-fPIC", "-shared"]
SEED = 20261021


class KVec(C.Structure):   # kvec_t(T): {size_t n, m; T *a}
    _fields_ = [("n", C.c_size_t), ("m", C.c_size_t), ("a", C.c_void_p)]


class ShmrAln(C.Structure):   # shmr_aln_t: two kvecs of mm_idx_t (uint32)
    _fields_ = [("idx0", KVec), ("idx1", KVec)]


def compile_reference(tmp):
    so = os.path.join(tmp, "libshmr_aln_ref.so")
    subprocess.check_call(["gcc", *CFLAGS, "-I", SRC, *[os.path.join(SRC, s) for s in SOURCES], "-o", so])
    lib = C.CDLL(so)
    lib.shmr_aln.restype = C.POINTER(KVec)
    lib.shmr_aln.argtypes = [C.POINTER(KVec), C.POINTER(KVec), C.c_uint8, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.free_shmr_alns.argtypes = [C.POINTER(KVec)]
    return lib


def ref_shmr_aln(lib, mm0, mm1, max_diff=100, max_dist=1200, max_repeat=1):
    """the reference's chains as [(idx0 list, idx1 list)]"""
    mm0, mm1 = np.ascontiguousarray(mm0, A.MM_DTYPE), np.ascontiguousarray(mm1, A.MM_DTYPE)
    v0, v1 = KVec(len(mm0), len(mm0), mm0.ctypes.data), KVec(len(mm1), len(mm1), mm1.ctypes.data)
    alns = lib.shmr_aln(C.byref(v0), C.byref(v1), 0, max_diff, max_dist, max_repeat)
    try:
        v = alns.contents
        arr = C.cast(v.a, C.POINTER(ShmrAln))
        take = lambda kv: np.ctypeslib.as_array(C.cast(kv.a, C.POINTER(C.c_uint32)), (kv.n,)).tolist() if kv.n else []
        return [(take(arr[i].idx0), take(arr[i].idx1)) for i in range(v.n)]
    finally:
        lib.free_shmr_alns(alns)


def directed_cases():
    """[(name, mm0, mm1, params)]"""
    mk = A.mm_list
    cases = []
    add = lambda name, mm0, mm1, **kw: cases.append((name, mm0, mm1, dict(dict(max_diff=100, max_dist=1200, max_repeat=1), **kw)))
    some = mk([1, 2, 3], [100, 200, 300])
    add("empty_0", mk([], []), some); add("empty_1", some, mk([], [])); add("empty_both", mk([], []), mk([], []))
    add("no_shared", some, mk([4, 5, 6], [100, 200, 300]))
    add("one_shared", mk([9, 1, 8], [50, 100, 150]), mk([7, 1], [10, 50]))
    add("one_shared_opposite", mk([9, 1, 8], [50, 100, 150], [0, 1, 0]), mk([7, 1], [10, 50]))
    for mr in (1, 3):
        # hash 5 exactly max_repeat times, hash 6 once more, between other shimmers; list 1 asks for both, twice each
        h0 = [1] + [5] * mr + [2] + [6] * (mr + 1) + [3]
        mm0 = mk(h0, 100 + 40 * np.arange(len(h0)))
        add(f"rep{mr}_at", mm0, mk([5, 4, 5], [90, 400, 500]), max_repeat=mr)
        add(f"rep{mr}_over", mm0, mk([6, 4, 6], [90, 400, 500]), max_repeat=mr)
    add("twice_in_list1", mk([1], [100]), mk([1, 1], [10, 20]))
    add("before_last", mk([1, 2], [100, 200]), mk([2, 1], [210, 110]))
    add("diff_below", mk([1, 2], [1000, 1500]), mk([1, 2], [1000, 1401]))      # delta 0, then 99
    add("diff_at", mk([1, 2], [1000, 1500]), mk([1, 2], [1000, 1400]))         # delta 0, then 100
    add("dist_below", mk([1, 2], [1000, 2199]), mk([1, 2], [1000, 2199]))      # mm_dist 1,199
    add("dist_at", mk([1, 2], [1000, 2200]), mk([1, 2], [1000, 2200]))         # mm_dist 1,200
    # chain 0 (idx0 1, delta 0), chain 1 (idx0 0 < 1: opened, delta 20), then delta 10 against both
    add("tie_earlier", mk([2, 1, 3], [1010, 1000, 1500]), mk([1, 2, 3], [1000, 990, 1490]))
    add("later_smaller", mk([2, 1, 3], [1010, 1000, 1500]), mk([1, 2, 3], [1000, 990, 1485]))   # delta 15: 15 against chain 0, 5 against chain 1
    for k in (0, 63, 64, 127, 128):
        # chain j of 129 sits at idx0 128 - j (each before the last chain's: all opened), pos0 10000 + j, delta 2 j + 1; the candidate
        # at idx0 129, pos0 10300 has chain k's delta: diff 0 there, 2 |j - k| elsewhere, every chain qualifies
        j = np.arange(129)
        mm0 = mk(np.concatenate([1000 + j[::-1], [5000]]), np.concatenate([10000 + j[::-1], [10300]]))
        mm1 = mk(np.concatenate([1000 + j, [5000]]), np.concatenate([10000 + j - (2 * j + 1), [10300 - (2 * k + 1)]]))
        add(f"best_{k + 1}_of_129", mm0, mm1, max_diff=1000)
    P = 2**31 - 1
    add("near_2_31", mk([1, 2, 3, 4], [P - 600, P - 300, P, P]), mk([1, 2, 3, 4, 9], [0, 290, P, P - 50, P]))
    n = 4810
    h, pos = np.arange(n) + 10, 1300 * np.arange(n)
    add("stop_4810", mk(h, pos), mk(h, pos))
    g = np.arange(20)
    h3 = np.concatenate([h, 100000 + g, 200000 + g])          # 20 chains grow to 3 elements: +10 and +20 behind their first
    p3 = np.concatenate([pos, pos[:20] + 10, pos[:20] + 20])
    o = np.argsort(p3, kind="stable")
    add("no_stop_4810", mk(h3[o], p3[o]), mk(h3[o], p3[o]))
    return cases


def random_cases(rng):
    cases = []
    for k in range(12):
        mr = (1, 2, 5)[k % 3]
        alpha = (12, 30, 60, 200)[k // 3]
        n0, n1 = int(rng.integers(10, 80)), int(rng.integers(20, 200))
        one = lambda n: A.mm_list(rng.integers(0, alpha, n), np.cumsum(rng.integers(0, 120, n)), rng.integers(0, 2, n) if k % 2 else 0, span=rng.integers(10, 60, n))
        cases.append((f"rand_{k:02d}_a{alpha}_r{mr}", one(n0), one(n1), dict(max_diff=100, max_dist=1200, max_repeat=mr)))
    return cases


def real_cases():
    T, Cp, Rc = A.real_sequences()
    R = A.REAL
    sk = lambda seq, rid: U.orc_reduce(U.orc_reduce(U.orc_sketch_ascii(seq, R["w"], R["k"], rid), R["r"]), R["r"])
    t, c, r = sk(T, 0), sk(Cp, 2), sk(Rc, 3)
    p = dict(max_diff=100, max_dist=1200, max_repeat=1)
    return [("real_fwd", t, c, p), ("real_rc", t, r, p), ("real_self", t, t, p)]


def main():
    rng = np.random.default_rng(SEED)
    cases = directed_cases() + random_cases(rng) + real_cases()
    lists, list_index = [], {}

    def list_id(mm):
        key = mm.tobytes()
        if key not in list_index:
            list_index[key] = len(lists)
            lists.append(mm)
        return list_index[key]

    summary, case_lists, params, case_chain_off, lens, i0s, i1s = {}, [], [], [0], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        lib = compile_reference(tmp)
        for name, mm0, mm1, p in cases:
            ref = ref_shmr_aln(lib, mm0, mm1, **p)
            mine, (walked, stopped) = A.shmr_aln(mm0, mm1, **p)
            assert mine == ref, name
            case_lists.append((list_id(mm0), list_id(mm1)))
            params.append((p["max_diff"], p["max_dist"], p["max_repeat"]))
            for a, b in ref:
                lens.append(len(a)); i0s += a; i1s += b
            case_chain_off.append(len(lens))
            summary[name] = dict(n0=len(mm0), n1=len(mm1), chains=len(ref), elements=sum(len(a) for a, _ in ref), longest=max([len(a) for a, _ in ref], default=0),
                                 walked=walked, stopped=stopped)
            print(name, summary[name], flush=True)
    s = summary
    # what the cases are there for
    assert all(s[n]["chains"] == 0 for n in ("empty_0", "empty_1", "empty_both", "no_shared", "one_shared_opposite", "rep1_over", "rep3_over"))
    assert s["one_shared"]["elements"] == 1 and s["rep1_at"]["elements"] == 2 and s["rep3_at"]["elements"] == 6
    assert (s["twice_in_list1"]["chains"], s["twice_in_list1"]["elements"]) == (1, 2) and s["before_last"]["chains"] == 2
    assert [s[n]["chains"] for n in ("diff_below", "diff_at", "dist_below", "dist_at")] == [1, 2, 1, 2]
    assert s["tie_earlier"]["chains"] == 2 and s["later_smaller"]["chains"] == 2
    assert all(s[f"best_{k}_of_129"]["chains"] == 129 and s[f"best_{k}_of_129"]["longest"] == 2 for k in (1, 64, 65, 128, 129))
    assert s["stop_4810"]["stopped"] and s["stop_4810"]["walked"] == 4802 and s["stop_4810"]["chains"] == 4802
    assert not s["no_stop_4810"]["stopped"] and s["no_stop_4810"]["chains"] == 4810 and s["no_stop_4810"]["elements"] == 4850
    assert s["real_fwd"]["longest"] >= 20 and s["real_self"]["longest"] >= 20 and s["real_rc"]["longest"] <= 2
    mm = np.concatenate(lists)
    np.savez_compressed(A.GOLDEN, names=np.array([c[0] for c in cases]), mm=np.stack([mm["x"], mm["y"]], axis=1),
                        list_off=np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64), case_lists=np.array(case_lists, np.int64),
                        case_params=np.array(params, np.int64), case_chain_off=np.array(case_chain_off, np.int64),
                        chain_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), idx0=np.array(i0s, np.uint32), idx1=np.array(i1s, np.uint32))
    prov = dict(generator="tests/golden/make_golden_shmr_aln.py", seed=SEED, real=A.REAL, direction=0,
                sources={f: hashlib.sha256(open(os.path.join(SRC, f), "rb").read()).hexdigest() for f in SOURCES + HEADERS},
                compiler=subprocess.check_output(["gcc", "--version"], text=True).splitlines()[0], cflags=CFLAGS, glibc=" ".join(platform.libc_ver()),
                cases=[c[0] for c in cases], summary=summary, sha256=hashlib.sha256(open(A.GOLDEN, "rb").read()).hexdigest())
    with open(A.PROVENANCE, "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    print(f"wrote {A.GOLDEN}: {os.path.getsize(A.GOLDEN)} bytes, {len(cases)} cases, {len(lists)} lists")


if __name__ == "__main__":
    main()
