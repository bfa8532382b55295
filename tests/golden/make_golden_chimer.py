"""Generator of tests/golden/chimer_cases.npz and chimer_cases_sim.npz (the `sim` case's arrays, to keep either file small): record sets
built with tests/dedup_graph_util, the REAL reference shmr_dedup's text of each (oracle/_ref/shmr_dedup, built by `make -C oracle ref`),
and what the reference's own generate_string_graph (py/scripts/ovlp_to_graph.py, imported in place from the reference tree, nothing of it
copied) writes for that text with disable_chimer_bridge_removal=False and lfc=False: sg_edges_list and chimers_nodes.

The chimer bridge step pops from a set of node objects (bfs_nodes), so the script's result can change from run to run.  In the child
process the name `set` in the imported module is bound to a subclass of set whose pop() follows a policy:
  smallest   the element with the smallest (int(rid), end) -- THE PIN: its sg_edges_list bytes and sorted chimers_nodes lines are the fixture
  largest, random1, random2, builtin (the name is left alone)   -- run as well; the provenance records per case whether all five
             policies gave the pin's answer (`unanimous`)
Every policy runs under PYTHONHASHSEED 1 and 4242; the pin must give the same bytes under both, or the fixture is not written.
The flag-off file of the same records (disable_chimer_bridge_removal=True) is stored too (<name>_off).  networkx 3.4.2.

    python tests/golden/make_golden_chimer.py [path/to/reference/py/scripts]

Cases (read ids below 2^31; the generator asserts what each is there for).  A chain is reads with next and next-but-one overlaps:
  bridge               two chains of 8 and a read X with dv(A3, X), dv(X, B5): G 28 / TR 24 / C 4, both ends of X chosen
  bridge_tr            A3 -> X is reduced through A4 -> X: it stays TR, A4 -> X becomes C
  no_bridge_shared     A3 also points at B5, X's successor: test 1 fails, no C
  rejoin_near          X from A2 to A6 of one chain: the flows meet within reach, no end of X is chosen
  rejoin_tr_only       the flows at X:E meet only through A8 -> B6, which the reduction marked TR: flows use edges in any state
  cand_needs_unreduced X:E would be a candidate only if the TR edge A3 -> X counted: no C
  pool_choice          chains of 12 and the far cross-link A10 -> B6: both ends of X under `smallest`, one under `largest`
  leaf_start           a member of T without out-edges starts a flow
  depth                a chain of next overlaps only: X's successor is the 5th node after the start and would need a 5th pop
  sim                  chimer_util.chimeric_sim: simulated records plus chimeric reads
  none / single        as in make_golden_sgraph.py
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
import chimer_util as CU  # noqa: E402
import dedup_graph_util as DG  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "shmr_dedup")
SCRIPTS = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "--child" else "/root/reference/py/scripts"
POLICIES = ("smallest", "largest", "random1", "random2", "builtin")
SEEDS = ("1", "4242")
MIN_LEN, MIN_IDT = 4000, 96.0
rec = DG.rec


def policy_set(policy):
    import random
    rng = random.Random({"random1": 1, "random2": 2}.get(policy, 0))

    def key(node):
        rid, end = node.name.split(":")
        return int(rid), end

    class PolicySet(set):
        def pop(self):
            order = sorted(self, key=key)
            x = order[0] if policy == "smallest" else order[-1] if policy == "largest" else order[rng.randrange(len(order))]
            self.remove(x)
            return x

        def __or__(self, other):
            return PolicySet(set.__or__(self, other))

        def __and__(self, other):
            return PolicySet(set.__and__(self, other))
    return PolicySet


def child(scripts, text_path, min_len, min_idt, policy, out_path):
    """one run of the reference's function in this process (whose hash seed the parent chose); policy `off`: the flag-off file"""
    sys.path.insert(0, scripts)
    import ovlp_to_graph
    if policy not in ("builtin", "off"):
        ovlp_to_graph.set = policy_set(policy)
    past1 = set()
    bfs = ovlp_to_graph.StringGraph.bfs_nodes

    def counted(self, n, exclude=None, depth=5):
        past1.add(exclude.name)
        return bfs(self, n, exclude=exclude, depth=depth)
    ovlp_to_graph.StringGraph.bfs_nodes = counted
    text = open(text_path, "rb").read()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        with open("preads.ovl", "wb") as f:
            f.write(text + b"-\n")
        ovlp_to_graph.generate_string_graph(types.SimpleNamespace(overlap_file="preads.ovl", min_len=int(min_len), min_idt=float(min_idt), lfc=False,
                                                                  disable_chimer_bridge_removal=policy == "off"))
        sg = open("sg_edges_list", "rb").read()
        nodes = b"" if policy == "off" else b"".join(sorted(open("chimers_nodes", "rb").read().splitlines(True)))
        os.chdir("/")
    with open(out_path, "wb") as f:
        f.write(sg)
    with open(out_path + ".nodes", "wb") as f:
        f.write(nodes)
    with open(out_path + ".json", "w") as f:
        json.dump(dict(past_test1=len(past1)), f)


def run_policies(text: bytes, min_len, min_idt):
    """{policy: (sg_edges_list, sorted chimers_nodes, past_test1)}, `off` included; every policy under both hash seeds"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tp = os.path.join(tmp, "text")
        with open(tp, "wb") as f:
            f.write(text)
        for policy in POLICIES + ("off",):
            got = []
            for seed in SEEDS:
                op = os.path.join(tmp, "sg.%s.%s" % (policy, seed))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", SCRIPTS, tp, str(min_len), str(min_idt), policy, op], check=True,
                               env=dict(os.environ, PYTHONHASHSEED=seed))
                got.append((open(op, "rb").read(), open(op + ".nodes", "rb").read(), json.load(open(op + ".json"))["past_test1"]))
            if policy in ("smallest", "off") and got[0] != got[1]:
                sys.exit("policy %s: two hash seeds give two answers: the fixture is NOT written" % policy)
            out[policy] = got
    return out


def ref_text(recs) -> bytes:
    if len(recs) == 0:
        return b""
    return subprocess.run([REF], input=np.ascontiguousarray(recs).tobytes(), stdout=subprocess.PIPE, check=True).stdout


def dv(f, g, oh_f, oh_g=None, rl=9000, **kw):
    """f to the left of g on the same strand: the edges g:B -> f:B of length oh_f and f:E -> g:E of length oh_g"""
    oh_g = oh_f if oh_g is None else oh_g
    args = dict(q_bgn=oh_f, q_end=rl, t_end=rl - oh_g, rl0=rl, rl1=rl)
    args.update(kw)
    return rec(f, g, **args)


def chain(first, n, skip=True):
    """reads first + 1 .. first + n: next overlaps (1000) and, with skip, next-but-one (2000)"""
    r = [dv(first + i, first + i + 1, 1000) for i in range(1, n)]
    if skip:
        r += [dv(first + i, first + i + 2, 2000) for i in range(1, n - 1)]
    return r


def nm(rid, end):
    return b"%09d:%s" % (rid, end)


def type_of(sg, v, w):
    for ln in sg.split(b"\n")[:-1]:
        f = ln.split()
        if f[0] == v and f[1] == w:
            return f[7]
    raise KeyError((v, w))


def types_of(sg):
    t = [ln.split()[-1].decode() for ln in sg.split(b"\n")[:-1]]
    return {k: t.count(k) for k in ("G", "TR", "S", "R", "C")}


A, B, X, W = 100, 200, 300, 400     # chain A is reads 101 .., chain B reads 201 .., the chimeric read, a leaf


def directed_cases():
    """name -> (records, check(pin sg, pin nodes, all results)) -- check asserts what the case is there for"""
    two = chain(A, 8) + chain(B, 8)
    both_ends = b"".join(sorted([nm(X, b"B") + b"\n", nm(X, b"E") + b"\n"] * 2))
    one_end = nm(X, b"B") + b"\n" + nm(X, b"E") + b"\n"
    cases = {}

    def bridge(sg, nodes, res):
        assert types_of(sg) == dict(G=28, TR=24, S=0, R=0, C=4) and nodes == both_ends, (types_of(sg), nodes)
        assert types_of(res["off"][0][0]) == dict(G=32, TR=24, S=0, R=0, C=0)
    cases["bridge"] = (two + [dv(A + 3, X, 1500), dv(X, B + 5, 1500)], bridge)

    def bridge_tr(sg, nodes, res):
        assert type_of(sg, nm(A + 3, b"E"), nm(X, b"E")) == b"TR" and type_of(sg, nm(X, b"B"), nm(A + 3, b"B")) == b"TR"
        assert type_of(sg, nm(A + 4, b"E"), nm(X, b"E")) == b"C" and types_of(sg)["C"] == 4 and nodes == both_ends
    cases["bridge_tr"] = (two + [dv(A + 3, X, 1500), dv(A + 4, X, 500), dv(X, B + 5, 1500)], bridge_tr)

    def no_bridge_shared(sg, nodes, res):
        assert types_of(sg)["C"] == 0 and nodes == b"" and sg == res["off"][0][0] and res["smallest"][0][2] == 0
    cases["no_bridge_shared"] = (two + [dv(A + 3, X, 1500), dv(X, B + 5, 1500), dv(A + 3, B + 5, 2800)], no_bridge_shared)

    def rejoin_near(sg, nodes, res):
        assert types_of(sg)["C"] == 0 and nodes == b"" and res["smallest"][0][2] == 2      # both ends pass test 1, neither passes test 2
    cases["rejoin_near"] = (chain(A, 8) + [dv(A + 2, X, 1500), dv(X, A + 6, 1500)], rejoin_near)

    long_two = chain(A, 12) + chain(B, 12)
    tr_only = long_two + [dv(A + 3, X, 1500), dv(X, B + 5, 1500), dv(A + 8, B + 6, 2600), dv(A + 9, B + 6, 1200), dv(A + 1, B + 3, 1500)]

    def rejoin_tr_only(sg, nodes, res):
        assert type_of(sg, nm(A + 8, b"E"), nm(B + 6, b"E")) == b"TR"
        assert types_of(sg)["C"] == 0 and nodes == b"" and res["smallest"][0][2] == 2
    cases["rejoin_tr_only"] = (tr_only, rejoin_tr_only)

    def cand_needs_unreduced(sg, nodes, res):
        assert type_of(sg, nm(A + 3, b"E"), nm(X, b"E")) == b"TR" and types_of(sg)["C"] == 0 and nodes == b"" and res["smallest"][0][2] == 0
    cases["cand_needs_unreduced"] = (chain(A, 4) + chain(B, 8) + [dv(A + 3, X, 1500), dv(A + 4, X, 500), dv(A + 3, W, 1200), dv(X, B + 5, 1500)], cand_needs_unreduced)

    def pool_choice(sg, nodes, res):
        assert nodes == both_ends and res["largest"][0][1] == one_end, (nodes, res["largest"][0][1])
    cases["pool_choice"] = (long_two + [dv(A + 3, X, 1500), dv(X, B + 5, 1500), dv(A + 10, B + 6, 1500)], pool_choice)

    def leaf_start(sg, nodes, res):
        assert types_of(sg)["C"] == 4 and nodes == both_ends
        assert not any(ln.split()[0] == nm(W, b"E") for ln in sg.split(b"\n")[:-1])      # W:E has no out-edges
    cases["leaf_start"] = (two + [dv(A + 3, X, 1500), dv(X, B + 5, 1500), dv(A + 3, W, 1200)], leaf_start)

    def depth(sg, nodes, res):
        assert types_of(sg)["C"] == 4 and nodes == both_ends
    cases["depth"] = (chain(A, 12, skip=False) + [dv(A + 2, X, 1500), dv(X, A + 8, 1500)], depth)
    return cases


SIM = dict(seed=21, n_reads=360, genome=120_000, n_chimers=100)
SIM_MIN_LEN = 2000


def out_degrees(sg):
    deg = {}
    for ln in sg.split(b"\n")[:-1]:
        v = ln.split()[0]
        deg[v] = deg.get(v, 0) + 1
    return deg


def main():
    import networkx
    sys.path.insert(0, SCRIPTS)
    import ovlp_to_graph
    arrays, cases, summary = {}, {}, {}

    def case(name, recs, check, min_len=MIN_LEN, min_idt=MIN_IDT):
        recs = np.concatenate(recs) if isinstance(recs, list) else recs
        assert int((recs["y0"] >> np.uint64(32)).max()) < 2**31 and int((recs["y1"] >> np.uint64(32)).max()) < 2**31
        text = ref_text(recs)
        res = run_policies(text, min_len, min_idt)
        sg, nodes, past1 = res["smallest"][0]
        unanimous = all(r[:2] == (sg, nodes) for p in POLICIES for r in res[p])
        check(sg, nodes, res)
        arrays[name + "_recs"] = np.ascontiguousarray(recs.view(np.uint8).reshape(len(recs), -1).T)   # byte columns: they compress far better
        arrays[name + "_sg"] = np.frombuffer(sg, np.uint8)
        arrays[name + "_nodes"] = np.frombuffer(nodes, np.uint8)
        arrays[name + "_off"] = np.frombuffer(res["off"][0][0], np.uint8)
        cases[name] = dict(min_len=min_len, min_idt=min_idt)
        summary[name] = dict(records=len(recs), lines=text.count(b"\n"), edges=sg.count(b"\n"), **types_of(sg), chosen=nodes.count(b"\n") // 2, past_test1=past1,
                             unanimous=unanimous, max_out_degree=max(out_degrees(sg).values(), default=0), sha256=hashlib.sha256(sg).hexdigest(),
                             nodes_sha256=hashlib.sha256(nodes).hexdigest(), off_sha256=hashlib.sha256(res["off"][0][0]).hexdigest())
        print(name, json.dumps(summary[name]), flush=True)
        return sg, nodes, res

    for name, (recs, check) in directed_cases().items():
        case(name, recs, check)
    assert summary["pool_choice"]["unanimous"] is False
    assert all(summary[k]["unanimous"] for k in ("bridge", "bridge_tr", "no_bridge_shared", "leaf_start"))

    def sim(sg, nodes, res):
        s = types_of(sg)
        off = res["off"][0][0]
        other = [a for a, b in zip(sg.split(b"\n"), off.split(b"\n")) if a != b and not a.endswith(b" C")]
        assert nodes.count(b"\n") // 2 >= 20 and res["smallest"][0][2] > nodes.count(b"\n") // 2 and other and max(out_degrees(sg).values()) > 64, \
            (nodes.count(b"\n") // 2, res["smallest"][0][2], len(other), max(out_degrees(sg).values()), s)
    case("sim", CU.chimeric_sim(**SIM), sim, min_len=SIM_MIN_LEN)
    case("none", [dv(1, 2, 1000, dist=400), dv(2, 3, 1000, rl=3000), dv(3, 4, 1000, 0)], lambda sg, nodes, res: (sg, nodes) == (b"", b"") or sys.exit("none"))
    case("single", [dv(1, 2, 1000, dist=400), dv(5, 6, 1500), dv(2, 3, 1000, rl=3000)], lambda sg, nodes, res: sg.count(b"\n") == 2 or sys.exit("single"))

    prov = dict(generator="tests/golden/make_golden_chimer.py", reference="oracle/_ref/shmr_dedup",
                reference_sha256=hashlib.sha256(open(REF, "rb").read()).hexdigest(), reference_script="py/scripts/ovlp_to_graph.py",
                reference_script_sha256=hashlib.sha256(open(ovlp_to_graph.__file__, "rb").read()).hexdigest(), networkx=networkx.__version__,
                disable_chimer_bridge_removal=False, lfc=False, hash_seeds=[int(s) for s in SEEDS], pinned_policy="smallest", policies=list(POLICIES),
                sim=dict(SIM), cases=cases, summary=summary)
    second = {k: arrays.pop(k) for k in list(arrays) if k.startswith("sim_")}
    np.savez_compressed(os.path.join(HERE, "chimer_cases.npz"), cases=np.array(json.dumps(cases)), **arrays)
    np.savez_compressed(os.path.join(HERE, "chimer_cases_sim.npz"), **second)
    with open(os.path.join(HERE, "chimer_cases.provenance.json"), "w") as f:
        json.dump(prov, f, indent=1)
        f.write("\n")
    for name in ("chimer_cases.npz", "chimer_cases_sim.npz"):
        assert os.path.getsize(os.path.join(HERE, name)) < 1_000_000, (name, os.path.getsize(os.path.join(HERE, name)))
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:8])
    else:
        main()
