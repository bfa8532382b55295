"""The stated rule of the homopolymer-compressed sketch (tools/hpc_sketch_model.py: the machine's loop and the restatement the kernels
implement) reproduces every case of the fixture recorded from the compiled reference -- no GPU needed."""
import os
import sys

import numpy as np

import hpc_util as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import hpc_sketch_model as M   # noqa: E402


def test_the_fixture_holds_the_directed_and_the_random_cases():
    cases = H.golden_cases()
    want = H.all_cases()
    assert [(c.name, c.seq, c.w, c.k) for c in cases] == want and len(H.directed_cases()) >= 60 and len(cases) >= 260
    assert sum(len(c.l0) > 0 for c in cases) > 200
    spans = np.concatenate([c.l0["x"] & np.uint64(0xFF) for c in cases])
    assert spans.max() == 255 and (spans > 16).sum() > 1000     # spans are data: up to the last finite one
    assert all((c.l1 is not None) == ((c.w, c.k) == (H.W, H.K)) for c in cases)


def test_the_model_reproduces_every_fixture_case():
    for c in H.golden_cases():
        want = [(int(x), int(y)) for x, y in c.with_rid(c.l0, 5).tolist()]
        assert M.sketch(c.seq, c.w, c.k, 5) == want, c.name
        assert M.machine(c.seq, c.w, c.k, 5) == want, c.name


def test_span_255_is_finite_and_256_is_not():
    """the two directed strings differ by one base of one run: with it every k-mer over the run is infinite (whether a finite one is
    also a minimizer is up to its hash: the first test sees a span of 255 emitted somewhere in the fixture)"""
    by = {c.name: c for c in H.golden_cases()}
    for suffix, k in (("", H.K), ("_k6", 6)):
        a, b = (M.stream(by[n + suffix].seq, k) for n in ("span255", "span256"))
        assert len(a) == len(b)
        spans = [x & 0xFF for x, _, s in a if x != M.INF]
        assert max(spans) == 255 and 0 < spans.count(255) <= k     # the k-mers that hold the long run
        assert sum(x == M.INF and s >= 0 for x, _, s in b) == spans.count(255) and max(x & 0xFF for x, _, s in b if x != M.INF) == k
