"""The designs of tests/test_gpu_designed_lists.py on the CPU: building a design asserts its preconditions from the model
(designed_lists_util.build_map_model, a restatement of build_map's loop), and on every run of every design the model's record
count and visited-bucket count equal the oracle's."""
import pytest

import designed_lists_util as D


@pytest.mark.parametrize("name", list(D.DESIGNS))
def test_model_counts_equal_the_oracle(name):
    b = D.built(name)
    assert b.runs
    for i, kw in enumerate(b.runs):
        m = b.model(kw)
        _, st = D.oracle_of(name, i)
        assert (m.n_records, m.n_buckets(kw.get("ovlp_upper", 120))) == (st["n_records"], st["n_buckets"]), (name, kw)
