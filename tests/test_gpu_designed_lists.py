"""The overlap stage on DESIGNED shimmer lists (tests/designed_lists_util.py): the candidate join (pgx_pairs.hip) and the replay of
the inner khash tables (pgx_visit.hip: k_inner_lane, k_inner_wave, k_outer_counts, k_outer_place) on lists that place what simulated
reads hold only by chance -- first-key groups of every size around the lane / wavefront boundary (48 | 49), the wavefront limit
(3,153 | 3,154) and every khash resize boundary, each with and without a put of a present key after the group's last new key;
groups made of reversed records only; real-shaped keys that share one home slot (probe chains beyond 64 positions), 56-bit hashes
with hash 0 and bit 63 of the key, mixed spans; and one small design per rule of build_map's loop (strict start, inclusive keep,
the gap of 100, the anchor's advance, split count rows, read boundaries, chunk ownership, bucket sizes, position ties).
What a design contains is asserted by the model when the design is built (also on the CPU: tests/test_designed_lists_rule.py);
here the full record sequence and the counters equal the oracle's under the three ways the stage can run."""
import pytest

import designed_lists_util as D
from peregrine_amd import formats
from peregrine_amd.shimmer import ResidentDB

pytestmark = pytest.mark.gpu

DISPATCHES = {"device visit": dict(PGX_GPU_REPLAY="1", PGX_EARLY_OUTER_MIN="1", PGX_DEV_VISIT="1"),
              "host visit, device walk": dict(PGX_GPU_REPLAY="1", PGX_EARLY_OUTER_MIN="1", PGX_DEV_VISIT="0"),
              "host walk": dict(PGX_GPU_REPLAY="0")}
KNOBS = ("PGX_GPU_REPLAY", "PGX_EARLY_OUTER_MIN", "PGX_DEV_VISIT", "PGX_VISIT_WAVE_MAX", "PGX_REPLAY_BIG", "PGX_REPLAY_DUP")


def _run(monkeypatch, rdb, b, kw, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return rdb.overlap(b.mm, b.mc, **kw)


@pytest.mark.parametrize("name", list(D.DESIGNS))
def test_designed_lists_equal_the_oracle(name, monkeypatch):
    b = D.built(name)
    rdb = ResidentDB(b.db, 0)
    try:
        for i, kw in enumerate(b.runs):
            want, ost = D.oracle_of(name, i)
            m = b.model(kw)
            assert (m.n_records, m.n_buckets(kw.get("ovlp_upper", 120))) == (ost["n_records"], ost["n_buckets"])
            runs = list(DISPATCHES.items()) + ([("device visit + " + str(b.env), {**DISPATCHES["device visit"], **b.env})] if b.env else [])
            for how, env in runs:
                got, st = _run(monkeypatch, rdb, b, kw, env)
                ctx = (name, kw, how, st, ost)
                assert len(got) == len(want) and formats.ovlp_fields_equal(got, want), ctx
                assert (st["n_align_needed"], st["n_seen_skip"], st["n_pair_records"], st["n_buckets"]) == \
                    (ost["n_align"], ost["n_seen_skip"], ost["n_records"], ost["n_buckets"]), ctx
                if how.startswith("device visit"):
                    on_device = m.n_records > 0 and m.max_group() <= D.VISIT_WAVE_MAX
                    assert b.wave_overflow == (m.max_group() > D.VISIT_WAVE_MAX)
                    assert st["device_visit"] == (1 + m.n_big() if on_device else 0), ctx
                    if m.n_buckets(kw.get("ovlp_upper", 120)):
                        assert st["device_replay"] == 1, ctx
                else:
                    assert st["device_visit"] == 0, ctx
    finally:
        rdb.close()
