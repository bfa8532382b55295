"""The map merge's rule pinned on the CPU (tests/mapmerge_util.py): its two forms -- field 0 and field 1 as numbers then the whole line
bytewise, and the per-field numeric key the kernels compare -- agree with each other and, where GNU sort is installed, with
`LC_ALL=C sort -k 1 -g -k 2 -g` itself, on seeded lines dense in ties and digit-length boundaries and on the fixture the real shmr_map and
GNU sort wrote (tests/golden/mapmerge_cases.npz)."""
import numpy as np
import pytest

import mapmerge_util as M


def _cases():
    rng = np.random.default_rng(20261101)
    yield "boundaries", M.boundary_lines(rng, 4000)
    yield "runs", M.run_lines(rng, [1, 2, 63, 64, 65, 127, 128, 129, 300])
    yield "runs_wide", M.run_lines(rng, [5, 70, 200], wide=True)
    yield "field8", M.run_lines(rng, [40, 90], differ=(8,))
    yield "field2", M.run_lines(rng, [40, 90], differ=(2,))
    yield "mapped", M.mapped_lines(rng, 6000)
    yield "identical", ["3 14 15 9 2 6 1 5 3"] * 50
    maps, _ = M.load_fixture()
    yield "fixture", b"".join(maps).decode().splitlines()


CASES = dict(_cases())


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_forms_of_the_rule_agree(name):
    lines = CASES[name]
    assert M.rule_sorted(lines) == M.numeric_sorted(lines)
    assert M.lines_of(M.rows_of(lines)) == lines


def test_text_order_and_numeric_order_part_ways_behind_the_second_field():
    assert M.rule_sorted(["1 2 99 0 0 0 0 0 0", "1 2 100 0 0 0 0 0 0"]) == ["1 2 100 0 0 0 0 0 0", "1 2 99 0 0 0 0 0 0"]
    assert M.rule_sorted(["1 2 70 0 0 0 0 0 0", "1 2 7 0 0 0 0 0 0"]) == ["1 2 7 0 0 0 0 0 0", "1 2 70 0 0 0 0 0 0"]
    assert M.rule_sorted(["1 100 5 0 0 0 0 0 0", "1 99 5 0 0 0 0 0 0"]) == ["1 99 5 0 0 0 0 0 0", "1 100 5 0 0 0 0 0 0"]
    assert M.rule_sorted(["100 1 5 0 0 0 0 0 0", "99 1 5 0 0 0 0 0 0"]) == ["99 1 5 0 0 0 0 0 0", "100 1 5 0 0 0 0 0 0"]
    assert all(k < (1 << 34) and nd <= 10 for k, nd in (M.field_key(v) for v in M.BOUNDARY))   # 34 + 4 bits


@pytest.mark.parametrize("name", list(CASES))
def test_the_rule_is_gnu_sorts(name):
    got = M.gnu_sort(CASES[name])
    if got is None:
        pytest.skip("no sort on PATH")
    assert got == M.rule_sorted(CASES[name])


def test_the_fixture_holds_gnu_sorts_own_merge():
    maps, merged = M.load_fixture()
    lines = b"".join(maps).decode().splitlines()
    assert len(lines) > 500 and all(m.endswith(b"\n") for m in maps)
    assert M.text_of(M.rule_sorted(lines)) == merged
