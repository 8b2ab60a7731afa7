"""Preconditions of tests/test_gpu_async_order.py, decided on the CPU (no GPU): every case of tests/async_order.py builds a
truth and a decoy of one shape whose every mixture is a valid input, the two give different reference results (a decoy with
the truth's answer proves nothing), and the table covers every device-work entry of include/segvlad.h."""
import numpy as np
import pytest

import async_order as A


def test_names_are_unique_and_every_group_has_cases():
    names = [c.name for c in A.CASES]
    assert len(set(names)) == len(names)
    assert {c.group for c in A.CASES} == set(A.GROUPS)
    for c in A.CASES:
        assert c.fixture in A.FIXTURES and set(c.host) | set(c.fixed) | set(c.convert) <= set(c.build("truth")), c.name
        assert not set(c.convert) & set(c.host), c.name
        for _, release in c.steps:
            assert release is None or set(release) <= set(c.build("truth")), c.name
    # both storages of the masks and of the query rows are in the table
    assert any(c.convert.get("masks") == "bool" for c in A.CASES) and any(c.convert.get("masks") == "strided" for c in A.CASES)
    assert all(c.convert.get("Q") == "strided" for c in A.CASES if c.entries != ("search",) and "Q" in c.build("truth"))


def test_every_entry_of_the_header_is_covered_or_excluded_by_group():
    entries = set(A.header_entries())
    assert len(entries) > 50
    excluded = [e for group in A.EXCLUDED.values() for e in group]
    assert set(A.EXCLUDED) == {"lifetime", "option", "stats", "profiling", "comm"}
    assert len(excluded) == len(set(excluded)) and set(excluded) <= entries, sorted(set(excluded) - entries)
    covered = A.covered_entries()
    assert covered <= entries, sorted(covered - entries)
    assert not covered & set(excluded), sorted(covered & set(excluded))
    assert covered | set(excluded) == entries, sorted(entries - covered - set(excluded))


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_case_qualifies(name):
    c = A.BY_NAME[name]
    A.same_shapes(c)
    n = 0
    for mix in A.mixtures(c):
        c.valid(mix)
        n += 1
    assert n == 2 ** len(c.build("truth"))
    rt, rd = c.ref(c.build("truth")), c.ref(c.build("decoy"))
    assert sorted(rt) == sorted(rd) and rt
    differs = [k for k in rt if np.shape(rt[k]) != np.shape(rd[k]) or not np.array_equal(np.asarray(rt[k]), np.asarray(rd[k]))]
    assert differs, "truth and decoy give the same reference result"
    # every array output whose content follows the inputs differs (scalars, all-zero flag words and constants apart)
    print(f"{name}: reference outputs that tell truth from decoy: {differs} of {sorted(rt)}")
    if c.group == "search" and "d2" in rt and "idx" in rt:
        assert "idx" in differs and "d2" in differs
    if name == "search_rigorous_redo":
        idx = A.knn_ref(A.N40, A.D, 160, "truth", 30, True)[1][10:]                  # the truth's bands ARE the duplicate block
        assert (idx >= A.DUP0).all() and (idx < A.DUP0 + A.N_DUP).all()
    if name == "range_search":
        assert rt["lims"][-1] > len(rt["lims"]) - 1 and (np.diff(rt["lims"]) >= 1).all()


def test_rle_runs_agree_between_truth_and_decoy_and_hold_odd_lengths():
    (ct, ot), (cd, od) = A.rle_of("truth"), A.rle_of("decoy")
    assert np.array_equal(ot, od) and np.array_equal(np.diff(ot), 2 * A.WIDTHS + 1) and not np.array_equal(ct, cd)
    assert len(ct) == int((2 * A.WIDTHS + 1).sum())


def test_group_sequences_hold_every_case_once():
    for g in A.GROUPS:
        items = A.group_items(g)
        assert [n for n, _ in items] == [c.name for c in A.CASES if c.group == g]
        assert {v for _, v in items} == {"plain", "convert"}
