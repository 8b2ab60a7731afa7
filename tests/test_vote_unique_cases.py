"""The vote's one-to-one flag on the host: the reference of tests/vote_unique_ref.py on literal lists, engine.blank_unique and
_lib.vote_mode against it, the mirror of the launcher's regime rule, and the conditions that make the inputs of
tests/test_gpu_vote_unique.py worth running (the flag must bite, sims must matter, the order of flag and cap must matter, and the
vote must change)."""
import os

import numpy as np
import pytest

import search_tail_ref as R
import vote_cap_ref as V
import vote_unique_ref as U
from revisit_anything_amd import _lib
from revisit_anything_amd.engine import blank_capped, blank_unique

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference on literal lists -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(U.LITERAL))
def test_literal_lists(name):
    c = U.LITERAL[name]
    assert U.blank_unique(c["matches"], c["sims"], c["off"], c["n_ref"]).tolist() == c["with_sims"].tolist()
    assert U.blank_unique(c["matches"], None, c["off"], c["n_ref"]).tolist() == c["without"].tolist()


def test_literal_lists_say_what_they_claim():
    c = U.LITERAL["rank_major_tie"]
    assert c["matches"][0, 1] == c["matches"][1, 0] and c["sims"][0, 1] == c["sims"][1, 0]
    assert c["with_sims"][1, 0] == 5 and c["with_sims"][0, 1] == -1      # (q=1, r=0) beats (q=0, r=1)
    z = U.LITERAL["zeros"]["sims"]
    assert np.signbit(z[0, 0]) and not np.signbit(z[1, 0]) and z[0, 0] == z[1, 0]
    assert np.isnan(U.LITERAL["nan"]["sims"]).sum() == 3 and np.isinf(U.LITERAL["inf"]["sims"]).sum() == 3
    w = U.LITERAL["wide_ids"]["matches"]
    assert (w[1, 1] & 0xFFFFFFFF) == w[1, 0] and w[1, 1] != w[1, 0]       # equal in their low 32 bits only


# ---- engine.blank_unique and _lib.vote_mode -----------------------------------------------------------------------------
def test_blank_unique_equals_reference():
    for name, c in U.LITERAL.items():
        assert np.array_equal(blank_unique(c["matches"], c["sims"], c["off"], c["n_ref"]), c["with_sims"]), name
        assert np.array_equal(blank_unique(c["matches"], None, c["off"], c["n_ref"]), c["without"]), name
    rng = np.random.default_rng(3)
    off = np.array([0, 7, 7, 20, 40], np.int32)
    idx = rng.integers(-3, 60, size=(40, 33)).astype(np.int64)           # ids below 0 and past the map among them
    sims = rng.choice(np.array([-0.0, 0.0, 0.5, 1.0, np.nan, np.inf, -np.inf], np.float32), size=idx.shape)
    for s in (sims, None):
        assert np.array_equal(blank_unique(idx, s, off, 50), U.blank_unique(idx, s, off, 50))
    assert blank_unique(idx[:0], None, np.array([0], np.int32), 50).shape == (0, 33)
    for name in ("fast_last_64x64", "bench_depth_50x200"):
        c = U.case(name, True)
        n = len(c["img_of_seg"])
        assert np.array_equal(blank_unique(c["matches"], c["sims"], c["off"], n), U.blanked(name, True, True, None))
        assert np.array_equal(blank_unique(c["matches"], None, c["off"], n), U.blanked(name, True, False, None))
        assert np.array_equal(blank_capped(blank_unique(c["matches"], c["sims"], c["off"], n), c["img_of_seg"], 1), U.blanked(name, True, True, 1))
    import torch

    assert np.array_equal(blank_unique(torch.from_numpy(idx), torch.from_numpy(sims), off, 50), U.blank_unique(idx, sims, off, 50))
    with pytest.raises(ValueError):
        blank_unique(idx[0], None, off, 50)
    with pytest.raises(ValueError):
        blank_unique(idx, sims[:, :5], off, 50)


def test_vote_mode():
    assert _lib.VOTE_UNIQUE_REF == 0x80
    for base in (_lib.VOTE_WT_BORDA_IM, _lib.VOTE_COUNT):
        assert _lib.vote_mode(base, unique_ref=True) == base | 0x80
        assert _lib.vote_mode(base, None, True) == base | 0x80
        assert _lib.vote_mode(base, 3, True) == base | 0x80 | 0x300
        assert _lib.vote_mode(base | 0x80) == base | 0x80                # an int mode that carries the flag keeps it
        assert _lib.vote_mode(base | 0x80, 2) == base | 0x80 | 0x200
        assert _lib.vote_mode(base | 0x80 | 0x200, 2, True) == base | 0x80 | 0x200
        # as before
        assert _lib.vote_mode(base) == base and _lib.vote_mode(base, 5) == base | 0x500 and _lib.vote_mode(base, 5, False) == base | 0x500
    with pytest.raises(ValueError):
        _lib.vote_mode(0x281, 3, True)


def test_header_states_the_contract():
    hdr = " ".join(open(os.path.join(ROOT, "include", "segvlad.h")).read().replace("*", " ").split())
    assert "#define SEGVLAD_VOTE_UNIQUE_REF 0x80" in hdr
    for words in ("base = mode & 0x7f",
                  "a NaN loses to every number",
                  "the smallest p wins",
                  "every non-winning valid entry's id replaced by -1",
                  "the one-to-one blanking comes first",
                  "at most 4096 entries",
                  "32 bytes per entry"):
        assert words in hdr, words
    assert hdr.count("int segvlad_vote(") == 1 and "segvlad_vote_unique" not in hdr    # a mode bit, not an entry point


# ---- the mirror of the launcher -----------------------------------------------------------------------------------------
def test_regime_mirror():
    assert U.LDS_ENTRIES == 4096 and U.table_size(U.LDS_ENTRIES) * U.SLOT_BYTES == 128 * 1024
    (s0, k0), (s1, k1), (s2, k2) = U.EDGE_SHAPES
    assert s0 * k0 == U.LDS_ENTRIES and s1 * k1 == U.LDS_ENTRIES + 1 and s2 * k2 == 16385
    assert U.launch_regime([3, s0, 2], k0) == ([0, 1, 2], [], 1)
    assert U.launch_regime([3, s1, 2], k1) == ([0, 2], [1], 4)
    assert U.launch_regime([s1], k1) == ([], [0], 3)
    assert U.launch_regime([0, 0], 7) == ([], [], 0)
    assert U.global_scratch_bytes([3, s1, 2, s1, 9], k1) == (2 * s1 + 2) * k1 * 32
    for name in U.SHAPES:
        c = U.case(name, False)
        lds, big, n = U.launch_regime(c["counts"], c["k"])
        assert lds and n == (4 if big else 1)
    assert {bool(U.launch_regime(U.case(n, False)["counts"], U.case(n, False)["k"])[1]) for n in U.SHAPES} == {False, True}


@pytest.mark.parametrize("segs,k", U.EDGE_SHAPES)
def test_stress_cases_stress(segs, k):
    T = U.table_size(segs * k)
    rows = slice(3, 3 + segs)
    c = U.stress_case("one_id", segs, k)
    b = U.blank(c, c["sims"])
    assert len(np.unique(c["matches"][rows])) == 1 and (b[rows] >= 0).sum() == 1
    assert np.argwhere(b[rows] >= 0)[0].tolist() == [segs // 2, k // 2]   # the one entry above all the others
    assert (c["matches"][:3, 0] == c["matches"][3, 0]).all() and (b[:3, 0] >= 0).sum() == 1   # the small image keeps a claim of its own
    c = U.stress_case("table_multiples", segs, k)
    ids = np.unique(c["matches"][rows])
    assert (ids % T == 0).all() and len(ids) >= 10
    c = U.stress_case("wrap_chain", segs, k)
    ids = np.unique(c["matches"][rows])
    assert len(ids) > 3 and all(U.home_slot(i, T) >= T - 3 for i in ids)
    slot_of, wraps = U.probe_chain(c["matches"][rows].T.reshape(-1), T)
    assert wraps >= 1 and min(slot_of.values()) == 0                     # the chain goes on at the table's first slot
    for kind in U.STRESS_KINDS:                                          # equal sims meet on one id: the tie rule decides
        c = U.stress_case(kind, segs, k)
        assert not np.array_equal(U.blank(c, c["sims"]), U.blank(c, None))


# ---- the inputs of the GPU parity test ----------------------------------------------------------------------------------
@pytest.mark.parametrize("invalid", [False, True], ids=["plain", "invalid_ids"])
@pytest.mark.parametrize("name", U.SHAPES)
def test_gpu_inputs_make_the_flag_bite(name, invalid):
    c = U.case(name, invalid)
    im, off = c["img_of_seg"], c["off"]
    with_sims, without = U.blanked(name, invalid, True, None), U.blanked(name, invalid, False, None)
    # at least a quarter of the valid entries of the largest image are duplicate claims
    assert U.largest_image_share(c, with_sims) >= 0.25
    assert U.largest_image_share(c, without) == U.largest_image_share(c, with_sims)     # one winner per id either way
    # sims decide: other winners than the first visited
    assert not np.array_equal(with_sims, without)
    # the one-to-one blanking in front of the cap is not the cap in front of it
    cap_first = U.blank_unique(V.blank(c["matches"], im, 1), c["sims"], off, len(im))
    assert not np.array_equal(U.blanked(name, invalid, True, 1), cap_first)
    # the vote changes in both bases
    top = lambda rows: R.padded(rows, 5)
    plain, flagged = top(R.vote_wt_ranking(c["matches"], c["sims"], off, im)), top(R.vote_wt_ranking(with_sims, c["sims"], off, im))
    assert not (np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1], flagged[1]))
    plain, flagged = top(R.vote_count_ranking(c["matches"], off, im)), top(R.vote_count_ranking(without, off, im))
    assert not (np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1], flagged[1]))
    # invalid entries stay as they are
    valid = (c["matches"] >= 0) & (c["matches"] < len(im))
    assert np.array_equal(with_sims[~valid], c["matches"][~valid])


def test_no_duplicates_case_has_none():
    c = U.no_duplicates_case()
    assert np.array_equal(U.blank(c, c["sims"]), c["matches"]) and np.array_equal(U.blank(c, None), c["matches"])
    assert (c["matches"] == -1).sum() > 100 and (c["matches"] == 20_000).sum() > 50
