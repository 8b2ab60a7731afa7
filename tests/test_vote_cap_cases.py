"""The vote's per-image cap on the host: the reference of tests/vote_cap_ref.py on rows whose answer is obvious, engine.blank_capped
and _lib.vote_mode against it, the header's words, and the conditions that make the inputs of tests/test_gpu_vote_cap.py worth
running (the cap must bite, and it must change the scores)."""
import os

import numpy as np
import pytest

import search_tail_ref as R
import vote_cap_ref as V
from revisit_anything_amd import _lib
from revisit_anything_amd.engine import blank_capped

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# segment -> image: segments 0..5 carry the images [3, 3, 1, 3, -1, 1], segment 6 image -1 as well
IMG = np.array([3, 3, 1, 3, -1, 1, -1], np.int32)


def test_hand_made_row():
    row = np.array([[0, 1, 2, 3, 4, 5]], np.int64)                       # images 3 3 1 3 -1 1
    assert V.blank(row, IMG, 1).tolist() == [[0, -1, 2, -1, 4, -1]]
    assert V.blank(row, IMG, 2).tolist() == [[0, 1, 2, -1, 4, 5]]
    # an id past the map and a -1 are not valid: they neither vote nor count, and stay what they are
    row = np.array([[0, 7, 1, -1, 3, 9]], np.int64)
    assert V.blank(row, IMG, 1).tolist() == [[0, 7, -1, -1, -1, 9]]
    assert V.blank(row, IMG, 2).tolist() == [[0, 7, 1, -1, -1, 9]]
    # a negative image id is an image like any other: its second hit is capped
    row = np.array([[4, 6, 4, 2]], np.int64)                              # images -1 -1 -1 1
    assert V.blank(row, IMG, 1).tolist() == [[4, -1, -1, 2]]
    assert V.blank(row, IMG, 2).tolist() == [[4, 6, -1, 2]]
    # rows are independent
    rows = np.array([[0, 1, 3], [1, 3, 0]], np.int64)
    assert V.blank(rows, IMG, 1).tolist() == [[0, -1, -1], [1, -1, -1]]


@pytest.mark.parametrize("m", [6, 7, 255])
def test_cap_at_least_k_returns_the_input(m):
    row = np.array([[0, 1, 2, 3, 4, 5], [0, 0, 0, 0, 9, -1]], np.int64)
    assert np.array_equal(V.blank(row, IMG, m), row)
    assert np.array_equal(blank_capped(row, IMG, m), row)
    c = R.vote_case("nowl_first_2731x3")                                 # k = 3: m = 3 blanks nothing
    assert np.array_equal(V.blank(c["matches"], c["img_of_seg"], 3), c["matches"])


@pytest.mark.parametrize("m", [1, 2, 3, 7])
def test_blank_capped_equals_reference(m):
    rng = np.random.default_rng(m)
    img = rng.integers(-2, 12, size=90).astype(np.int32)
    idx = rng.integers(-3, 100, size=(40, 33)).astype(np.int64)          # ids below 0 and past the map among them
    assert np.array_equal(blank_capped(idx, img, m), V.blank(idx, img, m))
    assert np.array_equal(blank_capped(idx[:, :1], img, m), idx[:, :1])
    assert blank_capped(idx[:0], img, m).shape == (0, 33)
    for name in ("fast_last_64x64", "bench_depth_50x200"):
        c = V.case(name, True)
        assert np.array_equal(blank_capped(c["matches"], c["img_of_seg"], m), V.blank(c["matches"], c["img_of_seg"], m))
    import torch

    assert np.array_equal(blank_capped(torch.from_numpy(idx), torch.from_numpy(img), m), V.blank(idx, img, m))


def test_blank_capped_refuses_bad_caps():
    idx = np.zeros((2, 3), np.int64)
    for bad in (0, -1, 256, 1.5, True):
        with pytest.raises(ValueError):
            blank_capped(idx, IMG, bad)
    with pytest.raises(ValueError):
        blank_capped(idx[0], IMG, 1)


def test_vote_mode():
    assert _lib.VOTE_PER_IMAGE_SHIFT == 8
    for base in (_lib.VOTE_WT_BORDA_IM, _lib.VOTE_COUNT):
        assert _lib.vote_mode(base) == base and _lib.vote_mode(base, None) == base
        for m in range(1, 256):
            assert _lib.vote_mode(base, m) == base | (m << 8)
        for bad in (0, 256, -1, -255, 1 << 16):
            with pytest.raises(ValueError):
                _lib.vote_mode(base, bad)
    assert _lib.vote_mode(0x300 | 1) == 0x301                           # an int mode that carries the bits is accepted
    assert _lib.vote_mode(0x301, 3) == 0x301
    with pytest.raises(ValueError):
        _lib.vote_mode(0x301, 2)


def test_header_states_the_contract():
    hdr = " ".join(open(os.path.join(ROOT, "include", "segvlad.h")).read().replace("*", " ").split())
    assert "#define SEGVLAD_VOTE_PER_IMAGE(m) ((m) << 8)" in hdr
    for words in ("fewer than m valid entries at ranks r' < r of the same row carry the same g",
                  "every non-voting entry's id replaced by -1",
                  "bit for bit in pred_out and score_out",
                  "m >= k blanks nothing",
                  "does not back-fill the lists"):
        assert words in hdr, words


# ---- the inputs of the GPU parity test ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", V.CAPS)
@pytest.mark.parametrize("invalid", [False, True], ids=["plain", "invalid_ids"])
@pytest.mark.parametrize("name", V.SHAPES)
def test_gpu_inputs_make_the_cap_bite(name, invalid, m):
    c = V.case(name, invalid)
    share = V.blanked_share(c, m)
    assert share >= 0.002, share
    args = (c["sims"], c["off"], c["img_of_seg"], 5)
    capped = R.vote_wt(V.blanked(name, invalid, m), *args)
    plain = R.vote_wt(c["matches"], *args)
    differ = (capped[1].view(np.uint64) != plain[1].view(np.uint64)).any(axis=1)
    assert int(differ.sum()) >= 2, differ


def test_gpu_inputs_cover_the_regimes_and_the_chunks():
    assert V.SHAPES == R.REGIME_SHAPES + ["bench_depth_50x200"]
    assert sorted(R.VOTE_CASES[n][1] for n in V.SHAPES) == [3, 17, 64, 113, 200]
    assert {R.case_regime(V.case(n, False)["counts"], V.case(n, False)["k"])[0] for n in V.SHAPES} == \
        {"fast", "weights_in_lds", "no_weight_array", "global"}
    assert V.CHUNK_SHAPES[:2] == [(3, 65), (5, 1024)] and V.CHUNK_SHAPES[2][1] > 1024
    for segs, k in V.CHUNK_SHAPES:
        c = V.chunk_case(segs, k)
        b = V.blank(c["matches"], c["img_of_seg"], 1)
        big = slice(0, segs)
        assert (b[big, 64:] != c["matches"][big, 64:]).any()             # an entry behind the first chunk is capped ...
        assert (b[big, 64:] >= 0).any()                                  # ... and one of them still votes
        if k > 1024:
            assert (b[big, 1024:] != c["matches"][big, 1024:]).any()


def test_revisit_index_has_revisits():
    rows, img, q, off = V.revisit_index()
    assert 200 <= len(rows) <= 1000 and rows.shape[1] == 64 and len(img) == len(rows)
    assert np.bincount(img).min() >= 6                                   # every image stores its place several times
    d2 = ((q[:, None, :] - rows[None]) ** 2).sum(-1)
    top = np.argsort(d2, axis=1)[:, :20]
    assert V.blanked_share(dict(matches=top, img_of_seg=img), 1) >= 0.1
