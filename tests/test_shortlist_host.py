"""Host side of the shortlist search: the padding helper, the validation of host shortlists, and the timing tool's CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pad_shortlists():
    from revisit_anything_amd.engine import pad_shortlists

    a = pad_shortlists([[3, 1], [], [7, 7, 2]])
    assert a.dtype == np.int32 and a.shape == (3, 3)
    assert a.tolist() == [[3, 1, -1], [-1, -1, -1], [7, 7, 2]]
    assert pad_shortlists([[], []]).shape == (2, 1)
    assert pad_shortlists([[4]], M=5).tolist() == [[4, -1, -1, -1, -1]]
    with pytest.raises(ValueError):
        pad_shortlists([[1, 2, 3]], M=2)


def test_check_shortlist():
    from revisit_anything_amd.engine import check_shortlist

    ok = np.array([[0, -1], [4, 4]], np.int64)
    check_shortlist(ok, 2, 5)
    for bad, n_img, n_ref in ((np.array([[-2, 0]]), 1, 5), (np.array([[5]]), 1, 5), (ok, 3, 5), (np.zeros((1, 4097), np.int64), 1, 5),
                              (np.zeros((1, 0), np.int64), 1, 5), (np.zeros(3, np.int64), 3, 5)):
        with pytest.raises(ValueError):
            check_shortlist(bad, n_img, n_ref)


def test_shortlist_sim_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "shortlist_sim.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--m" in r.stdout
