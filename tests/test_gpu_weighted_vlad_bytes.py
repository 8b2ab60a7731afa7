"""The weighted describe-stage kernels against the bytes recorded before their shared headers were split out
(tests/golden/weighted_vlad_bytes.json, written by tools/make_weighted_vlad_bytes.py; the records are tests/weighted_vlad_bytes.py's).

These kernels sum in one fixed order by design (tests/test_gpu_burst_seg.py: two calls, a B = 1 call: the same bytes), so the bar
is digest equality.  The digests depend on the compiler's code generation: on a HIP version other than the recorded one the test
fails and says so; it does not skip."""
import pytest

import weighted_vlad_bytes as WB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    rec, here = WB.load(), WB.hip_version()
    assert rec["hip"] == here, (f"tests/golden/weighted_vlad_bytes.json was recorded under HIP {rec['hip']}, this library is built by HIP {here}: "
                                "bit equality is only defined under the recorded toolchain (re-record at a known-good commit)")
    return rec["records"]


def test_the_file_holds_the_records_of_the_table(recorded):
    want = {gid: None for gid in WB.groups()}
    assert sorted(recorded) == sorted(want)


@pytest.mark.parametrize("gid", list(WB.groups()))
def test_the_bytes_are_the_recorded_ones(recorded, gid):
    got, want = WB.groups()[gid](), recorded[gid]
    assert sorted(got) == sorted(want), gid
    moved = [(sid, key) for sid in want for key in want[sid] if got[sid].get(key) != want[sid][key]]
    print(f"{gid}: {len(want)} settings, {sum(len(v) for v in want.values())} digests, {len(moved)} moved")
    assert not moved, (gid, moved)
