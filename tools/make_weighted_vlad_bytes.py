"""tests/golden/weighted_vlad_bytes.json: SHA-256 digests of the weighted describe-stage outputs over the records of
tests/weighted_vlad_bytes.py, with the HIP version of the compiler that built the library.  Needs a GPU.

The file records what the kernels wrote at the commit BEFORE a change that must not move a byte (it was first written at the
parent of the commit that split out csrc/mfma_f32_dev.h, csrc/gram_tile_dev.h and csrc/weighted_agg_dev.h).  Run it at that
commit, never at the one under test.

    python tools/make_weighted_vlad_bytes.py [output path]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import weighted_vlad_bytes as WB  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else WB.GOLDEN
    records = {}
    for gid, run in WB.groups().items():
        records[gid] = run()
        print(gid, len(records[gid]), "settings", flush=True)
    with open(path, "w") as f:
        json.dump({"hip": WB.hip_version(), "records": records}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(path, sum(len(v) for v in records.values()), "records")


if __name__ == "__main__":
    main()
