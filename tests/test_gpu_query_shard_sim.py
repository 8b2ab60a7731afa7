"""tools/query_shard_sim.py runs end to end at a reduced shape and prints its JSON line (keys only; no timing asserted)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_shard_sim_smoke():
    cmd = [sys.executable, os.path.join(ROOT, "tools", "query_shard_sim.py"), "--worlds", "2,4", "--iters", "1", "--warmup", "1",
           "--query-images", "8", "--db-images", "64", "--segments", "8", "--clusters", "16", "--dim", "128", "--height", "224",
           "--width", "224", "--pca-dim", "64", "--build-batch", "16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["tool"] == "query_shard_sim" and set(rec["per_rank"]) == {"2", "4"}
    assert "NOT executed" in rec["collective_stand_in"]
    for w, v in rec["per_rank"].items():
        assert {"per_rank_ms", "stages_ms", "implied_images_per_s", "query_images_described", "collective_bytes_not_executed"} <= set(v)
        assert "vote" in v["stages_ms"] and v["query_images_described"] == 8 // int(w)
