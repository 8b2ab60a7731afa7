"""The tile walk of the fp16 kNN filter (csrc/f16_walk.h: what knn_f16_filter_kernel's tile_of / rev_of / kofs and its launcher's
sequence length call) runs on the CPU: tests/f16_walk_main.cpp, compiled with the host compiler, checks over a table of tile
counts, block heights, walk bits, resident workgroup counts and row depths that every tile is visited exactly once and that every
step's k-order is a permutation of its k-tiles.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revisit-anything_amd", "csrc")


def test_walk_header_is_plain_cxx():
    src = open(os.path.join(CSRC, "f16_walk.h")).read()
    includes = [ln.split()[1] for ln in src.split("\n") if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes   # neither ctx.h nor the HIP runtime


def test_walk_covers_every_tile_once_and_every_k_tile_once(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler (CXX, g++, c++)")
    exe = str(tmp_path / "f16_walk_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(ROOT, "tests", "f16_walk_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    # 7 tiles_m x 8 tiles_n x 7 block heights x 8 walk values x 3 resident counts; the k-order once per walk and each of 6 depths
    assert r.stdout.split() == ["walk", "cases", "9408", "k-order", "cases", "18816", "failures", "0"], r.stdout
