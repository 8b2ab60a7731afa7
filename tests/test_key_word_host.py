"""The (distance, id) word every exact search path orders by (csrc/key_word.h: f2key_ / key2f_, sv_word / sv_word_d2 / sv_word_id,
SV_WORD_NONE, sv_np2 -- what the kernels and launchers call through knn_dev.h) runs on the CPU: tests/key_word_main.cpp, compiled
with the host compiler, checks the key round trip and order over a table of floats (zeros, denormals, adjacent floats, extremes,
infinities), the (distance, then id) order of packed words, that no finite distance packs to the empty word, unpacking, and the
sort length at every power of two up to 2^20 and its neighbours.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "revisit-anything_amd", "csrc")


def test_key_word_header_is_plain_cxx():
    src = open(os.path.join(CSRC, "key_word.h")).read()
    includes = [ln.split()[1] for ln in src.split("\n") if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes   # neither ctx.h nor the HIP runtime


def test_key_word_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.fail("no host C++ compiler (CXX, g++, c++)")
    exe = str(tmp_path / "key_word_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{CSRC}", os.path.join(ROOT, "tests", "key_word_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout, r.stderr[-4000:])
    assert r.returncode == 0, r.stderr[-4000:]
    # 15 table floats: 15 round trips, 15 x 15 ordered pairs, 15 x 3 ids; np2: n = 0, 1, 2 and 19 powers x 3 neighbours
    assert r.stdout.split() == ["keys", "15", "order", "pairs", "225", "words", "45", "np2", "cases", "60", "failures", "0"], r.stdout
