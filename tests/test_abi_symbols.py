"""The C-ABI library builds (cross-compiled for gfx950), loads without a GPU and exports every symbol
that include/segvlad.h declares; the ctypes table binds exactly that set.  No compute calls here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "segvlad.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(segvlad_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_expected_surface():
    names = header_functions()
    for must in ("segvlad_create", "segvlad_set_vocab", "segvlad_incidence", "segvlad_images", "segvlad_pca_apply",
                 "segvlad_db_add", "segvlad_search", "segvlad_merge_topk", "segvlad_vote", "segvlad_cluster_aggregate"):
        assert must in names


def test_library_builds_loads_and_exports_every_declared_symbol():
    from revisit_anything_amd import _lib, build

    csrc = os.path.join(ROOT, "revisit-anything_amd", "csrc")
    assert sorted(build.SOURCES) == sorted(f for f in os.listdir(csrc) if f.endswith(".hip")), "build.SOURCES is not the set of csrc/*.hip"
    path = build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    for name in header_functions():
        assert hasattr(lib, name), f"{name} declared in segvlad.h but not exported by {path}"
    assert sorted(_lib.SIGNATURES) == header_functions()
    assert lib.segvlad_version() >= 100


def test_error_codes_without_context():
    from revisit_anything_amd import _lib

    lib = _lib.load()
    assert lib.segvlad_set_vocab(None, None, 1, 4) == -1           # SEGVLAD_ERR_ARG: null context
    assert lib.segvlad_last_error(None) == b"null context"


def test_product_fails_loudly_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from revisit_anything_amd._lib import SegVLADError
    from revisit_anything_amd.engine import SegVLADEngine

    with pytest.raises(SegVLADError):
        SegVLADEngine(0)
    from revisit_anything_amd import func_vpr

    with pytest.raises(SegVLADError):
        func_vpr.normalizeFeat([[1.0, 2.0]])


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "revisit-anything_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in txt.replace("segvlad_oracle", "oracle") or f == "_nothing_", (
                    f"{f} mentions the oracle: the product path must not route through it")


def test_every_context_buffer_is_released_by_destroy():
    """segvlad_destroy must free every grow-only device buffer the context declares (four were missing).  Since
    round 4 the buffers are declared through two X-macro lists that segvlad_create (tags, guard mode), the guard check and
    segvlad_destroy all walk: no buffer may be declared outside them, and destroy must release through the walk."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ctx = open(os.path.join(root, "revisit-anything_amd", "csrc", "ctx.h")).read()
    body = ctx[ctx.index("struct segvlad_ctx {"):]
    body = body[:body.index("int fail(")]
    stray = [d for d in re.findall(r"^\s*DevBuf\s+([^;(]+);", body, flags=re.M) if d.strip() != "n"]
    assert stray == [], f"DevBuf members declared outside SV_PERSISTENT_BUFS / SV_SCRATCH_BUFS: {stray}"
    listed = re.findall(r"X\((\w+)\)", body)
    assert len(listed) > 60 and len(set(listed)) == len(listed)
    assert "SV_PERSISTENT_BUFS(SV_VISIT_BUF)" in body and "SV_SCRATCH_BUFS(SV_VISIT_BUF)" in body and "for (auto& b : stage) f(b);" in body
    api = open(os.path.join(root, "revisit-anything_amd", "csrc", "api.hip")).read()
    dtor = api[api.index("int segvlad_destroy("):api.index("const char* segvlad_last_error")]
    assert "for_each_buf([](DevBuf& b) { b.release(); })" in dtor
    # every buffer some translation unit uses is one of the listed ones
    used = set()
    d = os.path.join(root, "revisit-anything_amd", "csrc")
    for f in os.listdir(d):
        used.update(re.findall(r"ctx->((?:s|db|pca|vocab)\w*)\.(?:reserve|as<|p\b|cap\b)", open(os.path.join(d, f)).read()))
    assert used - set(listed) == set(), sorted(used - set(listed))


def test_hot_entry_points_never_read_the_environment():
    """switches are read once at context creation; ablation kernels only exist behind SEGVLAD_ABLATIONS."""
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d = os.path.join(root, "revisit-anything_amd", "csrc")
    for f in os.listdir(d):
        src = open(os.path.join(d, f)).read()
        # strip the development-only blocks
        src_ship = re.sub(r"#ifdef SEGVLAD_ABLATIONS.*?#endif", "", src, flags=re.S)
        for m in re.finditer(r"getenv\(", src_ship):
            line_start = src_ship.rfind("\n", 0, m.start())
            ctx_txt = src_ship[max(0, src_ship.rfind("int segvlad_", 0, m.start())):m.start()]
            assert f == "api.hip" and "segvlad_create" in ctx_txt.split("int segvlad_")[-1][:40] or "segvlad_create" in ctx_txt[-3000:], \
                f"getenv outside segvlad_create in {f}: {src_ship[line_start:m.end() + 40]!r}"
