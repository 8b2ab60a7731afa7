"""The records of tests/golden/weighted_vlad_bytes.json: SHA-256 digests of what the weighted describe-stage kernels
(csrc/soft_vlad_kernels.hip, csrc/burst_kernels.hip, csrc/burst_seg_kernels.hip, and csrc/assign_kernels.hip + csrc/vlad_kernels.hip
behind hard + off) write,
recorded once at the commit before their shared headers (csrc/mfma_f32_dev.h, csrc/gram_tile_dev.h, csrc/weighted_agg_dev.h) were
split out.  These kernels sum in one fixed order, so a refactor of them is held to the recorded bytes, not to a tolerance.

A plain module: tools/make_weighted_vlad_bytes.py writes the file from `groups()`, tests/test_gpu_weighted_vlad_bytes.py rebuilds
every record and compares.  The file is a recorded result; re-recording (after a toolchain change, say) is a deliberate act."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np

import describe_shape_cases as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_vlad_bytes.json")

# k2_d36_n65: D no whole 32-chunk, one partial tile.  k33_d96_n129: a second tile of one token, Kpad = 64.  k65_d200_n333: D % 32 != 0,
# Kpad = 128.  k128_d64_n513_s129: SC = 3, five tiles, the segment-chunk early exit.
CASES = ("k2_d36_n65", "k33_d96_n129", "k65_d200_n333", "k128_d64_n513_s129")
ASSIGNS = (("hard", None), ("soft", 10.0), ("soft_pooled", 10.0))
MAIN = (8.0, 7.0, 1.0)
BURSTS = (None, MAIN, (2.0, 0.0, 0.5))        # 2:0:0.5 is the powf branch of the discount
SCOPES = ("image", "segment")
ELEVEN_CASE, ELEVEN_ORDER = "k33_d96_n129", (0, 2, 1, 0, 2, 2, 0, 1, 2, 0, 2)     # tests/test_gpu_burst_seg.py's batch of eleven
PCA_CASE = "k33_d96_n129"
KEYS = ("out", "block_norms", "labels", "gap")


def settings(assigns=ASSIGNS, bursts=BURSTS):
    """(assign, burst, scope): the scope only where the burst discount is on"""
    return [(a, p, s) for a in assigns for p in bursts for s in (SCOPES if p is not None else ("image",))]


def setting_id(assign, burst, scope):
    a = assign[0] if assign[1] is None else f"{assign[0]}:{assign[1]:g}"
    return f"{a}|off" if burst is None else f"{a}|{burst[0]:g}:{burst[1]:g}:{burst[2]:g}|{scope}"


def hip_version():
    """The 'HIP version' line of the compiler that builds the library"""
    from revisit_anything_amd import build

    out = subprocess.run([build._hipcc(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode()
    return re.search(r"HIP version:\s*(\S+)", out).group(1)


def _digest(t):
    a = np.ascontiguousarray(t.cpu().numpy())
    return hashlib.sha256(f"{a.dtype}{a.shape}".encode() + a.tobytes()).hexdigest()


def _set(eng, assign, burst, scope):
    eng.set_vlad_assign(*assign)
    eng.set_vlad_burst(burst)
    eng.set_vlad_burst_scope(scope)


def _engine(C, pca=None):
    import async_order as A

    eng = A.make_engine(True)      # the guarded library, as the burst tests run it
    eng.set_vocab(C)
    if pca is not None:
        eng.pca_set(*pca, whiten=True)
    return eng


def _images(eng, tok, bits, offs, adj):
    r = eng.seg_vlad(tok, bits, offs, adj, want_labels=True, want_gap=True, want_block_norms=True)
    return {k: _digest(r[k]) for k in KEYS}


def _table(name, with_adj):
    d = T.build(name)
    eng = _engine(d["C"])
    try:
        out = {}
        for a, p, s in settings():
            _set(eng, a, p, s)
            out[setting_id(a, p, s)] = _images(eng, d["tok"], d["bits"], d["offs"], d["adj"] if with_adj else None)
        return out
    finally:
        eng.close()


def _eleven():
    """B = 11: the by-XCD dealing of both Gram kernels with a padded grid"""
    d = T.build(ELEVEN_CASE)
    tok, bits, offs, adj = T.pack_batch(*([d[k][b] for b in ELEVEN_ORDER] for k in ("toks", "incs", "adjs")))
    eng = _engine(d["C"])
    try:
        out = {}
        for a, p, s in settings(ASSIGNS[:2], (MAIN,)):
            _set(eng, a, p, s)
            out[setting_id(a, p, s)] = _images(eng, tok, bits, offs, adj)
        return out
    finally:
        eng.close()


def _pca():
    """seg_vlad_pca with want_desc: the planes form, the split of the weighted descriptor into fp16 planes behind the aggregation"""
    d = T.build(PCA_CASE)
    eng = _engine(d["C"], T.pca_model(PCA_CASE))
    try:
        out = {}
        for a, p, s in settings(ASSIGNS[:2], (None, MAIN)):
            _set(eng, a, p, s)
            r = eng.seg_vlad_pca(d["tok"], d["bits"], d["offs"], d["adj"], l2norm=True, want_desc=True)
            out[setting_id(a, p, s)] = {"y": _digest(r["out"]), "out": _digest(r["desc"])}
        return out
    finally:
        eng.close()


def groups():
    """{group id: a function of nothing -> {setting id: {output: digest}}}; a group shares one engine"""
    g = {f"{name}|{'adj' if with_adj else 'noadj'}": (lambda n=name, w=with_adj: _table(n, w)) for name in CASES for with_adj in (True, False)}
    g[f"{ELEVEN_CASE}|b11"] = _eleven
    g[f"{PCA_CASE}|pca"] = _pca
    return g


def load():
    with open(GOLDEN) as f:
        return json.load(f)
