"""tests/golden/vlad_soft.npz: the reference's VLAD.generate in SOFT mode (utilities.py:862-887) on the two token sets of
anyloc_cases.npz (vocabulary vocab_indoor_k32_d1536.npy, 34 x 45 tokens), at soft_temp 1 and 10.

VLAD.generate / generate_res_vec are extracted from the reference's utilities.py exactly as tools/make_golden.py does for the hard
mode (class methods compiled from its syntax tree; nothing of its text is kept).  Sub-samples and an 8-column random projection
are stored, like anyloc_cases.npz, to keep the file small.

    python tools/make_soft_vlad_golden.py <reference checkout>
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from revisit_anything_amd import synth  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REVISIT_ANYTHING_REF", "")
OUT = os.path.join(ROOT, "tests", "golden")
TEMPS = (1.0, 10.0)
SEEDS = (2010, 2011)


def reference_generate():
    import einops as ein

    ucls = [n for n in ast.parse(open(f"{REF}/utilities.py").read()).body if isinstance(n, ast.ClassDef) and n.name == "VLAD"][0]
    meths = [m for m in ucls.body if isinstance(m, ast.FunctionDef) and m.name in ("generate", "generate_res_vec", "can_use_cache_vlad")]
    uns = dict(np=np, torch=torch, F=F, ein=ein, os=os, Union=__import__("typing").Union, List=__import__("typing").List)
    exec(compile(ast.Module(body=meths, type_ignores=[]), f"{REF}/utilities.py", "exec"), uns)
    return uns


def soft_vlad(uns, voc, tokens, temp):
    """VLAD(vlad_mode='soft', soft_temp=temp).generate on the normalised tokens, as aggFt calls it (func_vpr.py:941-943)."""
    vobj = types.SimpleNamespace(num_clusters=voc.shape[0], desc_dim=voc.shape[1], intra_norm=True, norm_descs=True, vlad_mode="soft",
                                 soft_temp=temp, cache_dir=None, c_centers=torch.from_numpy(voc), kmeans=object())
    vobj.can_use_cache_vlad = lambda: False
    vobj.generate_res_vec = lambda q, cid=None: uns["generate_res_vec"](vobj, q, cid)
    xq = F.normalize(torch.from_numpy(tokens.reshape(1, voc.shape[1], -1)), dim=1).permute(0, 2, 1).squeeze()
    return uns["generate"](vobj, xq).numpy()


def main():
    if not os.path.isfile(os.path.join(REF, "utilities.py")):
        sys.exit("usage: make_soft_vlad_golden.py <reference checkout>   (or REVISIT_ANYTHING_REF): utilities.py not found")
    voc = np.load(os.path.join(OUT, "vocab_indoor_k32_d1536.npy"))
    uns = reference_generate()
    Gm = np.random.Generator(np.random.PCG64(780)).standard_normal((voc.size, 8))
    av = {"temps": np.asarray(TEMPS), "seeds": np.asarray(SEEDS)}
    for j, seed in enumerate(SEEDS):
        tk = synth.make_tokens(voc, 34 * 45, seed=seed, noise=0.2)
        for temp in TEMPS:
            g = soft_vlad(uns, voc, tk, temp)
            av[f"vlad{j}_t{int(temp)}_sub"] = g[::37].astype(np.float64)
            av[f"vlad{j}_t{int(temp)}_proj"] = g.astype(np.float64) @ Gm
    np.savez_compressed(os.path.join(OUT, "vlad_soft.npz"), **av)
    print("vlad_soft.npz", {k: v.shape for k, v in av.items()})


if __name__ == "__main__":
    main()
