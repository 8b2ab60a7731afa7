"""The unguarded library's stream order (tests/async_order.py has the rules and the table): every device-work entry of
include/segvlad.h on a PLAIN context, its inputs arriving late on a side stream and overwritten the moment the call returns,
against the same call on a guarded context and on a plain one, both serial:

    guarded serial == plain serial == plain delayed, bit for bit.

The guarded result of every case is also held to its reference (Case.check), so the identity inherits the suite's fp64
references at these shapes.  Every context runs with its options at their defaults (search_stats off: it would make a search
wait for its stream).  The cases run alone (both storages of the inputs), as one back-to-back sequence
per group on one stream, as the same sequence alternating between two streams, and in bench.py's pipelined arrangement of two
contexts.  Run with `-m gpu` on an MI355X; conftest.py's guard stays on for everything else (the plain contexts are made with
the environment variable set around their constructor only)."""
import numpy as np
import pytest
import torch

import async_order as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def delay():
    """The delay and its precondition, once per module: a consumer that does not wait for the side stream must see the decoy."""
    d = A.Delay()
    seen = d.prove()
    print(f"\n[async order] delay: {seen['gemms']} GEMMs of {d.ms_per_gemm:.3f} ms for {seen['asked_ms']:.0f} ms asked, "
          f"{seen['measured_ms']:.1f} ms measured; the unordered stand-in consumer saw the {seen['seen']}")
    if seen["seen"] != "decoy" or seen["measured_ms"] < A.MIN_DELAY_MS:
        pytest.fail(f"delay too short: the cases below would pass vacuously ({seen})")
    return d


_serial = {}


def _serial_legs(items):
    """The two serial legs of a sequence, computed once and shared (read-only) by the tests that compare against them: a
    group's two sequence tests, a case's two storages.  Only the last few sequences are kept."""
    key = tuple(items)
    if key not in _serial:
        _serial[key] = {leg: A.run_leg(items, leg) for leg in A.LEGS[:2]}
        for old in list(_serial)[:-4]:
            del _serial[old]
    return _serial[key]


def _three_legs(items, delay, n_streams=1):
    log = []
    by_leg = dict(_serial_legs(items))
    by_leg[A.LEGS[2]] = A.run_leg(items, A.LEGS[2], delay, n_streams=n_streams, log=log)
    print(f"[async order] {len(items)} call(s) on {n_streams} stream(s), delays (ms): {log[0]['delay_ms']}")
    A.compare_legs(items, by_leg)
    return by_leg


@pytest.mark.parametrize("name,variant", A.ITEMS, ids=[f"{n}-{v}" for n, v in A.ITEMS])
def test_case_alone(delay, name, variant):
    items = [(name, variant)]
    by_leg = _three_legs(items, delay)
    c = A.BY_NAME[name]
    if c.check is not None:                       # the guarded result against the references
        truth = c.build("truth")
        c.check(truth, by_leg[A.LEGS[0]][0], c.ref(truth))


@pytest.mark.parametrize("name", ["incidence", "images", "search_small"])
def test_the_harness_sees_a_call_issued_on_another_stream(delay, name):
    """The harness's own teeth: the same delayed leg with the context bound to the DEFAULT stream -- what a launch without a
    dependency on S amounts to -- reads the decoy (valid memory), and the comparison names the delayed leg."""
    items = [(name, "plain")]
    by_leg = dict(_serial_legs(items))
    by_leg[A.LEGS[2]] = A.run_leg(items, A.LEGS[2], delay, wrong_stream=True)
    with pytest.raises(AssertionError, match="the plain delayed leg differs from the other two"):
        A.compare_legs(items, by_leg)


@pytest.mark.parametrize("group", A.GROUPS)
def test_group_back_to_back_on_one_stream(delay, group):
    _three_legs(A.group_items(group), delay)


@pytest.mark.parametrize("group", A.GROUPS)
def test_group_alternating_between_two_streams(delay, group):
    """include/segvlad.h, segvlad_set_stream: the old stream's work must be ordered before the switch -- an event dependency
    (wait_stream) is such an order."""
    _three_legs(A.group_items(group), delay, n_streams=2)


# ---- bench.py's pipelined arrangement: two contexts, describe(i + 1) on its own stream issued before search(i) ------------------------
N_STEPS, N_IMG, SEGS, P_PIPE = 4, 10, 12, 64


def _pipe_inputs():
    """Four DIFFERENT query batches of 10 images x 12 segments, and a 40 000-row index of 64-d rows."""
    off = (np.arange(N_IMG + 1) * SEGS).astype(np.int32)
    batches = []
    for i in range(N_STEPS):
        masks = A.rect_masks("truth", seed=10 + i, n=N_IMG * SEGS)
        batches.append((torch.from_numpy(np.array(masks)).cuda(), torch.from_numpy(np.array(A.tokens_of("truth", seed=20 + i, n_img=N_IMG))).cuda()))
    return off, batches


def _pipe_engines(guard):
    eng, eng_d = A.make_engine(guard), A.make_engine(guard)
    eng_d.set_vocab(A.vocab())
    eng_d.pca_set(*A.pca_model(P_PIPE), whiten=True)
    eng_d.set_option("pca_path", "planes")        # (one form for every batch: the runs are compared digit for digit)
    eng.db_add(*A.index_rows(A.N40, P_PIPE))
    return eng, eng_d


def _describe(eng_d, batch, off):
    return eng_d.describe(batch[0], batch[1], off, A.H, A.W, A.PATCH, A.ORDER, pca=True, l2norm=True)


def _retrieve(eng, dsc, off):
    qd = dsc["out"]
    d2, idx = eng.search(qd, 20)
    sims, m = eng.sims_from_d2(d2, idx, 10)
    pred, sc = eng.vote(m, sims, off, n_top=5)
    return {"desc": qd, "adj": dsc["adj"], "flags": dsc["flags"], "d2": d2, "idx": idx, "sims": sims, "pred": pred, "scores": sc}


def _finish(engines, out):
    """The one synchronisation of a run, its results on the host, its contexts closed."""
    try:
        torch.cuda.synchronize()
        return [{k: v.cpu().numpy() for k, v in o.items()} for o in out]
    finally:
        for e in engines:
            e.close()


def _pipe_serial(guard, off, batches):
    eng, eng_d = _pipe_engines(guard)
    out = []
    for b in batches:
        qd = _describe(eng_d, b, off)
        eng_d.synchronize()
        out.append(_retrieve(eng, qd, off))
        eng.synchronize()
    return _finish((eng, eng_d), out)


def _pipe_pipelined(off, batches):
    eng, eng_d = _pipe_engines(False)
    torch.cuda.synchronize()
    s_desc = torch.cuda.Stream()
    cur = torch.cuda.current_stream()

    def describe_async(i):
        s_desc.wait_stream(cur)
        with torch.cuda.stream(s_desc):
            qd = _describe(eng_d, batches[i], off)
            ev = torch.cuda.Event()
            ev.record(s_desc)
        return qd, ev

    out = []
    nxt = describe_async(0)
    for i in range(len(batches)):
        qd, ev = nxt
        if i + 1 < len(batches):
            nxt = describe_async(i + 1)
        cur.wait_event(ev)
        qd["out"].record_stream(cur)              # allocated on the describe stream, consumed on this one
        out.append(_retrieve(eng, qd, off))               # (no host synchronisation in here: search_stats is off, 120 rows take the device tail)
    return _finish((eng, eng_d), out)


def test_pipelined_describe_and_search_on_two_contexts():
    off, batches = _pipe_inputs()
    torch.cuda.synchronize()
    legs = {"guarded serial": _pipe_serial(True, off, batches), "plain serial": _pipe_serial(False, off, batches)}
    _pipe_pipelined(off, batches[:2])             # warm-up (sizes both contexts' scratch), as bench.py does
    legs["plain pipelined"] = _pipe_pipelined(off, batches)
    g = legs["guarded serial"]
    for i in range(1, N_STEPS):                   # a descriptor left over from the step before would not be the right answer here
        assert not np.array_equal(g[i]["desc"], g[i - 1]["desc"]) and not np.array_equal(g[i]["idx"], g[i - 1]["idx"])
    problems = [f"step {i} output '{k}': the {leg} leg differs from the guarded serial one"
                for leg in ("plain serial", "plain pipelined") for i in range(N_STEPS) for k in g[i]
                if legs[leg][i][k].tobytes() != g[i][k].tobytes()]
    assert not problems, "\n".join(problems)
    # the guarded descriptors and distances against the oracle (tolerances of tests/test_gpu_frows.py / test_gpu_parity.py)
    O = A.O()
    mean, comps, var = A.pca_model(P_PIPE)
    R = A.index_rows(A.N40, P_PIPE)[0]
    for i, (masks, tok) in enumerate(batches):
        masks, tok = masks.cpu().numpy(), tok.cpu().numpy()
        desc = []
        for b in range(N_IMG):
            m = masks[off[b]:off[b + 1]]
            adj = g[i]["adj"][b * SEGS * SEGS:(b + 1) * SEGS * SEGS].reshape(SEGS, SEGS).astype(bool)
            if g[i]["flags"][b] == 0:             # generic centroids: the device's triangulation is Qhull's
                assert np.array_equal(adj, O.nbr_masks_agg_fast_single(list(m), A.ORDER))
            desc.append(O.seg_vlad_from_masks(tok[b], m, A.vocab(), A.H, A.W, adj, A.PATCH))
        y = O.pca_transform(np.concatenate(desc), mean, comps, var, whiten=True)
        y /= np.linalg.norm(y, axis=1, keepdims=True)
        assert np.abs(g[i]["desc"] - y).max() < A.PCA_REL_TOL * np.abs(y).max()
        rd2, ridx = O.knn_l2(R, g[i]["desc"], 20)
        A.check_knn(None, g[i], {"d2": rd2, "idx": ridx})
