"""What every trainer records, pinned: each configuration of tests/golden/make_plan_golden.py is rebuilt on a CPU session and
its plans - call sequence, descriptors, scalars, buffer wiring, workspace sizes, prepare_multi job tables - its variable
inventory, the layout of the flat trainable buffer and the initial weights must equal tests/golden/plan_signatures.json
exactly.  The host layer only chooses which kernel runs on which layer with which buffers: this is that choice."""
import hashlib
import importlib.util
import os

import pytest

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_plan_golden", os.path.join(_GOLDEN_DIR, "make_plan_golden.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

CASES = [(key, kind, kw, N) for key, kind, kw, Ns in mk.configurations() for N in Ns]


@pytest.fixture(scope="module")
def golden():
    return mk.load_golden()


def test_golden_covers_exactly_the_configurations(golden):
    assert list(golden) == [c[0] for c in mk.configurations()]
    for key, _, _, Ns in mk.configurations():
        assert list(golden[key]["plans"]) == [str(N) for N in Ns], key


@pytest.mark.parametrize("key,kind,kw,N", CASES, ids=["%s N=%d" % (c[0], c[3]) for c in CASES])
def test_recorded_plans_match_the_golden(golden, key, kind, kw, N):
    store, plans, full = mk.record(kind, kw, N)
    want = golden[key]
    assert store["tf_names"] == want["tf_names"], "%s: variable inventory changed" % key
    assert store["train_ranges"] == want["train_ranges"], "%s: order or layout of the flat trainable buffer changed" % key
    assert store["train_numel"] == want["train_numel"], key
    assert store["init_crc32c"] == want["init_crc32c"], "%s: initialize() draws other weights" % key
    wplans = want["plans"][str(N)]
    assert list(plans) == list(wplans), (key, list(plans), list(wplans))
    for pname, got in plans.items():
        w = wplans[pname]
        if got == w:
            continue
        gn, wn, H = mk.unrle(got["names"]), mk.unrle(w["names"]), mk.HEX
        sig = full[pname]
        for i in range(max(len(gn), len(wn))):
            if i >= len(gn) or i >= len(wn) or gn[i] != wn[i] or got["calls"][H * i:H * i + H] != w["calls"][H * i:H * i + H]:
                pytest.fail("%s N=%d %s: first differing call is #%d: recorded %s, golden has %s (%d calls recorded, %d in "
                            "the golden)\nrecorded call: %s" % (key, N, pname, i, gn[i] if i < len(gn) else None,
                                                                 wn[i] if i < len(wn) else None, len(gn), len(wn),
                                                                 mk._dump(sig[i]) if i < len(sig) else None))
        pytest.fail("%s N=%d %s: the plan's SHA-256 differs, in a call whose %d hex digits do not" % (key, N, pname, H))
    assert hashlib.sha256(mk._dump(full["plan_train"]).encode()).hexdigest() == wplans["plan_train"]["sha256"]


def _without_workspace_sizes(sig):
    """the signature with every shared-workspace byte count masked: a trainer's graphs share one workspace, sized by the
    largest of them"""
    def arg(a):
        return {k: None for k in a} if isinstance(a, dict) and ("ws_bytes" in a or "side_ws_bytes" in a) else a
    return [c if isinstance(c, str) else [c[0], c[1], [arg(a) for a in c[2]]] for c in sig]


@pytest.mark.parametrize("kind,kw,N,other,fresh_N", [
    ("trainer", dict(num_skip=1), 8, 7, 7), ("trainer", dict(num_skip=1, embedding=True), 8, 7, 7),
    ("class", dict(), 24, 1, 12)], ids=["trainer", "trainer-embedding", "class"])
def test_graph_for_another_batch_size_records_what_a_fresh_trainer_records(kind, kw, N, other, fresh_N):
    """`_graph_for(other)` after a larger primary graph (replicas of the models: the same variables, new buffers and
    plans; `other` counts frames for Trainer, clips of 12 frames for TrainerClass) records the plans a fresh trainer
    builds at that size"""
    tr, _, _, _ = mk.build(kind, kw, N, "cpu")
    g = tr._graph_for(other)
    assert g is not tr.primary and g.N == fresh_N
    got = {p: _without_workspace_sizes(mk.signature(getattr(g, p))) for p in ("plan_train", "plan_eval")}
    _, _, fresh, _ = mk.build(kind, kw, fresh_N, "cpu")
    for p, sig in got.items():
        assert sig == _without_workspace_sizes(mk.signature(getattr(fresh, p))), p
