"""TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' of the TTA merge (mq_tta_merge_special, csrc/tta.hip) without a GPU: the kernel
SOURCES through the host emulation (tests/simt) against the numpy restatement tests/tta_special_ref.py, which tests/golden/tta_special
(tools/gen_golden_tta_special.py: the reference's own merge_result_from_multi_scales / bbox_vote / soft_bbox_vote, run in place) pins.
Cases, conditions on the inputs and comparison rules: tests/tta_special_cases.py, shared with tests/test_gpu_tta_special.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tta_special_cases as sc  # noqa: E402
import tta_special_ref as ref  # noqa: E402
from mq_det_amd import get_cfg, tta  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta_special")
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")
CPU = torch.device("cpu")


def load_gold():
    with open(GOLD + ".json") as f:
        js = json.load(f)
    return js, dict(np.load(GOLD + ".npz"))


@pytest.fixture(scope="module")
def gold():
    return load_gold()


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def gold_boxlists(js, a, device=CPU):
    out = []
    for b, wh in enumerate(js["image_wh"]):
        bl = BoxList(torch.from_numpy(a[f"in_boxes{b}"]).to(device), tuple(wh), mode="xyxy")
        bl.add_field("scores", torch.from_numpy(a[f"in_scores{b}"]).to(device))
        bl.add_field("labels", torch.from_numpy(a[f"in_labels{b}"]).to(device))
        out.append(bl)
    return out


def gold_expected(js, a, key):
    """The restated reference on the fixture's rows (for the per-row tolerances), after it is shown equal to the recorded reference."""
    c = js["cases"][key]
    want = [ref.merge_special(a[f"in_boxes{b}"], a[f"in_scores{b}"], a[f"in_labels{b}"], js["classes"], c["mode"], c["TH"], js["INFERENCE_TH"],
                              c["PRE_NMS_TOP_N"]) for b in range(len(js["image_wh"]))]
    assert [len(w["scores"]) for w in want] == c["out_counts"]
    for b, w in enumerate(want):
        for f in ("boxes", "scores", "labels"):
            assert np.array_equal(w[f], a[f"{key}_{f}{b}"]), (key, b, f)
    return want


def test_config_default_is_the_reference_default():
    assert get_cfg().MODEL.RETINANET.INFERENCE_TH == 0.05
    assert get_cfg().TEST.SPECIAL_NMS == "none"


def test_restated_reference_equals_the_recorded_reference(gold):
    js, a = gold
    assert sorted(js["cases"]) == sorted(f"{m}_{n}" for m, lst in sc.CASES.items() for n, th, _ in lst if th > 0)
    for key, c in js["cases"].items():
        assert (c["TH"], c["PRE_NMS_TOP_N"]) == [(th, top) for n, th, top in sc.CASES[c["mode"]] if f"{c['mode']}_{n}" == key][0]
        gold_expected(js, a, key)
    i = a["in_labels0"] == js["vote_class"]
    for fn, soft in (("bbox_vote", None), ("soft_bbox_vote", js["INFERENCE_TH"])):
        rows, _, _ = ref._vote(a["in_boxes0"][i], a["in_scores0"][i], js["vote_TH"], soft)
        assert len(rows) > 8
        assert np.array_equal(rows[:, :4].astype(np.float32), a[f"{fn}_boxes"]) and np.array_equal(rows[:, 4].astype(np.float32), a[f"{fn}_scores"])


def test_the_fixture_rows_are_the_shared_cases_rows(gold):
    js, a = gold
    for b, (bx, s, lb) in enumerate(sc.prep_restated(sc.build_dets(), sc.WH)):
        ok = ~np.isnan(s)
        assert ok.sum() == len(s) - (b == 0)                                        # the one NaN score
        assert np.array_equal(bx[ok], a[f"in_boxes{b}"]) and np.array_equal(s[ok], a[f"in_scores{b}"]) and np.array_equal(lb[ok], a[f"in_labels{b}"])


def test_the_cases_hold_what_they_claim():
    rows = sc.prep_restated(sc.build_dets(), sc.WH)
    dets = sc.build_dets()
    assert len(dets) == 4 and [d[3] for d in dets] == [False, True, False, True] and len({tuple(d[1]) for d in dets}) == 4
    for bx, s, lb in rows:
        n = {c: int((lb == c).sum()) for c in sc.CLASSES}
        assert n[7] == 0 and n[1] == 1 and n[4] == 2 and n[9] > sc.FORCED_CAP and n[5] > 2 and n[3] > 2
        assert ((lb == 6) | (lb == 11)).sum() > 0
    for mode in ref.MODES:
        (_, th, hi), (_, _, lo), (_, zero, _) = sc.CASES[mode]
        full = [len(w["scores"]) for w in sc.expected(mode, th, hi)]
        assert zero == 0.0 and all(lo < f < hi for f in full)
    vote = sc.expected("vote", 0.5, 1000)
    for (bx, s, lb), w in zip(rows, vote):
        ok = ~np.isnan(s)
        assert (w["labels"] == 5).sum() == 1 and w["avg"][w["labels"] == 5][0] == (lb[ok] == 5).sum()      # one cluster of the whole class
        assert (w["labels"] == 3).sum() == (lb[ok] == 3).sum() and not w["avg"][w["labels"] == 3].any()       # no overlaps: untouched
        assert (w["labels"] == 4).sum() == 1 and w["avg"][w["labels"] == 4][0] == 2


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_special_merge_kernels_match_the_restated_reference(emu, mode):
    dets = sc.build_dets()
    tta._WARNED_CLASSES = True
    for name, th, top_n in sc.CASES[mode]:
        want = sc.expected(mode, th, top_n)
        sc.check_conditions(mode, th, want)
        for cap in (None, sc.FORCED_CAP):
            stats = {}
            got = tta.merge(dets, sc.WH, sc.make_cfg(mode, th, top_n), CPU, row_cap=cap, stats=stats)
            # (TEST.TH = 0 returns the rows as they are: no per-class step runs, with either cap)
            assert (stats["workspace_classes"] > 0) == (cap is not None and th > 0), (name, cap, stats)
            for r, wh in zip(got, sc.WH):
                assert r.size == wh and r.mode == "xyxy" and r.fields() == ["scores", "labels"]
            sc.compare(mode, th, sc.host(got), want, f"{mode} {name} cap {cap}")


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_recorded_fixture_through_merge_result_from_multi_scales(emu, gold, mode):
    js, a = gold
    for name, th, top_n in sc.CASES[mode]:
        if th <= 0:
            continue
        want = gold_expected(js, a, f"{mode}_{name}")
        sc.check_conditions(mode, th, want)
        for cap in (None, sc.FORCED_CAP):
            stats = {}
            got = tta.merge_result_from_multi_scales(gold_boxlists(js, a), sc.make_cfg(mode, th, top_n), row_cap=cap, stats=stats)
            assert (stats["workspace_classes"] > 0) == (cap is not None)
            sc.compare(mode, th, sc.host(got), want, f"fixture {mode} {name} cap {cap}")


def none_cfg():
    cfg = sc.make_cfg("none", 0.5, 40)
    return cfg


def check_mode_none(device):
    """merge_result_from_multi_scales with 'none' = tta.merge on the same rows behind one identity transform, bit for bit, and = the
    restated per-class NMS merge tests/test_tta_cpu.py pins against the reference."""
    import test_tta_cpu as tc
    js, a = load_gold()
    cfg = none_cfg()
    bls = gold_boxlists(js, a, device)
    got = sc.host(tta.merge_result_from_multi_scales(bls, cfg))
    K = max(len(bl) for bl in bls)
    packed = torch.zeros(len(bls), K, 6)
    for b, bl in enumerate(bls):
        packed[b, :len(bl)] = torch.cat([bl.bbox.cpu(), bl.get_field("scores").cpu()[:, None], bl.get_field("labels").cpu().float()[:, None]], 1)
    wh = [tuple(w) for w in js["image_wh"]]
    dets = [(packed, [len(bl) for bl in bls], wh, False, None)]
    direct = sc.host(tta.merge([(packed.to(device),) + dets[0][1:]], wh, cfg, device))
    restated = tc.merge_restated(dets, wh, cfg)
    for g, d, (rb, rs, rl) in zip(got, direct, restated):
        assert 0 < len(g) == len(d)
        for x, y, z in ((g.bbox, d.bbox, rb), (g.get_field("scores"), d.get_field("scores"), rs), (g.get_field("labels"), d.get_field("labels"), rl)):
            assert torch.equal(x, y) and torch.equal(x, z)


@needs_simt
def test_mode_none_of_the_public_function_is_the_existing_merge(emu):
    check_mode_none(CPU)


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_result_does_not_depend_on_the_schedule(emu, mode):
    import simt
    dets = sc.build_dets()
    name, th, top_n = sc.CASES[mode][1]
    outs = []
    try:
        for sched, seed in (("ascending", 0), ("descending", 0), ("random", 7)):
            simt.set_schedule(sched, seed)
            outs.append(sc.host(tta.merge(dets, sc.WH, sc.make_cfg(mode, th, top_n), CPU, row_cap=sc.FORCED_CAP)))
    finally:
        simt.set_schedule("ascending")
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("scores"), y.get_field("scores"))
            assert torch.equal(x.get_field("labels"), y.get_field("labels"))


@needs_simt
def test_equal_scores_go_to_the_lower_original_row(emu):
    """Two disjoint rows of one class with the same score, in either packing order: the lower original row comes first in every mode."""
    for mode in ref.MODES:
        cfg = sc.make_cfg(mode, 0.3, 1000)
        for flip in (False, True):
            rows = [[1.0, 1.0, 9.0, 9.0, 0.5, 9.0], [20.0, 20.0, 29.0, 29.0, 0.5, 9.0]]
            packed = torch.tensor([rows[::-1] if flip else rows])
            got = tta.merge([(packed, [2], [(64, 48)], False, None)], [(64, 48)], cfg, CPU)[0]
            assert torch.equal(got.bbox, packed[0, :, :4]) and torch.equal(got.get_field("scores"), packed[0, :, 4])


def test_soft_vote_refuses_an_inference_threshold_that_grows_the_row_count():
    cfg = sc.make_cfg("soft-vote", 0.5, 1000)
    cfg.MODEL.RETINANET.INFERENCE_TH = 0.0
    with pytest.raises(ValueError, match="MODEL.RETINANET.INFERENCE_TH"):
        tta.merge(sc.build_dets(), sc.WH, cfg, CPU)


@needs_simt
def test_unknown_mode_is_refused_and_the_binding_defaults_to_none(emu):
    import inspect
    assert inspect.signature(emu.tta_merge).parameters["mode"].default == "none"
    cfg = sc.make_cfg("hard-vote", 0.5, 1000)
    with pytest.raises(ValueError, match="SPECIAL_NMS"):
        tta.merge(sc.build_dets(), sc.WH, cfg, CPU)
