"""LVIS Fixed AP (mq_det_amd.evaluation.LvisFixedAPEvaluator, csrc/ap_eval.hip) without a GPU: the kernel SOURCES through the host emulation
(tests/simt) against tests/golden/lvis_eval_{small,medium}, which tools/gen_golden_lvis_eval.py records by running the reference's lvis.py /
lvis_eval.py in place (LvisEvaluatorFixedAP.update + _summarize_fixed); one pair of more than 2 000 detections and 500 ground truths (the
kernel's slow path) against the restatement of evaluate_img in tests/lvis_eval_ref.py; the refusals of ids the fp32 rows cannot hold."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lvis_eval_ref as ref  # noqa: E402
from mq_det_amd.evaluation import LvisFixedAPEvaluator  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lvis_eval_")
FAST_GT = 512                                   # csrc/ap_eval.hip LvisRules::fast_gt
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


def load_case(name):
    with open(GOLD + name + ".json") as f:
        js = json.load(f)
    return js, dict(np.load(GOLD + name + ".npz"))


def predictions(js, a, device="cpu"):
    """the fixture's mdetr-style predictions, in the order the generator fed them"""
    out = []
    for i in js["image_order"]:
        m = a["image_id"] == i
        out.append((i, {"scores": torch.from_numpy(a["scores"][m]).to(device), "labels": torch.from_numpy(a["labels"][m]).to(device),
                        "boxes": torch.from_numpy(a["boxes"][m]).to(device)}))
    return out


def run_case(js, a, device="cpu"):
    """the engine's calls: update per three images, synchronize_between_processes, summarize"""
    ev = LvisFixedAPEvaluator(js["gt"], topk=js["topk"], device=device)
    preds = predictions(js, a, device)
    for n in range(0, len(preds), 3):
        ev.update(preds[n:n + 3])
    ev.synchronize_between_processes()
    strings = ev.summarize()
    return ev, strings


def pair_flags(ev, keys=None):
    """{(image id, category id): (matched [4, 10, D], ignored [4, 10, D], gt count [4])} from the match kernel's outputs (all pairs, or the
    pairs of the given (image id, category id) keys)"""
    e = ev.eval
    K = ev.K
    img = ev.img_ids_f.cpu().long().tolist()
    cat = ev.cat_ids_f.cpu().long().tolist()
    pkeys = e["pair_key"].cpu().tolist()
    if keys is None:
        sel = range(len(pkeys))
    else:
        ipos, cpos = {v: n for n, v in enumerate(img)}, {v: n for n, v in enumerate(cat)}
        where = {k: n for n, k in enumerate(pkeys)}
        sel = [where[ipos[i] * K + cpos[c]] for i, c in keys]
    bits = e["dt_bits"].cpu().numpy().view(np.uint64)
    pair_dt, gt_count = e["pair_dt"].cpu().tolist(), e["gt_count"].cpu().tolist()
    sh = np.arange(40, dtype=np.uint64)
    out = {}
    for p in sel:
        s, n = pair_dt[p]
        b = bits[s:s + n]
        m = ((b[:, 0:1] >> sh) & np.uint64(1)).astype(bool).T.reshape(4, 10, n)
        ig = ((b[:, 1:2] >> sh) & np.uint64(1)).astype(bool).T.reshape(4, 10, n)
        out[(img[pkeys[p] // K], cat[pkeys[p] % K])] = (m, ig, gt_count[p])
    return out


def check_case(name, ev, strings, flags=True):
    js, a = load_case(name)
    assert np.array_equal(ev.eval["precision"].cpu().numpy(), a["precision"]), name
    assert np.array_equal(ev.eval["recall"].cpu().numpy(), a["recall"]), name
    assert list(ev.results) == list(js["results"])
    for k, v in js["results"].items():
        assert abs(ev.results[k] - v) <= 1e-12, (k, ev.results[k], v)
        assert type(ev.results[k]) is float
    assert strings == js["strings"]
    if flags:
        got = pair_flags(ev)
        assert len(got) * 4 == len(js["flags"])
        for f in js["flags"]:
            m, ig, cnt = got[(f["image_id"], f["category_id"])]
            D = m.shape[2]
            assert np.array_equal(m[f["area"]], np.asarray(f["dt_m"], bool).reshape(10, D)), f
            assert np.array_equal(ig[f["area"]], np.asarray(f["dt_ig"], bool).reshape(10, D)), f
            assert cnt[f["area"]] == int(np.count_nonzero(np.asarray(f["gt_ig"]) == 0)), f


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def test_small_fixture_covers_every_rule():
    """the hand-made fixture reaches what it is meant to: -1 entries, truncation, ignored / id-0 / zero-area ground truths, foreign ids,
    IoUs of exactly 0.5 and 0.75"""
    js, a = load_case("small")
    p = a["precision"]
    assert (p == -1).any() and (p > 0).any() and (p == 0).any()
    gt = js["gt"]
    cats, imgs = {c["id"] for c in gt["categories"]}, {i["id"] for i in gt["images"]}
    assert {c["frequency"] for c in gt["categories"]} == {"r", "c", "f"}
    assert any(x["id"] == 0 for x in gt["annotations"]) and any(x.get("ignore") for x in gt["annotations"])
    assert any(x["area"] == 0 for x in gt["annotations"])
    assert any(x["category_id"] not in cats for x in gt["annotations"]) and any(x["image_id"] not in imgs for x in gt["annotations"])
    assert set(a["image_id"].tolist()) - imgs and set(a["labels"].tolist()) - cats and imgs - set(a["image_id"].tolist())
    assert int((a["labels"] == 1).sum()) > js["topk"]
    assert any(np.asarray(f["dt_ig"]).any() for f in js["flags"]) and any(np.asarray(f["gt_ig"]).any() for f in js["flags"])
    assert ref.bbiou([0, 0, 5, 10], [0, 0, 10, 10]) == 0.5 and ref.bbiou([0, 0, 7.5, 10], [0, 0, 10, 10]) == 0.75


def test_restatement_reproduces_the_fixtures():
    """tests/lvis_eval_ref.py (used where no fixture exists: the big pair, the GPU scale test, the engine test) = the reference's code"""
    for name in ("small", "medium"):
        js, a = load_case(name)
        ev = LvisFixedAPEvaluator(js["gt"], topk=js["topk"], device="cpu")
        for item in predictions(js, a):
            ev.update([item])
        ev.acc._fold()
        p, r, res, strings, _ = ref.summarize_fixed(js["gt"], ev.acc.rows.numpy(), js["topk"])
        assert np.array_equal(p, a["precision"]) and np.array_equal(r, a["recall"]) and strings == js["strings"], name


@needs_simt
def test_small_fixture_is_exact(emu):
    js, a = load_case("small")
    ev, strings = run_case(js, a)
    check_case("small", ev, strings)


@needs_simt
def test_medium_fixture_is_exact(emu):
    js, a = load_case("medium")
    ev, strings = run_case(js, a)
    check_case("medium", ev, strings, flags=False)


def big_pair(seed=3, n_dt=2100, n_gt=560):
    """one image, one category: more than 2 000 detections and 500 ground truths (the match kernel's slow path), small / medium / large
    boxes, ignored ground truths, ties"""
    g = np.random.default_rng(seed)
    gx, gy = g.random(n_gt) * 900, g.random(n_gt) * 900
    gw = g.choice([8.0, 20.0, 40.0, 90.0, 150.0], n_gt) * (0.8 + 0.4 * g.random(n_gt))
    gh = g.choice([8.0, 20.0, 40.0, 90.0], n_gt) * (0.8 + 0.4 * g.random(n_gt))
    anns = [{"id": n + 1, "image_id": 7, "category_id": 3, "bbox": [float(gx[n]), float(gy[n]), float(gw[n]), float(gh[n])],
             "area": float(gw[n] * gh[n]), "ignore": int(n % 11 == 0)} for n in range(n_gt)]
    gt = {"images": [{"id": 7, "neg_category_ids": [], "not_exhaustive_category_ids": []}], "annotations": anns,
          "categories": [{"id": 3, "frequency": "f"}]}
    src = g.integers(0, n_gt, n_dt)
    x = (gx[src] + g.standard_normal(n_dt) * gw[src] * 0.1).astype(np.float32)
    y = (gy[src] + g.standard_normal(n_dt) * gh[src] * 0.1).astype(np.float32)
    w = (gw[src] * (1 + 0.15 * g.standard_normal(n_dt))).astype(np.float32)
    h = (gh[src] * (1 + 0.15 * g.standard_normal(n_dt))).astype(np.float32)
    s = (np.floor(g.random(n_dt) * 512) / 512).astype(np.float32)
    rows = np.stack([np.full(n_dt, 7, np.float32), np.full(n_dt, 3, np.float32), s, x, y, w, h], 1)
    return gt, rows


def check_big_pair(device):
    gt, rows = big_pair()
    ev = LvisFixedAPEvaluator(gt, topk=10000, device=device)
    ev.acc.update(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3:])
    ev.synchronize_between_processes()
    ev.summarize()
    pr = ev.acc.rows.cpu().numpy()
    assert ev.eval["pair_gt"][0, 1].item() > FAST_GT and ev.eval["pair_dt"][0, 1].item() > 2000
    m, ig, cnt = pair_flags(ev)[(7, 3)]
    img_ids, cat_ids, gts, dts, nel, _ = ref.prepare(gt, pr, 10000)
    for ai, rng in enumerate(ref.AREA_RNG):
        wm, wi, gig, _ = ref.evaluate_img(dts[(7, 3)], gts[(7, 3)], rng, False)
        assert np.array_equal(m[ai], wm) and np.array_equal(ig[ai], wi), ai
        assert cnt[ai] == int(np.count_nonzero(gig == 0))
    p, r, _, strings, _ = ref.summarize_fixed(gt, pr, 10000)
    assert np.array_equal(ev.eval["precision"].cpu().numpy(), p) and np.array_equal(ev.eval["recall"].cpu().numpy(), r)


@needs_simt
def test_one_big_pair_matches_the_restated_evaluate_img(emu):
    check_big_pair("cpu")


@pytest.mark.parametrize("field", ["images.id", "categories.id", "annotations.image_id", "annotations.category_id"])
def test_ids_the_fp32_rows_cannot_hold_are_refused(field):
    js, _ = load_case("small")
    gt = copy.deepcopy(js["gt"])
    big = (1 << 24) + 1
    if field == "images.id":
        gt["images"][0]["id"] = big
    elif field == "categories.id":
        gt["categories"][0]["id"] = big
    else:
        gt["annotations"][0][field.split(".")[1]] = big
    with pytest.raises(ValueError, match=field.replace(".", r"\.")):
        LvisFixedAPEvaluator(gt, device="cpu")


def test_gt_from_a_path_and_an_lvis_like_object(tmp_path):
    js, _ = load_case("small")
    p = tmp_path / "gt.json"
    p.write_text(json.dumps(js["gt"]))
    obj = type("LVIS", (), {"dataset": js["gt"]})()
    a, b = LvisFixedAPEvaluator(str(p), device="cpu"), LvisFixedAPEvaluator(obj, device="cpu")
    assert torch.equal(a.gt_box, b.gt_box) and torch.equal(a.gt_key, b.gt_key) and a.freq_groups == b.freq_groups
    assert not hasattr(a, "accumulate")          # the engine's try / except around accumulate() relies on it
