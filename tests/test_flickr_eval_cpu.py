"""Flickr30k Entities Recall@k (mq_det_amd.evaluation.FlickrRecallEvaluator, csrc/flickr_eval.hip) without a GPU: the kernel SOURCES through the
host emulation (tests/simt) on CPU tensors.  The two fixtures (tools/gen_golden_flickr_eval.py) are outputs of the reference's own code on
the hand-made Entities directory tests/golden/flickr_entities; tests/flickr_eval_ref.py (pinned by the generator on the same fixtures)
stands in where they do not reach: over 64 detections or ground truths, ties, zero-area boxes."""
import json
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)

import flickr_eval_ref as ref  # noqa: E402
from mq_det_amd.evaluation import FlickrRecallEvaluator, read_entities_sentences  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
ENT = os.path.join(GOLDEN, "flickr_entities")
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


def load_case(name):
    with open(os.path.join(GOLDEN, f"flickr_eval_{name}.json")) as f:
        js = json.load(f)
    return js, np.load(os.path.join(GOLDEN, f"flickr_eval_{name}.npz"))


def boxlist(boxes, scores, labels, size, device="cpu"):
    bl = BoxList(torch.from_numpy(np.ascontiguousarray(boxes)).reshape(-1, 4).to(device), tuple(size), mode="xyxy")
    bl.add_field("scores", torch.from_numpy(np.ascontiguousarray(scores)).to(device))
    bl.add_field("labels", torch.from_numpy(np.ascontiguousarray(labels)).to(device))
    return bl


def feed_raw(ev, js, a, device="cpu", which=None):
    """the model's raw BoxLists through update_boxlist"""
    for n, s in enumerate(js["sentences"]):
        if which is not None and n not in which:
            continue
        lo, hi = a["off"][n], a["off"][n + 1]
        ev.update_boxlist(s["image_id"], s["sentence_id"], boxlist(a["boxes"][lo:hi], a["scores"][lo:hi], a["labels"][lo:hi], s["size"], device),
                          s["n_phrases"], js["plus"], torch.tensor(s["orig_size"]))


def from_fixture_gt(js, device="cpu", **kw):
    return FlickrRecallEvaluator(js["gt_sentences"], js["gt_boxes"], topk=js["topk"], iou_thresh=js["iou_thresh"], device=device, **kw)


def check_score(score, js):
    assert list(score.items()) == [(k, v) for k, v in js["score"]]                 # equal keys in equal order, equal floats


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


# ---------------------------------------------------------------------------------------------------------------- fixtures
def test_fixture_directory_holds_every_required_case():
    js, a = load_case("small")
    sents = FlickrRecallEvaluator.from_entities_dir(ENT, "test", device="cpu")
    raw = {i: read_entities_sentences(os.path.join(ENT, "Sentences", f"{i}.txt")) for i in sents.sentences}
    phrases = [p for ss in raw.values() for s in ss for p in s]
    assert len(raw) == 4 and sum(len(ss) for ss in raw.values()) == 12
    assert any(p["phrase_id"] not in sents.gt_boxes[i] for i, ss in raw.items() for s in ss for p in s)          # a phrase without boxes
    assert any(s is None for ss in sents.sentences.values() for s in ss)                                          # a sentence left with none
    assert any(len(p["phrase_type"]) == 2 for p in phrases) and any(len(p["phrase_type"]) == 0 for p in phrases)
    assert any(len(b) > 1 for d in sents.gt_boxes.values() for b in d.values())
    counts = sorted({len(b) - 1 for p in js["post"] for b in p["boxes"]})
    assert {0, 1, 5, 10, 11} <= set(counts)
    for n, s in enumerate(js["sentences"]):                                                                       # no ties within a sentence
        sc = a["scores"][a["off"][n]:a["off"][n + 1]]
        assert len(np.unique(sc)) == len(sc)
    ious = [ref.box_iou(b, js["gt_boxes"][p["image_id"]][ph["phrase_id"]]) for p in js["post"]
            if js["gt_sentences"][p["image_id"]][p["sentence_id"]] for b, ph in zip(p["boxes"], js["gt_sentences"][p["image_id"]][p["sentence_id"]])]
    assert any((i == 0.5).any() for i in ious) and any(np.isnan(i).any() for i in ious)
    first_hit = {int(np.argmax(np.nan_to_num(i).max(1) >= 0.5)) + 1 for i in ious if (np.nan_to_num(i).max(1) >= 0.5).any()}
    assert {2, 6, 11} <= first_hit


@pytest.mark.parametrize("name", ["small", "merged"])
def test_entities_parsers_give_the_recorded_ground_truth(name):
    js, _ = load_case(name)
    ev = FlickrRecallEvaluator.from_entities_dir(ENT, js["subset"], merge_boxes=js["merge_boxes"], device="cpu")
    assert {k: v for k, v in ev.sentences.items()} == js["gt_sentences"] and list(ev.sentences) == list(js["gt_sentences"])
    assert ev.gt_boxes == js["gt_boxes"]
    assert [f"{i}_{s}" for i, s in ev.slot_name] == js["all_ids"]
    other = FlickrRecallEvaluator.from_entities_dir(ENT, "val", device="cpu")
    assert list(other.sentences) == ["1001"]


@pytest.mark.parametrize("name", ["small", "merged"])
def test_restatement_reproduces_the_reference(name):
    js, a = load_case(name)
    check_score(ref.evaluate(js["gt_sentences"], js["gt_boxes"], js["post"], js["topk"], js["iou_thresh"]), js)
    for n, (s, p) in enumerate(zip(js["sentences"], js["post"])):
        lo, hi = a["off"][n], a["off"][n + 1]
        q = ref.post_process(s["image_id"], s["sentence_id"], a["boxes"][lo:hi], a["scores"][lo:hi], a["labels"][lo:hi], s["size"], s["orig_size"],
                             s["n_phrases"], js["plus"])
        assert q["boxes"] == p["boxes"]


@needs_simt
@pytest.mark.parametrize("name", ["small", "merged"])
def test_fixture_is_exact(emu, name):
    js, a = load_case(name)
    ev = FlickrRecallEvaluator.from_entities_dir(ENT, js["subset"], merge_boxes=js["merge_boxes"], topk=js["topk"], device="cpu")
    ev.update(js["post"])                                                          # the reference's post-processed dicts
    check_score(ev.summarize(), js)
    hits_a = ev.eval["hits"].clone()
    ev = from_fixture_gt(js)
    feed_raw(ev, js, a)                                                            # the raw BoxLists
    check_score(ev.summarize(), js)
    assert torch.equal(ev.eval["hits"], hits_a)
    # the rows of the two routes hold the same boxes per phrase in the same order (the dicts' lists end with the dummy box)
    ev2 = from_fixture_gt(js)
    ev2.update(js["post"])
    ev2.evaluate()
    for (ds, dn), (es, en) in zip(ev.eval["phrase_dt"].tolist(), ev2.eval["phrase_dt"].tolist()):
        assert en == dn + 1 and torch.equal(ev.eval["dt_box"][ds:ds + dn], ev2.eval["dt_box"][es:es + dn])
        assert ev2.eval["dt_box"][es + dn].abs().sum() == 0


@needs_simt
def test_merge_boxes_at_construction_equals_the_merged_fixture(emu):
    js, a = load_case("merged")
    small, _ = load_case("small")
    ev = FlickrRecallEvaluator(small["gt_sentences"], small["gt_boxes"], merge_boxes=True, device="cpu")
    assert ev.gt_boxes == js["gt_boxes"]
    feed_raw(ev, js, a)
    check_score(ev.summarize(), js)


# ---------------------------------------------------------------------------------------------------------------- beyond the fixtures
def random_case(seed=5):
    """three images; phrases with 65 and 130 detections, one with 70 ground-truth boxes, quantised scores (ties), a zero-area ground truth"""
    from mq_det_amd.utils.synth import synthetic_flickr
    gt, boxes, preds = synthetic_flickr(n_img=3, sent_per_img=3, phrases_per_sent=3.0, det_per_sent=40, seed=seed, hit_frac=0.3, score_levels=16)
    g = np.random.default_rng(seed)
    img, s, size, orig, n_ph, b, sc, ph = preds[0]
    h, w = orig
    ratio = np.array([size[0] / w, size[1] / h] * 2)
    pid0 = gt[img][s][0]["phrase_id"]
    x, y = g.integers(0, w - 40, 70), g.integers(0, h - 40, 70)
    boxes[img][pid0] = np.stack([x, y, x + g.integers(8, 40, 70), y + g.integers(8, 40, 70)], 1).tolist()         # 70 ground truths
    target = np.asarray(boxes[img][pid0][69], dtype=np.float64)

    def many(n, phrase, hit_at):
        bb = np.stack([g.random(n) * w * 0.2, g.random(n) * h * 0.2, w * 0.2 + g.random(n) * 5, h * 0.2 + g.random(n) * 5], 1)
        ss = np.sort(np.floor(g.random(n) * 16) / 16 * 0.5)[::-1].copy()
        bb[hit_at] = target if phrase == 0 else np.asarray(boxes[img][gt[img][s][phrase]["phrase_id"]][0], dtype=np.float64)
        ss[hit_at] = ss.min() - 0.01                                                                               # the hit comes last: rank n
        return (bb * ratio).astype(np.float32), ss.astype(np.float32), np.full(n, phrase, dtype=np.int64)
    extra = [many(130, 0, 129)] + ([many(65, 1, 64)] if n_ph > 1 else [])
    preds[0] = (img, s, size, orig, n_ph, np.concatenate([e[0] for e in extra]), np.concatenate([e[1] for e in extra]), np.concatenate([e[2] for e in extra]))
    img2, s2 = preds[4][0], preds[4][1]
    pz = gt[img2][s2][0]["phrase_id"]
    boxes[img2][pz] = [[30, 40, 30, 90]] + boxes[img2][pz]                                                          # zero area: NaN with the dummy box
    return gt, boxes, preds


def check_random_case(device, plus=1):
    gt, boxes, preds = random_case()
    assert any(len(p[5]) >= 130 for p in preds) and any(len(b) == 70 for d in boxes.values() for b in d.values())
    ev = FlickrRecallEvaluator(gt, boxes, topk=(1, 5, 10, 64, 65, 100, -1), device=device)
    post = []
    for img, s, size, orig, n_ph, b, sc, ph in preds:
        ev.update_boxlist(img, s, boxlist(b, sc, ph + plus, size, device), n_ph, plus, orig)
        post.append(ref.post_process(img, s, b, sc, ph + plus, size, orig, n_ph, plus))
    score = ev.summarize()
    want = ref.evaluate(gt, boxes, post, topk=(1, 5, 10, 64, 65, 100, -1))
    assert list(score.items()) == list(want.items())
    assert 0 < score["Recall@1_all"] < score["Upper_bound_all"] <= 1
    assert max(ev.eval["phrase_dt"][:, 1].tolist()) >= 130 and max(ev.phrase_gt[:, 1].tolist()) == 70
    ties = sum(len(sc) - len(np.unique(sc)) for *_, sc, _ in preds)
    assert ties > 0
    # the same through the reference-style dicts
    ev2 = FlickrRecallEvaluator(gt, boxes, topk=(1, 5, 10, 64, 65, 100, -1), device=device)
    ev2.update(post)
    assert list(ev2.summarize().items()) == list(want.items())
    return ev


@needs_simt
def test_random_case_over_64_with_ties_matches_the_restatement(emu):
    check_random_case("cpu")


@needs_simt
def test_nan_rule_zero_area_ground_truth_against_the_dummy_box(emu):
    """a phrase whose ground truths are a zero-area box and a normal one, hit at rank 1 with two detections: the dummy box is entry 2, so
    Recall@1 and Recall@2 are hits, Recall@3 and the upper bound are NaN >= 0.5 -> misses"""
    gt = {"7": [[{"phrase_id": "1", "phrase_type": ["other"]}]]}
    boxes = {"7": {"1": [[10, 10, 10, 50], [100, 100, 200, 200]]}}
    ev = FlickrRecallEvaluator(gt, boxes, topk=(1, 2, 3, -1), device="cpu")
    bl = boxlist(np.array([[100, 100, 200, 200], [0, 0, 5, 5]], np.float32), np.array([0.9, 0.8], np.float32), np.array([0, 0]), (300, 300))
    ev.update_boxlist("7", 0, bl, 1, 0, (300, 300))
    score = ev.summarize()
    assert [score[f"{k}_all"] for k in ("Recall@1", "Recall@2", "Recall@3", "Upper_bound")] == [1.0, 1.0, 0.0, 0.0]
    post = [ref.post_process("7", 0, bl.bbox.numpy(), [0.9, 0.8], [0, 0], (300, 300), (300, 300), 1, 0)]
    assert ref.evaluate(gt, boxes, post, topk=(1, 2, 3, -1)) == score


# ---------------------------------------------------------------------------------------------------------------- rules and refusals
@needs_simt
def test_first_prediction_of_a_sentence_wins(emu):
    js, a = load_case("small")
    ev = from_fixture_gt(js)
    feed_raw(ev, js, a)
    for s in js["sentences"][:3]:                                                  # again, with boxes that hit nothing and a wrong length
        ev.update_boxlist(s["image_id"], s["sentence_id"], boxlist(np.zeros((2, 4), np.float32), np.array([0.5, 0.4], np.float32),
                                                                   np.array([1, 1]), s["size"]), 9, js["plus"], s["orig_size"])
    with pytest.warns(UserWarning, match="multiple predictions"):
        score = ev.summarize()
    check_score(score, js)
    assert ev.eval["flags"].tolist()[0] == 2                                       # sentence 2 of image 1001 is not evaluated: ignored, not a duplicate


@needs_simt
def test_refusals(emu):
    js, a = load_case("small")
    ev = from_fixture_gt(js)
    empty = boxlist(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), (10, 10))
    with pytest.raises(RuntimeError, match="Unknown image id"):
        ev.update_boxlist("999", 0, empty, 1, 1, (10, 10))
    with pytest.raises(RuntimeError, match="Unknown sentence id"):
        ev.update_boxlist("1001", 3, empty, 1, 1, (10, 10))
    with pytest.raises(RuntimeError, match="Unknown image id"):
        ev.update([{"image_id": 999, "sentence_id": 0, "boxes": [[[0.0, 0.0, 0.0, 0.0]]], "scores": [[]]}])
    with pytest.raises(RuntimeError, match="Unknown sentence id"):
        ev.update([{"image_id": 1001, "sentence_id": -1, "boxes": [[[0.0, 0.0, 0.0, 0.0]]], "scores": [[]]}])
    feed_raw(ev, js, a, which=set(range(len(js["sentences"]))) - {4})
    with pytest.raises(RuntimeError, match="Missing predictions: sentence 1 in image 1002"):
        ev.summarize()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev.update_boxlist("1002", 1, empty, 2, 1, (10, 10))                        # zero detections: evaluated all the same
        ev.update_boxlist("1001", 2, empty, 1, 1, (10, 10))                        # not evaluated: ignored silently
        score = ev.summarize()
    assert score["Upper_bound_all"] < dict(js["score"])["Upper_bound_all"]
    bad = from_fixture_gt(js)
    feed_raw(bad, js, a, which=set(range(len(js["sentences"]))) - {0})
    bad.update_boxlist("1001", 0, empty, 2, 1, (10, 10))                           # three phrases expected
    with pytest.raises(RuntimeError, match="number of phrase lists"):
        bad.summarize()
    bad = from_fixture_gt(js)
    feed_raw(bad, js, a, which=set(range(len(js["sentences"]))) - {0})
    bad.update_boxlist("1001", 0, boxlist(np.zeros((1, 4), np.float32), np.ones(1, np.float32), np.array([4]), (10, 10)), 3, 1, (10, 10))
    with pytest.raises(RuntimeError, match="phrase index outside"):
        bad.summarize()
    with pytest.raises(ValueError):
        FlickrRecallEvaluator(js["gt_sentences"], js["gt_boxes"], topk=(1, 0), device="cpu")


@needs_simt
def test_unexpected_predictions_in_dicts_warn_and_are_ignored(emu):
    js, _ = load_case("small")
    ev = from_fixture_gt(js)
    with pytest.warns(UserWarning, match="no predictions were expected"):
        ev.update(js["post"])
    check_score(ev.summarize(), js)


def test_write_results(tmp_path):
    js, _ = load_case("small")
    score = dict((k, v) for k, v in js["score"])
    path = tmp_path / "bbox.csv"
    FlickrRecallEvaluator.write_results(score, path)
    lines = path.read_text().split("\n")
    assert lines[0] == "metric, avg " and lines[1] == f"Recall@1_all, {score['Recall@1_all']} " and lines[-1] == "" and len(lines) == len(score) + 2


# ---------------------------------------------------------------------------------------------------------------- exchange
@needs_simt
def test_gloo_world2_exchange(emu):
    """two gloo ranks feed disjoint halves of the small fixture (rank 1 also repeats one of rank 0's sentences: dropped, rank order is arrival
    order); after synchronize_between_processes both summarize to the fixture's score"""
    with socket.socket() as s_:
        s_.bind(("127.0.0.1", 0))
        port = str(s_.getsockname()[1])
    script = os.path.join(HERE, "_gloo_flickr_worker.py")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", port, script], env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("FLICKR_GATHER_OK") == 2
