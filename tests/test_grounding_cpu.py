"""Phrase grounding without a GPU: the per-item token index / label table `forward_grounding` shares with `forward_chunks`, and
`mq_det_amd.grounding.evaluate_grounding` with a stand-in model (grouping, calls, updates, `plus` for both architectures)."""
import inspect
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

from mq_det_amd import grounding  # noqa: E402
from mq_det_amd.evaluation import FlickrRecallEvaluator  # noqa: E402,F401  (absent on the parent commit)
from mq_det_amd.modeling.detector import GeneralizedVLRCNN_New  # noqa: E402
from mq_det_amd.modeling.query_selector import build_item_token_index, build_token_index, prepare_positive_map  # noqa: E402
from mq_det_amd.structures import BoxList, ImageList  # noqa: E402

MAPS = [{1: [1, 2], 2: [4]}, {1: [1], 2: [3, 4, 5], 3: [7], 4: [9, 10], 5: [12]}, {1: [2], 2: [4, 5], 3: [8]}]


def test_forward_grounding_is_part_of_the_detector():
    sig = inspect.signature(GeneralizedVLRCNN_New.forward_grounding)
    assert list(sig.parameters) == ["self", "images", "captions", "positive_maps", "return_raw"]
    fwd = inspect.signature(GeneralizedVLRCNN_New.forward)
    assert list(fwd.parameters)[:7] == ["self", "images", "targets", "captions", "positive_map", "greenlight_map", "return_backbone_features"]


@pytest.mark.parametrize("onehot", [False, True])
def test_item_token_index_equals_the_per_item_tables_padded(onehot):
    prepared = [prepare_positive_map(pm, 256, 16, onehot) for pm in MAPS]
    tok3, lab2 = build_item_token_index([(p[3], p[4]) for p in prepared])
    assert tok3.dtype == lab2.dtype == torch.int32
    L, MT = (5, 1) if onehot else (5, 3)
    assert tuple(tok3.shape) == (3, L, MT) and tuple(lab2.shape) == (3, L)
    for i, p in enumerate(prepared):
        tok, lab = build_token_index(p[3], p[4], "cpu")
        n, m = tok.shape
        assert n == len(MAPS[i]) and torch.equal(tok3[i, :n, :m], tok) and torch.equal(lab2[i, :n], lab)
        assert (tok3[i, n:] == -1).all() and (tok3[i, :n, m:] == -1).all() and (lab2[i, n:] == 0).all()


def make_batches(n_items=5, batch=2):
    """targets as the Flickr loader builds them: caption, positive_map_eval [phrases, tokens], original_img_id, sentence_id, orig_size"""
    items = []
    for n in range(n_items):
        n_ph = 1 + n % 3
        pm = torch.zeros(n_ph, 16)
        for p in range(n_ph):
            pm[p, 1 + 2 * p:2 + 2 * p + (p % 2)] = 1
        t = BoxList(torch.zeros(0, 4), (40, 30), mode="xyxy")
        t.add_field("caption", f"caption number {n}")
        t.add_field("positive_map_eval", pm)
        t.add_field("original_img_id", 100 + n // 2)
        t.add_field("sentence_id", n % 2)
        t.add_field("orig_size", torch.tensor([60 + n, 80 + n]))
        items.append(t)
    out = []
    for b0 in range(0, n_items, batch):
        ts = items[b0:b0 + batch]
        out.append((ImageList(torch.full((len(ts), 3, 32, 32), float(b0)), [(30, 40)] * len(ts)), ts, list(range(b0, b0 + len(ts))), "extra"))
    return out, items


class Recorder:
    def __init__(self):
        self.updates, self.synced, self.written = [], 0, None

    def update_boxlist(self, image_id, sentence_id, boxlist, n_phrases, plus, orig_size):
        self.updates.append((image_id, sentence_id, boxlist, n_phrases, plus, orig_size))

    def synchronize_between_processes(self):
        self.synced += 1

    def summarize(self):
        assert self.synced == 1
        return {"Recall@1_all": 0.5}

    def write_results(self, score, path):
        self.written = (score, path)


def detections(caption, pm):
    bl = BoxList(torch.tensor([[1.0, 2.0, 3.0, 4.0]]) * len(caption), (40, 30), mode="xyxy")
    bl.add_field("labels", torch.tensor([max(pm)]))
    bl.add_field("scores", torch.tensor([0.5]))
    return bl


def stand_in(arch, batched):
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(RPN_ARCHITECTURE=arch))
    calls = []

    class Batched:
        def forward_grounding(self, images, captions, positive_maps):
            calls.append(("grounding", images.tensors.shape[0], list(captions), list(positive_maps)))
            return [detections(c, pm) for c, pm in zip(captions, positive_maps)]

    class PerItem:
        def __call__(self, images, captions=None, positive_map=None):
            calls.append(("forward", images.tensors.shape[0], list(captions), positive_map, images.image_sizes))
            return [detections(captions[0], positive_map)]
    m = Batched() if batched else PerItem()
    m.cfg = cfg
    return m, calls


@pytest.mark.parametrize("arch,plus", [("VLDYHEAD", 1), ("RPN", 0)])
@pytest.mark.parametrize("batched", [True, False])
def test_evaluate_grounding_groups_calls_and_updates(arch, plus, batched, tmp_path):
    batches, items = make_batches()
    model, calls = stand_in(arch, batched)
    ev = Recorder()
    out = tmp_path / "bbox.csv"
    score = grounding.evaluate_grounding(model, batches, ev, device="cpu", output_file=str(out))
    assert score == {"Recall@1_all": 0.5} and ev.written == (score, str(out))
    assert grounding.label_offset(model.cfg) == plus
    maps = [grounding.create_positive_map_label_to_token_from_positive_map(t.get_field("positive_map_eval"), plus) for t in items]
    assert maps[1] == {plus: [1], plus + 1: [3, 4]} and maps[2] == {plus: [1], plus + 1: [3, 4], plus + 2: [5]}
    if batched:                                                                    # one call per batch, of any size
        assert [(c[0], c[1]) for c in calls] == [("grounding", 2), ("grounding", 2), ("grounding", 1)]
        assert [cap for c in calls for cap in c[2]] == [t.get_field("caption") for t in items]
        assert [pm for c in calls for pm in c[3]] == maps
    else:                                                                          # MQ-GroundingDINO: one model(...) call per item
        assert [(c[0], c[1]) for c in calls] == [("forward", 1)] * 5
        assert [c[2] for c in calls] == [[t.get_field("caption")] for t in items] and [c[3] for c in calls] == maps
        assert all(c[4] == [(30, 40)] for c in calls)
    assert len(ev.updates) == 5
    for (img, sid, bl, n_ph, p, orig), t, pm in zip(ev.updates, items, maps):
        assert (img, sid, n_ph, p) == (t.get_field("original_img_id"), t.get_field("sentence_id"), len(pm), plus)
        assert torch.equal(orig, t.get_field("orig_size")) and int(bl.get_field("labels")[0]) == max(pm)
        assert torch.equal(bl.bbox, detections(t.get_field("caption"), pm).bbox)
