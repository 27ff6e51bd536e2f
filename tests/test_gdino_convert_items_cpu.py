"""gdino_pipeline.convert (the dense class map of GroundingDINO.forward) against tests/golden/gdino_convert_items: what the reference's own
convert_groundingdino_to_glip_output returns for five items with their OWN positive maps, recorded in place by
tools/gen_golden_gdino_convert.py (label ids up to 1203, 1 .. 40 labels of 1 .. 5 tokens, a token listed twice, an item where nothing and one
where everything passes, a label with an empty token list, two image sizes, boxes across every border).

Bounds.  Every class score lies >= 1e-5 from the threshold and the best label leads the second by >= 1e-5 (asserted by the generator and
again here, on the data as loaded); an fp32 sum of at most 5 scores below 1 is off by at most about 5 * 2^-24 = 3e-7 whatever the order,
so no summation order can flip a decision: keep sets, labels, counts and order are compared exactly, no case left out.  Scores:
|d| <= MT * 2^-23 (MT = 5 roundings of the products by 1 / len and of the running sum on our side, as many in the reference's mean, each
<= 2^-24 for values below 1).  Boxes: the same fp32 operations in the same order -- bit-equal."""
import json
import os

import numpy as np
import torch

from mq_det_amd.modeling import gdino_pipeline as gp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gdino_convert_items")
MARGIN = 1e-5


def load_fixture():
    with open(GOLD + ".json") as f:
        meta = json.load(f)
    return meta, dict(np.load(GOLD + ".npz")), [{int(k): v for k, v in pm.items()} for pm in meta["positive_maps"]]


def assert_margins(prob, pms, thr):
    for i, pm in enumerate(pms):
        s = torch.stack([prob[i].double()[:, v].mean(-1) for v in pm.values() if len(v)], 1)
        assert bool(((s - thr).abs() >= MARGIN).all()), f"item {i}: a class score within {MARGIN} of the threshold"
        if s.shape[1] > 1:
            top = s.topk(2, dim=1)[0]
            assert bool(((top[:, 0] - top[:, 1]) >= MARGIN).all()), f"item {i}: two labels within {MARGIN} at the maximum"


def test_fixture_covers_what_it_says():
    meta, a, pms = load_fixture()
    assert a["prob"].shape == (5, 197, 256) and a["boxes"].shape == (5, 197, 4) and meta["num_classes"] == 1204 and meta["margin"] == MARGIN
    assert sorted(len(pm) for pm in pms) == [1, 10, 17, 23, 40] and max(max(pm) for pm in pms) == 1203
    lens = {len(v) for pm in pms for v in pm.values()}
    assert lens == {0, 1, 2, 3, 4, 5} and any(len(set(v)) < len(v) for pm in pms for v in pm.values())
    assert meta["counts"][1] == 0 and meta["counts"][2] == 197 and meta["counts"][3] == 0 and len({tuple(s) for s in meta["sizes_hw"]}) == 2
    b = torch.from_numpy(a["boxes"])
    x1, y1, x2, y2 = b[..., 0] - b[..., 2] / 2, b[..., 1] - b[..., 3] / 2, b[..., 0] + b[..., 2] / 2, b[..., 1] + b[..., 3] / 2
    assert all(bool((x1[i] < 0).any() and (y1[i] < 0).any() and (x2[i] > 1).any() and (y2[i] > 1).any()) for i in range(5))
    assert_margins(torch.from_numpy(a["prob"]).float(), pms, meta["threshold"])


def test_convert_equals_the_reference_item_by_item():
    meta, a, pms = load_fixture()
    prob, boxes = torch.from_numpy(a["prob"]).float(), torch.from_numpy(a["boxes"])
    thr, T, C = meta["threshold"], prob.shape[-1], meta["num_classes"] - 1
    assert_margins(prob, pms, thr)
    bound = 5 * 2.0 ** -23
    for i, pm in enumerate(pms):
        cmap, empty = torch.zeros(T, C), False
        for k, v in pm.items():
            if not v:
                empty = True
            for t in v:
                cmap[t, k - 1] += 1.0 / len(v)                              # a token listed twice counts twice
        packed, keep = gp.convert(prob[i:i + 1], boxes[i:i + 1], cmap, empty, torch.tensor([meta["sizes_hw"][i]], dtype=torch.float32), thr)
        packed, keep = packed[0], keep[0]
        assert torch.equal(keep, torch.from_numpy(a["keep"][i])), f"item {i}: keep set"
        assert int(keep.sum()) == meta["counts"][i]
        rows = packed[keep]                                                  # query order, as the reference's boolean mask
        assert torch.equal(rows[:, :4], torch.from_numpy(a[f"det_boxes{i}"])), f"item {i}: boxes differ from the reference's bits"
        assert torch.equal(rows[:, 5].long(), torch.from_numpy(a[f"det_labels{i}"])), f"item {i}: labels"
        if len(rows):
            assert float((rows[:, 4] - torch.from_numpy(a[f"det_scores{i}"])).abs().max()) <= bound
        assert bool((packed[~keep, 4] == -1).all())
