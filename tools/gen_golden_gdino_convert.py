#!/usr/bin/env python3
"""Write tests/golden/gdino_convert_items.npz + .json: what the reference's own MQ-GroundingDINO output conversion returns for stacked
(chunk, image) items with their own positive maps, executed in place (oracle/_refload.py shells).

Runs GroundingDINO.convert_groundingdino_to_glip_output (groundingdino.py:291-335) -- and through it convert_grounding_to_od_logits
(rpn/inference.py:772-792, "MEAN"), BoxList.clip_to_image and remove_small_boxes -- once per item on a stub `self` that carries
cfg.MODEL.DYHEAD.NUM_CLASSES = 1204 and box_threshold; the kept query indices come from the same convert_grounding_to_od_logits call the
method makes.  Only the inputs and the recorded outputs are stored.  (tests/golden/gdino_convert.npz is the older single-map fixture of
oracle/gen_golden_gdino.py; this one has its own name.)

Items (I = 5, nq = 197, T = 256): 40 labels up to id 1203 with 1..5 tokens, one list with a repeated token; one label where nothing
passes; 17 labels where every query passes; a label with an empty token list (the NaN quirk: nothing passes); two image sizes; boxes that
cross every border.  Conditions asserted here and again by tests/test_gdino_convert_items_cpu.py: every class score is >= MARGIN from
box_threshold, and the best label of a query leads the second best by >= MARGIN.

    python tools/gen_golden_gdino_convert.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "gdino_convert_items")
I, NQ, T, LIVE = 5, 197, 256, 200                         # token positions LIVE .. T - 1 are padding: score 0
THR, MARGIN = 0.25, 1e-5
SIZES = [(480, 640), (333, 500), (480, 640), (333, 500), (480, 640)]          # (height, width)


def token_lists(rng, n, force_repeat=False):
    out = []
    for j in range(n):
        k = 1 + j % 5 if j < 5 else int(rng.integers(1, 6))                   # every length 1..5 appears
        out.append([int(t) for t in rng.choice(LIVE, size=k, replace=False)])
    if force_repeat:
        out[2] = [out[2][0], out[2][1], out[2][0]]                             # a token listed twice counts twice
    return out


def class_scores64(prob, pm):
    """[nq, L] float64 class scores of one item (labels in sorted order); an empty list gives NaN"""
    labs = sorted(pm)
    p = prob.double()
    return labs, torch.stack([p[:, pm[l]].mean(-1) if pm[l] else torch.full((p.shape[0],), float("nan"), dtype=torch.float64) for l in labs], 1)


def margins_ok(prob, pm):
    """per query: every score MARGIN away from THR, the best label MARGIN ahead of the second"""
    _, s = class_scores64(prob, {k: v for k, v in pm.items() if v})
    ok = ((s - THR).abs() >= MARGIN).all(1)
    if s.shape[1] > 1:
        top = s.topk(2, dim=1)[0]
        ok &= (top[:, 0] - top[:, 1]) >= MARGIN
    return ok


def main():
    from oracle import _refload
    g = _refload.load_gdino()
    ns = g.base
    gd = g.groundingdino
    rng = np.random.default_rng(20)
    gen = torch.Generator().manual_seed(20)
    n_labels = [40, 1, 17, 9, 23]
    shift = [-4.0, -10.0, 3.0, -1.0, -3.5]                                      # item 1: nothing passes; item 2: everything passes
    maps = []
    for i, n in enumerate(n_labels):
        ids = rng.choice(np.arange(1, 1204), size=n, replace=False)
        if i == 0:
            ids[0], ids[1] = 1203, 1                                          # the ends of the label range
        ids = sorted(int(x) for x in set(ids.tolist()))
        while len(ids) < n:
            c = int(rng.integers(2, 1203))
            if c not in ids:
                ids = sorted(ids + [c])
        maps.append(dict(zip(ids, token_lists(rng, n, force_repeat=(i == 0)))))
    maps[3][int(max(maps[3]) + 1)] = []                                        # the empty token list
    prob = torch.zeros(I, NQ, T)
    for i in range(I):
        for _ in range(50):
            bad = ~margins_ok(prob[i], maps[i]) if prob[i].any() else torch.ones(NQ, dtype=torch.bool)
            if not bad.any():
                break
            fresh = torch.sigmoid(torch.randn(int(bad.sum()), LIVE, generator=gen) * 2.0 + shift[i])
            prob[i, bad, :LIVE] = fresh.half().float()                         # fp16-representable: stored as fp16
        assert margins_ok(prob[i], maps[i]).all(), i
    # boxes: centres beyond every border, sizes up to 0.8 -- each of the four borders is crossed in every item, some boxes lie outside
    cxcy = torch.rand(I, NQ, 2, generator=gen) * 1.3 - 0.15
    wh = torch.rand(I, NQ, 2, generator=gen) * 0.8
    boxes = torch.cat([cxcy, wh], -1)
    x1, y1, x2, y2 = (cxcy[..., 0] - wh[..., 0] / 2, cxcy[..., 1] - wh[..., 1] / 2, cxcy[..., 0] + wh[..., 0] / 2, cxcy[..., 1] + wh[..., 1] / 2)
    for i in range(I):
        assert (x1[i] < 0).any() and (y1[i] < 0).any() and (x2[i] > 1).any() and (y2[i] > 1).any()

    stub = types.SimpleNamespace(cfg=_refload.CfgNode({"MODEL": {"DYHEAD": {"NUM_CLASSES": 1204}}}), box_threshold=THR)
    convert = gd.GroundingDINO.convert_groundingdino_to_glip_output
    arrays = {"prob": prob.half().numpy(), "boxes": boxes.numpy()}
    assert torch.equal(prob.half().float(), prob)
    counts, keep = [], torch.zeros(I, NQ, dtype=torch.bool)
    for i in range(I):
        out = {"pred_logits": prob[i:i + 1], "pred_boxes": boxes[i:i + 1]}
        res = convert(stub, out, maps[i], [SIZES[i]])[0]
        assert isinstance(res, ns.bounding_box.BoxList)
        sc = ns.inference.convert_grounding_to_od_logits(logits=prob[i:i + 1], box_cls=prob.new_zeros(1, NQ, 1203), positive_map=maps[i],
                                                         score_agg="MEAN")
        keep[i] = sc.max(-1)[0][0] > THR
        assert int(keep[i].sum()) == len(res)
        counts.append(len(res))
        arrays[f"det_boxes{i}"] = res.bbox.numpy()
        arrays[f"det_scores{i}"] = res.get_field("scores").numpy()
        arrays[f"det_labels{i}"] = res.get_field("labels").numpy().astype(np.int64)
    arrays["keep"] = keep.numpy()
    assert counts[1] == 0 and counts[2] == NQ and counts[3] == 0 and 0 < counts[0] < NQ and 0 < counts[4] < NQ, counts
    meta = {"threshold": THR, "margin": MARGIN, "num_classes": 1204, "live_tokens": LIVE, "sizes_hw": [list(s) for s in SIZES], "counts": counts,
            "positive_maps": [{str(k): v for k, v in m.items()} for m in maps]}
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", counts, os.path.getsize(OUT + ".npz"))


if __name__ == "__main__":
    main()
