#!/usr/bin/env python3
"""Write tests/golden/query_bank.npz + query_bank.json: what the reference's own bank-building code leaves in the bank, executed in place.

  * `GeneralizedVLRCNN_New.extract_query` (modeling/detector/generalized_vl_rcnn_new.py:232-288) runs from where it lies (oracle/_refload.py
    reference_classes) as an unbound method on a stub `self` with `visual_features` given; the stub's pooler returns the prepared candidate
    rows as [boxes, C, 1, 1] (or [5, boxes, C, 1, 1] without SELECT_FPN_LEVEL: the reference's mean over the bins is then the identity), so no
    native op is needed.  expand_bbox, the label concatenation and the admission loop are the reference's code.  Cases: repeated calls on a
    growing bank, exclusion on / off / alternating, the capacity reached in the middle of a call, duplicates inside one call, labels that are
    absent, five scales without exclusion; three row widths (256: the kernel's register path, 64: its 16-byte path, 5 x 30: its scalar path).
  * `online_update` (engine/inference.py:383-499) runs in place (reference_functions) for two turns at batch 1 on the stand-in model and data
    of tests/query_bank_ref.py; `model.extract_query` is the reference's method again.
The fixture stores the candidates and, per call, the bank as candidate indices per label (the generator asserts that the reference's rows are
those candidates bit for bit); for the online-update run the saved bank of every turn.

Condition (asserted here and again by the tests): every similarity the reference computes, recomputed in fp64, lies at least 1e-4 from the
threshold, so that a different summation order cannot flip a decision.

    python tools/gen_golden_query_bank.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import json
import os
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "query_bank")

import query_bank_ref as qr  # noqa: E402

CASES = {
    # name: (seed, S, C, maxq, labels, [(n candidates image 0, n candidates image 1, exclude)] per call)
    "sel_exclude": (3, 1, 256, 6, [1, 3, 4, 7, 12], [(14, 10, True), (9, 12, True), (16, 8, True), (6, 14, True)]),
    "sel_plain": (4, 1, 64, 5, [0, 2, 9], [(10, 9, False), (8, 12, False), (11, 7, False)]),
    "all_plain": (5, 5, 30, 4, [2, 5, 6], [(7, 6, False), (5, 8, False)]),
    "sel_mixed": (6, 1, 256, 8, [1, 2, 40], [(12, 8, False), (10, 12, True), (9, 9, False), (13, 10, True)]),
}


def reference():
    from oracle import _refload
    ns = _refload.load()
    import torch.nn.functional as F
    from torch import nn
    g = {"nn": nn, "F": F, "einsum": torch.einsum, "BoxList": ns.bounding_box.BoxList, "to_image_list": ns.image_list.to_image_list}
    cls = _refload.reference_classes("maskrcnn_benchmark/modeling/detector/generalized_vl_rcnn_new.py", ["GeneralizedVLRCNN_New"],
                                     ["expand_bbox"], extra_globals=g)["GeneralizedVLRCNN_New"]
    return _refload, ns, cls


def boxes_for(BoxList, n, labels, rng):
    """n boxes well inside a 640 x 480 image (expand_bbox keeps every one, in order)"""
    x1, y1 = rng.uniform(100, 300, n), rng.uniform(100, 200, n)
    bl = BoxList(torch.tensor(np.stack([x1, y1, x1 + rng.uniform(20, 90, n), y1 + rng.uniform(20, 90, n)], 1), dtype=torch.float32), (640, 480),
                 mode="xyxy")
    bl.add_field("labels", torch.from_numpy(labels))
    return bl


def main():
    _refload, ns, Ref = reference()
    BoxList = ns.bounding_box.BoxList
    arrays, meta = {}, {"cases": {}}
    for name, (seed, S, C, maxq, labels, calls) in CASES.items():
        cfg = _refload.reference_cfg()
        cfg.VISION_QUERY.SELECT_FPN_LEVEL = S == 1
        thr = float(cfg.VISION_QUERY.SIMILARITY_THRESHOLD)
        rng = np.random.default_rng(seed)
        stub = types.SimpleNamespace(cfg=cfg)
        bank = defaultdict(list)
        all_c, all_l, call_meta, banks = [], [], [], []
        for (n0, n1, exclude) in calls:
            cands, labs = qr.clustered(rng, n0 + n1, S, C, labels)
            prepared = torch.from_numpy(cands).permute(1, 0, 2)[..., None, None].contiguous()          # [S, boxes, C, 1, 1]
            stub.pooler = lambda feats, targets, p=prepared: p[0] if S == 1 else p
            targets = [boxes_for(BoxList, n0, labs[:n0], rng), boxes_for(BoxList, n1, labs[n0:], rng)]
            bank = Ref.extract_query(stub, targets=targets, query_images=bank, visual_features=[torch.zeros(1)] * 5, exclude_similar=exclude,
                                     device="cpu", max_query_number=maxq)
            lo = sum(len(c) for c in all_c)
            all_c.append(cands)
            all_l.append(labs)
            call_meta.append({"lo": lo, "hi": lo + n0 + n1, "split": lo + n0, "exclude": exclude, "maxq": maxq})
            banks.append({int(k): v.clone() for k, v in bank.items() if torch.is_tensor(v)})
        cands, labs = np.concatenate(all_c), np.concatenate(all_l)
        want, dmin, above, below = qr.replay(cands, labs, call_meta, thr)
        assert dmin >= qr.MARGIN, (name, dmin)
        assert not any(c["exclude"] for c in call_meta) or (above > 0 and below > 0), (name, above, below)
        full = False
        for w, got in zip(want, banks):                      # the reference's bank is the replay's, and its rows are the candidates bit for bit
            assert sorted(w) == sorted(got), (name, sorted(w), sorted(got))
            for l, ids in w.items():
                assert torch.equal(got[l], torch.from_numpy(cands[ids])), (name, l)
                full |= len(ids) == maxq
        assert full, name                                    # some label reached the capacity
        arrays[name + "_cands"], arrays[name + "_labels"] = cands, labs
        meta["cases"][name] = {"S": S, "C": C, "thr": thr, "calls": call_meta, "above": above, "below": below, "min_margin": dmin,
                               "banks": [{str(l): ids for l, ids in w.items()} for w in want]}
        print(name, "rows", len(cands), "comparisons above / below", above, below, "min margin %.3g" % dmin, "bank", {l: len(v) for l, v in want[-1].items()})

    # ---- online_update, two turns, batch 1
    cfg = _refload.reference_cfg()
    over = {"SCORE_THRESHOLD": 0.5, "MAX_TEST_QUERY_NUMBER": 7, "SELECT_FPN_LEVEL": True, "QUERY_BANK_PATH": ""}
    for k, v in over.items():
        cfg.VISION_QUERY[k] = v
    cfg.DATASETS.TEST = ("standin_val",)
    cfg.TEST.SUBSET, cfg.TEST.EVAL_TASK = 5, "detection"
    image_ids = [3, 8, 9, 21, 34, 55]                        # the last one is cut by TEST.SUBSET
    queries = ["chunk #%d" % c for c in range(qr.N_CHUNKS)]
    maps = [{1: [1], 2: [2], 3: [3]}] * qr.N_CHUNKS
    model = qr.StandInModel(cfg, BoxList, Ref.extract_query)
    saved = []
    real_save = torch.save

    def save(obj, path):
        saved.append({int(k): v.clone() for k, v in obj.items() if torch.is_tensor(v)})
        real_save(dict(saved[-1]), path)                     # (a plain dict: the weights-only unpickler cannot rebuild a defaultdict)
    fn = _refload.reference_functions("maskrcnn_benchmark/engine/inference.py", ["online_update"],
                                      {"tqdm": lambda x: x, "create_queries_and_maps_from_dataset": lambda *a, **k: (queries, maps)})["online_update"]
    with tempfile.TemporaryDirectory() as tmp:
        torch.save = save
        try:
            fn(model, qr.Loader(qr.loader(image_ids, 1)), device="cpu", cfg=cfg, num_turns=2, save_name=os.path.join(tmp, "bank.pth"))
        finally:
            torch.save = real_save
    assert len(saved) == 2 and len(model.loads) == 1 and model.loads[0][1] == sum(len(v) for v in saved[0].values()) > 0
    thr = float(cfg.VISION_QUERY.SIMILARITY_THRESHOLD)
    cands, banks, dmin, above, below = qr.log_replay(model.log, over["MAX_TEST_QUERY_NUMBER"], thr)
    assert dmin >= qr.MARGIN and above > 0 and below > 0, (dmin, above, below)
    for l, ids in banks[-1].items():
        assert torch.equal(saved[1][l], cands[ids]), l
    assert sum(len(v) for v in saved[1].values()) > sum(len(v) for v in saved[0].values()), [{l: len(v) for l, v in b.items()} for b in saved]
    for t, bank in enumerate(saved):
        for l, v in bank.items():
            arrays[f"online_turn{t}_label{l}"] = v.numpy()
    meta["online"] = {"cfg": over, "subset": 5, "image_ids": image_ids, "queries": queries, "maps": [{str(k): v for k, v in m.items()} for m in maps],
                      "thr": thr, "turns": [{str(l): len(v) for l, v in b.items()} for b in saved], "loaded_rows": model.loads[0][1],
                      "min_margin": dmin, "above": above, "below": below}
    print("online_update turns", meta["online"]["turns"], "comparisons above / below", above, below, "min margin %.3g" % dmin)
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes")


if __name__ == "__main__":
    main()
