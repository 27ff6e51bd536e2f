#!/usr/bin/env python3
"""Write tests/golden/set_loss/cases.npz + cases.json: what the reference's own set criterion computes, executed in place on the CPU.

`HungarianMatcher` (groundingdino_new/models/GroundingDINO/matcher.py) and `SetCriterion` (loss.py) are compiled from where they lie
(oracle/_refload.py reference_classes; nothing is copied) with the reference's box_ops functions and focal-loss layers around them (box_area,
which box_ops takes from torchvision, is supplied here); SetCriterion's constructor is bypassed and the attributes it would set are set here
from the same classes.  Inputs are integer draws regenerated from a seed by tests/set_loss_cases.draw (bit-stable, checksummed): logits k / 8
with |k| <= 32 and -inf padding, boxes and gts in 1/1024 steps, the positive map from the same draws.  Stored per case: the cost matrix of every (layer,
image) exactly as the reference hands it to scipy (recorded at the call), the reference's indices per layer and all returned losses.

Condition on every stored matrix (asserted here in fp64 and again by the CPU test): the optimum is unique by a positive gap to the second-best
assignment (forbid each matched pair in turn, re-solve, take the minimum).  For `small` the gap is at least 2 G eps, eps = 1e-4 + 1e-4 max|C|:
a cost within the gate then provably yields the same indices.  A draw that misses is replaced as a whole (`--search` prints the first seed
that passes); no gt is ever dropped.

    python tools/gen_golden_set_loss.py          (needs the reference checkout and scipy; test infrastructure, never run on the GPU box)
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "set_loss", "cases")

import set_loss_cases as sc  # noqa: E402
import set_loss_ref as sr  # noqa: E402


def box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def reference(recorder):
    from oracle import _refload
    from scipy.optimize import linear_sum_assignment
    ns = _refload.load()
    focal = importlib.import_module("maskrcnn_benchmark.layers.sigmoid_focal_loss")
    import torch.nn.functional as F
    from torch import nn
    names = ["box_cxcywh_to_xyxy", "box_xyxy_to_cxcywh", "box_iou", "generalized_box_iou"]
    box = _refload.reference_classes("groundingdino_new/util/box_ops.py", [], names, extra_globals={"box_area": box_area})

    def lsa(c):
        recorder.append(c.clone())
        return linear_sum_assignment(c)
    Matcher = _refload.reference_classes("groundingdino_new/models/GroundingDINO/matcher.py", ["HungarianMatcher"],
                                         extra_globals={"nn": nn, "linear_sum_assignment": lsa, **box})["HungarianMatcher"]
    g = {"nn": nn, "F": F, "box_ops": types.SimpleNamespace(**box), "get_world_size": lambda: 1, "is_dist_avail_and_initialized": lambda: False,
         "TokenSigmoidFocalLoss": focal.TokenSigmoidFocalLoss}
    Criterion = _refload.reference_classes("groundingdino_new/models/GroundingDINO/loss.py", ["SetCriterion"], extra_globals=g)["SetCriterion"]
    return ns, focal, Matcher, Criterion


def main():
    search = "--search" in sys.argv
    recorder = []
    ns, focal, Matcher, Criterion = reference(recorder)
    BoxList = ns.bounding_box.BoxList
    arrays, meta = {}, {"t_full": sc.T_FULL, "coef": list(sc.COEF), "cost": list(sc.COST), "alpha": sc.ALPHA, "gamma": sc.GAMMA, "cases": {}}
    crit = Criterion.__new__(Criterion)
    torch.nn.Module.__init__(crit)
    crit.matcher = Matcher(cost_class=sc.COST[0], cost_bbox=sc.COST[1], cost_giou=sc.COST[2], focal_alpha=sc.ALPHA)
    crit.weight_dict = dict(zip(("loss_ce", "loss_bbox", "loss_giou"), sc.COEF))
    crit.losses = ["labels", "boxes"]
    crit.token_loss_func = focal.TokenSigmoidFocalLoss(sc.ALPHA, sc.GAMMA)
    for name, spec in sc.SPECS.items():
        seed = spec["seed"]
        while True:
            d = sc.draw(spec, seed)
            L, B, nq = d["logits"].shape[:3]
            targets = []
            off = 0
            for c in spec["counts"]:
                g = d["gt"][off:off + c]
                t = BoxList(sr.xyxy(g) * torch.tensor([[sc.SIZE[0], sc.SIZE[1]] * 2], dtype=torch.float32), sc.SIZE, mode="xyxy")
                t.add_field("normed_cxcy_boxes", g)
                targets.append(t)
                off += c
            full = d["logits_full"]                               # [L, B, nq, 256]: what the reference's head hands over
            outputs = {"pred_logits": full[-1], "pred_boxes": d["boxes"][-1],
                       "aux_outputs": [{"pred_logits": full[l], "pred_boxes": d["boxes"][l]} for l in range(L - 1)]}
            del recorder[:]
            losses, idx = crit(outputs, targets, return_indices=True, text_mask=d["mask_full"] > 0, positive_map=d["pm"])
            # the reference returns aux 0 .. L - 2, then the main output; it solved main first
            mats = recorder[B:] + recorder[:B]
            costs = [m.t().contiguous() for m in mats]            # gt-major [G_b, nq]
            gaps = [sr.gap_to_second_best(c.numpy(), sc.scipy_solve) for c in costs if len(c)]
            need = [0.0] * len(gaps)
            if spec.get("wide_gap"):
                need = [2 * len(c) * (1e-4 + 1e-4 * float(c.abs().max())) for c in costs if len(c)]
            ok = all(g_ > n_ for g_, n_ in zip(gaps, need))
            if ok or not search:
                break
            seed += 1000
        assert ok, (name, seed, min(gaps), "run with --search and put the seed it prints into set_loss_cases.SPECS")
        if seed != spec["seed"]:
            print(name, "first passing seed:", seed)
        assert len(idx) == L and all(len(i) == B for i in idx)
        flat = torch.cat([c.reshape(-1) for c in costs]) if costs else torch.zeros(0)
        match = np.concatenate([np.concatenate([sc.match_of(i, j, c) for (i, j), c in zip(idx[l], spec["counts"])]) for l in range(L)])
        arrays.update({f"{name}_cost": flat.numpy(), f"{name}_match": match.astype(np.int32)})
        meta["cases"][name] = {"seed": seed, "checksum": sc.checksum(d), "losses": {k: float(v) for k, v in losses.items()},
                               "min_gap": float(min(gaps)) if gaps else None}
        print(name, "seed", seed, "min gap", min(gaps) if gaps else None, "cost bytes", flat.numel() * 4,
              {k: round(float(v), 5) for k, v in losses.items()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes")


if __name__ == "__main__":
    main()
