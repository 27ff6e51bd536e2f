#!/usr/bin/env python3
"""Write tests/golden/tta_special.npz + tta_special.json: what the reference's own merge returns with TEST.SPECIAL_NMS = 'soft-nms',
'vote' and 'soft-vote', executed in place.

maskrcnn_benchmark/data/datasets/evaluation/box_aug.py runs from where it lies (tools/gen_golden_tta.py load_box_aug): its
merge_result_from_multi_scales, boxlist_nms, bbox_vote and soft_bbox_vote are the reference's code.  Two stand-ins:
  * box_aug.soft_nms (_C.soft_nms, csrc/cpu/soft_nms.cpp, a compiled extension) is the numpy restatement tests/tta_special_ref.py soft_nms;
  * torch.Tensor.cuda is the identity while the reference runs (bbox_vote / soft_bbox_vote end in .cuda()).
Cases: every mode on the two images of tests/tta_special_cases.py (seven classes out of order, 147 detection slots each, about 130 rows left in the
original frame after the area band), without and with the top-N cut; and bbox_vote / soft_bbox_vote alone on the rows of one class.

    python tools/gen_golden_tta_special.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "tta_special")


def main():
    from gen_golden_tta import load_box_aug
    import tta_special_cases as sc
    import tta_special_ref as ref
    box_aug, _, bb, cfg = load_box_aug()

    def soft_nms(boxes, scores, thresh, sigma):
        keep, new, _ = ref.soft_nms(boxes.numpy(), scores.numpy(), thresh, sigma)
        return torch.from_numpy(keep), torch.from_numpy(new)
    box_aug.soft_nms = soft_nms
    warnings.simplefilter("ignore", DeprecationWarning)     # np.row_stack in the reference
    rows = []
    for bx, s, lb in sc.prep_restated(sc.build_dets(), sc.WH):
        ok = ~np.isnan(s)                                    # the device merge drops a NaN score; the reference never sees it
        rows.append((bx[ok], s[ok], lb[ok]))
    arrays, cases = {}, {}
    for b, (bx, s, lb) in enumerate(rows):
        arrays[f"in_boxes{b}"], arrays[f"in_scores{b}"], arrays[f"in_labels{b}"] = bx, s, lb.astype(np.int64)
    cfg.TEST.SELECT_CLASSES, cfg.TEST.NUM_CLASSES = tuple(sc.CLASSES), 81
    cfg.MODEL.RETINANET.INFERENCE_TH = sc.INFERENCE_TH
    saved_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for mode, lst in sc.CASES.items():
            for name, th, top_n in lst:
                if th <= 0:
                    continue
                cfg.TEST.SPECIAL_NMS, cfg.TEST.TH, cfg.TEST.PRE_NMS_TOP_N = mode, th, top_n
                bls = []
                for (bx, s, lb), wh in zip(rows, sc.WH):
                    bl = bb.BoxList(torch.from_numpy(bx.copy()), wh, mode="xyxy")
                    bl.add_field("scores", torch.from_numpy(s.copy()))
                    bl.add_field("labels", torch.from_numpy(lb.astype(np.int64)))
                    bls.append(bl)
                res = box_aug.merge_result_from_multi_scales(bls)
                key = f"{mode}_{name}"
                cases[key] = {"mode": mode, "TH": th, "PRE_NMS_TOP_N": top_n, "out_counts": [len(r) for r in res]}
                for b, r in enumerate(res):
                    assert r.bbox.dtype == torch.float32 and r.get_field("scores").dtype == torch.float32
                    arrays[f"{key}_boxes{b}"] = r.bbox.numpy()
                    arrays[f"{key}_scores{b}"] = r.get_field("scores").numpy()
                    arrays[f"{key}_labels{b}"] = r.get_field("labels").numpy()
        # the two votes alone, on the largest class of image 0
        bx, s, lb = rows[0]
        i = lb == sc.CLASSES[0]
        for fn, th in (("bbox_vote", 0.5), ("soft_bbox_vote", 0.5)):
            vb, vs = getattr(box_aug, fn)(torch.from_numpy(bx[i]), torch.from_numpy(s[i]), th)
            arrays[f"{fn}_boxes"], arrays[f"{fn}_scores"] = vb.numpy(), vs.numpy()
    finally:
        torch.Tensor.cuda = saved_cuda
    meta = {"classes": list(sc.CLASSES), "image_wh": [list(w) for w in sc.WH], "INFERENCE_TH": sc.INFERENCE_TH, "vote_class": sc.CLASSES[0],
            "vote_TH": 0.5, "seed": sc.SEED, "cases": cases, "numpy": np.__version__}
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, indent=None, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", {k: v["out_counts"] for k, v in cases.items()})


if __name__ == "__main__":
    main()
