#!/usr/bin/env python3
"""Write tests/golden/atss_loss/cases.npz + cases.json: what the reference's own ATSS loss code computes, executed in place on the CPU.

`ATSSLossComputation` (maskrcnn_benchmark/modeling/rpn/loss.py:520-1201) is compiled from where it lies (oracle/_refload.py
reference_classes; nothing is copied) with the reference's own BoxCoder, boxlist_iou, cat_boxlist, concat_box_prediction_layers, focal-loss
layers, comm helpers and AnchorGenerator around it; its constructor (which downloads a tokenizer) is bypassed and the attributes it would set
are set here from the same classes.  Per case `prepare_targets` and `__call__` run on gt boxes drawn by tests/atss_loss_ref.draw_boxes and on
head outputs regenerated from integer draws (atss_loss_ref.head_draws: bit-stable, checksummed).  Stored per case: gt boxes and labels (unique
inside an image, so the matched gt of an anchor can be read off the reference's class labels), the sparse positive map, text masks, cell
anchors, level sizes, seeds, and the reference's matched indices, labels, regression targets, token-label rows (asserted here to be exactly the
positive-map row of the matched gt, or the background row), the seven returned losses and num_pos.

Conditions (asserted here in fp64 and again by the tests): per (gt, level) the k-th and (k+1)-th smallest centre distances differ by >= 1e-3
px; every candidate IoU is >= 1e-5 from its gt's threshold; every candidate's centre margin is >= 1e-3 from 0.01; the two best IoUs of an
anchor claimed twice differ by >= 1e-6.  The box seeds below meet all four with EVERY drawn gt kept: a seed that misses a condition is
replaced as a whole (`--search` prints the first seed that passes), no gt is ever dropped from a draw.

    python tools/gen_golden_atss_loss.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "atss_loss", "cases")

import atss_loss_ref as ar  # noqa: E402

CANVAS = (160, 224)                                          # levels 20x28, 10x14, 5x7, 3x4 (12 anchors), 2x2 (fewer than TOPK)
T_FULL = 256
CASES = {
    # name: box seed, head seed, gts per image, live text tokens, TOKEN_ALPHA, one tiny gt in image 0
    "main": dict(seed=1, head=101, counts=(1, 7, 40), live=40, alpha=0.25, tiny=False),
    "tiny": dict(seed=2, head=102, counts=(3, 2), live=24, alpha=0.25, tiny=True),
    "full": dict(seed=3, head=103, counts=(2, 5), live=256, alpha=0.25, tiny=False),
    "alpha_neg": dict(seed=4, head=104, counts=(4, 3), live=33, alpha=-1.0, tiny=False),
}


def draw_case(spec, seed):
    rng = np.random.default_rng(seed)
    H, W = CANVAS
    gts, labels, pms = [], [], []
    for b, n in enumerate(spec["counts"]):
        cluster = (0.45 * W, 0.5 * H, 9.0) if n >= 30 else None          # the 40: heavy overlap
        box = ar.draw_boxes(rng, n, W, H, cluster=cluster) if cluster is None else ar.draw_boxes(rng, n, W, H, lo=30.0, hi=0.6, cluster=cluster)
        if spec["tiny"] and b == 0:
            cx, cy = 100.37, 71.61                                        # 0.015 px wide: no anchor centre can lie inside by more than 0.01
            box[0] = [cx, cy, cx + 0.015, cy + 0.015]
        gts.append(box)
        labels.append((rng.permutation(n) + 1 + 7 * b).astype(np.int64))   # unique inside the image
        pm = np.zeros((n, T_FULL), dtype=np.float32)
        for j in range(n):
            span = int(rng.integers(1, 4))
            start = int(rng.integers(1, max(2, spec["live"] - span)))
            pm[j, start:start + span] = np.float32(1.0 / span)
        pms.append(pm)
    return gts, labels, pms


def reference():
    from oracle import _refload
    ns = _refload.load()
    imp = importlib.import_module
    focal = imp("maskrcnn_benchmark.layers.sigmoid_focal_loss")
    comm = imp("maskrcnn_benchmark.utils.comm")
    amp = imp("maskrcnn_benchmark.utils.amp")
    utils = sys.modules["maskrcnn_benchmark.modeling.utils"]
    coder = sys.modules["maskrcnn_benchmark.modeling.box_coder"]
    import torch.nn.functional as F
    from torch import nn
    g = {"nn": nn, "F": F, "boxlist_iou": ns.boxlist_ops.boxlist_iou, "cat_boxlist": ns.boxlist_ops.cat_boxlist,
         "concat_box_prediction_layers": utils.concat_box_prediction_layers, "get_world_size": comm.get_world_size, "reduce_sum": comm.reduce_sum,
         "custom_fwd": amp.custom_fwd, "custom_bwd": amp.custom_bwd, "INF": 1e8, "SigmoidFocalLoss": focal.SigmoidFocalLoss,
         "TokenSigmoidFocalLoss": focal.TokenSigmoidFocalLoss}
    cls = _refload.reference_classes("maskrcnn_benchmark/modeling/rpn/loss.py", ["ATSSLossComputation"], extra_globals=g)["ATSSLossComputation"]
    return _refload, ns, cls, focal, coder


def build_loss(_refload, Loss, focal, coder, alpha):
    cfg = _refload.reference_cfg("configs/pretrain/mq-glip-t.yaml")
    fc = cfg.MODEL.DYHEAD.FUSE_CONFIG
    fc.TOKEN_ALPHA = alpha
    assert fc.USE_DOT_PRODUCT_TOKEN_LOSS and not (fc.USE_TOKEN_LOSS or fc.USE_CONTRASTIVE_ALIGN_LOSS or fc.USE_CLASSIFICATION_LOSS
                                                  or fc.USE_SHALLOW_CONTRASTIVE_LOSS or fc.USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS or fc.MLM_LOSS)
    assert tuple(cfg.MODEL.RPN.ASPECT_RATIOS) == (1.0,) and cfg.MODEL.RPN.SCALES_PER_OCTAVE == 1 and cfg.MODEL.ATSS.TOPK == 9
    loss = Loss.__new__(Loss)
    torch.nn.Module.__init__(loss)
    loss.cfg = cfg                                            # what ATSSLossComputation.__init__ sets, minus the tokenizer download
    loss.cls_loss_func = focal.SigmoidFocalLoss(cfg.MODEL.FOCAL.LOSS_GAMMA, cfg.MODEL.FOCAL.LOSS_ALPHA)
    loss.centerness_loss_func = torch.nn.BCEWithLogitsLoss(reduction="sum")
    loss.box_coder = coder.BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
    loss.token_loss_func = focal.TokenSigmoidFocalLoss(fc.TOKEN_ALPHA, fc.TOKEN_GAMMA)
    return cfg, loss


def main():
    search = "--search" in sys.argv
    _refload, ns, Loss, focal, coder = reference()
    BoxList = ns.bounding_box.BoxList
    H, W = CANVAS
    sizes = ar.level_sizes(H, W)
    arrays, meta = {}, {"canvas": list(CANVAS), "sizes": [list(s) for s in sizes], "t_full": T_FULL, "cases": {}}
    for name, spec in CASES.items():
        cfg, loss = build_loss(_refload, Loss, focal, coder, spec["alpha"])
        B = len(spec["counts"])
        gen = ns.anchor_generator.make_anchor_generator_complex(cfg)
        images = ns.image_list.ImageList(torch.zeros(B, 3, H, W), [(H, W)] * B)
        anchors = gen(images, [torch.zeros(B, 1, h, w) for (h, w) in sizes])
        levels = [a.bbox.clone() for a in anchors[0]]
        cells = torch.stack([l[0] for l in levels])            # the anchor of location (0, 0) per level
        mine = ar.grid_anchors(sizes, cells)
        assert all(torch.equal(a, b) for a, b in zip(levels, mine)) and torch.equal(cells, ar.cell_anchors())
        seed = spec["seed"]
        while True:
            gts, labels, pms = draw_case(spec, seed)
            ok, worst = ar.conditions_hold(levels, [torch.from_numpy(g) for g in gts], cfg.MODEL.ATSS.TOPK)
            if ok or not search:
                break
            seed += 1000
        assert ok, (name, seed, worst, "run with --search and put the seed it prints into CASES")
        if seed != spec["seed"]:
            print(name, "first passing box seed:", seed)
        A = sum(h * w for h, w in sizes)
        draws = ar.head_draws(spec["head"], B, A, T_FULL)
        mask = np.zeros((B, T_FULL), dtype=np.int64)
        mask[:, :spec["live"]] = 1
        targets = []
        for g, l in zip(gts, labels):
            t = BoxList(torch.from_numpy(g), (W, H), mode="xyxy")
            t.add_field("labels", torch.from_numpy(l))
            targets.append(t)
        pm = torch.from_numpy(np.concatenate(pms))
        cls_l, reg_t, tok_l, _, _, _, _ = loss.prepare_targets(targets, anchors, None, pm, None)
        # matched gt per anchor from the (unique) labels; the reference's other outputs must be consistent with it
        matched = np.full((B, A), -1, dtype=np.int32)
        flat = torch.cat(levels)
        for b in range(B):
            lab = torch.from_numpy(labels[b])
            eq = cls_l[b][:, None] == lab[None]
            assert bool(((eq.sum(1) == 1) == (cls_l[b] > 0)).all())
            m = torch.where(cls_l[b] > 0, eq.int().argmax(1), torch.full_like(cls_l[b], -1))
            matched[b] = m.numpy()
            gtb, pmb = torch.from_numpy(gts[b]), torch.from_numpy(pms[b])
            assert torch.equal(reg_t[b], loss.box_coder.encode(gtb[m.clamp(min=0)], flat))
            want = pmb[m.clamp(min=0)].clone()
            bg = torch.zeros(T_FULL)
            bg[-1] = 1
            want[m < 0] = bg
            assert torch.equal(tok_l[b], want), name
            mine_m = ar.assign_image(levels, gtb, cfg.MODEL.ATSS.TOPK)
            assert torch.equal(mine_m, m), (name, b, "the restatement and the reference disagree")
        lo = 0
        box_cls, box_reg, ctr, dots = [], [], [], []
        logits = ar.logits_of(torch.from_numpy(draws["tok"]), torch.from_numpy(draws["tk"]), torch.from_numpy(draws["tbias"]), torch.float32)
        for (h, w) in sizes:
            n = h * w
            box_reg.append(torch.from_numpy(draws["reg"][:, lo:lo + n]).reshape(B, h, w, 4).permute(0, 3, 1, 2).contiguous())
            ctr.append(torch.from_numpy(draws["ctr"][:, lo:lo + n]).reshape(B, h, w, 1).permute(0, 3, 1, 2).contiguous())
            box_cls.append(torch.from_numpy(draws["cls"][:, lo:lo + n]).reshape(B, h, w, 1).permute(0, 3, 1, 2).contiguous())
            dots.append(logits[:, lo:lo + n].contiguous())
            lo += n
        out = loss(box_cls, box_reg, ctr, targets, anchors, captions=None, positive_map=pm, dot_product_logits=dots,
                   text_masks=torch.from_numpy(mask))
        names = ("loss_cls", "loss_reg", "loss_centerness", "loss_token", "loss_contrastive_align", "loss_dot_product_token", "loss_shallow_contrastive")
        losses = {k: (None if v is None else float(v)) for k, v in zip(names, out)}
        num_pos = int(sum(int((c > 0).sum()) for c in cls_l))
        claimed = 0
        for b in range(B):                                       # how many anchors several gts claim (the 40-gt image: many)
            _, mg = ar.assign_image([l.double() for l in levels], torch.from_numpy(gts[b]).double(), 9, torch.float64, want_margins=True)
            claimed += mg["tie"] != float("inf")
        if spec["tiny"]:
            assert not (matched[0] == 0).any() and (matched[0] >= 0).any()
        if name == "main":
            assert claimed > 0
        rows, cols = np.nonzero(np.concatenate(pms))
        arrays.update({f"{name}_gt": np.concatenate(gts), f"{name}_labels": np.concatenate(labels),
                       f"{name}_pm_idx": np.stack([rows, cols], 1).astype(np.int32), f"{name}_pm_val": np.concatenate(pms)[rows, cols],
                       f"{name}_mask": mask.astype(np.uint8), f"{name}_cells": cells.numpy(), f"{name}_matched": matched,
                       f"{name}_cls": torch.stack(cls_l).numpy().astype(np.int32), f"{name}_reg": torch.stack(reg_t).numpy()})
        meta["cases"][name] = {"counts": list(spec["counts"]), "box_seed": seed, "head_seed": spec["head"], "live": spec["live"],
                               "alpha": spec["alpha"], "gamma": float(cfg.MODEL.DYHEAD.FUSE_CONFIG.TOKEN_GAMMA), "topk": int(cfg.MODEL.ATSS.TOPK),
                               "reg_weight": float(cfg.MODEL.ATSS.REG_LOSS_WEIGHT), "checksum": ar.checksum(draws), "losses": losses,
                               "num_pos": num_pos, "margins": worst}
        print(name, "num_pos", num_pos, "losses", {k: v for k, v in losses.items() if v is not None}, "margins", worst)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes")


if __name__ == "__main__":
    main()
