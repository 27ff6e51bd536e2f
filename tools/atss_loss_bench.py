#!/usr/bin/env python3
"""Time of the forward-only ATSS objective on one MI355X: MQ-GLIP-T (bench.py's synthetic-weight model, 5-shot vision queries, the
40-class caption) at B = 8, 800 x 1333, with about 10 and about 100 gt boxes per image.

  * `ATSSLoss` alone on a head the model produced once (assignment + box terms + token focal loss; with the fused head operands this
    includes the one mq_align_fused_fwd launch that yields the box / centerness rows),
  * the BASELINE on the same device and the same head outputs: the from-scratch torch restatement of tests/atss_loss_ref.py -- a per-image
    loop over dense [A, G] matrices and the materialised [B, A, T] fp32 logits (which are produced before the clock starts, as the
    reference's head has written them anyway),
  * `forward_losses` as a whole, new pixels every call.

The two loss paths run in the same process, alternating, `--reps` timed calls each after `--warmup` untimed ones; each call ends in a
device synchronise; medians and min / max are reported, the peak device memory of one call of each (over what is allocated before it), and
the device->host synchronisations of one call of each counted under torch's sync debug mode.  The structural claim to verify: the device path
allocates less than one [B, A, T] fp32 tensor and waits for the device zero times per call.  One JSON line per gt count.

    python tools/atss_loss_bench.py [--reps 20] [--warmup 3] [--gts 10,100]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def make_targets(n_gt, B, hw, pm, t_full, seed):
    """B images of about n_gt boxes (n_gt - 2 .. n_gt + 2) with labels of the caption's positive map `pm` and their positive-map rows"""
    import atss_loss_ref as ar
    from mq_det_amd.structures import BoxList
    rng = np.random.default_rng(seed)
    labels_all = sorted(pm)
    H, W = hw
    targets, rows = [], []
    for b in range(B):
        n = max(1, n_gt + int(rng.integers(-2, 3)))
        t = BoxList(torch.from_numpy(ar.draw_boxes(rng, n, W, H, lo=16.0, hi=0.5)), (W, H), mode="xyxy")
        lab = rng.choice(labels_all, n)
        t.add_field("labels", torch.from_numpy(lab.astype(np.int64)))
        r = torch.zeros(n, t_full)
        for j, l in enumerate(lab.tolist()):
            r[j, pm[l]] = 1.0 / len(pm[l])
        targets.append(t)
        rows.append(r)
    return targets, torch.cat(rows), rows


def count_syncs(fn):
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
            return sum("synchroniz" in str(w.message) for w in caught)
    finally:
        torch.cuda.set_sync_debug_mode("default")


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def measure(args):
    if not torch.cuda.is_available():
        raise SystemExit("atss_loss_bench needs a GPU: a time taken elsewhere says nothing")
    import atss_loss_ref as ar
    import bench
    from mq_det_amd import losses, ops
    from mq_det_amd.structures import ImageList
    dev = torch.device("cuda:0")
    cfg, model, chunks = bench.build_model(dev)
    caption, pm = chunks[0]
    B = args.batch
    H, W = bench.IMG_HW
    Hp, Wp = -(-H // 32) * 32, -(-W // 32) * 32
    g = torch.Generator().manual_seed(0)
    pixels = torch.zeros(B, 3, Hp, Wp)
    pixels[:, :, :H, :W] = torch.randn(B, 3, H, W, generator=g)
    pixels = pixels.to(dev)
    t_full = cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN
    lines = []
    for n_gt in args.gts:
        targets, pmt, rows = make_targets(n_gt, B, (H, W), pm, t_full, seed=n_gt)
        images = lambda: ImageList(pixels.clone(), [(H, W)] * B)         # noqa: E731 -- new pixels every call (the clone is the "data loader")
        captured = {}
        real_call = losses.ATSSLoss.__call__

        def capture(self, head, anchors, tg, pmap, masks):
            captured.update(head=head, anchors=anchors, targets=tg, pm=pmap, masks=masks, crit=self)
            return real_call(self, head, anchors, tg, pmap, masks)
        losses.ATSSLoss.__call__ = capture
        try:
            whole = model.forward_losses(images(), targets, [caption] * B, positive_map=pmt)
        finally:
            losses.ATSSLoss.__call__ = real_call
        head, anchors, crit, masks = captured["head"], captured["anchors"], captured["crit"], captured["masks"]
        if "tok" not in head:
            raise SystemExit("the model handed over the GEMM-fallback head: nothing to measure")
        pm_dev = pmt.to(dev)
        ours = lambda: crit(head, anchors, targets, pm_dev, masks)      # noqa: E731
        # the baseline's inputs, materialised before its clock starts
        A, T = head["tok"].shape[1], head["tbias"].shape[1]
        tokidx = torch.zeros(1, 1, dtype=torch.int32, device=dev)
        fused = ops.align_fused(head["tok"], head["tk16"], head["tbias"], head["wbc"], head["bbc"], head["scales"], tokidx, head["sizes"], 2.0,
                                kv_max=head.get("max_kv", 0), want_logits=True)
        reg, ctr = torch.cat(fused["reg"], 1).contiguous(), fused["ctr"]
        logits = (fused["logits"] + head["tbias"][:, None, :]).clamp(-50000, 50000)
        del fused
        gts = [t.bbox.to(dev) for t in targets]
        labs = [t.get_field("labels").to(dev) for t in targets]
        pms = [r.to(dev) for r in rows]
        levels = [a.float() for a in anchors]
        mask_t = masks[:, :T]
        base = lambda: ar.losses_ref(levels, gts, labs, pms, reg, ctr, logits, mask_t, crit.alpha, crit.gamma, topk=crit.topk,      # noqa: E731
                                     reg_weight=crit.reg_weight, token_weight=crit.token_weight)
        fwd = lambda: model.forward_losses(images(), targets, [caption] * B, positive_map=pmt)      # noqa: E731
        t_ours, t_base, t_fwd = [], [], []
        for rep in range(args.warmup + args.reps):
            order = (("ours", ours, t_ours), ("base", base, t_base)) if rep % 2 == 0 else (("base", base, t_base), ("ours", ours, t_ours))
            for _, fn, sink in order:
                ms, out = timed(fn)
                if rep >= args.warmup:
                    sink.append(ms)
            ms, _ = timed(fwd)
            if rep >= args.warmup:
                t_fwd.append(ms)
        o, r = ours(), base()
        same = bool(all(torch.equal(o["matched"][b].long(), r["matched"][b]) for b in range(B)))
        rel = {k: abs(float(o[k]) - r[k]) / abs(r[k]) for k in ("loss_reg", "loss_centerness", "loss_dot_product_token")}
        line = {"gts_per_image": n_gt, "batch": B, "canvas": [H, W], "anchors": A, "text_positions": T, "num_pos": r["num_pos"],
                "reps": args.reps, "atss_loss": stats(t_ours), "torch_restatement": stats(t_base), "forward_losses": stats(t_fwd),
                "ratio_restatement_over_atss_loss": round(statistics.median(t_base) / statistics.median(t_ours), 2),
                "peak_bytes": {"atss_loss": peak_bytes(ours), "torch_restatement": peak_bytes(base), "forward_losses": peak_bytes(fwd),
                               "one_BAT_fp32_tensor": B * A * T * 4, "restatement_inputs_materialised_before_its_clock": logits.numel() * 4},
                "host_syncs_per_call": {"atss_loss": count_syncs(ours), "torch_restatement": count_syncs(base), "forward_losses": count_syncs(fwd)},
                "assignment_equal": same, "loss_rel_diff": {k: float("%.3g" % v) for k, v in rel.items()},
                "whole_losses": {k: round(float(whole[k]), 6) for k in ("loss_reg", "loss_centerness", "loss_dot_product_token")}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--gts", type=lambda s: [int(v) for v in s.split(",")], default=[10, 100])
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
