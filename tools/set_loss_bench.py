#!/usr/bin/env python3
"""Time the set criterion of MQ-GroundingDINO at B = 8, nq = 900, L = 6: the device path (mq_set_cost_fwd + mq_hungarian_fwd + mq_set_loss_fwd
per step, no host synchronisation inside) against the reference-shaped path on the same machine (the torch cost on the device, `.cpu()`, a host
solve per image, once per layer).  ~10 and ~100 gts per image, spread and clustered (clustered gts compete for the same queries: longer
augmenting paths).  One warm-up, three repeats, wall and device-event times; one line per measurement.

    python tools/set_loss_bench.py            (needs the GPU)
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import set_loss_ref as sr  # noqa: E402
from mq_det_amd import ops  # noqa: E402

L, B, NQ, T, LIVE = 6, 8, 900, 256, 120
COST = dict(cost_class=1.0, cost_bbox=5.0, cost_giou=2.0, focal_alpha=0.25)

try:
    from scipy.optimize import linear_sum_assignment as _lsa
    SOLVER = "scipy"

    def host_solve(c):
        return _lsa(c)[1]
except ImportError:
    SOLVER = "restatement (tests/set_loss_ref.lsap)"
    host_solve = sr.lsap


def draw(per_image, clustered, seed, dev):
    rng = np.random.default_rng(seed)
    logits = torch.full((L, B, NQ, T), -float("inf"))
    logits[..., :LIVE] = torch.from_numpy(rng.integers(-32, 33, (L, B, NQ, LIVE)) / 8.0).float()
    c = rng.uniform(0.2, 0.8, (L, B, NQ, 2))
    boxes = torch.from_numpy(np.concatenate([c, rng.uniform(0.05, 0.4, (L, B, NQ, 2))], -1)).float()
    counts = [int(x) for x in rng.integers(max(1, per_image - per_image // 5), per_image + per_image // 5 + 1, B)]
    G = sum(counts)
    gc = rng.uniform(0.47, 0.53, (G, 2)) if clustered else rng.uniform(0.2, 0.8, (G, 2))
    gt = torch.from_numpy(np.concatenate([gc, rng.uniform(0.15, 0.25, (G, 2)) if clustered else rng.uniform(0.05, 0.4, (G, 2))], -1)).float()
    pm = torch.zeros(G, T)
    for g in range(G):
        s = int(rng.integers(1, LIVE - 3))
        pm[g, s:s + int(rng.integers(1, 4))] = 1.0
    mask = torch.zeros(B, T, dtype=torch.int32)
    mask[:, :LIVE] = 1
    offs = np.concatenate([[0], np.cumsum(counts)])
    return {"logits": logits.to(dev), "boxes": boxes.to(dev), "gt": gt.to(dev), "pm": pm.to(dev), "mask": mask.to(dev), "counts": counts,
            "gt_off": torch.tensor(offs, dtype=torch.int32, device=dev), "offs": offs}


def device_step(d):
    cost = ops.set_cost(d["logits"], d["boxes"], d["gt"], d["pm"], d["gt_off"], **COST)
    match_q, q2g = ops.hungarian(cost, d["gt_off"], d["counts"])
    return ops.set_loss(d["logits"], d["boxes"], d["gt"], d["pm"], d["gt_off"], d["mask"], q2g, match_q), match_q


def torch_cost(logits, boxes, gt, pm, a=0.25):
    """matcher.py:52-82 on the device, one layer: -> [B nq, G]"""
    p = logits.flatten(0, 1).sigmoid()
    neg = (1 - a) * (p ** 2) * (-(1 - p + 1e-8).log())
    pos = a * ((1 - p) ** 2) * (-(p + 1e-8).log())
    d = pos - neg
    cls = torch.stack([d[:, row > 0].mean(-1) for row in pm]).t()
    bx = boxes.flatten(0, 1)
    return 5.0 * torch.cdist(bx, gt, p=1) + 1.0 * cls - 2.0 * sr.giou_matrix(sr.xyxy(bx), sr.xyxy(gt))


def baseline_step(d):
    """per layer: cost on the device, one device->host copy, a host solve per image (the loss terms are left out: this is the matcher alone)"""
    out = []
    for l in range(L):
        C = torch_cost(d["logits"][l], d["boxes"][l], d["gt"], d["pm"]).view(B, NQ, -1).cpu()
        out.append([host_solve(C[b, :, d["offs"][b]:d["offs"][b + 1]].t().numpy()) for b in range(B)])
    return out


def timed(fn, d):
    fn(d)                                                        # warm-up
    torch.cuda.synchronize()
    res = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(d)
        b.record()
        torch.cuda.synchronize()
        res.append(((time.perf_counter() - t0) * 1e3, a.elapsed_time(b)))
    return res


def main():
    dev = torch.device("cuda:0")
    ops.load_library()
    print(f"set_loss_bench B={B} nq={NQ} L={L} T={T} live={LIVE} host solver: {SOLVER}")
    for per_image, clustered in ((10, False), (100, False), (10, True), (100, True)):
        d = draw(per_image, clustered, 7, dev)
        tag = f"gts/image~{per_image} {'clustered' if clustered else 'spread'} (total {sum(d['counts'])})"
        ops.start_timing()
        _, match_q = device_step(d)
        parts = ops.stop_timing()
        ref = baseline_step(d)
        mq = match_q.cpu().numpy()
        cost = ops.set_cost(d["logits"], d["boxes"], d["gt"], d["pm"], d["gt_off"], **COST).cpu().numpy()
        worst = 0.0
        for l in range(L):
            for b in range(B):
                o0, o1 = d["offs"][b], d["offs"][b + 1]
                worst = max(worst, abs(sr.total(cost[l, o0:o1], mq[l, o0:o1]) - sr.total(cost[l, o0:o1], ref[l][b])))
        print(f"{tag}: kernels ms " + " ".join(f"{k}={v[1]:.3f}" for k, v in parts.items()) + f"; |device total - host total| max {worst:.2e}")
        for name, fn in (("device cost+solve+loss", device_step), ("baseline torch cost + .cpu() + host solve", baseline_step)):
            r = timed(fn, d)
            print(f"{tag}: {name}: wall ms " + " ".join(f"{w:.2f}" for w, _ in r) + " | device-event ms " + " ".join(f"{e:.2f}" for _, e in r))


if __name__ == "__main__":
    main()
