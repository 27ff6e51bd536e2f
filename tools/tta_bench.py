#!/usr/bin/env python
"""Images/s of MQ-GLIP-T with test-time augmentation (mq_det_amd.tta.im_detect_bbox_aug) at the default TEST.SCALES and TEST.FLIP.

    python tools/tta_bench.py [--batch 8] [--steps 2] [--warmup 1] [--graph] [--candidates] [--classes N]

B seeded smooth images of LVIS-like sizes (640x480, 480x640, 500x375, ...), the 40-class caption of bench.py's workload.  Prints one JSON
line: images/s; the split of a step into ingest / forwards / merge (device events); the ingest kernel's bytes (uint8 read once per scale +
fp32 canvases written, from the shapes) and share of HBM peak; and, when PIL is importable, the same ingest done the reference's way on the
host (PIL resize + ToTensor + Normalize + pad + H2D copy), single-threaded.  --graph replays the forwards as HIP graphs (the model keeps
MODEL.HIP_GRAPH_CACHE = 8 of the 12 shapes per batch) instead of running them eagerly, the default of the TTA call.  --candidates sets TEST.USE_MULTISCALE: the reference's protocol, every
transform returns its un-suppressed candidates (up to 5 x PRE_NMS_TOP_N rows per image) and the merge is the only suppression step; the
line then also carries the candidate rows that reached the merge.  --classes N scores only the first N labels of the caption (N = 1: every
candidate in one class, the single-workgroup case of mq_tta_merge_nms)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
SIZES = [(480, 640), (640, 480), (375, 500), (427, 640), (640, 427), (480, 640), (500, 375), (333, 500)]      # (h, w)


def smooth(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [127.5 + 120 * np.sin(x / g.uniform(9, 40) + g.uniform(0, 6)) * np.cos(y / g.uniform(9, 40) + g.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.stack(ch, -1), 0, 255).astype(np.uint8)


def host_ingest(imgs, cfg, dev):
    """The reference's box_aug.py ingest on the host: per scale and flip, PIL resize + ToTensor + Normalize + to_image_list + H2D."""
    from PIL import Image
    from mq_det_amd import tta
    from mq_det_amd.structures import to_image_list
    pil = [Image.fromarray(a) for a in imgs]
    m = torch.as_tensor(cfg.INPUT.PIXEL_MEAN, dtype=torch.float32)[:, None, None]
    s = torch.as_tensor(cfg.INPUT.PIXEL_STD, dtype=torch.float32)[:, None, None]
    t0 = time.perf_counter()
    for scale in cfg.TEST.SCALES:
        for flip in (False, True):
            ts = []
            for im in pil:
                oh, ow = tta.get_size(im.size, scale, cfg.TEST.MAX_SIZE)
                r = im.resize((ow, oh), Image.BILINEAR)
                if flip:
                    r = r.transpose(Image.FLIP_LEFT_RIGHT)
                t = torch.from_numpy(np.array(r)).permute(2, 0, 1).contiguous().float().div(255)[[2, 1, 0]] * 255
                ts.append(t.sub(m).div(s))
            to_image_list(ts, cfg.DATALOADER.SIZE_DIVISIBILITY).tensors.to(dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def ingest_bytes(imgs, cfg):
    from mq_det_amd import tta
    total = 0
    for scale in cfg.TEST.SCALES:
        out = [tta.get_size((a.shape[1], a.shape[0]), scale, cfg.TEST.MAX_SIZE) for a in imgs]
        d = cfg.DATALOADER.SIZE_DIVISIBILITY
        Hp = -(-max(h for h, _ in out) // d) * d
        Wp = -(-max(w for _, w in out) // d) * d
        total += sum(a.size for a in imgs) + len(imgs) * 3 * Hp * Wp * 4 * (2 if cfg.TEST.FLIP else 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--candidates", action="store_true")
    ap.add_argument("--classes", type=int, default=0)
    args = ap.parse_args()
    import bench
    from mq_det_amd import ops, tta
    dev = torch.device("cuda:0")
    cfg, model, chunks = bench.build_model(dev)
    caption, pmap = chunks[0]
    if args.classes > 0:
        pmap = {k: pmap[k] for k in sorted(pmap)[:args.classes]}
    cfg.TEST.USE_MULTISCALE = bool(args.candidates)
    imgs = [smooth(*SIZES[i % len(SIZES)], seed=i) for i in range(args.batch)]
    tta.USE_HIP_GRAPH = args.graph
    for _ in range(args.warmup):
        tta.im_detect_bbox_aug(model, imgs, dev, [caption] * args.batch, pmap)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        tta.im_detect_bbox_aug(model, imgs, dev, [caption] * args.batch, pmap)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / args.steps
    split = {}
    tta.TIMING = split
    tta.im_detect_bbox_aug(model, imgs, dev, [caption] * args.batch, pmap)
    tta.TIMING = None
    rows = {}
    if args.candidates:                                 # rows per image the merge was handed (live candidates / slots)
        real = tta.merge

        def spy(dets, *a, **k):
            rows.update(merge_rows_live_per_image=[sum(d[1][b] for d in dets) for b in range(args.batch)],
                        merge_row_slots=sum(d[0].shape[1] for d in dets))
            return real(dets, *a, **k)
        tta.merge = spy
        try:
            tta.im_detect_bbox_aug(model, imgs, dev, [caption] * args.batch, pmap)
        finally:
            tta.merge = real
    ops.start_timing()                                  # the ingest kernel alone, HIP events around each launch
    up = tta.Upload(imgs, dev)
    for scale in cfg.TEST.SCALES:
        tta.ingest(up, scale, cfg.TEST.MAX_SIZE, cfg, bool(cfg.TEST.FLIP))
    kt = ops.stop_timing().get("tta_ingest", (0, 0.0, 0))
    nbytes = ingest_bytes(imgs, cfg)
    try:
        import PIL  # noqa: F401
        host = {"host_ingest_ms_per_batch": round(host_ingest(imgs, cfg, dev), 1)}
    except ImportError:
        host = {"host_ingest": "not available"}
    out = {"metric": "tta_images_per_s", "value": round(args.batch / wall, 3), "batch": args.batch, "steps": args.steps,
           "graph": bool(args.graph), "candidates": bool(args.candidates), "classes": len(pmap), "transforms": len(cfg.TEST.SCALES) * (2 if cfg.TEST.FLIP else 1), "step_ms": round(wall * 1e3, 1),
           "split_ms": {k: round(v, 2) for k, v in split.items()},
           "ingest_kernel": {"launches": kt[0], "ms": round(kt[1], 3), "bytes": nbytes,
                             "gb_per_s": round(nbytes / max(kt[1], 1e-9) / 1e6, 1),
                             "share_of_hbm_peak": round(nbytes / max(kt[1], 1e-9) / 1e6 / HBM_PEAK_GBS, 3)}}
    out.update(host)
    out.update(rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
