"""TEST.USE_MULTISCALE with the reference's protocol on the MI355X: the per-class NMS at any row count (mq_tta_merge_nms) past the 16 384
rows of mq_ml_nms, through its workspace path and against mq_ml_nms on the device; the tiny model in split-precise mode with the switch on
against the fp32 oracle's candidates and against a test-side TTA built from them; one full-depth fp16 property run; the new kernel under
the poison halos of tests/halo.py.  Every test runs its body in a process of its own under a time limit (a fault or a hang fails that
test, not the session)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import tta_candidate_cases as cc  # noqa: E402
from mq_det_amd import get_cfg, tta  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")

# the tiny-model inputs: see _body_tiny_f32_vs_oracle
TINY_SCALES, TINY_RANGES, TINY_MAX_SIZE = (160,), ((0, 10000),), 600
TINY_IMAGES = ((100, 100, 13), (128, 128, 14))               # (h, w, seed of the smooth image)


def _body_large_merge():
    """T = 3, B = 2, K = 6000 slots with about 200 live rows per transform: N = 18 000 > 16 384 through the default nms_path."""
    from mq_det_amd import ops
    wh = [(640, 480), (500, 375)]
    dets = cc.large_dets(41, 3, 2, 6000, 200, wh, n_cls=6)
    assert 3 * 6000 > ops.TTA_MERGE_MAX_ROWS
    cfg = cc.make_cfg(range(1, 7), 0.5, 300)
    stats = {}
    got = tta.merge(cc.to_device(dets, DEV), wh, cfg, DEV, stats=stats)
    want = cc.merge_restated(dets, wh, cfg)
    assert all(0 < len(w[1]) for w in want) and stats["workspace_classes"] == 0
    cc.compare_exact(got, want, "N = 18 000")
    print(f"OK N = 18000: {[len(r) for r in got]} rows", flush=True)


def _body_workspace_class():
    """One class of about 3050 rows an image (3000 in one transform), above the LDS cap of 512 asked for here: the workspace path, with
    more kept heads (about 890) than the 614 its LDS list holds; the other five classes have 42 .. 58 rows (workspace only at cap 32)."""
    wh = [(640, 480), (500, 375)]
    dets = cc.large_dets(42, 3, 2, 3000, 150, wh, n_cls=6, one_class_rows=3000)
    cfg = cc.make_cfg(range(1, 7), 0.5, 1000)
    want = cc.merge_restated(dets, wh, cfg)
    for cap, n_ws in ((512, 2), (None, 0), (4096, 0), (32, None)):
        stats = {}
        got = tta.merge(cc.to_device(dets, DEV), wh, cfg, DEV, row_cap=cap, stats=stats, nms_path="segmented")
        cc.compare_exact(got, want, f"cap {cap}")
        assert stats["workspace_classes"] == n_ws if n_ws is not None else stats["workspace_classes"] > 2, (cap, stats)
        print(f"OK 3000-row class, cap {cap}: workspace classes {stats['workspace_classes']}, {[len(r) for r in got]} rows", flush=True)
    assert all((w[2] == 1).sum() > 512 * 6 // 5 for w in want)           # more kept heads than the LDS list of cap 512 holds


def _body_dense_equals_ml_nms():
    """tests/test_gpu_tta.py's 7200-row dense case forced through the new kernel: exact against the restated merge, and its keep flags
    and merged rows equal to the mq_ml_nms path on the device."""
    import test_tta_cpu as tc
    from mq_det_amd import ops
    cfg = get_cfg()
    wh = [(640, 480), (500, 375)]
    dets = tc.random_dets(31, 24, len(wh), 300, wh, n_cls=6, dense=True)
    dd = cc.to_device(dets, DEV)
    seen = {}
    real = ops.tta_merge_nms

    def spy(boxes_s, labels_s, nvalid, cls_rank, thresh, row_cap=None, stats=None):
        keep = real(boxes_s, labels_s, nvalid, cls_rank, thresh, row_cap=row_cap, stats=stats)
        seen.update(args=(boxes_s, labels_s, nvalid, thresh), keep=keep.clone())
        return keep
    ops.tta_merge_nms = spy
    try:
        seg = tta.merge(dd, wh, cfg, DEV, nms_path="segmented")
    finally:
        ops.tta_merge_nms = real
    auto = tta.merge(dd, wh, cfg, DEV)
    boxes_s, labels_s, nvalid, thresh = seen["args"]
    k_ml = ops.ml_nms(boxes_s, labels_s, nvalid, thresh, as_bool=False)
    assert torch.equal(seen["keep"], k_ml) and 0 < int(k_ml.sum()) < k_ml.numel()
    assert cc.same_boxlists(seg, auto)
    cc.compare_exact(seg, cc.merge_restated(dets, wh, cfg), "dense 7200")
    print(f"OK dense 7200 rows: keep equal to mq_ml_nms, {[len(r) for r in seg]} rows", flush=True)


def _body_halo():
    """mq_tta_merge_nms (both paths) with every argument between NaN poison halos: nothing written outside them, no NaN in the result."""
    from halo import poisoned_args
    wh = [(640, 480), (500, 375)]
    dets = cc.large_dets(43, 3, 2, 700, 300, wh, n_cls=3, one_class_rows=700)
    cfg = cc.make_cfg(range(1, 4), 0.5, 1000)
    want = cc.merge_restated(dets, wh, cfg)
    for cap in (None, 128):
        with poisoned_args("nan"):
            got = tta.merge(cc.to_device(dets, DEV), wh, cfg, DEV, row_cap=cap, nms_path="segmented")
            torch.cuda.synchronize()
        cc.compare_exact(got, want, f"halo cap {cap}")
        assert all(torch.isfinite(r.bbox).all() and torch.isfinite(r.get_field("scores")).all() for r in got)
    print("OK mq_tta_merge_nms under NaN halos", flush=True)


def tiny_images():
    import test_gpu_tta as tg
    return [tg._smooth(h, w, seed) for h, w, seed in TINY_IMAGES]


def oracle_candidate_dets(sd, spec, cfg, imgs, ids, am, pm, bank):
    """The test-side TTA of the reference's protocol: the fp32 oracle on the Pillow canvas of every transform, its "pre_nms" rows (the
    un-suppressed candidates of ATSSPostProcessor with bbox_aug_enabled) as the transform's detections -> dets for the restated merge."""
    import test_gpu_tta as tg
    from oracle import detector as od
    B = len(imgs)
    idsB, amB = ids[:1].expand(B, -1).contiguous(), am[:1].expand(B, -1).contiguous()
    dets = []
    with torch.no_grad():
        for scale, rng, fl in tg._transforms(cfg):
            il = tg._pil_batch(imgs, cfg, scale, fl)
            ref = od.forward(sd, spec, il.tensors, [tuple(s) for s in il.image_sizes], idsB, amB, pm, bank)
            K = max(1, max(len(d["pre_nms"]["scores"]) for d in ref))
            packed = torch.zeros(B, K, 6)
            for b, d in enumerate(ref):
                p = d["pre_nms"]
                o = torch.argsort(p["scores"], descending=True, stable=True)
                packed[b, :len(o)] = torch.cat([p["boxes"].float()[o], p["scores"].float()[o, None], p["labels"].float()[o, None]], 1)
            dets.append((packed, [len(d["pre_nms"]["scores"]) for d in ref], [(w, h) for (h, w) in il.image_sizes], fl, rng))
    return dets


def tiny_cfg(cfg):
    cfg.TEST.SCALES, cfg.TEST.RANGES, cfg.TEST.MAX_SIZE = TINY_SCALES, TINY_RANGES, TINY_MAX_SIZE
    cfg.TEST.USE_MULTISCALE = True
    return cfg


def _tiny_setup():
    import test_gpu_tta as tg
    pc = tg._f32_mode()
    spec, sd, cfg, model, P = pc.tiny(DEV)
    _, _, ids, am, pm, bank = pc.make_inputs(spec)
    model.load_query_bank(bank)
    tiny_cfg(cfg)
    imgs = tiny_images()
    B = len(imgs)
    wrapped = tg._IdsModel(model, ids[:1].expand(B, -1).contiguous(), am[:1].expand(B, -1).contiguous())
    return pc, spec, sd, cfg, wrapped, imgs, ids, am, pm, bank


def _body_tiny_f32_vs_oracle():
    """Split-precise build, tiny model, TEST.USE_MULTISCALE on: the device TTA (candidates from every transform, merged once) vs a
    test-side TTA built from the fp32 oracle's pre_nms rows on the Pillow canvases and the restated merge.  Every one of the oracle's
    top-100 merged detections is matched (same label, IoU > 0.9) with |ds| < 1e-3.
    Inputs: the smooth images of seeds 13 (100 x 100) and 14 (128 x 128), TEST.SCALES (160,) -- the smallest scale at which the tiny
    model's coarsest level still has 2 x 2 cells -- with flip: 956 and 1109 candidates, 184 and 203 merged rows in the oracle.
    STABILITY OF THE EXPECTED RESULT, checked on the CPU when the test was written (14 perturbations of every candidate box of the oracle:
    6 uniform draws, 6 random-sign draws at full amplitude, all coordinates up, all down): at +-1e-5 of the image size the oracle's merge
    keeps the same rows, labels and scores bit for bit; at +-1e-4 5 of 28 (image, perturbation) merges change (3 inside the top 100), at
    +-3e-4 16, at +-1e-3 every one.  No seeds or scales of this model reach +-1e-3: its random weights leave about 1000 dense candidates
    per transform and image, so some of the ~200 kept heads always have a candidate within 0.5 % of TEST.TH (eight combinations of seeds,
    sizes and scales tried: 21 .. 28 of 28 merges change at +-1e-3, with (160, 224) and seeds 4 / 5 -- the inputs of the post-NMS test
    -- 11 of 28 already at +-1e-5).  The inputs chosen are the most stable ones found."""
    pc, spec, sd, cfg, wrapped, imgs, ids, am, pm, bank = _tiny_setup()
    got = tta.im_detect_bbox_aug(wrapped, imgs, DEV, captions=["tiny"] * len(imgs), positive_map_label_to_token=pm)
    assert len(wrapped.calls) == 2
    dets = oracle_candidate_dets(sd, spec, cfg, imgs, ids, am, pm, bank)
    want = cc.merge_restated(dets, [(a.shape[1], a.shape[0]) for a in imgs], cfg)
    bad = 0
    for b, (r, (rb, rs, rl)) in enumerate(zip(got, want)):
        frac = pc._match_detections(r.bbox.cpu(), r.get_field("scores").cpu(), r.get_field("labels").cpu(), torch.from_numpy(rb),
                                    torch.from_numpy(rs), torch.from_numpy(rl), top=100, ds=1e-3)
        print(f"{'OK' if frac == 1.0 else 'MISMATCH'} image {b}: device {len(r)} oracle {len(rs)} matched {frac:.4f}", flush=True)
        bad += frac != 1.0
        assert len(rs) > 0
    assert not bad


def _body_tiny_candidates():
    """Split-precise build, tiny model, the switch on: per image the device returns as many candidates as the oracle's pre_nms holds, and
    every one of the oracle's rows is matched (same label, IoU > 0.9, |ds| < 1e-3)."""
    import test_gpu_tta as tg
    from oracle import detector as od
    pc, spec, sd, cfg, wrapped, imgs, ids, am, pm, bank = _tiny_setup()
    il = tg._pil_batch(imgs, cfg, TINY_SCALES[0], False)
    B = len(imgs)
    with torch.no_grad():
        ref = od.forward(sd, spec, il.tensors, [tuple(s) for s in il.image_sizes], ids[:1].expand(B, -1).contiguous(),
                         am[:1].expand(B, -1).contiguous(), pm, bank)
        from mq_det_amd.structures import ImageList
        got = wrapped(ImageList(il.tensors.to(DEV), il.image_sizes), positive_map=pm)
    bad = 0
    for b, (r, d) in enumerate(zip(got, ref)):
        p = d["pre_nms"]
        n = len(p["scores"])
        frac = pc._match_detections(r.bbox.cpu(), r.get_field("scores").cpu(), r.get_field("labels").cpu(), p["boxes"].float(),
                                    p["scores"].float(), p["labels"], top=n, ds=1e-3)
        print(f"{'OK' if frac == 1.0 and len(r) == n else 'MISMATCH'} image {b}: device {len(r)} oracle {n} (detections {len(d['scores'])}) "
              f"matched {frac:.4f}", flush=True)
        bad += frac != 1.0 or len(r) != n
        assert n > len(d["scores"]) > 0
    assert not bad


def _body_full_depth_props():
    """Default fp16 build, one 480 x 640 image, TEST.SCALES (800,) + flip, the 40-class caption, the switch on."""
    import parity_checks as pc
    import test_gpu_tta as tg
    from oracle.weights import make_query_bank
    spec, sd, cfg, model = pc._bench_model(DEV)
    ids, am, pm, nv = pc.caption_ids(spec, 1, 40, (1, 2, 3, 4, 3, 2))
    model.load_query_bank(make_query_bank(pm.keys(), spec))
    cfg.TEST.SCALES, cfg.TEST.RANGES, cfg.TEST.FLIP, cfg.TEST.USE_MULTISCALE = (800,), ((0, 10000),), True, True
    img = tg._smooth(480, 640, 6)
    wrapped = tg._IdsModel(model, ids, am)
    per_transform = []
    real = tta.merge

    def spy(dets, *a, **k):
        per_transform.extend(dets)
        return real(dets, *a, **k)
    tta.merge = spy
    try:
        got = tta.im_detect_bbox_aug(wrapped, [img], DEV, captions=["caption"], positive_map_label_to_token=pm)
    finally:
        tta.merge = real
    assert len(per_transform) == 2
    A = cfg.MODEL.ATSS
    for packed, counts, wh, fl, rng in per_transform:
        (w, h), = wh
        assert (h, w) == (800, 1066)
        hw = [(-(-(-(-h // 32) * 32) // s), -(-(-(-w // 32) * 32) // s)) for s in (8, 16, 32, 64, 128)]
        bound = sum(min(A.PRE_NMS_TOP_N, a * b * 40) for a, b in hw)
        n = counts[0]
        assert packed.shape == (1, bound, 6) and 0 < n <= bound, (packed.shape, bound, n)
        p = packed[0, :n].cpu()
        assert torch.isfinite(p).all()
        assert (p[:, 0] >= 0).all() and (p[:, 1] >= 0).all() and (p[:, 2] <= w - 1).all() and (p[:, 3] <= h - 1).all()
        assert (p[:, 2] >= p[:, 0]).all() and (p[:, 3] >= p[:, 1]).all()
        assert (p[:, 4] > A.INFERENCE_TH).all() and (p[:-1, 4] >= p[1:, 4]).all()
        assert set(p[:, 5].long().tolist()) <= set(range(1, 41))
    r, = got
    bx, sc, lb = r.bbox.cpu(), r.get_field("scores").cpu(), r.get_field("labels").cpu()
    assert r.size == (640, 480) and lb.dtype == torch.int64 and len(r) > 0
    assert torch.isfinite(bx).all() and torch.isfinite(sc).all()
    assert (bx[:, 0] >= -1e-3).all() and (bx[:, 2] <= 640 + 1e-3).all() and (bx[:, 1] >= -1e-3).all() and (bx[:, 3] <= 480 + 1e-3).all()
    assert set(lb.tolist()) <= set(tta.class_list(cfg)) and set(lb.tolist()) <= set(range(1, 41))
    top = int(cfg.TEST.PRE_NMS_TOP_N)
    assert len(r) <= top or int((sc > sc.min()).sum()) < top          # more than PRE_NMS_TOP_N rows only as ties with the last score
    print(f"OK full depth: candidates {[d[1][0] for d in per_transform]}, merged {len(r)}", flush=True)


def _run(body, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), body], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{body}: rc {r.returncode}\n{out[-4000:]}"
    return out


def test_merge_past_the_row_limit_of_mq_ml_nms():
    _run("large_merge", 300)


def test_a_class_above_the_lds_cap_takes_the_workspace_path():
    _run("workspace_class", 300)


def test_dense_rows_through_the_segmented_kernel_equal_mq_ml_nms():
    _run("dense_equals_ml_nms", 300)


def test_segmented_nms_writes_no_halo_and_no_nan():
    _run("halo", 300)


def test_tta_candidates_split_precise_tiny_model_matches_the_fp32_oracle():
    _run("tiny_f32_vs_oracle", 600)


def test_tiny_model_candidates_match_the_oracle_pre_nms():
    _run("tiny_candidates", 300)


def test_full_depth_fp16_candidate_tta_properties():
    _run("full_depth_props", 600)


if __name__ == "__main__":
    globals()["_body_" + sys.argv[1]]()
