"""Test-time augmentation on the MI355X: the ingest and merge kernels against Pillow / the reference-pinned merge; the whole TTA call in the
split-precise build against the fp32 oracle; full-depth MQ-GLIP-T at the 1800 x 2400 canvas of the largest default scale against the oracle
and, in fp16, under the poison halos; the default build at B = 8 with the full default TTA.  Every test runs its body in a process of its
own under a time limit (a fault or a hang fails that test, not the session)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import test_tta_cpu as tc  # noqa: E402
from mq_det_amd import get_cfg, tta  # noqa: E402
from mq_det_amd.structures import ImageList  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def _smooth(h, w, seed):
    """Seeded smooth RGB image (gradients + low-frequency waves): every resampling tap matters, nothing saturates."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [127.5 + 120 * np.sin(x / g.uniform(9, 40) + g.uniform(0, 6)) * np.cos(y / g.uniform(9, 40) + g.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.stack(chans, -1), 0, 255).astype(np.uint8)


def _body_ingest():
    cfg = get_cfg()
    imgs = [_smooth(480, 640, 1), _smooth(640, 480, 2), _smooth(375, 500, 3)]
    up = tta.Upload(imgs, DEV)
    biggest = 0
    for scale in cfg.TEST.SCALES:
        plain, flipped, sizes = tta.ingest(up, scale, cfg.TEST.MAX_SIZE, cfg, True)
        plain, flipped = plain.cpu(), flipped.cpu()
        for b, a in enumerate(imgs):
            for fl, canvas in ((False, plain), (True, flipped)):
                want = tc._pil_canvas(a, scale, cfg.TEST.MAX_SIZE, fl, "bgr255", cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD)
                h, w = want.shape[1:]
                biggest = max(biggest, h * w)
                assert sizes[b] == (h, w)
                assert torch.equal(canvas[b, :, :h, :w], want), (scale, b, fl)
                assert not canvas[b, :, h:].any() and not canvas[b, :, :, w:].any()
    assert biggest == 1800 * 2400


def _body_merge_fixture():
    for name in ("band", "noband", "unsorted"):
        _merge_fixture(name)


def _merge_fixture(name):
    import json
    with open(tc.GOLD + ".json") as f:
        js = json.load(f)
    a = dict(np.load(tc.GOLD + ".npz"))
    cfg, dets, orig_wh = tc._fixture_dets(js, a, name)
    dets = [(d[0].to(DEV),) + tuple(d[1:]) for d in dets]
    res = tta.merge(dets, orig_wh, cfg, DEV)
    assert [len(r) for r in res] == js["cases"][name]["out_counts"]
    for b, r in enumerate(res):
        assert r.bbox.is_cuda
        assert torch.equal(r.bbox.cpu(), torch.from_numpy(a[f"{name}_boxes{b}"]))
        assert torch.equal(r.get_field("scores").cpu(), torch.from_numpy(a[f"{name}_scores{b}"]))
        assert torch.equal(r.get_field("labels").cpu(), torch.from_numpy(a[f"{name}_labels{b}"]))


def _body_merge_many_rows():
    """24 transforms x 300 rows = 7200 rows per image (> 6656, the limit of mq_ml_nms_topk): the full sweep, vs the restated merge."""
    cfg = get_cfg()
    wh = [(640, 480), (500, 375)]
    dets = tc.random_dets(31, 24, len(wh), 300, wh, n_cls=6, dense=True)
    res = tta.merge([(d[0].to(DEV),) + tuple(d[1:]) for d in dets], wh, cfg, DEV)
    for b, (rb, rs, rl) in enumerate(tc.merge_restated(dets, wh, cfg)):
        assert len(rs) == len(res[b]) > 0
        assert torch.equal(rb, res[b].bbox.cpu()) and torch.equal(rs, res[b].get_field("scores").cpu())
        assert torch.equal(rl, res[b].get_field("labels").cpu())


class _IdsModel:
    """The tiny parity model behind the reference's call signature: captions are fixed token ids (the tiny model has no tokenizer)."""

    def __init__(self, model, ids, am):
        self.m, self.ids, self.am, self.cfg, self.calls = model, ids.to(DEV), am.to(DEV), model.cfg, []

    def __call__(self, images, captions=None, positive_map=None):
        n = images.tensors.shape[0]
        self.calls.append(tuple(images.image_sizes))
        return self.m(images, captions=None, positive_map=positive_map, input_ids=self.ids[:n], attention_mask=self.am[:n])

    @property
    def last_packed(self):
        return self.m.last_packed

    @property
    def use_hip_graph(self):
        return self.m.use_hip_graph

    @use_hip_graph.setter
    def use_hip_graph(self, v):
        self.m.use_hip_graph = v


def _pil_batch(imgs, cfg, scale, flip):
    from mq_det_amd.structures import to_image_list
    cs = [tc._pil_canvas(a, scale, cfg.TEST.MAX_SIZE, flip, "bgr255", cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD) for a in imgs]
    return to_image_list(cs, cfg.DATALOADER.SIZE_DIVISIBILITY)


def _transforms(cfg):
    rngs = cfg.TEST.RANGES if len(cfg.TEST.RANGES) == len(cfg.TEST.SCALES) else [None] * len(cfg.TEST.SCALES)
    return [(scale, rng, fl) for scale, rng in zip(cfg.TEST.SCALES, rngs) for fl in ((False, True) if cfg.TEST.FLIP else (False,))]


def _check_props(got, imgs, cfg):
    ok = set(tta.class_list(cfg))
    for r, a in zip(got, imgs):
        h, w = a.shape[:2]
        assert r.size == (w, h) and r.mode == "xyxy" and r.get_field("labels").dtype == torch.int64
        n = len(r)
        assert 0 <= n <= len(_transforms(cfg)) * (cfg.MODEL.ATSS.DETECTIONS_PER_IMG + 16)
        if n:
            bx, sc = r.bbox.cpu(), r.get_field("scores").cpu()
            assert torch.isfinite(bx).all() and torch.isfinite(sc).all()
            assert (bx[:, 0] >= -1e-3).all() and (bx[:, 2] <= w + 1e-3).all() and (bx[:, 1] >= -1e-3).all() and (bx[:, 3] <= h + 1e-3).all()
            assert (bx[:, 2] >= bx[:, 0]).all() and (bx[:, 3] >= bx[:, 1]).all()
            assert set(r.get_field("labels").cpu().tolist()) <= ok


def _f32_mode():
    import parity_checks as pc
    from mq_det_amd import ops
    os.environ["MQ_F32_OPERANDS"] = "1"
    ops.configure()
    pc.use_dtype(torch.float32)
    return pc


def _body_tiny_f32_vs_oracle():
    """Split-precise build, tiny model: device TTA vs a test-side TTA that feeds the fp32 oracle (oracle.detector.forward) the Pillow canvases
    of every transform and applies the fixture-pinned merge.  Every one of the oracle's top-100 merged detections is matched (same label,
    IoU > 0.9) with |ds| < 1e-3."""
    from oracle import detector as od
    pc = _f32_mode()
    spec, sd, cfg, model, P = pc.tiny(DEV)
    _, _, ids, am, pm, bank = pc.make_inputs(spec)
    model.load_query_bank(bank)
    cfg.TEST.SCALES, cfg.TEST.RANGES, cfg.TEST.MAX_SIZE = (160, 224, 320), ((0, 10000), (32, 10000), (0, 200)), 600
    imgs = [_smooth(100, 140, 4), _smooth(130, 90, 5)]
    B = len(imgs)
    idsB, amB = ids[:1].expand(B, -1).contiguous(), am[:1].expand(B, -1).contiguous()
    wrapped = _IdsModel(model, idsB, amB)
    got = tta.im_detect_bbox_aug(wrapped, imgs, DEV, captions=["tiny"] * B, positive_map_label_to_token=pm)
    _check_props(got, imgs, cfg)
    dets = []
    with torch.no_grad():
        for scale, rng, fl in _transforms(cfg):
            il = _pil_batch(imgs, cfg, scale, fl)
            ref = od.forward(sd, spec, il.tensors, [tuple(s) for s in il.image_sizes], idsB, amB, pm, bank)
            K = max(1, max(len(d["scores"]) for d in ref))
            packed = torch.zeros(B, K, 6)
            for b, d in enumerate(ref):
                n = len(d["scores"])
                packed[b, :n] = torch.cat([d["boxes"].float(), d["scores"].float()[:, None], d["labels"].float()[:, None]], 1)
            dets.append((packed, [len(d["scores"]) for d in ref], [(w, h) for (h, w) in il.image_sizes], fl, rng))
    want = tc.merge_restated(dets, [(a.shape[1], a.shape[0]) for a in imgs], cfg)
    bad = 0
    for b, (r, (rb, rs, rl)) in enumerate(zip(got, want)):
        frac = pc._match_detections(r.bbox.cpu(), r.get_field("scores").cpu(), r.get_field("labels").cpu(), rb, rs, rl, top=100, ds=1e-3)
        print(f"{'OK' if frac == 1.0 else 'MISMATCH'} image {b}: device {len(r)} oracle {len(rs)} matched {frac:.4f}", flush=True)
        bad += frac != 1.0
    assert len(rs) > 0 and not bad


def _big_input(spec, cfg, dev):
    """One 480 x 640 image at the largest default scale: the device ingest's 1800 x 2400 canvas (padded 1824 x 2400), a 40-class caption."""
    import parity_checks as pc
    from oracle.weights import make_query_bank
    ids, am, pm, nv = pc.caption_ids(spec, 1, 40, (1, 2, 3, 4, 3, 2))
    bank = make_query_bank(pm.keys(), spec)
    up = tta.Upload([_smooth(480, 640, 6)], dev)
    canvas, _, sizes = tta.ingest(up, cfg.TEST.SCALES[-1], cfg.TEST.MAX_SIZE, cfg, False)
    assert sizes == [(1800, 2400)] and tuple(canvas.shape[2:]) == (1824, 2400)
    return canvas, sizes, ids, am, pm, bank


def _count_post_select():
    from mq_det_amd import ops
    calls = []
    real = ops.post_select

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    ops.post_select = spy
    return calls


def _body_full_depth_1800_f32_vs_oracle():
    """Full-depth MQ-GLIP-T (Swin-T, 6 fusion layers, 5-shot vision queries) on the 1800 x 2400 canvas (~90 000 FPN tokens) in the split-precise
    build vs the fp32 oracle: the oracle's top-100 detections matched (same label, IoU > 0.9) with |ds| < 1e-3."""
    from oracle import detector as od
    from mq_det_amd.structures import ImageList
    pc = _f32_mode()
    spec, sd, cfg, model = pc._bench_model(DEV)
    canvas, sizes, ids, am, pm, bank = _big_input(spec, cfg, DEV)
    model.load_query_bank(bank)
    post_calls = _count_post_select()
    model.use_hip_graph = False
    with torch.no_grad():
        r = model(ImageList(canvas, sizes), captions=None, positive_map=pm, input_ids=ids.to(DEV), attention_mask=am.to(DEV))[0]
        torch.cuda.synchronize()
        print(f"post-processing: {'fused kernels' if post_calls else 'torch chain (ops.post_select_supported is False at this size)'}", flush=True)
        import time
        t0 = time.time()
        ref = od.forward(sd, spec, canvas.cpu(), sizes, ids, am, pm, bank)[0]
        print(f"oracle forward {time.time() - t0:.0f} s", flush=True)
    frac = pc._match_detections(r.bbox.cpu(), r.get_field("scores").cpu(), r.get_field("labels").cpu(), ref["boxes"], ref["scores"],
                                ref["labels"], top=100, ds=1e-3)
    print(f"{'OK' if frac == 1.0 else 'MISMATCH'} 1800x2400: device {len(r)} oracle {len(ref['scores'])} top-100 matched {frac:.4f}", flush=True)
    assert len(ref["scores"]) > 0 and frac == 1.0


def _body_full_depth_1800_fp16_halo():
    """The same forward in fp16 with every library argument between NaN poison halos (tests/halo.py): no halo written (raises at ops._chk),
    no NaN in the detections."""
    import parity_checks as pc
    from halo import poisoned_args
    from mq_det_amd.structures import ImageList
    spec, sd, cfg, model = pc._bench_model(DEV)
    canvas, sizes, ids, am, pm, bank = _big_input(spec, cfg, DEV)
    model.load_query_bank(bank)
    model.use_hip_graph = False
    with torch.no_grad(), poisoned_args("nan"):
        r = model(ImageList(canvas, sizes), captions=None, positive_map=pm, input_ids=ids.to(DEV), attention_mask=am.to(DEV))[0]
        torch.cuda.synchronize()
    assert len(r) > 0 and torch.isfinite(r.bbox).all() and torch.isfinite(r.get_field("scores")).all()
    print(f"OK fp16 1800x2400 under NaN halos: {len(r)} detections", flush=True)


def _body_default_build_b8():
    """The default build (fp16, MQ-GLIP-T, 40-class caption, 5-shot bank), B = 8 LVIS-like images, the full default TTA (12 scales x flip):
    property checks, and the output equals the fixture-pinned merge applied to direct model calls on the Pillow canvases of every transform."""
    ROOT = os.path.dirname(HERE)
    sys.path.insert(0, ROOT)
    import bench
    cfg, model, chunks = bench.build_model(DEV)
    caption, pmap = chunks[0]
    sizes = [(480, 640), (640, 480), (375, 500), (427, 640), (640, 427), (480, 640), (500, 375), (333, 500)]
    imgs = [_smooth(h, w, 10 + i) for i, (h, w) in enumerate(sizes)]
    got = tta.im_detect_bbox_aug(model, imgs, DEV, [caption] * len(imgs), pmap)
    _check_props(got, imgs, cfg)
    assert sum(len(r) for r in got) > 0
    graphs, model.use_hip_graph = model.use_hip_graph, False            # the TTA call runs its forwards eagerly (tta.USE_HIP_GRAPH)
    dets = []
    with torch.no_grad():
        for scale, rng, fl in _transforms(cfg):
            il = _pil_batch(imgs, cfg, scale, fl)
            res = model(ImageList(il.tensors.to(DEV), il.image_sizes), captions=[caption] * len(imgs), positive_map=pmap)
            dets.append((model.last_packed.cpu(), [len(r) for r in res], [(w, h) for (h, w) in il.image_sizes], fl, rng))
    model.use_hip_graph = graphs
    want = tc.merge_restated(dets, [(a.shape[1], a.shape[0]) for a in imgs], cfg)
    for b, (r, (rb, rs, rl)) in enumerate(zip(got, want)):
        assert torch.equal(r.bbox.cpu(), rb) and torch.equal(r.get_field("scores").cpu(), rs) and torch.equal(r.get_field("labels").cpu(), rl), b
    print(f"OK B=8 default TTA: {[len(r) for r in got]} detections", flush=True)


HERE = os.path.dirname(os.path.abspath(__file__))


def _run(body, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), body], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{body}: rc {r.returncode}\n{out[-4000:]}"
    return out


def test_ingest_on_device_is_bit_exact_to_pillow_at_the_default_scales():
    _run("ingest", 300)


def test_merge_on_device_matches_the_reference_merge():
    _run("merge_fixture", 300)


def test_merge_on_device_past_the_early_stop_nms_limit():
    """24 transforms x 300 rows = 7200 rows per image (> 6656, the limit of mq_ml_nms_topk): the full sweep, vs the restated merge."""
    _run("merge_many_rows", 300)


def test_tta_split_precise_tiny_model_matches_the_fp32_oracle():
    _run("tiny_f32_vs_oracle", 600)


def test_full_depth_1800x2400_split_precise_matches_the_fp32_oracle():
    _run("full_depth_1800_f32_vs_oracle", 1200)


def test_full_depth_1800x2400_fp16_writes_no_halo_and_no_nan():
    _run("full_depth_1800_fp16_halo", 600)


def test_default_build_b8_full_default_tta():
    _run("default_build_b8", 900)


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    globals()["_body_" + sys.argv[1]]()
