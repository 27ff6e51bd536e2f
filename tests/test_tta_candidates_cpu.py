"""TEST.USE_MULTISCALE with the reference's protocol -- every transform returns its un-suppressed candidates and the merge is the only
suppression step -- without a GPU: the per-class NMS at any row count (mq_tta_merge_nms, csrc/tta.hip) through the kernel-source emulation
(tests/simt) against the restated merge of tests/tta_candidate_cases.py and against mq_ml_nms, byte for byte; the detector's candidate
mode with the emulated ops of tests/ops_emulation.py on the tiny model; check_supported with the switch on and off."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tta_candidate_cases as cc  # noqa: E402
from mq_det_amd import get_cfg, tta  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


@pytest.fixture(scope="module")
def draws():
    """Every toy draw with its restated merge, computed once and never modified."""
    return [(name, dets, wh, cfg, cc.merge_restated(dets, wh, cfg)) for name, dets, wh, cfg in cc.toy_draws()]


def test_the_draws_hold_what_they_claim(draws):
    by = {d[0]: d for d in draws}
    _, dets, wh, cfg, want = by["mixed_ranges"]
    assert tta.class_list(cfg) == list(cc.CLASSES_MIXED) and list(cc.CLASSES_MIXED) != sorted(cc.CLASSES_MIXED)
    assert [d[3] for d in dets] == [False, True, False, True] and all(d[4] is not None for d in dets)
    raw_nan = sum(int(torch.isnan(d[0][b, :d[1][b], 4]).sum()) for d in dets for b in range(len(wh)))
    assert raw_nan == 1
    for bx, sc, lb in cc.prep_restated(dets, wh):
        n = {c: int((lb == c).sum()) for c in cc.CLASSES_MIXED}
        assert n[7] == 0 and n[1] == 1 and n[3] == cc.ROW_CAP and n[9] == cc.ROW_CAP + 1 and n[2] > cc.ROW_CAP and n[5] > cc.ROW_CAP
        assert ((lb == 6) | (lb == 11)).sum() > 0
    no_band = cc.prep_restated(by["mixed_noranges_cut"][1], wh)
    assert all(d[4] is None for d in by["mixed_noranges_cut"][1])
    assert sum(len(r[1]) for r in no_band) > sum(len(r[1]) for r in cc.prep_restated(dets, wh))          # the band removes rows
    assert all(len(w[1]) >= 30 for w in by["mixed_noranges_cut"][4]) and all(len(w[1]) > 30 for w in want)   # the cut cuts
    # TEST.TH <= 0: the rows as they are (class-list order), cut or not
    for key in ("mixed_th0", "mixed_th_negative"):
        _, d_, wh_, cfg_, w_ = by[key]
        assert cfg_.TEST.TH <= 0
        for (bx, sc, lb), (rb, rs, rl) in zip(cc.prep_restated(d_, wh_), w_):
            inlist = np.isin(lb, cc.CLASSES_MIXED)
            assert len(rs) == inlist.sum() if key == "mixed_th0" else 40 <= len(rs) < inlist.sum()
    _, dets, wh, cfg, want = by["one_class"]
    (bx, sc, lb), = cc.prep_restated(dets, wh)
    assert (lb == 4).all() and len(lb) == 180 and cc.ROW_CAP * 6 // 5 < len(want[0][1]) < 180       # kept heads past the LDS list of the workspace path
    _, dets, wh, cfg, want = by["all_suppressed"]
    assert len(want[0][1]) == 1 and want[0][1][0] == np.float32(0.99)
    _, dets, wh, cfg, want = by["none_suppressed"]
    assert [len(w[1]) for w in want] == [36, 36, 0]
    _, dets, wh, cfg, want = by["equal_scores"]
    for (bx, sc, lb), (rb, rs, rl) in zip(cc.prep_restated(dets, wh), want):
        assert len(np.unique(sc)) <= 7 and len(sc) == 180
        first = bx[:60]                                       # the duplicates of later transforms never survive their first copy
        assert all((first == r).all(1).any() for r in rb)
        assert len(rs) > 25                                   # ties at the cut are kept


@needs_simt
def test_segmented_merge_matches_the_restated_merge(emu, draws):
    tta._WARNED_CLASSES = True
    for name, dets, wh, cfg, want in draws:
        for cap in (cc.ROW_CAP, None):
            stats = {}
            got = tta.merge(dets, wh, cfg, CPU, row_cap=cap, stats=stats, nms_path="segmented")
            cc.compare_exact(got, want, f"{name} cap {cap}")
            for r, size in zip(got, wh):
                assert r.size == size and r.mode == "xyxy" and r.fields() == ["scores", "labels"]
            if cfg.TEST.TH > 0 and cap is not None and name.startswith(("mixed", "one_class", "equal")):
                assert stats["workspace_classes"] > 0, name
            if cap is None or cfg.TEST.TH <= 0:
                assert stats["workspace_classes"] == 0, name


def _both_keeps(emu, dets, wh, cfg, cap):
    """keep of mq_tta_merge_nms and of mq_ml_nms on the very lists mq_tta_merge_prep leaves, and the two merged outputs."""
    seen = {}
    real = emu.tta_merge_nms

    def spy(boxes_s, labels_s, nvalid, cls_rank, thresh, row_cap=None, stats=None):
        keep = real(boxes_s, labels_s, nvalid, cls_rank, thresh, row_cap=row_cap, stats=stats)
        seen.update(args=(boxes_s, labels_s, nvalid, thresh), keep=keep.clone())
        return keep
    emu.tta_merge_nms = spy
    try:
        seg = tta.merge(dets, wh, cfg, CPU, row_cap=cap, nms_path="segmented")
    finally:
        emu.tta_merge_nms = real
    boxes_s, labels_s, nvalid, thresh = seen["args"]
    return seen["keep"], emu.ml_nms(boxes_s, labels_s, nvalid, thresh, as_bool=False), seg, tta.merge(dets, wh, cfg, CPU)


@needs_simt
def test_keep_flags_equal_mq_ml_nms_byte_for_byte(emu, draws):
    tta._WARNED_CLASSES = True
    ran = 0
    for name, dets, wh, cfg, _ in draws:
        if cfg.TEST.TH <= 0:
            continue
        for cap in (cc.ROW_CAP, None):
            k_seg, k_ml, seg, auto = _both_keeps(emu, dets, wh, cfg, cap)
            assert k_seg.dtype == k_ml.dtype == torch.uint8 and torch.equal(k_seg, k_ml), (name, cap)
            assert cc.same_boxlists(seg, auto), (name, cap)
            ran += 1
    assert ran == 12


@needs_simt
def test_dense_random_rows_equal_mq_ml_nms(emu):
    """random_dets(31, 24, 2, 300, ..., dense=True) of tests/test_gpu_tta.py (7200 rows an image on the device), cut to 6 transforms x 2
    images x 150 rows for the emulator: 900 rows an image, 12 classes of about 75 rows, more than one 256-row chunk per class only with
    fewer classes -- so also with 2 classes (about 450 rows each: two chunks, kept heads crossing them)."""
    import test_tta_cpu as tc
    wh = [(640, 480), (375, 500)]
    for n_cls, cap in ((12, None), (2, None), (2, 64)):
        dets = [(d[0][:, :150].contiguous(), [min(c, 150) for c in d[1]]) + tuple(d[2:]) for d in tc.random_dets(31, 24, 2, 300, wh, n_cls=n_cls + 1, dense=True)[:6]]
        cfg = cc.make_cfg(tuple(range(1, n_cls + 1)), 0.5, 300)
        tta._WARNED_CLASSES = True
        k_seg, k_ml, seg, auto = _both_keeps(emu, dets, wh, cfg, cap)
        assert torch.equal(k_seg, k_ml) and 0 < int(k_seg.sum()) < k_seg.numel()
        assert cc.same_boxlists(seg, auto)
        cc.compare_exact(seg, cc.merge_restated(dets, wh, cfg), f"dense {n_cls}")


@needs_simt
def test_result_does_not_depend_on_the_schedule(emu, draws):
    import simt
    tta._WARNED_CLASSES = True
    for name in ("mixed_ranges", "one_class", "equal_scores"):
        _, dets, wh, cfg, _ = [d for d in draws if d[0] == name][0]
        outs = []
        try:
            for sched, seed in (("ascending", 0), ("descending", 0), ("random", 7)):
                simt.set_schedule(sched, seed)
                k_seg, _, seg, _ = _both_keeps(emu, dets, wh, cfg, cc.ROW_CAP)
                outs.append((k_seg, seg))
        finally:
            simt.set_schedule("ascending")
        for k, o in outs[1:]:
            assert torch.equal(k, outs[0][0]) and cc.same_boxlists(o, outs[0][1]), name


@needs_simt
def test_merge_result_from_multi_scales_inherits_the_path(emu, draws):
    from mq_det_amd.structures import BoxList
    _, dets, wh, cfg, _ = [d for d in draws if d[0] == "one_class"][0]
    (bx, sc, lb), = cc.prep_restated(dets, wh)
    bl = BoxList(torch.from_numpy(bx), wh[0], mode="xyxy")
    bl.add_field("scores", torch.from_numpy(sc))
    bl.add_field("labels", torch.from_numpy(lb))
    stats = {}
    got = tta.merge_result_from_multi_scales([bl], cfg, row_cap=cc.ROW_CAP, stats=stats, nms_path="segmented")
    assert stats["workspace_classes"] == 1
    assert cc.same_boxlists(got, tta.merge_result_from_multi_scales([bl], cfg))
    cc.compare_exact(got, cc.merge_restated(dets, wh, cfg), "public")
    with pytest.raises(ValueError, match="nms_path"):
        tta.merge_result_from_multi_scales([bl], cfg, nms_path="bitmask")


@needs_simt
def test_more_rows_than_mq_ml_nms_takes_go_to_the_segmented_kernel(emu):
    """N = 16 400 slots an image (one more 16-row step than TTA_MERGE_MAX_ROWS) with 40 live rows: the default path no longer raises."""
    dets, wh, cfg = cc.draw_all_suppressed()
    packed = torch.zeros(1, emu.TTA_MERGE_MAX_ROWS + 16, 6)
    packed[:, :40] = dets[0][0]
    big = [(packed, dets[0][1], dets[0][2], False, None)]
    got = tta.merge(big, wh, cfg, CPU)
    cc.compare_exact(got, cc.merge_restated(dets, wh, cfg), "above the old limit")


class _NoForward:
    def __init__(self, cfg):
        self.cfg, self.calls = cfg, 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("no forward may run")


@pytest.mark.parametrize("mode", ["soft-nms", "vote", "soft-vote"])
def test_check_supported_takes_the_special_modes_with_the_switch_on(mode):
    cfg = get_cfg()
    cfg.TEST.SPECIAL_NMS = mode
    with pytest.raises(NotImplementedError, match="TEST.SPECIAL_NMS"):
        tta.check_supported(_NoForward(cfg))
    cfg.TEST.USE_MULTISCALE = True
    tta.check_supported(_NoForward(cfg))


def test_check_supported_sizes_candidate_rows_against_the_per_class_limit():
    from mq_det_amd import ops
    cfg = get_cfg()
    cfg.MODEL.ATSS.DETECTIONS_PER_IMG = 700                 # 24 transforms x (700 + 16) rows > 16 384
    with pytest.raises(ValueError, match="exceed"):
        tta.check_supported(_NoForward(cfg))
    cfg.TEST.USE_MULTISCALE = True                          # 24 x 5 x 1000 = 120 000 candidate rows: fine
    assert len(cfg.TEST.SCALES) * 2 * 5 * cfg.MODEL.ATSS.PRE_NMS_TOP_N > ops.TTA_MERGE_MAX_ROWS
    tta.check_supported(_NoForward(cfg))
    cfg.MODEL.ATSS.PRE_NMS_TOP_N = 200000                   # 24 x 5 x 200 000 > 2^24
    with pytest.raises(ValueError, match="exceed"):
        tta.check_supported(_NoForward(cfg))
    # what stays refused with the switch on
    cfg = get_cfg()
    cfg.TEST.USE_MULTISCALE, cfg.TEST.SELECT_CLASSES = True, (3, 1, 3)
    with pytest.raises(NotImplementedError, match="repeats a class"):
        tta.check_supported(_NoForward(cfg))
    from mq_det_amd.config import get_gdino_cfg
    gcfg = get_gdino_cfg()
    gcfg.TEST.USE_MULTISCALE = True
    m = _NoForward(gcfg)
    with pytest.raises(NotImplementedError, match="GroundingDINO"):
        tta.im_detect_bbox_aug(m, [np.zeros((8, 8, 3), np.uint8)], "cpu")
    assert m.calls == 0


def test_online_update_keeps_its_refusal():
    import inspect
    from mq_det_amd import query_bank
    assert 'raise NotImplementedError("online_update with TEST.USE_MULTISCALE")' in inspect.getsource(query_bank)


# ------------------------------------------------------------------------------------------------ the detector's candidate mode (emulated ops)
@pytest.fixture(scope="module")
def tiny():
    from oracle import tiny_spec
    from oracle.weights import make_state_dict
    spec = tiny_spec()
    sd = make_state_dict(spec, 0)
    cfg = get_cfg()
    cfg.MODEL.SWINT.DEPTHS = spec.swin_depths
    cfg.MODEL.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS = spec.bert_layers
    cfg.MODEL.LANGUAGE_BACKBONE.QV_START = spec.qv_start
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = spec.vocab
    cfg.MODEL.DYHEAD.NUM_CONVS = spec.dyhead_convs
    cfg.MODEL.DYHEAD.NUM_CLASSES = spec.num_classes
    cfg.MODEL.ATSS.DETECTIONS_PER_IMG = spec.detections_per_img
    cfg.MODEL.DYHEAD.LEVEL_STREAMS = False
    return spec, sd, cfg


def _tiny_model(tiny, monkeypatch):
    import ops_emulation as oe
    from mq_det_amd import ops
    from mq_det_amd.modeling import detector, pipeline
    spec, sd, cfg0 = tiny
    oe.patch_into(monkeypatch, ops)
    calls = {"ml_nms": 0, "post_finalize": 0}
    for name in calls:
        def wrap(*a, _f=getattr(ops, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, name, wrap)

    def prepare(self, device=None):
        self._validate_config()
        self._plan = pipeline.build_plan(self.state_dict(), self.cfg, torch.device("cpu"), dtype=torch.float32)
        self._plan_key, self.use_hip_graph = torch.device("cpu"), False
        return self._plan
    monkeypatch.setattr(detector.GeneralizedVLRCNN_New, "prepare", prepare)
    model = detector.GeneralizedVLRCNN_New(cfg0.clone(), tokenizer=object())
    model.load_state_dict(sd, strict=True)
    model.eval()
    return model, calls


def test_detector_returns_the_candidates_with_the_switch_on(tiny, monkeypatch):
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    spec, sd, _ = tiny
    model, calls = _tiny_model(tiny, monkeypatch)            # built BEFORE the key is set: it is read at every forward
    images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
    model.load_query_bank(bank)
    il = ImageList(images, sizes)
    kw = dict(positive_map=pm, input_ids=ids, attention_mask=am)
    with torch.no_grad():
        before = model(il, **kw)
        packed_before = model.last_packed.clone()
    assert calls["ml_nms"] == 1 and calls["post_finalize"] <= 1
    seen = dict(calls)
    model.cfg.TEST.USE_MULTISCALE = True
    with torch.no_grad():
        raw = model(il, return_raw=True, **kw)
        cand = model(il, **kw)
    assert calls == seen                                     # no NMS and no final selection in the mode, raw or not
    post = raw["post"]["pre_nms"]
    assert "keep" not in post
    L = len([k for k, v in pm.items() if len(v)])
    tot = sum(min(model.cfg.MODEL.ATSS.PRE_NMS_TOP_N, f.shape[-2] * f.shape[-1] * L) for f in raw["feats"])
    assert model.last_packed.shape == (len(sizes), tot, 6)
    assert model.last_tie_overflow == [False] * len(sizes)
    for b, (h, w) in enumerate(sizes):
        n = int(post["nvalid"][b])
        assert len(before[b]) < n == len(cand[b])            # un-suppressed: more rows than the detections
        assert cand[b].size == (w, h) and cand[b].mode == "xyxy"
        assert torch.equal(cand[b].bbox, post["boxes"][b, :n]) and torch.equal(cand[b].get_field("scores"), post["scores"][b, :n])
        lab = cand[b].get_field("labels")
        assert lab.dtype == torch.int64 and torch.equal(lab, post["labels"][b, :n].to(torch.int64))
        s = cand[b].get_field("scores")
        assert (s[:-1] >= s[1:]).all() and (s > model.cfg.MODEL.ATSS.INFERENCE_TH).all()
        assert torch.equal(model.last_packed[b, :n, :4], cand[b].bbox)
    # per chunk
    kv = int(am[0].sum())
    model.tokenize = lambda caps, dev: (ids[:1].expand(len(caps), -1).contiguous(), am[:1].expand(len(caps), -1).contiguous(), kv)
    with torch.no_grad():
        chunked = model.forward_chunks(il, [("caption a", pm), ("caption b", pm)])
    assert calls == seen and len(chunked) == 2
    for res in chunked:
        for b in range(len(sizes)):
            assert len(res[b]) == len(cand[b])
            assert torch.allclose(res[b].get_field("scores"), cand[b].get_field("scores"), atol=1e-5)
    # grounding entry point
    with torch.no_grad():
        g = model.forward_grounding(il, ["caption a"] * len(sizes), [pm] * len(sizes))
    assert calls == seen and [len(x) for x in g] == [len(x) for x in cand]
    # and back: today's detections, unchanged
    model.cfg.TEST.USE_MULTISCALE = False
    with torch.no_grad():
        after = model(il, **kw)
    assert calls["ml_nms"] == seen["ml_nms"] + 1
    assert torch.equal(model.last_packed, packed_before)
    assert cc.same_boxlists(before, after)


def test_the_graph_key_tells_the_modes_apart(tiny, monkeypatch):
    model, _ = _tiny_model(tiny, monkeypatch)
    off = model._mode_key()
    model.cfg.TEST.USE_MULTISCALE = True
    on = model._mode_key()
    assert off != on and off == (False,) and on == (True,)
    keys = []
    model._graphs, model.graph_cache_size, model.graph_warm_calls = {}, 4, 10
    from collections import OrderedDict, defaultdict
    model._graphs, model.cache_stats = OrderedDict(), defaultdict(int)
    model._probe = lambda x, kv: keys.append(tuple(model._graphs)) or x
    for flag in (False, True, False):
        model.cfg.TEST.USE_MULTISCALE = flag
        model._run("_probe", (torch.zeros(2, 3), 17), True)
    assert len(model._graphs) == 2                           # one entry per mode for the same program and shapes
