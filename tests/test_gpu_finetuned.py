"""Fine-tuned checkpoints on the MI355X (DESIGN.md "Fine-tuned checkpoints"): the tuned prompt (MODEL.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER)
against the oracle, the vision offset (VISION_QUERY.ADD_VISION_LAYER, csrc/query_bank.hip mq_bank_select_add_fwd) and the learnable bank
(VISION_QUERY.LEARNABLE_BANK) through every entry point of the tiny MQ-GLIP of tests/parity_checks.py (160 x 192, B = 2), and a HIP-graph
replay across `load_state_dict`."""
import os
import sys

import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_finetuned_cpu as fc  # noqa: E402
import test_query_select_cpu as sc  # noqa: E402
from mq_det_amd.query_bank import QueryBank  # noqa: E402

pytestmark = pytest.mark.gpu

# 0.1 x randn, the first choice, moves the oracle's head text hidden by 5.4 x the fp16 gate only; 0.3 x randn moves it by 17.8 x (CPU, fp32)
W_SCALE = 0.3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    from mq_det_amd import ops
    ops.load_library()
    return torch.device("cuda:0")


def prompt_w(H, seed=7, scale=W_SCALE):
    return scale * torch.randn(1000, H, generator=torch.Generator().manual_seed(seed))


def _equal_detections(a, b):
    """bit-equal detections: the same program on the same operands (tests/test_gpu_parity.py)"""
    return (len(a) == len(b) and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
            and torch.equal(a.get_field("labels"), b.get_field("labels")))


def tiny_model(dev, linear=False, learnable=False, vision=False):
    """parity_checks._tiny with the fine-tuning switches: (spec, oracle state dict, model on the device, not prepared)"""
    import parity_checks as pc
    from oracle import tiny_spec
    from oracle.weights import make_state_dict
    from mq_det_amd import get_cfg
    from mq_det_amd.modeling.detector import GeneralizedVLRCNN_New
    spec = tiny_spec()
    sd = make_state_dict(spec, 0)
    cfg = get_cfg()
    cfg.MODEL.SWINT.EMBED_DIM, cfg.MODEL.SWINT.NUM_HEADS = spec.swin_embed, spec.swin_heads
    cfg.MODEL.SWINT.WINDOW_SIZE, cfg.MODEL.SWINT.OUT_CHANNELS = spec.window, spec.swin_dims
    cfg.MODEL.SWINT.DEPTHS = spec.swin_depths
    cfg.MODEL.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS = spec.bert_layers
    cfg.MODEL.LANGUAGE_BACKBONE.QV_START = spec.qv_start
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = spec.vocab
    cfg.MODEL.DYHEAD.NUM_CONVS = spec.dyhead_convs
    cfg.MODEL.DYHEAD.NUM_CLASSES = spec.num_classes
    cfg.MODEL.ATSS.DETECTIONS_PER_IMG = spec.detections_per_img
    cfg.MODEL.COMPUTE_DTYPE = pc._DTYPE_NAME[pc.H16]
    cfg.MODEL.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER = linear
    cfg.VISION_QUERY.LEARNABLE_BANK, cfg.VISION_QUERY.ADD_VISION_LAYER = learnable, vision
    return spec, sd, GeneralizedVLRCNN_New(cfg, tokenizer=object())


# ---------------------------------------------------------------------------------------------- 9: the prompt offset against the oracle
_ORACLE = {}


def oracle_with_offset(spec, sd, inputs, W):
    """oracle.detector.forward with `W[:T]` added to `embedded` and `hidden` between the language backbone and the head
    (vldyhead.py:955-958), and the same without: (detections, head) of each.  CPU, fp32; computed once per operand rounding."""
    import parity_checks as pc
    from oracle import detector as od
    from oracle.backbone import fpn_forward, swin_forward
    from oracle.head import vldyhead
    from oracle.language import language_backbone
    from oracle.postprocess import atss_postprocess, grid_anchors
    if pc.H16 in _ORACLE:
        return _ORACLE[pc.H16]
    images, sizes, ids, am, pm, bank = inputs
    B = images.shape[0]
    with torch.no_grad():
        feats = fpn_forward(sd, "backbone.fpn", swin_forward(sd, "backbone.body", images, spec))
        labels, amap = od.labels_and_maps(pm, spec.max_query_len)
        vision, vmask = od.select_queries(bank, [labels] * B, [amap] * B, spec.num_query_per_class)
        lang = language_backbone(sd, "language_backbone.body", ids, am, vision, od.pooled_fpn_tokens(feats), vmask, spec)
        anchors = grid_anchors([f.shape[-2:] for f in feats], spec)
        out = []
        T = lang["hidden"].shape[1]
        for w in (W, None):
            l = dict(lang)
            if w is not None:
                l["embedded"], l["hidden"] = w[:T][None] + lang["embedded"], w[:T][None] + lang["hidden"]
            head = vldyhead(sd, "rpn.head", feats, l, spec)
            out.append((atss_postprocess(head["bbox_reg"], head["centerness"], head["dot_product_logits"], anchors, sizes, pm, spec), head))
    _ORACLE[pc.H16] = out
    return out


def prompt_offset_rows(dev, min_separation=10.0):
    """The rows of check_full_model that lie behind the offset, for the tiny model with ADD_LINEAR_LAYER and W = W_SCALE x randn loaded."""
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    from mq_det_amd.utils.checkpoint import load_reference_checkpoint
    spec, sd, model = tiny_model(dev, linear=True)
    W = prompt_w(spec.bert_hidden)
    res = load_reference_checkpoint(model, {"model": {"module." + k: v for k, v in {**sd, "rpn.tunable_linear.weight": W}.items()}}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.to(dev)
    inputs = pc.make_inputs(spec)
    images, sizes, ids, am, pm, bank = inputs
    (dets, h), (_, h_plain) = oracle_with_offset(spec, sd, inputs, W)
    live = am.bool()
    # precondition (CPU, fp32): the offset moves the compared tensor by far more than the gate, else the rows below could pass without it
    gate = 1.5e-2 * pc.TOL_SCALE * max(1.0, float(h["hidden"][live].abs().max()))
    moved = float((h["hidden"][live] - h_plain["hidden"][live]).abs().max())
    assert moved > min_separation * gate, (moved, gate)
    model.load_query_bank(bank)
    with torch.no_grad():
        raw = model(ImageList(images.to(dev), sizes), captions=None, positive_map=pm, return_raw=True, input_ids=ids.to(dev),
                    attention_mask=am.to(dev))
    tag = " [prompt offset]"
    rows = [pc._stat("full: head text hidden (caption tokens)" + tag, raw["head"]["hidden"].cpu()[live], h["hidden"][live], tol=1.5e-2)]
    # ... and the same tensor is far from the oracle WITHOUT the offset: the model applied it
    off = pc._stat("full: head text hidden vs the oracle without W" + tag, raw["head"]["hidden"].cpu()[live], h_plain["hidden"][live], tol=1.5e-2)
    assert not off["ok"] and off["max_err"] > 0.5 * moved, off
    for l in range(5):
        cls_ref = torch.stack([h["dot_product_logits"][l].sigmoid()[:, :, torch.tensor(pm[k])].mean(-1) for k in pm], -1)
        rows.append(pc._stat(f"full: class scores lvl{l}" + tag, raw["post"]["cls"][l], cls_ref, tol=3.3e-2))
    post = raw["post"]
    for b in range(len(dets)):
        n = int(post["counts"][b])
        gb, gs, gl = post["boxes"][b, :n].cpu(), post["scores"][b, :n].cpu(), post["labels"][b, :n].cpu()
        rb, rs, rl = dets[b]["boxes"], dets[b]["scores"], dets[b]["labels"]
        top = torch.argsort(rs, descending=True)[:50]
        matched = 0
        for i in top.tolist():                                                      # the matching rule of check_full_model
            same = (gl == rl[i])
            if not same.any():
                continue
            lt, br = torch.max(gb[:, :2], rb[i, :2]), torch.min(gb[:, 2:], rb[i, 2:])
            inter_a = (br - lt + 1).clamp(min=0).prod(1)
            a1 = (gb[:, 2] - gb[:, 0] + 1) * (gb[:, 3] - gb[:, 1] + 1)
            a2 = (rb[i, 2] - rb[i, 0] + 1) * (rb[i, 3] - rb[i, 1] + 1)
            iou = torch.where(same, inter_a / (a1 + a2 - inter_a), torch.zeros_like(a1))
            j = int(iou.argmax())
            if iou[j] > (0.9 if pc.TOL_SCALE == 1.0 else 0.8) and abs(float(gs[j] - rs[i])) < 0.02 * pc.TOL_SCALE:
                matched += 1
        frac = matched / max(1, len(top))
        rows.append({"name": f"full: top-50 detections matched img{b} n_hip={n} n_ref={len(rb)}" + tag, "max_err": 1 - frac, "mean_err": 0.0,
                     "ref_absmax": 1.0, "norm_err": 1 - frac, "tol": 0.2, "ok": frac >= 0.8})
    for r in rows:
        print(f"{r['name']}: max_err={r['max_err']:.3e} norm={r['norm_err']:.3e} tol={r['tol']} elem_viol={r.get('elem_viol_frac', 0):.1e}", flush=True)
    return rows


def _assert_rows(rows):
    bad = [r for r in rows if not r["ok"]]
    assert not bad, "\n".join(f"{r['name']}: max_err={r['max_err']:.3e} norm={r['norm_err']:.3e} tol={r['tol']}" for r in bad)


def test_prompt_offset_against_the_oracle(dev):
    _assert_rows(prompt_offset_rows(dev))


def test_prompt_offset_against_the_oracle_bf16(dev):
    """bf16 operands: every gate x TOL_SCALE = 8.  The head's hidden states are LayerNorm outputs, so no W moves them by more than about 70 x
    the fp16 gate (measured on the oracle for 1 x ... 5 x randn): 10 x the bf16 gate cannot be had.  The same W as in the fp16 test moves them
    by 2.2 x the bf16 gate; the run asserts 2 x, and that the result is outside the gate of the oracle without W."""
    import parity_checks as pc
    pc.use_dtype(torch.bfloat16)
    try:
        _assert_rows(prompt_offset_rows(dev, min_separation=2.0))
    finally:
        pc.use_dtype(torch.float16)


def test_prompt_offset_against_the_oracle_split_precise(dev):
    """MODEL.COMPUTE_DTYPE = float32 with the fp32-operand kernels: 1e-3 of the range, and no element outside 1e-3 + 1e-3 |ref|."""
    import parity_checks as pc
    from mq_det_amd import ops
    prev = os.environ.get("MQ_F32_OPERANDS")
    os.environ["MQ_F32_OPERANDS"] = "1"
    ops.configure()
    pc.use_dtype(torch.float32)
    try:
        rows = prompt_offset_rows(dev)
        _assert_rows(rows)
        stat_rows = [r for r in rows if "elem_viol_frac" in r]
        assert len(stat_rows) == 6 and all(r["tol"] <= 1e-3 for r in stat_rows)
        assert all(r["elem_viol_frac"] == 0.0 for r in stat_rows), [(r["name"], r["elem_viol_frac"]) for r in stat_rows]
    finally:
        pc.use_dtype(torch.float16)
        if prev is None:
            os.environ.pop("MQ_F32_OPERANDS", None)
        else:
            os.environ["MQ_F32_OPERANDS"] = prev
        ops.configure()


# ---------------------------------------------------------------------------------------------- 10, 12: a fully fine-tuned tiny model
class _Tuned:
    """The tiny model with all three switches on, loaded from a checkpoint in the reference's layout: W and Wv non-zero, a learnable bank of
    at most NUM_QUERY_PER_CLASS rows per label (no draw: calls of different batch shapes select the same rows)."""

    def __init__(self, dev):
        import parity_checks as pc
        from mq_det_amd.structures import ImageList
        from mq_det_amd.utils.checkpoint import load_reference_checkpoint
        self.spec, self.sd, self.model = tiny_model(dev, linear=True, learnable=True, vision=True)
        images, sizes, ids, am, self.pm, bank0 = pc.make_inputs(self.spec)
        k = self.model.cfg.VISION_QUERY.NUM_QUERY_PER_CLASS
        g = torch.Generator().manual_seed(12)
        counts = [k, 1, 2, k, 3, 1]
        self.bank = {l: torch.randn(n, *bank0[l].shape[1:], generator=g) for (l, n) in zip(bank0, counts)}
        C = next(iter(self.bank.values())).shape[-1]
        self.W = [prompt_w(self.spec.bert_hidden, seed=s) for s in (7, 8)]
        self.Wv = 0.5 * torch.randn(1000, C, generator=g)
        self.ckpt = lambda w: {"model": {"module." + k_: v for k_, v in {
            **self.sd, "rpn.tunable_linear.weight": w, "query_selector.tunable_vision_linear.weight": self.Wv,
            **{f"query_selector.query_bank.{l}": v for l, v in self.bank.items()}}.items()}, "iteration": 3}
        res = load_reference_checkpoint(self.model, self.ckpt(self.W[0]), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        self.model.to(dev)
        self.dev = dev
        self.il = lambda: ImageList(images.to(dev), sizes)
        self.kw = dict(captions=None, positive_map=self.pm, input_ids=ids.to(dev), attention_mask=am.to(dev))
        kv = int(am[0].sum())
        self.tokenize = lambda caps, d: (ids[:1].expand(len(caps), -1).contiguous().to(d), am[:1].expand(len(caps), -1).contiguous().to(d), kv)


@pytest.fixture(scope="module")
def tuned(dev):
    return _Tuned(dev)


def test_entry_points_agree_with_every_offset_on(dev, tuned):
    """`forward_chunks` over two chunks and `forward_grounding` over two items with different query counts (padding rows inside a real
    forward), W and Wv non-zero: the resident bank against the learnable parameters (dict path) bit for bit -- the criterion of
    tests/test_gpu_query_select.py --, and the chunked call against per-call `model(...)` by the rule for comparisons across batch shapes
    (tests/test_gpu_parity.py _same_detections)."""
    from test_gpu_parity import _same_detections
    from mq_det_amd.utils.checkpoint import load_reference_checkpoint
    s, model = tuned, tuned.model
    load_reference_checkpoint(model, s.ckpt(s.W[0]), strict=True)
    labs = list(s.pm)
    chunks = [("caption a", {l: s.pm[l] for l in labs[:4]}), ("caption b", {l: s.pm[l] for l in labs[3:]})]
    caps, maps = ["caption a", "caption b"], [{l: s.pm[l] for l in labs[:4]}, {l: s.pm[l] for l in labs[4:]}]
    saved = model.use_hip_graph
    try:
        model.tokenize = s.tokenize
        model.use_hip_graph = False
        runs = []
        sel = model.query_selector
        for resident in (False, True):
            if resident:
                model.load_query_bank(QueryBank.from_state_dict(model.state_dict(), dev))
                assert sel._resident() is not None and isinstance(sel.query_bank, nn.ParameterDict)
            else:
                assert sel._resident() is None and isinstance(sel.query_bank, nn.ParameterDict)
            outs = []
            for call in (lambda: [model(s.il(), **{**s.kw, "positive_map": pm}) for _, pm in chunks],
                         lambda: model.forward_chunks(s.il(), chunks), lambda: model.forward_grounding(s.il(), caps, maps)):
                model.clear_caches()
                outs.append(call())
            runs.append(outs)
        (pd, cd, gd), (pr, cr, gr) = runs
        assert sum(len(o) for o in cd[0]) > 0 and len(cd) == len(cr) == 2
        for x, y in ((pr, pd), (cr, cd)):
            for chunk_r, chunk_d in zip(x, y):
                for a, b in zip(chunk_r, chunk_d):
                    assert _equal_detections(a, b)
        for a, b in zip(gr, gd):
            assert _equal_detections(a, b)
        for per_call, chunk in zip(pr, cr):
            for a, b in zip(chunk, per_call):
                assert _same_detections(a, b)
        # the vision offset reaches the forward: with Wv = 0 the same call gives other detections
        sd = {k: v for k, v in model.state_dict().items()}
        sd["query_selector.tunable_vision_linear.weight"] = torch.zeros_like(s.Wv)
        model.load_state_dict(sd, strict=True)
        model.clear_caches()
        plain = model.forward_grounding(s.il(), caps, maps)
        assert not all(_equal_detections(a, b) for a, b in zip(plain, gr))
    finally:
        model.use_hip_graph = saved
        model.__dict__.pop("tokenize", None)
        model.load_query_bank(None)                                                 # select from the parameters again
        model.clear_caches()


def test_graph_replay_follows_load_state_dict(dev, tuned):
    from mq_det_amd.utils.checkpoint import load_reference_checkpoint
    s, model = tuned, tuned.model
    saved = model.use_hip_graph
    try:
        eager = []
        model.use_hip_graph = False
        for w in s.W:
            load_reference_checkpoint(model, s.ckpt(w), strict=True)
            eager.append(model(s.il(), **s.kw))
        assert sum(len(o) for o in eager[0]) > 0
        assert not all(_equal_detections(a, b) for a, b in zip(*eager))             # another prompt, other detections
        model.use_hip_graph = True
        il = s.il()
        for n, w in enumerate(s.W):
            load_reference_checkpoint(model, s.ckpt(w), strict=True)                # drops the plan and every captured graph
            assert not model._graphs
            replays = model.cache_stats["graph_replay"]
            for call in range(4):                                                   # eager, capture + replay, replays
                out = model(il, **s.kw)
                for a, b in zip(out, eager[n]):
                    assert _equal_detections(a, b), (n, call)
            assert any(e.get("stage") == 2 for e in model._graphs.values()), "HIP graph was not captured"
            assert model.cache_stats["graph_replay"] >= replays + 2
    finally:
        model.use_hip_graph = saved
        model.clear_caches()


# ---------------------------------------------------------------------------------------------- 11: the selector on the device
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("S", [1, 5])
def test_select_with_a_vision_offset_on_the_device(dev, S, dtype):
    from mq_det_amd import ops
    for C in (256, 6):
        bank = QueryBank.from_dict(sc.make_dict(C, S), dev)
        res, ref = fc.offset_selectors(bank, fc.seeded_wv(C))
        res.to(dev)
        plain = sc.selectors(bank)[1]
        for n_items in (1, 2):
            v, i = sc.same_select(res, ref, [sc.LABELS] * n_items, [sc.PMAP] * n_items, dtype=dtype, device=dev)
            assert v.is_cuda and i.is_cuda
            v0, _ = sc.seeded(lambda: plain.select([sc.LABELS] * n_items, [sc.PMAP] * n_items, sc.T, dev, dtype), 5)[0]
            assert not torch.equal(v, v0)
        v, _ = sc.same_select(res, ref, *sc.RAGGED, dtype=dtype, device=dev)
        lens = [sum(min(sc.COUNTS.get(l, 0), sc.K) for l in labs) * S for labs in sc.RAGGED[0]]
        for i, n in enumerate(lens):                                                # padding rows: exact zeros
            assert not v[i, n:].view(torch.int32 if dtype == torch.float32 else torch.int16).any()
        items = 62
        sc.same_select(res, ref, [sc.LABELS] * items, [sc.PMAP] * items, dtype=dtype, device=dev, seed=9)
        assert not res.deterministic(sc.LABELS)
        ops.start_timing()
        try:
            res.select([sc.LABELS] * 2, [sc.PMAP] * 2, sc.T, dev, dtype)
        finally:
            rec = ops.stop_timing()
        assert set(rec) == {"bank_select"} and rec["bank_select"][0] == 1, rec
        with pytest.raises(ValueError, match="ADD_VISION_LAYER"):                   # more rows than the offset has: refused before the launch
            res.tunable_vision_linear.weight = nn.Parameter(fc.seeded_wv(C)[:11 * S - 1].to(dev), requires_grad=False)
            res._drop_memos()
            res.select([sc.LABELS], [sc.PMAP], sc.T, dev, dtype)
