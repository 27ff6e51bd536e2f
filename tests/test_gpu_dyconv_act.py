"""KERNELS["DYCONV_EPILOGUE_LN"] on the device: mq_dyconv_coef_relu_group + mq_dyconv_fuse_act_group (csrc/dyconv.hip).
  * the kernel checks of tests/dyconv_act_checks.py (the ones tests/test_dyconv_act_cpu.py runs through the emulation), fp16 and bf16, in a
    process of their own -- a wrong address on the device is a memory fault, not an exception;
  * the head of the tiny model with the switch 1 against 0: LN(v) of every fusion layer, the final token buffer and the head's outputs within
    the tolerance check_dyconv uses for "LN(dyconv(x))" (2.5e-3 of the range; 8 x for bf16);
  * one DyConv layer + the next LayerNorm against the oracle (oh.dyconv + F.layer_norm, as check_dyconv restates it): the new path's error
    is at most 1.5 x the old path's on the same inputs;
  * the tiny full model with the switch on: every replay of its captured HIP graph returns the bytes of the eager forward."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

pytestmark = pytest.mark.gpu

SIZES = [(20, 24), (10, 12), (5, 6), (3, 3), (2, 2)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    from mq_det_amd import ops
    ops.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def kernels_ok(dev):
    """The kernel checks in a process of their own, once per session; the in-process tests below run only on kernels that passed them."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "kernels"], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "OK kernels" in r.stdout, f"rc {r.returncode}\n{(r.stdout + r.stderr)[-3000:]}"
    return True


def test_kernels_isolated(kernels_ok):
    assert kernels_ok


@pytest.fixture(params=[torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def pc(request):
    import parity_checks
    parity_checks.use_dtype(request.param)
    yield parity_checks
    parity_checks.use_dtype(torch.float16)


def _head_run(pc, dev, switch):
    """vldyhead of the tiny model on seeded inputs with KERNELS["DYCONV_EPILOGUE_LN"] = switch -> (LN(v) per fusion layer, head dict)"""
    from mq_det_amd import ops
    from mq_det_amd.modeling import pipeline
    spec, sd, cfg, model, P = pc.tiny(dev)
    g = torch.Generator().manual_seed(51)
    feats = [torch.randn(2, 256, h, w, generator=g).to(pc.H16).to(dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    hidden = torch.randn(2, 64, spec.bert_hidden, generator=g).to(pc.H16).to(dev)
    am = torch.ones(2, 64)
    am[0, 30:] = 0
    lang = {"hidden": hidden, "key_bias": ((1.0 - am) * -1e30).to(dev)}
    v_lns, real = [], pipeline.vl_image_side
    saved = ops.KERNELS["DYCONV_EPILOGUE_LN"]

    def spy(P_, b, v_ln, *a, **k):
        v_lns.append(v_ln)
        return real(P_, b, v_ln, *a, **k)
    pipeline.vl_image_side = spy
    ops.KERNELS["DYCONV_EPILOGUE_LN"] = switch
    try:
        with torch.no_grad():
            head = pipeline.vldyhead(P, cfg, feats, lang)
        torch.cuda.synchronize()
    finally:
        pipeline.vl_image_side = real
        ops.KERNELS["DYCONV_EPILOGUE_LN"] = saved
    assert len(v_lns) == cfg.MODEL.DYHEAD.NUM_CONVS >= 2
    return v_lns, head


def test_head_switch_on_against_off(dev, kernels_ok, pc):
    from mq_det_amd import ops
    launched = []
    real = ops.dyconv_fuse_act_group
    ops.dyconv_fuse_act_group = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
    try:
        v1, h1 = _head_run(pc, dev, 1)
        n_on = len(launched)
        v0, h0 = _head_run(pc, dev, 0)
    finally:
        ops.dyconv_fuse_act_group = real
    assert n_on == len(v1) and len(launched) == n_on, "the switch does not select the fused pass (or selects it when off)"
    assert torch.equal(v1[0], v0[0])                      # layer 0's LN(v) is the same launch on the same input
    res = [pc._stat(f"DYCONV_EPILOGUE_LN 1 vs 0: LN(v) of fusion layer {i}", a, b.float().cpu(), tol=2.5e-3) for i, (a, b) in enumerate(zip(v1, v0)) if i]
    res += [pc._stat(f"DYCONV_EPILOGUE_LN 1 vs 0: head['{k}']", h1[k], h0[k].float().cpu(), tol=2.5e-3) for k in ("tok", "tk16", "tbias", "hidden") if k in h0]
    assert "tok" in h0 and "tok" in h1
    for r in res:
        print(f"{r['name']}: norm_err {r['norm_err']:.3e} (tol {r['tol']:.1e})")
    bad = [r for r in res if not r["ok"]]
    assert not bad, "\n".join(f"{r['name']}: norm_err {r['norm_err']:.3e} > {r['tol']:.1e}" for r in bad)


def test_layer_against_the_oracle_no_worse_than_before(dev, kernels_ok, pc):
    from oracle import head as oh
    from mq_det_amd import ops
    from mq_det_amd.modeling import pipeline
    spec, sd, cfg, model, P = pc.tiny(dev)
    g = torch.Generator().manual_seed(16)
    feats = [torch.randn(2, 256, h, w, generator=g).to(pc.H16) for h, w in SIZES]
    b = "rpn.head.dyhead_tower.2"
    gw, gb = P["rpn.head.dyhead_tower.3.b_attn.layer_norm_v.weight"], P["rpn.head.dyhead_tower.3.b_attn.layer_norm_v.bias"]
    with torch.no_grad():
        ref = oh.dyconv(sd, b, [f.float() for f in feats], spec)
        ref_tok = torch.cat([r.flatten(2).transpose(1, 2) for r in ref], 1)
        ref_ln = F.layer_norm(ref_tok, (256,), gw.float().cpu(), gb.float().cpu(), 1e-5)
        tok, szs = pipeline._to_tokens([f.to(dev).contiguous(memory_format=torch.channels_last) for f in feats])
        tok = tok.contiguous()
        pre, coef = pipeline.dyconv_tokens(P, cfg, b, tok, szs, defer_relu=True)
        old_ln = ops.dyrelu_layer_norm(pre, coef, szs, gw, gb, 1e-5)
        new_ln = pipeline.dyconv_tokens_act(P, cfg, b, tok, szs, ln=(gw, gb, 1e-5))
        old_tok = pipeline.dyconv_tokens(P, cfg, b, tok, szs)
        new_tok = pipeline.dyconv_tokens_act(P, cfg, b, tok, szs)
    for name, new, old, want in (("LN(dyconv(x))", new_ln, old_ln, ref_ln), ("dyconv(x)", new_tok, old_tok, ref_tok)):
        rn, ro = pc._stat(f"{name}, fused pass", new, want, tol=2.5e-3), pc._stat(f"{name}, today's path", old, want, tol=2.5e-3)
        print(f"{name} vs the oracle: new {rn['norm_err']:.3e} old {ro['norm_err']:.3e}")
        assert rn["ok"], f"{name}: norm_err {rn['norm_err']:.3e} > {rn['tol']:.1e}"
        assert rn["norm_err"] <= 1.5 * ro["norm_err"], f"{name}: error against the oracle {rn['norm_err']:.3e} > 1.5 x {ro['norm_err']:.3e}"


def test_last_layer_grouped_apply_equals_the_per_level_launches(dev, kernels_ok, pc):
    """KERNELS["DYRELU_APPLY_GROUPED"]: dyconv_tokens without defer_relu (the last DyConv layer) applies DYReLU in one launch -- the same bits"""
    from mq_det_amd import ops
    from mq_det_amd.modeling import pipeline
    spec, sd, cfg, model, P = pc.tiny(dev)
    g = torch.Generator().manual_seed(17)
    feats = [torch.randn(2, 256, h, w, generator=g).to(pc.H16).to(dev).contiguous(memory_format=torch.channels_last) for h, w in SIZES]
    tok, szs = pipeline._to_tokens(feats)
    tok = tok.contiguous()
    launched, real, saved = [], ops.dyrelu_apply_group_, ops.KERNELS["DYRELU_APPLY_GROUPED"]
    ops.dyrelu_apply_group_ = lambda *a, **k: (launched.append(1), real(*a, **k))[1]
    try:
        with torch.no_grad():
            ops.KERNELS["DYRELU_APPLY_GROUPED"] = 1
            new = pipeline.dyconv_tokens(P, cfg, "rpn.head.dyhead_tower.2", tok, szs)
            n_on = len(launched)
            ops.KERNELS["DYRELU_APPLY_GROUPED"] = 0
            old = pipeline.dyconv_tokens(P, cfg, "rpn.head.dyhead_tower.2", tok, szs)
    finally:
        ops.dyrelu_apply_group_, ops.KERNELS["DYRELU_APPLY_GROUPED"] = real, saved
    assert n_on == 1 and len(launched) == 1, "the switch does not select the grouped launch (or selects it when off)"
    assert torch.equal(new, old)


def _equal_detections(a, b):
    return (len(a) == len(b) and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
            and torch.equal(a.get_field("labels"), b.get_field("labels")))


def test_hip_graph_replay_matches_eager_with_the_switch_on(dev, kernels_ok, monkeypatch):
    import parity_checks as pc
    from mq_det_amd import ops
    from mq_det_amd.structures import ImageList
    monkeypatch.setenv("MQ_DYCONV_EPILOGUE_LN", "1")
    pc._CACHE.clear()                                     # a model whose prepare() reads the switch
    launched = []
    real = ops.dyconv_fuse_act_group
    monkeypatch.setattr(ops, "dyconv_fuse_act_group", lambda *a, **k: (launched.append(1), real(*a, **k))[1])
    try:
        spec, sd, cfg, model, P = pc.tiny(dev)
        images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
        model.load_query_bank(bank)
        il = ImageList(images.to(dev), sizes)
        kw = dict(captions=None, positive_map=pm, input_ids=ids.to(dev), attention_mask=am.to(dev))
        model.use_hip_graph = False
        ref = model(il, **kw)
        assert launched, "the model did not take the fused pass"
        model.use_hip_graph = True
        model.clear_caches()
        outs = [model(il, **kw) for _ in range(4)]           # eager, capture + replay, replay, replay
        assert any(e.get("stage") == 2 for e in model._graphs.values()), "HIP graph was not captured"
        for out in outs:
            for a, b_ in zip(out, ref):
                assert _equal_detections(a, b_)
    finally:
        pc._CACHE.clear()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import dyconv_act_checks as dc
    for row in dc.run_all(torch.device("cuda:0")):
        pass
    torch.cuda.synchronize()
    print("OK kernels")
