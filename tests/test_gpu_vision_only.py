"""Vision-only evaluation on the MI355X (VISION_QUERY.MASK_DURING_INFERENCE True, TEXT_DROPOUT 1.0; generalized_vl_rcnn_new.py:397-407): the
words of every label that has vision queries reach the language backbone as [MASK].  The expected result is always the SAME model with the
mode off, given `input_ids=` with the [MASK] id already written at the expected positions (caller-supplied ids are never masked): the same
kernels on the same values give the same bytes, the argument of test_backbone_and_caption_caches.  Tiny model of parity_checks.py, the
synthetic tokenizer, six-class captions.  Every test runs its body in a process of its own under a time limit (a fault or a hang fails that
test, not the session)."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def _f32_mode():
    import parity_checks as pc
    from mq_det_amd import ops
    os.environ["MQ_F32_OPERANDS"] = "1"
    ops.configure()
    pc.use_dtype(torch.float32)
    return pc


class _Setup:
    """Three six-class captions (labels 1-6, 7-12, 13-18) of the synthetic tokenizer, a bank with rows for all 18 labels, two small images."""

    def __init__(self, pc=None):
        if pc is None:
            import parity_checks as pc
        from transformers import AutoTokenizer
        from mq_det_amd.structures import ImageList
        from mq_det_amd.utils.tokenizer import build_synthetic_tokenizer, synthetic_caption, positive_map_from_spans
        from oracle import tiny_spec
        from oracle.weights import make_query_bank
        self.pc, self.spec = pc, tiny_spec()
        self.tk = AutoTokenizer.from_pretrained(build_synthetic_tokenizer(tempfile.mkdtemp(), size=self.spec.vocab))
        assert self.tk.mask_token_id is not None
        self.caps = []
        for c in range(3):
            cap, spans = synthetic_caption(6, start=10 * c, words=(1, 2))
            self.caps.append((cap, positive_map_from_spans(self.tk, cap, spans, list(range(1 + 6 * c, 7 + 6 * c)))))
        self.bank = make_query_bank(range(1, 19), self.spec)
        self.images, self.sizes, *_ = pc.make_inputs(self.spec)
        self.ImageList = ImageList

    def model(self, mode_on, bank="all", caches=False):
        """A freshly built tiny model (the same seeded weights every time) with the tokenizer and `bank` loaded."""
        spec, self.sd, cfg, model, _ = self.pc._tiny(DEV)
        model.tokenizer = self.tk
        cfg.VISION_QUERY.MASK_DURING_INFERENCE, cfg.VISION_QUERY.TEXT_DROPOUT = bool(mode_on), 1.0 if mode_on else 0.0
        if bank is not None:
            model.load_query_bank(self.bank if isinstance(bank, str) else bank)
        model.backbone_cache = model.use_hip_graph = caches
        return model

    def without(self, *labels):
        return {k: v for k, v in self.bank.items() if k not in labels}

    def il(self):
        return self.ImageList(self.images.to(DEV).clone(), self.sizes)

    def ids(self, model, cap, pm, masked_labels):
        """The tokenizer's ids of `cap` for both images with the [MASK] id at the tokens of `masked_labels`, and the attention mask."""
        ids, am, _ = model.tokenize([cap] * 2, DEV)
        ids = ids.clone()
        for lab in masked_labels:
            ids[:, pm[lab]] = self.tk.mask_token_id
        return ids, am


def _equal(out, ref):
    from test_gpu_parity import _equal_detections
    assert len(out) == len(ref)
    return all(_equal_detections(a, b) for a, b in zip(out, ref))


def _body_masked_equals_caller_masked_ids():
    s = _Setup()
    A, B = s.model(True), s.model(False)
    n = 0
    for cap, pm in s.caps[:2]:
        out = A(s.il(), captions=[cap] * 2, positive_map=pm)
        ids, am = s.ids(B, cap, pm, list(pm))
        ref = B(s.il(), captions=None, positive_map=pm, input_ids=ids, attention_mask=am)
        assert _equal(out, ref), cap
        plain_ids, _ = s.ids(B, cap, pm, [])
        assert not torch.equal(plain_ids, ids)
        plain = B(s.il(), captions=None, positive_map=pm, input_ids=plain_ids, attention_mask=am)
        assert not _equal(plain, ref), "masking the words changes nothing on these weights: the check cannot tell the modes apart"
        assert _equal(plain, B(s.il(), captions=[cap] * 2, positive_map=pm))     # mode off: the tokenizer's ids as they are
        n += sum(len(o) for o in out)
    assert n > 0
    print(f"OK vision-only == caller-masked ids ({n} detections)", flush=True)


def _body_f32_vs_oracle():
    """MODEL.COMPUTE_DTYPE float32: language hidden states and class scores of the mode-on forward against the fp32 oracle fed the masked ids,
    through parity_checks._stat like the tiny split-precise check (check_full_model under use_dtype(float32): F32_TOL of the reference's range
    and the element-wise 1e-3 + 1e-3 |ref| count)."""
    from oracle import detector as od
    from test_gpu_parity import _assert_f32
    pc = _f32_mode()
    s = _Setup(pc)
    A = s.model(True)
    cap, pm = s.caps[0]
    ids, am = s.ids(A, cap, pm, list(pm))
    ids, am = ids.cpu(), am.cpu()
    with torch.no_grad():
        _, inter = od.forward(s.sd, s.spec, s.images, s.sizes, ids, am, pm, s.bank, return_intermediates=True)
        raw = A(s.il(), captions=[cap] * 2, positive_map=pm, return_raw=True)
    live = am.bool()
    res = [pc._stat("full: language hidden, vision-only", raw["lang"]["hidden"].cpu()[live], inter["lang"]["hidden"][live], tol=2e-2)]
    h = inter["head"]
    for l in range(5):
        cls_ref = torch.stack([h["dot_product_logits"][l].sigmoid()[:, :, torch.tensor(pm[k])].mean(-1) for k in pm], -1)
        res.append(pc._stat(f"full: class scores lvl{l}, vision-only", raw["post"]["cls"][l], cls_ref, tol=3.3e-2))
    for r in res:
        print(f"{'OK' if r['ok'] else 'MISMATCH'} {r['name']}: norm_err {r['norm_err']:.3e} tol {r['tol']:g} elem_viol {r['elem_viol_frac']:.1e}", flush=True)
    assert all(r["tol"] <= pc.F32_TOL for r in res)
    _assert_f32(res)
    # the oracle can tell the modes apart as well: the unmasked caption gives other hidden states
    plain, _ = s.ids(A, cap, pm, [])
    with torch.no_grad():
        _, inter0 = od.forward(s.sd, s.spec, s.images, s.sizes, plain.cpu(), am, pm, s.bank, return_intermediates=True)
    assert not pc._stat("full: language hidden, masked vs plain", inter0["lang"]["hidden"][live], inter["lang"]["hidden"][live], tol=2e-2)["ok"]


def _body_label_without_rows_keeps_its_words():
    s = _Setup()
    cap, pm = s.caps[0]
    bank = s.without(4)
    A, B = s.model(True, bank), s.model(False, bank)
    out = A(s.il(), captions=[cap] * 2, positive_map=pm)
    ids, am = s.ids(B, cap, pm, [lab for lab in pm if lab != 4])
    assert _equal(out, B(s.il(), captions=None, positive_map=pm, input_ids=ids, attention_mask=am))
    all_ids, _ = s.ids(B, cap, pm, list(pm))
    assert not _equal(out, B(s.il(), captions=None, positive_map=pm, input_ids=all_ids, attention_mask=am)), "label 4 was masked"
    print("OK a label without bank rows keeps its words", flush=True)


def _protocol_loop(s, model, refs):
    """The LVIS protocol of test_backbone_and_caption_caches: every caption for the same pixels, four images; -> cache_stats of the loop."""
    model.cache_stats = {k: 0 for k in model.cache_stats}
    for rep in range(4):
        il = s.il()
        for (cap, pm), ref in zip(s.caps, refs):
            assert _equal(model(il, captions=[cap] * 2, positive_map=pm), ref), (rep, cap[:20])
    return dict(model.cache_stats)


def _uncached(s, model):
    caches = model.backbone_cache, model.use_hip_graph
    model.backbone_cache = model.use_hip_graph = False
    refs = [model(s.il(), captions=[cap] * 2, positive_map=pm) for cap, pm in s.caps]
    model.backbone_cache, model.use_hip_graph = caches
    return refs


def _cached_loops(s):
    """One model: the protocol loop with the mode off, then with the mode on, each against its own uncached forwards."""
    A = s.model(True, caches=True)
    VQ = A.cfg.VISION_QUERY
    VQ.MASK_DURING_INFERENCE = False
    off_refs = _uncached(s, A)
    off = _protocol_loop(s, A, off_refs)
    A.clear_caches()
    VQ.MASK_DURING_INFERENCE = True
    on_refs = _uncached(s, A)
    assert not any(_equal(a, b) for a, b in zip(on_refs, off_refs))
    on = _protocol_loop(s, A, on_refs)
    print(f"cache_stats mode off {off}\ncache_stats mode on  {on}", flush=True)
    return A, off, on, on_refs


def _body_caches_and_graph_replay():
    s = _Setup()
    A, off, on, _ = _cached_loops(s)
    assert off["front_hit"] > 0 and off["graph_replay"] > 0
    assert on["front_hit"] >= off["front_hit"] and on["graph_replay"] >= off["graph_replay"], (on, off)
    assert on["backbone_hit"] == off["backbone_hit"] and on["backbone_miss"] == off["backbone_miss"], (on, off)
    # a replay takes the memoised masked ids: the same tensor objects call after call, one pair per caption
    cap, pm = s.caps[0]
    tok = A.tokenize([cap] * 2, DEV)[0]
    pm_key, labels, cleaned = _pm(pm, A)
    ids = [A._masked_ids(tok, (cap,) * 2, pm_key, labels, cleaned, DEV)[0] for _ in range(2)]
    assert ids[0] is ids[1] and bool((ids[0] == s.tk.mask_token_id).any())
    print("OK caches and graph replay with the mode on", flush=True)


def _pm(pm, model):
    from mq_det_amd.modeling.query_selector import prepare_positive_map
    pm, labels, pm_key, *_ = prepare_positive_map(pm, model.cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN)
    return pm_key, labels, pm


def _body_bank_change():
    s = _Setup()
    A, _, _, on_refs = _cached_loops(s)
    bank = s.without(2, 5)
    fresh = s.model(True, bank)
    refs = [fresh(s.il(), captions=[cap] * 2, positive_map=pm) for cap, pm in s.caps]
    assert not _equal(refs[0], on_refs[0])                   # the bank matters: stale ids, a stale front or a stale graph input would show
    A.load_query_bank(bank)                                  # no clear_caches()
    il = s.il()
    replays = A.cache_stats["graph_replay"]
    for rep in range(4):                                     # eager, capture + replay, replays -- and the cached pixels / fronts from call 2 on
        for (cap, pm), ref in zip(s.caps, refs):
            assert _equal(A(il, captions=[cap] * 2, positive_map=pm), ref), (rep, cap[:20])
    assert A.cache_stats["graph_replay"] > replays
    A.use_hip_graph = False
    for (cap, pm), ref in zip(s.caps, refs):                 # eager, through the feature and front caches
        assert _equal(A(il, captions=[cap] * 2, positive_map=pm), ref)
    print("OK bank change without clear_caches()", flush=True)


def _body_forward_chunks():
    from test_gpu_parity import _same_detections
    s = _Setup()
    A = s.model(True)
    on_refs = _uncached(s, A)
    A.backbone_cache = A.use_hip_graph = True
    il = s.il()
    for _ in range(3):                                       # eager, capture, replay
        batched = A.forward_chunks(il, s.caps)
    assert len(batched) == len(s.caps)
    for out, ref in zip(batched, on_refs):
        assert all(_same_detections(a, b) for a, b in zip(out, ref))
    A.cfg.VISION_QUERY.MASK_DURING_INFERENCE = False
    off_refs = _uncached(s, A)
    differs = [not all(_same_detections(a, b) for a, b in zip(out, ref)) for out, ref in zip(batched, off_refs)]
    print(f"chunks that differ from the mode-off loop: {differs}", flush=True)
    assert any(differs)
    off_batched = A.forward_chunks(s.il(), s.caps)           # the mode-off chunks are still the mode-off loop (fronts keyed by the signature)
    for out, ref in zip(off_batched, off_refs):
        assert all(_same_detections(a, b) for a, b in zip(out, ref))
    print("OK forward_chunks with the mode on", flush=True)


def _body_language_only():
    s = _Setup()
    A, B = s.model(False), s.model(False, bank=None)
    A.cfg.VISION_QUERY.ENABLED = False
    A.cfg.VISION_QUERY.MASK_DURING_INFERENCE, A.cfg.VISION_QUERY.TEXT_DROPOUT = True, 1.0       # without ENABLED the two keys do nothing
    for cap, pm in s.caps[:2]:
        assert _equal(A(s.il(), captions=[cap] * 2, positive_map=pm), B(s.il(), captions=[cap] * 2, positive_map=pm))
    print("OK language-only", flush=True)


def _run(body, timeout=300):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), body], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{body}: rc {r.returncode}\n{out[-4000:]}"
    return out


def test_vision_only_equals_the_mode_off_model_on_caller_masked_ids():
    _run("masked_equals_caller_masked_ids")


def test_vision_only_split_precise_matches_the_fp32_oracle_on_masked_ids():
    _run("f32_vs_oracle")


def test_label_without_bank_rows_keeps_its_words():
    _run("label_without_rows_keeps_its_words")


def test_vision_only_through_the_caches_and_graph_replay():
    _run("caches_and_graph_replay")


def test_bank_change_changes_the_mask_without_clear_caches():
    _run("bank_change")


def test_forward_chunks_masks_every_chunk():
    _run("forward_chunks")


def test_language_only_with_a_bank_loaded_equals_no_bank():
    _run("language_only")


if __name__ == "__main__":
    globals()["_body_" + sys.argv[1]]()
