"""Vision-only evaluation (VISION_QUERY.MASK_DURING_INFERENCE + TEXT_DROPOUT), host side, no GPU: the mask function against a restatement of
the reference's loop, its use of Python's global generator, the four switches, the refusal of PURE_TEXT_RATE, the memo of the masked ids and
the mask signature that the caption-keyed caches carry.  The device side is tests/test_gpu_vision_only.py."""
import random
import types

import pytest
import torch

from mq_det_amd import get_cfg
from mq_det_amd.modeling.query_selector import QuerySelector, prepare_positive_map, text_dropout_mask, text_dropout_rate

T, MASK_ID = 32, 103
PM = {1: [1, 2], 2: [4], 3: [6, 7, 8], 9: []}                # label 9 has no token: not a label of the caption (no draw for it)
HAS = {1: True, 2: False, 3: True}                          # label 2 has no bank rows


def _mode_on(cfg, p=1.0):
    cfg.VISION_QUERY.MASK_DURING_INFERENCE, cfg.VISION_QUERY.TEXT_DROPOUT = True, p
    return cfg


def _inputs(B):
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1000, 2000, (B, T), generator=g)    # no id equals MASK_ID: a masked position is visible as a changed id
    am = torch.zeros(B, T, dtype=torch.long)
    am[:, :12] = 1
    return ids, am


def _restated(input_ids, attention_mask, positive_map, has_vision_query, p):
    """The reference's eval-time masking restated: maskrcnn_benchmark/modeling/detector/generalized_vl_rcnn_new.py:295-305 (the labels of the
    caption = the keys of the positive map with a token, in dict order, and their [L, T] token map) and :397-407 (for every image, for every
    label: draw; if the draw is below TEXT_DROPOUT and the label has a vision query, write the [MASK] id at the label's tokens).  Only
    input_ids change.  `has_vision_query`: {label: bool}, the selector's flag of :362."""
    labels = [k for k, v in positive_map.items() if len(v) != 0]                                  # :298
    all_map = torch.zeros(len(labels), input_ids.shape[1])                                        # :300
    for j, label in enumerate(labels):                                                            # :301-303
        all_map[j, positive_map[label]] = 1
    all_map = all_map / (all_map.sum(-1)[:, None] + 1e-6)                                         # :304
    flags = [1 if has_vision_query[label] else 0 for label in labels]
    ids = input_ids.clone()
    for i in range(ids.shape[0]):                                                                 # :402 (the same caption for every image)
        pos = all_map.to(torch.bool)                                                              # :403
        for j, position in enumerate(pos):                                                        # :404
            if random.random() < p:                                                               # :405
                if flags[j] == 1:                                                                 # :406
                    ids[i, position] = MASK_ID                                                    # :407
    return ids, attention_mask


@pytest.mark.parametrize("B", [1, 2])
def test_mask_equals_the_restated_reference_loop(B):
    ids, am = _inputs(B)
    pm, labels, *_ = prepare_positive_map(PM, T)
    assert labels == [1, 2, 3]
    state = random.getstate()
    mask = text_dropout_mask(labels, pm, HAS.__getitem__, T, 1.0, B)
    assert random.getstate() == state                        # TEXT_DROPOUT >= 1, REFERENCE_RNG_STREAM off: no draw
    assert mask.shape == (B, T) and mask.dtype == torch.bool
    want = torch.zeros(T, dtype=torch.bool)
    want[[1, 2, 6, 7, 8]] = True                             # exactly the tokens of labels 1 and 3
    for b in range(B):
        assert torch.equal(mask[b], want)
    ref_ids, ref_am = _restated(ids, am, PM, HAS, 1.0)
    assert torch.equal(ids.masked_fill(mask, MASK_ID), ref_ids)
    assert torch.equal(ref_am, am) and ref_am is am          # the attention mask is not an input of the mask function: untouched
    assert text_dropout_mask(labels, pm, lambda lab: False, T, 1.0, B) is None        # no label has bank rows: nothing to mask


def test_partial_dropout_consumes_the_global_generator_like_the_reference():
    B, p = 2, 0.5
    ids, am = _inputs(B)
    pm, labels, *_ = prepare_positive_map(PM, T)
    hand = random.Random(7)
    draws = [[hand.random() for _ in labels] for _ in range(B)]                       # image-major, one per (image, label)
    assert len({d < p for row in draws for d in row}) == 2                            # the seed gives both outcomes
    random.seed(7)
    mask = text_dropout_mask(labels, pm, HAS.__getitem__, T, p, B)
    assert random.getstate() == hand.getstate()              # exactly B x n_labels draws, label 2 (no bank rows) included
    want = torch.zeros(B, T, dtype=torch.bool)
    for i in range(B):
        for j, lab in enumerate(labels):
            if draws[i][j] < p and HAS[lab]:
                want[i, pm[lab]] = True
    assert want.any() and not torch.equal(want[0], want[1])  # the two images differ with this seed: a per-image mask
    assert torch.equal(mask, want)
    random.seed(7)
    ref_ids, _ = _restated(ids, am, PM, HAS, p)
    assert torch.equal(ids.masked_fill(mask, MASK_ID), ref_ids) and random.getstate() == hand.getstate()
    # REFERENCE_RNG_STREAM with TEXT_DROPOUT 1.0: the draws are consumed, the mask is the deterministic one
    random.seed(7)
    mask_rng = text_dropout_mask(labels, pm, HAS.__getitem__, T, 1.0, B, reference_rng=True)
    assert random.getstate() == hand.getstate()
    assert torch.equal(mask_rng, text_dropout_mask(labels, pm, HAS.__getitem__, T, 1.0, B))


def test_switches_and_the_pure_text_rate_refusal():
    assert text_dropout_rate(get_cfg()) == 0.0
    assert text_dropout_rate(_mode_on(get_cfg())) == 1.0 and text_dropout_rate(_mode_on(get_cfg(), 0.4)) == 0.4
    for key, value in (("NEW_MASK_TOKEN", True), ("ENABLED", False), ("TEXT_DROPOUT", 0.0), ("MASK_DURING_INFERENCE", False)):
        cfg = _mode_on(get_cfg())
        cfg.VISION_QUERY[key] = value
        assert text_dropout_rate(cfg) == 0.0, key
    cfg = _mode_on(get_cfg())
    cfg.VISION_QUERY.PURE_TEXT_RATE = 0.5
    with pytest.raises(NotImplementedError, match="PURE_TEXT_RATE"):
        text_dropout_rate(cfg)
    cfg.VISION_QUERY.MASK_DURING_INFERENCE = False           # the reference asserts it inside the masking branch only
    assert text_dropout_rate(cfg) == 0.0


def _cpu_model(cfg):
    from mq_det_amd import build_detection_model
    cfg.MODEL.SWINT.DEPTHS = (2, 2, 2, 2)
    cfg.MODEL.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS = 2
    cfg.MODEL.LANGUAGE_BACKBONE.QV_START = 1
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = 1100
    cfg.MODEL.DYHEAD.NUM_CONVS = 1
    return build_detection_model(cfg, tokenizer=types.SimpleNamespace(mask_token_id=MASK_ID))


def _bank(labels, cfg):
    return {lab: torch.zeros(2, 1, cfg.MODEL.BACKBONE.OUT_CHANNELS) for lab in labels}


def test_detector_masks_memoises_and_follows_the_bank():
    """GeneralizedVLRCNN_New._masked_ids on host tensors: the ids of the restatement; the SAME tensor object call after call (what lets a
    HIP-graph replay skip the copy); another object and another mask signature after the bank changed, without clear_caches(); the four
    switches hand the tokenizer's ids through untouched; validation refuses PURE_TEXT_RATE by name."""
    from mq_det_amd.modeling.graph_runner import is_memoised
    cfg = _mode_on(get_cfg())
    model = _cpu_model(cfg)
    model._validate_config()
    cpu = torch.device("cpu")
    ids, am = _inputs(2)
    pm, labels, pm_key, *_ = prepare_positive_map(PM, T)
    cap_key = ("a. b. c", "a. b. c")
    out = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    assert out[0] is ids and out[1:] == (cap_key, None)      # no bank: nothing is masked
    model.load_query_bank(_bank([1, 3, 5], cfg))
    state = random.getstate()
    got, key, sig = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    assert random.getstate() == state
    assert torch.equal(got, _restated(ids, am, PM, HAS, 1.0)[0]) and key == cap_key and sig is not None
    again, _, sig2 = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    assert again is got and sig2 == sig and is_memoised(got)
    out = model._masked_ids(ids, None, pm_key, labels, pm, cpu)
    assert out[0] is ids and out[1:] == (None, None)         # caller-supplied ids are the caller's
    model.load_query_bank(_bank([1, 2], cfg))                # other labels have rows now
    other, _, sig3 = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    assert other is not got and sig3 != sig
    assert torch.equal(other, _restated(ids, am, PM, {1: True, 2: True, 3: False}, 1.0)[0])
    model.query_selector.query_bank = _bank([1, 3, 5], cfg)  # also when the bank is handed over without load_query_bank
    back, _, sig4 = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    assert back is got and sig4 == sig
    # REFERENCE_RNG_STREAM: the draws of the reference, the memoised ids all the same; forward_chunks draws for its images
    model.query_selector.reference_rng = True
    hand = random.Random(3)
    [hand.random() for _ in range(2 * len(labels))]
    random.seed(3)
    assert model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)[0] is got and random.getstate() == hand.getstate()
    [hand.random() for _ in range(4 * len(labels))]
    one, _, _ = model._masked_ids(ids[:1], cap_key[:1], pm_key, labels, pm, cpu, n_images=4)
    assert torch.equal(one, got[:1]) and random.getstate() == hand.getstate()
    model.query_selector.reference_rng = False
    # 0 < TEXT_DROPOUT < 1: per-image draws, nothing memoised (no caption key comes back)
    cfg.VISION_QUERY.TEXT_DROPOUT = 0.5
    random.seed(7)
    part, key, sig = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
    random.seed(7)
    assert torch.equal(part, _restated(ids, am, PM, HAS, 0.5)[0]) and key is None and sig is None and not is_memoised(part)
    cfg.VISION_QUERY.TEXT_DROPOUT = 1.0
    for k, value in (("NEW_MASK_TOKEN", True), ("ENABLED", False), ("TEXT_DROPOUT", 0.0), ("MASK_DURING_INFERENCE", False)):
        old, cfg.VISION_QUERY[k] = cfg.VISION_QUERY[k], value
        out = model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)
        assert out[0] is ids and out[1:] == (cap_key, None), k
        model._validate_config()
        cfg.VISION_QUERY[k] = old
    cfg.VISION_QUERY.PURE_TEXT_RATE = 0.5
    with pytest.raises(NotImplementedError, match="PURE_TEXT_RATE"):
        model._validate_config()
    with pytest.raises(NotImplementedError, match="PURE_TEXT_RATE"):
        model._masked_ids(ids, cap_key, pm_key, labels, pm, cpu)


def test_has_vision_query_is_the_selectors_candidate_rule():
    from collections import defaultdict
    cfg = get_cfg()
    qs = QuerySelector(cfg)
    qs.load_query_bank(defaultdict(list, {1: torch.zeros(2, 1, 4), 2: [], 3: torch.zeros(0, 1, 4)}))
    assert [qs.has_vision_query(lab) for lab in (1, 2, 3, 4)] == [True, False, False, False]


def test_groundingdino_ignores_the_masking_keys(tmp_path):
    """groundingdino_new/ never reads VISION_QUERY.MASK_DURING_INFERENCE / TEXT_DROPOUT / NEW_MASK_TOKEN / PURE_TEXT_RATE: with all of them
    set (PURE_TEXT_RATE to a value MQ-GLIP refuses) get_gdino_cfg() builds and validates as before."""
    from mq_det_amd.config import get_gdino_cfg
    from mq_det_amd.modeling import gdino
    from mq_det_amd.utils.tokenizer import build_synthetic_tokenizer
    cfg = _mode_on(get_gdino_cfg())
    cfg.VISION_QUERY.NEW_MASK_TOKEN, cfg.VISION_QUERY.PURE_TEXT_RATE = False, 0.5
    cfg.GROUNDINGDINO.text_encoder_type = build_synthetic_tokenizer(str(tmp_path), size=2048)
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = 2048
    cfg.GROUNDINGDINO.swin_depths, cfg.GROUNDINGDINO.enc_layers, cfg.GROUNDINGDINO.dec_layers = (2, 2, 2, 2), 1, 1
    cfg.MODEL.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS = 7
    model = gdino.GroundingDINO(cfg)
    model._validate_config()
    assert not hasattr(model, "_masked_ids")
