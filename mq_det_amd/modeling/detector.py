"""GeneralizedVLRCNN_New -- the drop-in boundary (reference modeling/detector/generalized_vl_rcnn_new.py:90-519,
constructor registry modeling/detector/__init__.py:4-14).

Same constructor (`build_detection_model(cfg)`), same `forward(images, targets=None, captions=None,
positive_map=None, greenlight_map=None, return_backbone_features=False)` -> `list[BoxList]`, same attribute tree
(`backbone.body/.fpn`, `language_backbone`, `rpn.head`, `query_selector`, `tokenizer`) and the same
`state_dict()` keys, so `tools/test_grounding_net.py` / `engine/inference.py` / `GLIPDemo` can drive it
unchanged.  Inference only: training mode raises NotImplementedError.
The README's three evaluation modes are settings of this forward and need nothing from its callers: text + vision queries (default),
text only (`VISION_QUERY.ENABLED False`), vision only (`VISION_QUERY.MASK_DURING_INFERENCE True VISION_QUERY.TEXT_DROPOUT 1.0`,
:397-407 -> `_masked_ids`).
Differences by design: fp16 compute on MI355X HIP kernels; B > 1 is allowed with vision queries (the
reference asserts B == 1, :354); post-processing has a single device->host sync per forward.
"""
import os

import torch

from .. import ops as _ops
from ..query_bank import QueryBank
from ..structures import BoxList, to_image_list
from . import pipeline
from .device_model import DeviceModel, compute_dtype  # noqa: F401  (compute_dtype: re-exported)
from .graph_runner import Memo
from .params import PROMPT_OFFSET_ROWS, Container, build_param_tree
from .query_selector import (build_item_token_index, build_token_index, consume_text_dropout_draws, prepare_positive_map,
                             text_dropout_mask, text_dropout_rate)


def expand_bbox(box_list, expand_ratio=1.5):
    """generalized_vl_rcnn_new.py:32-49: grow every box about its centre, clip to the image, drop empty boxes."""
    out = []
    for boxes in box_list:
        assert boxes.mode == "xyxy"
        bbox = boxes.bbox
        w, h = bbox[:, 2] - bbox[:, 0], bbox[:, 3] - bbox[:, 1]
        dw, dh = (w * expand_ratio - w) / 2, (h * expand_ratio - h) / 2
        nb = BoxList(bbox + torch.stack([-dw, -dh, dw, dh], dim=1), boxes.size, mode="xyxy")
        nb.add_field("labels", boxes.get_field("labels"))
        out.append(nb.clip_to_image(remove_empty=True))
    return out


def pool_into_bank(cfg, pooler, visual_features, targets, query_images, exclude_similar, max_query_number):
    """Shared tail of `extract_query` (generalized_vl_rcnn_new.py:264-288 == groundingdino.py:397-421): ROI-pool the (already
    expanded) target boxes -- from their own FPN level (SELECT_FPN_LEVEL) or from all five --, average the bins inside the kernel,
    and append the features to the bank of their label up to `max_query_number`, optionally skipping near-duplicates."""
    query_feats = pooler(visual_features, targets, reduce_mean=True)                # [boxes, C] or [scales, boxes, C]
    if cfg.VISION_QUERY.SELECT_FPN_LEVEL:
        query_feats = query_feats[None]
    else:
        assert len(visual_features) == len(query_feats) == 5
    query_feats = query_feats.permute(1, 0, 2)                                      # boxes, scales, channels
    labels = torch.cat([t.get_field("labels") for t in targets])
    assert len(labels) == len(query_feats)
    max_query_number = cfg.VISION_QUERY.MAX_QUERY_NUMBER if max_query_number is None else max_query_number
    thr = cfg.VISION_QUERY.SIMILARITY_THRESHOLD
    if isinstance(query_images, QueryBank):                                         # device-resident bank: the whole loop below in one launch
        query_images.update(query_feats, labels, max_query_number, exclude_similar, thr)
        return query_images
    for label, feat in zip(labels.tolist(), query_feats):
        cur = query_images[label] if (label in query_images or hasattr(query_images, "default_factory")) else []
        n = len(cur)
        if n >= max_query_number:
            continue
        if exclude_similar and n > 0:
            assert feat.shape[0] == 1
            bank = torch.nn.functional.normalize(cur.to(feat), p=2, dim=-1)
            new = torch.nn.functional.normalize(feat, p=2, dim=-1)
            if (torch.einsum("bnd,nd->bn", bank, new) > thr).sum() > 0:
                continue
        query_images[label] = feat[None] if n == 0 else torch.cat([cur.to(feat), feat[None]])
    return query_images


class GeneralizedVLRCNN_New(DeviceModel):
    _plan_memos = ("_anchor_cache", "_front_cache")

    def __init__(self, cfg, tokenizer=None, **kwargs):
        super().__init__(cfg)
        for name in ("backbone", "language_backbone", "rpn"):
            self.add_module(name, Container())
        build_param_tree(self, cfg)
        self.roi_heads = None                                     # RPN_ONLY (roi_heads/__init__.py:64-84)
        self._build_query_path()
        self.tokenizer = tokenizer if tokenizer is not None else self._load_tokenizer(cfg)
        self._anchor_cache = Memo(8)                              # keyed by feature-map geometry: a handful is live at once
        # host memos of a caption / an image-size list; their tensors are registered with memoised(): a graph replay skips copying them
        self._tok_cache, self._tokidx_cache, self._wh_cache, self._live_cache = (Memo(256, memoise=True) for _ in range(4))
        self._front_cache = Memo(cfg.MODEL.get("LANG_FRONT_CACHE", 64))   # image-independent BERT layers per caption (f1)
        self._mask_cache = Memo(256, memoise=True)                # token ids with the [MASK]ed category words (_masked_ids)
        # lanes of the staggered schedule (_staggered_program); 1 = the whole batch as one lane.  MQ_MICRO_BATCHES overrides (A/B runs)
        self.micro_batches = int(os.environ.get("MQ_MICRO_BATCHES", cfg.MODEL.get("MICRO_BATCHES", 1)))
        self.cache_stats.update(front_hit=0, front_miss=0)
        self.eval()

    @staticmethod
    def _load_tokenizer(cfg):
        from transformers import AutoTokenizer
        name = cfg.MODEL.LANGUAGE_BACKBONE.TOKENIZER_TYPE
        if not os.path.isdir(name):
            raise RuntimeError(
                f"tokenizer files for '{name}' are not on disk (no network here): point "
                "MODEL.LANGUAGE_BACKBONE.TOKENIZER_TYPE at a local directory whose basename is 'bert-base-uncased' "
                "(mq_det_amd.utils.tokenizer.build_synthetic_tokenizer writes one) or pass tokenizer=...")
        return AutoTokenizer.from_pretrained(name)

    def _build_plan(self, device, dtype):
        return pipeline.build_plan(self.state_dict(), self.cfg, device, dtype=dtype)

    def _validate_config(self):
        """Fail early, with the config key named, on settings of the reference this path does not implement (instead of a
        negative return code from a kernel in the middle of a forward)."""
        cfg = self.cfg
        M = cfg.MODEL
        agg = str(M.DYHEAD.get("SCORE_AGG", "MEAN")).upper()
        mdetr = cfg.TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM != -1
        if agg not in ("MEAN", "MAX", "ONEHOT") + (("POWER",) if mdetr else ()):
            # the reference's own rule: convert_grounding_to_od_logits (rpn/inference.py:772-792) knows MEAN / MAX / ONEHOT,
            # only the MDETR-style _v2 (:795-824) adds POWER; anything else raises NotImplementedError there too
            raise NotImplementedError(f"MODEL.DYHEAD.SCORE_AGG = {agg}: MEAN / MAX / ONEHOT"
                                      + (" / POWER" if mdetr else " (POWER only with TEST.MDETR_STYLE_AGGREGATE_CLASS_NUM != -1)"))
        if M.DYHEAD.FUSE_CONFIG.get("ADD_LINEAR_LAYER", False) and M.LANGUAGE_BACKBONE.MAX_QUERY_LEN > PROMPT_OFFSET_ROWS:
            raise NotImplementedError(f"MODEL.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER: rpn.tunable_linear holds {PROMPT_OFFSET_ROWS} token "
                                      "positions, MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN is larger")
        if M.LANGUAGE_BACKBONE.MAX_QUERY_LEN > 256 or M.LANGUAGE_BACKBONE.MAX_QUERY_LEN % 8:
            raise NotImplementedError("MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN must be a multiple of 8 and <= 256 (VLFuse kernels)")
        if M.BACKBONE.OUT_CHANNELS != 256 or M.DYHEAD.CHANNELS != 256:
            raise NotImplementedError("the VLDyHead kernels (VLFuse, DCNv2, DyConv epilogue) are written for 256 channels")
        if M.SWINT.WINDOW_SIZE ** 2 > 160:
            raise NotImplementedError("MODEL.SWINT.WINDOW_SIZE: windows of up to 160 tokens (7x7, 12x12) are supported")
        fc = M.DYHEAD.FUSE_CONFIG
        if fc.TYPE != "MHA-B" or fc.get("SEPARATE_BIDIRECTIONAL", False):
            raise NotImplementedError("MODEL.DYHEAD.FUSE_CONFIG: only TYPE = MHA-B without SEPARATE_BIDIRECTIONAL (mq-glip-*.yaml)")
        if cfg.VISION_QUERY.get("ADD_ADAPT_LAYER", False) or cfg.VISION_QUERY.get("QUERY_FUSION", False) or \
                cfg.VISION_QUERY.get("AUGMENT_IMAGE_WITH_QUERY", False):
            raise NotImplementedError("VISION_QUERY.ADD_ADAPT_LAYER / QUERY_FUSION / AUGMENT_IMAGE_WITH_QUERY are not implemented")
        text_dropout_rate(cfg)                                    # VISION_QUERY.MASK_DURING_INFERENCE with PURE_TEXT_RATE != 0

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def extract_query(self, images=None, targets=None, query_images=None, visual_features=None, exclude_similar=False,
                      device=None, max_query_number=None):
        """Vision-query extraction (generalized_vl_rcnn_new.py:232-288; callers: tools/extract_vision_query.py via
        tools/train_net.py:303, engine/inference.py:474,492 `online_update`).  targets: list[BoxList] (xyxy, field
        "labels") per image; query_images: the bank being built, `{label: Tensor[n, scales, C]}` (a `defaultdict(list)` in
        the reference); visual_features: FPN maps from `forward(..., return_backbone_features=True)`, or None -> Swin + FPN run
        here on `images`.  Boxes are grown by VISION_QUERY.EXPAND_RATIO, pooled with the aligned ROIAlign (HIP kernel, the
        7 x 7 bins averaged inside the kernel) from their FPN level (SELECT_FPN_LEVEL) or from all five, and appended to
        the bank of their label up to `max_query_number`, optionally skipping near-duplicates (cosine > SIMILARITY_THRESHOLD)."""
        cfg = self.cfg
        device = torch.device(device) if device else (images.tensors.device if images is not None else visual_features[0].device)
        targets = expand_bbox([t.to(device) for t in targets if t is not None], expand_ratio=cfg.VISION_QUERY.EXPAND_RATIO)
        if visual_features is None:
            images = to_image_list(images)
            dtype = self._ensure_plan(images.tensors.device)["backbone.body.patch_embed.proj.weight"].dtype
            x = images.tensors.to(dtype).contiguous(memory_format=torch.channels_last)
            visual_features, _ = self._backbone_stage(x)
        else:
            visual_features = [v.to(device) for v in visual_features]
        return pool_into_bank(cfg, self.pooler, visual_features, targets, query_images, exclude_similar, max_query_number)

    def tokenize(self, captions, device):
        """HF tokenizer on the host (generalized_vl_rcnn_new.py:378-383); memoised per caption tuple -- the LVIS
        protocol re-sends the same 31 chunk captions for every image (engine/inference.py:605-625)."""
        def make():
            LB = self.cfg.MODEL.LANGUAGE_BACKBONE
            # PAD_MAX = False ("longest" in the reference, generalized_vl_rcnn_new.py:378-383) pads to MAX_QUERY_LEN here as well:
            # padded positions are masked keys everywhere (BERT, GCP, VLFuse) and never scored, so the detections are the same;
            # forward() cuts the padded ROWS away again (`_live_len`: the first 16 ceil(max_kv / 16) positions go to the device programs)
            tok = self.tokenizer(list(captions), max_length=LB.MAX_QUERY_LEN, padding="max_length",
                                 return_special_tokens_mask=True, return_tensors="pt", truncation=True)
            am = tok["attention_mask"]
            # host-side bound of the per-caption key length (last attended position + 1): picks the kernel variant of
            # the VLFuse image-side attention, and is part of the HIP-graph key
            max_kv = int((am * torch.arange(1, am.shape[1] + 1)).max())
            return tok["input_ids"].to(device), am.to(device), max_kv
        return self._tok_cache.get((tuple(captions), str(device)), make)

    def _masked_ids(self, input_ids, cap_key, pm_key, labels, positive_map, dev, n_images=None):
        """Vision-only evaluation (VISION_QUERY.MASK_DURING_INFERENCE + TEXT_DROPOUT, generalized_vl_rcnn_new.py:397-407): the tokenizer's ids
        with the words of every label that has vision queries replaced by [MASK] -> (input_ids, cap_key, mkey).  Nothing else changes:
        attention mask, positive map, scoring maps and the vision-query index are those of the unmasked caption.
        `mkey` is the MASK SIGNATURE every memo of a caption carries beside the caption itself (the live-row slice, the front cache, the
        fronts of forward_chunks): None when nothing is masked -- mode off, no bank, no label of this caption in the bank --, else the
        cleaned positive map + the labels the bank has rows for.  It is recomputed from the bank on every call (a dict lookup per label,
        what `QuerySelector.deterministic` already does), so a bank that gained or lost labels changes it without `clear_caches()`.
        TEXT_DROPOUT >= 1 (the README's setting): the masked ids are a function of (caption, mkey) and memoised -- a hit costs no device
        work, and the SAME tensor object comes back, which is what lets a HIP-graph replay skip copying it.
        0 < TEXT_DROPOUT < 1: one draw of Python's global generator per (image, label) like the reference, and nothing about this call is
        memoised (`cap_key` comes back None: the forward then treats the ids like caller-supplied ones).
        `n_images` (forward_chunks: one id row per chunk serves every image): the images VISION_QUERY.REFERENCE_RNG_STREAM draws for."""
        p = text_dropout_rate(self.cfg)
        if p <= 0.0 or cap_key is None or not self._use_vq():
            return input_ids, cap_key, None
        sel = self.query_selector
        mask_id = getattr(self.tokenizer, "mask_token_id", None)
        if mask_id is None:
            raise RuntimeError("VISION_QUERY.MASK_DURING_INFERENCE: the tokenizer has no [MASK] token (mask_token_id is None)")
        B, T = input_ids.shape
        if p < 1.0:
            mask = text_dropout_mask(labels, positive_map, sel.has_vision_query, T, p, B)
            if mask is None:
                return input_ids, cap_key, None
            return input_ids.masked_fill(mask.to(dev), mask_id), None, None
        if sel.reference_rng:
            consume_text_dropout_draws(B if n_images is None else n_images, len(labels))
        masked = tuple(lab for lab in labels if sel.has_vision_query(lab))
        if not masked:
            return input_ids, cap_key, None
        mkey = (pm_key, masked)

        def make():
            mask = text_dropout_mask(masked, positive_map, lambda lab: True, T, 1.0, B)
            return input_ids.masked_fill(mask.to(dev), mask_id)
        return self._mask_cache.get((cap_key, mkey, str(dev)), make), cap_key, mkey

    def _live_len(self, T, max_kv):
        """Text positions the device programs run on: 16 ceil(max_kv / 16) (the key-block granularity of the attention kernels; VLFuse takes
        T % 8 == 0), or all T when the bound is unknown or MODEL.LANGUAGE_BACKBONE.COMPACT_TEXT is off."""
        if max_kv <= 0 or not self.cfg.MODEL.LANGUAGE_BACKBONE.get("COMPACT_TEXT", True):
            return T
        if self.cfg.VISION_QUERY.get("RETURN_ATTN_GATE_VALUE", False):
            # the reference's attn_gate.mean() averages over all B x MAX_QUERY_LEN positions (padded rows contribute the constant
            # tanh(gate(LN(0)))): the diagnostic value is only the reference's when every padded row is computed -- no compaction with it
            return T
        return min(T, -(-int(max_kv) // 16) * 16)

    def _live_slice(self, input_ids, attention_mask, Tl, cap_key, dev, mkey=None):
        """input_ids / attention_mask cut to their first Tl columns as contiguous tensors (memoised per caption and mask signature: the
        HIP-graph replay copies its inputs into static buffers, the same two tensors serve every call of a caption)."""
        def make():
            return input_ids[:, :Tl].contiguous(), attention_mask[:, :Tl].contiguous()
        return make() if cap_key is None else self._live_cache.get((cap_key, Tl, str(dev), mkey), make)

    def _im_wh(self, images, dev):
        """[B, 2] fp32 (width, height) of every image, memoised per size list."""
        return self._wh_cache.get((tuple(images.image_sizes), str(dev)), lambda: torch.tensor(
            [[w, h] for (h, w) in images.image_sizes], dtype=torch.float32, device=dev))

    def _anchors(self, feats):
        """Anchors of the five levels: constant per feature-map geometry (and plan)."""
        sizes = tuple(tuple(f.shape[-2:]) for f in feats)
        return self._anchor_cache.get(sizes, lambda: pipeline.grid_anchors(self._plan, sizes, self.cfg.MODEL.RPN.ANCHOR_STRIDE,
                                                                            feats[0].device))

    @staticmethod
    def _pad_raw_text(raw, T):
        """return_raw (parity ladders): the per-token tensors of a compacted forward back in the caller's [.., T, ..] shapes -- zeros at the
        padded positions (which the reference fills with values nothing reads)."""
        import torch.nn.functional as F

        def rows(t_):            # [B, Tl, C] -> [B, T, C]
            return t_ if t_ is None or t_.shape[1] >= T else F.pad(t_, (0, 0, 0, T - t_.shape[1]))

        def cols(t_):            # [.., Tl] -> [.., T]
            return t_ if t_ is None or t_.shape[-1] >= T else F.pad(t_, (0, T - t_.shape[-1]))
        lang, head = raw["lang"], raw["head"]
        for k in ("hidden", "hidden32", "embedded"):
            if torch.is_tensor(lang.get(k)):
                lang[k] = rows(lang[k])
        for k in ("masks", "key_bias"):
            if torch.is_tensor(lang.get(k)):
                lang[k] = cols(lang[k])
        if torch.is_tensor(head.get("hidden")):
            head["hidden"] = rows(head["hidden"])
        # (head["tbias"], head["dot"] and the alignment operands stay Tl wide: postprocess() may be called on this head again; their first
        # max_kv columns are what the ladders read)
        for a in raw.get("head_trace") or ():
            if torch.is_tensor(a.get("bert_hidden")):
                a["bert_hidden"] = rows(a["bert_hidden"])
        return raw

    # ------------------------------------------------------------------ device part (capturable in a HIP graph)
    def _backbone_stage(self, x):
        """Swin + FPN (+ the pooled FPN tokens the GCP pre-select attends to): depends on the pixels only."""
        P, cfg = self._plan, self.cfg
        feats = pipeline.fpn_forward(P, pipeline.swin_forward(P, cfg, x))
        pooled = pipeline.pooled_fpn_tokens(feats) if self._use_vq() else None
        return feats, pooled

    def _head_operands(self, feats, pooled, front, input_ids, attention_mask, vision, idx, max_kv, want_raw=False):
        """The head stage up to what `postprocess` (or `ATSSLoss`) is handed: (lang, head, trace)."""
        P, cfg = self._plan, self.cfg
        lang = pipeline.language_backbone(P, cfg, input_ids, attention_mask, vision, pooled, idx,
                                          want_gates=cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE, front=front, max_kv=max_kv,
                                          side_ok=bool(_ops.KERNELS["LANG_SIDE_STREAMS"] == 1 and feats[0].is_cuda
                                                       and cfg.MODEL.DYHEAD.get("LEVEL_STREAMS", True) and not want_raw))
        lang["max_kv"] = max_kv
        pipeline.prompt_offset(P, lang)                           # the tuned prompt of a fine-tuned checkpoint (ADD_LINEAR_LAYER); else nothing
        trace = [] if want_raw else None                          # raw mode: per-layer tensors, single-stream schedule
        head = pipeline.vldyhead(P, cfg, feats, lang, trace=trace)
        return lang, head, trace

    def _head_stage(self, feats, pooled, front, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv,
                    want_raw=False):
        """Image-dependent half of the language backbone (pre-select + GCP / BERT layers), VLDyHead, post-processing."""
        cfg = self.cfg
        lang, head, trace = self._head_operands(feats, pooled, front, input_ids, attention_mask, vision, idx, max_kv, want_raw=want_raw)
        anchors = self._anchors(feats)
        post = pipeline.postprocess(cfg, head, anchors, im_wh, tokidx, label_ids, want_cls=want_raw)
        if want_raw:
            return {"post": post, "head": head, "head_trace": trace, "lang": lang, "feats": feats, "anchors": anchors,
                    "vision": vision, "idx": idx, "pooled": pooled}
        if "packed" in post:                                      # fused post-processing hands over the packed block and counts as they are
            packed, counts = post["packed"], post["counts_packed"]
        else:
            packed = torch.cat([post["boxes"], post["scores"][..., None], post["labels"].float()[..., None]], -1)
            # one int per image for the single device->host transfer: live slots, bit 16 = more ties with the K-th score than tie slots
            counts = post["counts"] + post["tie_overflow"].to(post["counts"].dtype) * 65536
        gates = lang["vision_query_gates"]
        if gates is not None:                                     # reference: attn_gate.mean().item() per GCP layer (a float)
            gates = torch.stack([g.float().mean() for g in gates])
        return {"packed": packed, "counts": counts, "gates": gates}

    def _pixels(self, src, dtype):
        """The pixel tensor the device program takes: the caller's fp32 NCHW tensor AS IT IS when the patch-embedding kernel can read it
        (mq_patch_embed_fwd rounds to the operand type itself: no cast pass, no channels-last copy), else 16-bit channels-last pixels."""
        P = self._plan
        if _ops.KERNELS["PATCH_EMBED_FUSED"] == 1 and P.get("_r32") and src.dtype == torch.float32 and src.is_contiguous() \
                and src.shape[1] == 3 and "backbone.body.patch_embed.wpk_nchw" in P:
            return src
        return src.to(dtype).contiguous(memory_format=torch.channels_last)

    def _mode_key(self):
        return (pipeline.candidate_mode(self.cfg),)

    def _split_counts(self, counts):
        """Packed per-image counts -> live slots; remembers (and warns about) images whose ties with the K-th score did not fit.
        Candidate mode (TEST.USE_MULTISCALE, pipeline.postprocess): the counts are the plain numbers of candidates, no tie bit."""
        if pipeline.candidate_mode(self.cfg):
            self.last_tie_overflow = [False] * len(counts)
            return [int(c) for c in counts]
        self.last_tie_overflow = [bool(c >> 16) for c in counts]
        if any(self.last_tie_overflow):
            import warnings
            warnings.warn(f"{sum(self.last_tie_overflow)} image(s) had more detections tied with the DETECTIONS_PER_IMG-th score than "
                          "MODEL.ATSS.TIE_SLOTS output slots: the reference would return all of them (rpn/inference.py:757-766)")
        return [c & 0xFFFF for c in counts]

    def _full_program(self, x, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv=0, want_raw=False):
        """Whole device forward.  The image-independent part of the language backbone (embeddings + BERT layers below
        the first GCP block) runs on a side stream under the Swin backbone: its launches are tiny (B x 256 tokens)."""
        P, cfg = self._plan, self.cfg
        front = None
        if x.is_cuda and cfg.MODEL.DYHEAD.get("LEVEL_STREAMS", True) and _ops.KERNELS["FRONT_SIDE_STREAM"] == 1:
            main, text = torch.cuda.current_stream(), pipeline._side_streams(x.device, 1, "text")[0]
            text.wait_stream(main)
            with torch.cuda.stream(text):
                front = pipeline.language_front(P, cfg, input_ids, attention_mask, vision is not None, max_kv=max_kv)
        feats, pooled = self._backbone_stage(x)
        if front is not None:
            main.wait_stream(text)
        else:
            front = pipeline.language_front(P, cfg, input_ids, attention_mask, vision is not None, max_kv=max_kv)
        out = self._head_stage(feats, pooled, front, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv,
                               want_raw=want_raw)
        if not want_raw:
            out.update(feats=feats, pooled=pooled, front=front)
        return out

    def _staggered_program(self, x, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv=0):
        """The whole device forward with the batch cut into MODEL.MICRO_BATCHES lanes whose stages are issued as a SOFTWARE PIPELINE.
        Why: a forward is two runs of chip-filling kernels (Swin + FPN; the VLDyHead layers) separated / followed by long CHAINS of
        small launches that cannot use the chip -- the image-dependent half of the language backbone (pre-select, 6 GCP blocks + 6 BERT
        layers on B x 256 tokens: ~170 launches between FPN and the first fusion layer, ~2 ms at B = 8) and the post-processing (~145
        launches after the last one, ~1 ms).  With lanes a stage apart the chains of one lane run under the big kernels of another:

            main stream :  Swin/FPN(0)  Swin/FPN(1)  ...  head(0)        head(1)        ...
            stream L_m  :               language rest(0) | language rest(1)  (waits for FPN(m), feeds head(m))
            stream P_m  :                                                post(0) under head(1) ...   (the last lane's runs exposed)

        Every side stream forks from the CAPTURING stream (a fork from a forked stream crashes hipStreamEndCapture on ROCm 7.0 --
        tools/graph_probe.py, GPU call 4 of round 4), lanes only meet through events between streams that are already in the capture.
        Per-image results do not depend on the lane split: no kernel mixes batch items."""
        P, cfg = self._plan, self.cfg
        M = self.micro_batches
        Bn = x.shape[0]
        per = -(-Bn // M)
        cuts = [(a, min(a + per, Bn)) for a in range(0, Bn, per)]
        n = len(cuts)
        cut = lambda t, a, b, batched=True: t[a:b] if (t is not None and batched) else t      # noqa: E731
        dev = x.device
        main = torch.cuda.current_stream()
        S = pipeline._side_streams
        Fs, Ls, Ps = S(dev, n, "lane_front"), S(dev, n, "lane_lang"), S(dev, n, "lane_post")
        hold = []                                            # tensors that cross streams stay alive until every stream has joined `main`
        args = [dict(ids=cut(input_ids, a, b), am=cut(attention_mask, a, b), vision=cut(vision, a, b), idx=cut(idx, a, b),
                     tokidx=cut(tokidx, a, b, tokidx.dim() == 3), labels=cut(label_ids, a, b, label_ids.dim() == 2), wh=im_wh[a:b])
                for (a, b) in cuts]
        fronts, langs, outs = [None] * n, [None] * n, [None] * n
        for m in range(n):                                   # image-independent BERT layers: tiny launches beside the first Swin
            Fs[m].wait_stream(main)
            with torch.cuda.stream(Fs[m]):
                fronts[m] = pipeline.language_front(P, cfg, args[m]["ids"], args[m]["am"], vision is not None, max_kv=max_kv)
        feats = [None] * n
        for m, (a, b) in enumerate(cuts):
            f, pooled = self._backbone_stage(x[a:b])
            feats[m] = f
            Ls[m].wait_stream(main)                          # FPN(m) done
            Ls[m].wait_stream(Fs[m])
            with torch.cuda.stream(Ls[m]):
                langs[m] = pipeline.language_backbone(P, cfg, args[m]["ids"], args[m]["am"], args[m]["vision"], pooled, args[m]["idx"],
                                                      want_gates=False, front=fronts[m], max_kv=max_kv)
                langs[m]["max_kv"] = max_kv
                pipeline.prompt_offset(P, langs[m])
            hold.append((f, pooled, fronts[m], langs[m]))
        anchors = self._anchors(feats[0])
        for m in range(n):
            main.wait_stream(Ls[m])
            head = pipeline.vldyhead(P, cfg, feats[m], langs[m])
            hold.append(head)
            last = m == n - 1
            st = main if last else Ps[m]
            if not last:
                st.wait_stream(main)
            with torch.cuda.stream(st):                      # on a side stream: levels one after the other (no fork from a forked stream)
                post = pipeline.postprocess(cfg, head, anchors, args[m]["wh"], args[m]["tokidx"], args[m]["labels"], level_streams=last)
                if "packed" in post:
                    outs[m] = (post["packed"], post["counts_packed"])
                else:
                    packed = torch.cat([post["boxes"], post["scores"][..., None], post["labels"].float()[..., None]], -1)
                    outs[m] = (packed, post["counts"] + post["tie_overflow"].to(post["counts"].dtype) * 65536)
            hold.append(post)
        for m in range(n - 1):
            main.wait_stream(Ps[m])
        for m in range(n):
            main.wait_stream(Fs[m])
        res = {"packed": torch.cat([o[0] for o in outs]), "counts": torch.cat([o[1] for o in outs]), "gates": None, "_hold": hold}
        return res

    def _rest_program(self, feats, pooled, front, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv=0):
        """Device forward from cached Swin / FPN features and a cached language front (the LVIS protocol
        sends the same pixels 31 times, engine/inference.py:605-625, and the same 31 captions for every image)."""
        out = self._head_stage(list(feats), pooled, front, input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv)
        out.update(feats=list(feats), pooled=pooled, front=front)
        return out

    def clear_caches(self):
        """Drop the per-image feature cache, the per-caption language cache and every captured graph."""
        super().clear_caches()
        self._front_cache.clear()

    @torch.no_grad()
    def forward(self, images, targets=None, captions=None, positive_map=None, greenlight_map=None,
                return_backbone_features=False, return_raw=False, input_ids=None, attention_mask=None, reuse_backbone=None):
        """generalized_vl_rcnn_new.py:307-519, eval.  `reuse_backbone` (not in the reference; keyword only in spirit): None = follow
        MODEL.BACKBONE_CACHE; False = this call recomputes Swin / FPN whatever the cache holds.  The cache (f1) recognises the
        previous call's pixels by OBJECT IDENTITY + torch's version counter of `images.tensors`: a producer that refills the same
        tensor WITHOUT bumping the counter (numpy / DLPack views of its memory, `.data` writes, IPC or custom-kernel writers) must
        pass reuse_backbone=False (or call `clear_caches()` / set MODEL.BACKBONE_CACHE False) -- nothing else can see such a write.
        With cfg.TEST.USE_MULTISCALE true (read at every call; also `forward_chunks` and `forward_grounding`) the result is every image's
        UN-SUPPRESSED candidates, as the reference's post-processor returns them under that switch (pipeline.postprocess, candidate mode:
        no NMS, no DETECTIONS_PER_IMG cut, rows in score-descending order; `last_packed` [B, sum_l min(PRE_NMS_TOP_N, HW_l L), 6])."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        images = to_image_list(images)
        dev = images.tensors.device
        P, cfg = self._ensure_plan(dev), self.cfg
        dtype = P["backbone.body.patch_embed.proj.weight"].dtype
        Bn = images.tensors.shape[0]
        if input_ids is None:
            input_ids, attention_mask, max_kv = self.tokenize(captions, dev)
            cap_key = tuple(captions)
        else:                                                     # caller-supplied ids (tests): one host sync
            max_kv = int((attention_mask.cpu() * torch.arange(1, attention_mask.shape[1] + 1)).max())
            cap_key = None
        T = input_ids.shape[1]

        # host-side glue: all memoised, no device sync
        onehot = str(cfg.MODEL.DYHEAD.get("SCORE_AGG", "MEAN")).upper() == "ONEHOT"
        positive_map, labels_in_caption, pm_key, score_map, score_labels, max_kv = prepare_positive_map(positive_map, T, max_kv, onehot)
        # LIVE-ROW COMPACTION (round 5): everything behind the tokenizer runs on the first Tl = 16 ceil(max_kv / 16) text positions instead of
        # the MAX_QUERY_LEN = 256 the caption is padded to.  Padded positions are masked KEYS everywhere (BERT, GCP, VLFuse) and are never
        # scored, so no live output depends on them -- but as ROWS they went through every text-side GEMM, LayerNorm and elementwise kernel
        # (141-token caption: 44 % of those rows).  The key-length bucket is part of the HIP-graph key already, so Tl adds no graph.
        input_ids, cap_key, mkey = self._masked_ids(input_ids, cap_key, pm_key, labels_in_caption, positive_map, dev)
        Tl = self._live_len(T, max_kv)
        if Tl < T:
            input_ids, attention_mask = self._live_slice(input_ids, attention_mask, Tl, cap_key, dev, mkey)
        vision = idx = None
        if self._use_vq():
            vision, idx = self.query_selector.select_cached(pm_key, labels_in_caption, positive_map, Bn, Tl, dev, dtype)
            if vision.shape[1] == 0:                              # no label of this caption has a vision query: text only
                vision = idx = None
        tokidx, label_ids = self._tokidx_cache.get((len(score_labels), "onehot", str(dev)) if onehot else (pm_key, str(dev)),
                                                   lambda: build_token_index(score_map, score_labels, dev))
        im_wh = self._im_wh(images, dev)
        tail = (input_ids, attention_mask, vision, idx, tokidx, label_ids, im_wh, max_kv)
        if return_raw:
            x = images.tensors.to(dtype).contiguous(memory_format=torch.channels_last)
            raw = self._full_program(x, *tail, want_raw=True)
            return self._pad_raw_text(raw, T) if Tl < T else raw
        use_graph = self.use_hip_graph and not _ops.timing_active()

        # f1: the pixels of the previous call (same tensor object, not modified since) -> cached Swin / FPN features;
        # a caption seen before -> cached image-independent BERT layers
        src = images.tensors
        fkey = (cap_key, Bn, vision is not None, Tl, mkey)
        out = None

        def full():                                               # miss: the whole device forward; the caches keep CLONES of its features
            nonlocal out                                          # (under HIP-graph replay `out` are the graph's static buffers)
            x = self._pixels(src, dtype)
            staggered = (self.micro_batches > 1 and Bn > 1 and not self.backbone_cache and x.is_cuda
                         and not cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE and not return_backbone_features
                         and cfg.MODEL.DYHEAD.get("LEVEL_STREAMS", True))
            out = self._run("_staggered_program" if staggered else "_full_program", (x,) + tail, use_graph)
            if not self.backbone_cache:
                return None
            keep = self._tree_map(lambda t: t.clone(), {"feats": out["feats"], "pooled": out["pooled"], "front": out["front"]})
            if cap_key is not None:
                self._front_cache.get(fkey, lambda: keep["front"])
            return {"feats": keep["feats"], "pooled": keep["pooled"]}
        fc, hit = self._cached_features(src, reuse_backbone, full)
        if hit:
            front = self._front(fkey if cap_key is not None else None, lambda: pipeline.language_front(
                P, cfg, input_ids, attention_mask, vision is not None, max_kv=max_kv))
            out = self._run("_rest_program", (fc["feats"], fc["pooled"], front) + tail, use_graph)

        # fixed-shape detections [B, K, 6] for the RCCL all-gather (mq_det_amd.parallel.gather_detections); cloned: under
        # HIP-graph replay `out` are the graph's static buffers, which the next forward overwrites
        self.last_packed = packed = out["packed"].clone()
        gates = out["gates"]
        if gates is not None:
            counts, gates = torch.cat([out["counts"].float(), gates.float()]).tolist(), None
            counts, gates = [int(c) for c in counts[:Bn]], counts[Bn:]
        else:
            counts = out["counts"].tolist()                       # the one device->host sync of the forward
        counts = self._split_counts(counts)
        result = self._boxlists(packed, counts, images.image_sizes)
        if cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE:
            return result, gates
        if return_backbone_features:
            return result, [f.float().contiguous() for f in out["feats"]]
        return result

    @staticmethod
    def _boxlists(packed, counts, image_sizes, first=0):
        """[items, K, 6] packed detections (a tensor nobody else writes) + live counts -> list[BoxList]: three launches for the whole batch (boxes,
        scores and int64 labels as contiguous tensors), the BoxLists hold per-image VIEWS of them (round 4: three launches per image)."""
        boxes, scores, labels = packed[..., :4].contiguous(), packed[..., 4].contiguous(), packed[..., 5].to(torch.int64)
        result = []
        for b, (h, w) in enumerate(image_sizes):
            it, n = first + b, counts[first + b]
            bl = BoxList(boxes[it, :n], (int(w), int(h)), mode="xyxy")
            bl.add_field("labels", labels[it, :n])
            bl.add_field("scores", scores[it, :n])
            result.append(bl)
        return result

    # ------------------------------------------------------------------ phrase grounding: one caption and one positive map per image
    @torch.no_grad()
    def forward_grounding(self, images, captions, positive_maps, return_raw=False):
        """The grounding protocol (`TEST.EVAL_TASK = "grounding"`, engine/inference.py:615-625) for a BATCH: `captions` = B different
        strings, `positive_maps` = B dicts {label: [token positions]} of any sizes.  Item i equals `model(ImageList(images.tensors[i:i+1],
        images.image_sizes[i:i+1]), captions=[captions[i]], positive_map=positive_maps[i])[0]` on the same padded canvas up to summation
        order (the reference asserts one image per batch, :622), but the batch is ONE launch sequence through `_full_program` / `_run`,
        HIP graphs as in `forward`: per-item vision queries (`query_selector.select`), per-item [MASK]ed ids (`_masked_ids`), the
        per-item token index and label table `forward_chunks` passes to the scoring kernels.  The live text length is the longest
        caption's.  -> list[BoxList] (with VISION_QUERY.RETURN_ATTN_GATE_VALUE: (list, gates) like `forward`), or the raw dict."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        images = to_image_list(images)
        dev = images.tensors.device
        P, cfg = self._ensure_plan(dev), self.cfg
        dtype = P["backbone.body.patch_embed.proj.weight"].dtype
        Bn = images.tensors.shape[0]
        if len(captions) != Bn or len(positive_maps) != Bn:
            raise ValueError(f"forward_grounding: {Bn} images, {len(captions)} captions, {len(positive_maps)} positive maps")
        onehot = str(cfg.MODEL.DYHEAD.get("SCORE_AGG", "MEAN")).upper() == "ONEHOT"
        ids, ams, kvs, pms, labs, smaps = [], [], [], [], [], []
        for cap, pm in zip(captions, positive_maps):
            i, a, kv = self.tokenize([cap], dev)
            pm, lab, pm_key, smap, slab, kv = prepare_positive_map(pm, i.shape[1], kv, onehot)
            i, _, _ = self._masked_ids(i, (cap,), pm_key, lab, pm, dev)
            ids.append(i)
            ams.append(a)
            kvs.append(kv)
            pms.append(pm)
            labs.append(lab)
            smaps.append((smap, slab))
        T = ids[0].shape[1]
        max_kv = max(kvs) if min(kvs) > 0 else 0
        Tl = self._live_len(T, max_kv)                            # live-row compaction (see forward): the batch's longest caption
        input_ids, attention_mask = torch.cat(ids)[:, :Tl].contiguous(), torch.cat(ams)[:, :Tl].contiguous()
        vision = idx = None
        if self._use_vq():
            vision, idx = self.query_selector.select(labs, pms, Tl, dev, dtype)
            if vision.shape[1] == 0:                              # no label of any caption has a vision query: text only
                vision = idx = None
        tok3, lab2 = build_item_token_index(smaps)
        tail = (input_ids, attention_mask, vision, idx, tok3.to(dev), lab2.to(dev), self._im_wh(images, dev), max_kv)
        if return_raw:
            x = images.tensors.to(dtype).contiguous(memory_format=torch.channels_last)
            raw = self._full_program(x, *tail, want_raw=True)
            return self._pad_raw_text(raw, T) if Tl < T else raw
        out = self._run("_full_program", (self._pixels(images.tensors, dtype),) + tail, self.use_hip_graph and not _ops.timing_active())
        self.last_packed = packed = out["packed"].clone()         # (cloned: under replay `out` are the graph's static buffers)
        gates = out["gates"]
        if gates is not None:
            counts = torch.cat([out["counts"].float(), gates.float()]).tolist()
            counts, gates = [int(c) for c in counts[:Bn]], counts[Bn:]
        else:
            counts = out["counts"].tolist()                       # the one device->host sync of the forward
        result = self._boxlists(packed, self._split_counts(counts), images.image_sizes)
        return (result, gates) if cfg.VISION_QUERY.RETURN_ATTN_GATE_VALUE else result

    # ------------------------------------------------------------------ the training objective, forward only (mq_det_amd/losses.py)
    @torch.no_grad()
    def forward_losses(self, images, targets, captions=None, positive_map=None, input_ids=None, attention_mask=None):
        """The ATSS objective of the reference's training forward (rpn/loss.py:850-1201 under the mq-glip-*.yaml loss switches) on the
        DETERMINISTIC EVAL-MODE forward: no autograd, no dropout, `model.train()` keeps raising.  targets: one BoxList per image (xyxy,
        field 'labels', input-image coordinates, any device); captions: one string per image (one string serves the batch);
        positive_map [sum of gts, MAX_QUERY_LEN], default the concatenation of the targets' 'positive_map' fields as the reference's forward
        builds it.  Runs the eval programs up to the head stage -- per-image vision queries, [MASK]ed ids of the vision-only mode, the
        backbone cache, live-token compaction, as `forward_grounding` --, then `ATSSLoss` instead of `postprocess`.  The label -> token table
        the vision-query selection needs is read ON THE HOST from the labels and positive-map rows: pass them as the loader yields them
        (CPU tensors) and the call makes no device->host transfer.  Eager (no HIP graph).  With the fused head operands the token loss is
        formed without writing logits; the GEMM-fallback head (captions over 256 tokens, other widths) has materialised them already and the
        loss is evaluated on them by a plain torch path.  -> {'loss_reg', 'loss_centerness', 'loss_dot_product_token', 'loss_cls',
        'sums' [6] (losses.SUM_NAMES), 'matched' [B, A]}, all on the device.  `input_ids` / `attention_mask` [B, T] (tests, as in `forward`):
        caller-supplied token ids instead of captions, one host synchronisation for the key-length bound."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        from ..losses import ATSSLoss
        criterion = ATSSLoss(self.cfg)                            # refuses unsupported loss settings by name, before anything is launched
        images = to_image_list(images)
        dev = images.tensors.device
        P = self._ensure_plan(dev)
        dtype = P["backbone.body.patch_embed.proj.weight"].dtype
        Bn = images.tensors.shape[0]
        if input_ids is None:
            if captions is None:
                raise ValueError("forward_losses: captions (or input_ids and attention_mask) are needed")
            captions = [captions] * Bn if isinstance(captions, str) else list(captions)
            if len(captions) == 1 and Bn > 1:
                captions = captions * Bn
            toks = [self.tokenize([cap], dev) for cap in captions]
        else:
            kv_all = int((attention_mask.cpu() * torch.arange(1, attention_mask.shape[1] + 1)).max())
            toks = [(input_ids[b:b + 1].to(dev), attention_mask[b:b + 1].to(dev), kv_all) for b in range(len(input_ids))]
            captions = [None] * len(toks)
        if len(targets) != Bn or len(toks) != Bn:
            raise ValueError(f"forward_losses: {Bn} images, {len(targets)} targets, {len(toks)} captions")
        if positive_map is None:
            if not all("positive_map" in t.fields() for t in targets):
                raise ValueError("forward_losses: no positive_map given and the targets carry no 'positive_map' field")
            positive_map = torch.cat([t.get_field("positive_map") for t in targets], 0)
        ids, ams, kvs, pms, labs = [], [], [], [], []
        off = 0
        for cap, (i, a, kv), t in zip(captions, toks, targets):
            n = len(t.bbox)
            rows, lab_t = positive_map[off:off + n], t.get_field("labels")
            off += n
            table = {}
            if self._use_vq():                                    # {label: token positions} of this image, for the vision queries / [MASK]ing
                lab_l = lab_t.tolist()
                for r_, c_ in (rows > 0).nonzero().tolist():
                    table.setdefault(int(lab_l[r_]), set()).add(c_)
            pm, lab, pm_key, _, _, kv = prepare_positive_map({k: sorted(v) for k, v in table.items()}, i.shape[1], kv, False)
            i, _, _ = self._masked_ids(i, None if cap is None else (cap,), pm_key, lab, pm, dev)
            ids.append(i)
            ams.append(a)
            kvs.append(kv)
            pms.append(pm)
            labs.append(lab)
        T = ids[0].shape[1]
        max_kv = max(kvs) if min(kvs) > 0 else 0
        Tl = self._live_len(T, max_kv)
        full_mask = torch.cat(ams)
        input_ids, attention_mask = torch.cat(ids)[:, :Tl].contiguous(), full_mask[:, :Tl].contiguous()
        vision = idx = None
        if self._use_vq():
            vision, idx = self.query_selector.select(labs, pms, Tl, dev, dtype)
            if vision.shape[1] == 0:
                vision = idx = None
        feats, pooled = self._features(images)
        front = pipeline.language_front(P, self.cfg, input_ids, attention_mask, vision is not None, max_kv=max_kv)
        _, head, _ = self._head_operands(list(feats), pooled, front, input_ids, attention_mask, vision, idx, max_kv)
        return criterion(head, self._anchors(feats), targets, positive_map, full_mask)

    # ------------------------------------------------------------------ chunk batching
    def _features(self, images):
        """(feats, pooled) of an image batch through the per-image cache (Swin + FPN run once per distinct tensor)."""
        P = self._ensure_plan(images.tensors.device)
        src = images.tensors

        def make():
            feats, pooled = self._backbone_stage(self._pixels(src, P["backbone.body.patch_embed.proj.weight"].dtype))
            return {"feats": feats, "pooled": pooled}
        fc, _ = self._cached_features(src, None, make)
        return fc["feats"], fc["pooled"]

    def _features_usable(self, rec):
        """Features cached before a query bank was loaded lack the pooled FPN tokens the GCP pre-select attends to."""
        return rec["pooled"] is not None or not self._use_vq()

    def _front(self, key, make):
        """Image-independent BERT layers of a caption through their cache (`key` None: caller-supplied token ids, not cached)."""
        self.cache_stats["front_hit" if key is not None and key in self._front_cache else "front_miss"] += 1
        return make() if key is None else self._front_cache.get(key, make)

    def _front_for(self, caption, dev, use_vq, masked_ids=None, mkey=None):
        """Image-independent BERT layers of ONE caption (batch 1), cached per caption and mask signature (`masked_ids`: the caption's ids
        with the [MASK]ed words of `mkey`, _masked_ids)."""
        def make():
            ids, am, kv = self.tokenize([caption], dev)
            return pipeline.language_front(self._plan, self.cfg, ids if mkey is None else masked_ids, am, use_vq, max_kv=kv)
        return self._front(((caption,), 1, use_vq, mkey), make)

    @torch.no_grad()
    def forward_chunks(self, images, chunks, max_items=32):
        """The LVIS / ODinW evaluation protocol in ONE call: `chunks` = [(caption, positive_map), ...] (the 31 chunk captions of
        engine/inference.py:605-625) for the SAME image batch.  Equivalent to `[model(images, captions=[c] * B,
        positive_map=pm) for c, pm in chunks]`, but Swin + FPN run once, the image-independent BERT layers once per caption
        (cached across images), and the image-dependent rest runs with the chunks stacked along the batch dimension
        (up to `max_items` image x chunk items per launch sequence): B = 1 -- the reference's TEST.IMS_PER_BATCH -- no longer
        means a batch-1 forward.  Returns list (over chunks) of list[BoxList] (over images).
        Vision-only evaluation (_masked_ids) masks every chunk's ids with that chunk's positive map, like the loop above.  With
        0 < VISION_QUERY.TEXT_DROPOUT < 1 every (chunk, image) item draws its own mask, so no caption-level state can be shared between
        items: that setting runs the loop above as it is written."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        images = to_image_list(images)
        if self._per_item_text_dropout():
            outs = [self.forward(images, captions=[cap] * images.tensors.shape[0], positive_map=pm) for cap, pm in chunks]
            return [o[0] if isinstance(o, tuple) else o for o in outs]
        Bn = images.tensors.shape[0]
        results = []
        for packed, counts, g in self._chunk_groups(images, chunks, max_items):
            counts = self._split_counts(counts.tolist())          # the one device->host sync of the group
            for c in range(g):
                results.append(self._boxlists(packed, counts, images.image_sizes, first=c * Bn))
        return results

    @torch.no_grad()
    def forward_chunks_packed(self, images, chunks, max_items=32):
        """`forward_chunks` without its host steps: per launch group (packed [g * B, K2, 6], RAW counts [g * B] int32 on the device, g), the
        items chunk-major (item = chunk * B + image) -- what `LvisFixedAPEvaluator.update_packed` / `CocoAPEvaluator.update_packed` take.
        Nothing is read back: no `.tolist()`, no BoxLists, and `last_tie_overflow` is not maintained (the overflow bit stays in the counts).
        None with 0 < VISION_QUERY.TEXT_DROPOUT < 1, where `forward_chunks` loops `forward`: the caller then takes the BoxList path."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        images = to_image_list(images)
        if self._per_item_text_dropout():
            return None
        return [(packed, counts.clone(), g) for packed, counts, g in self._chunk_groups(images, chunks, max_items)]

    def _per_item_text_dropout(self):
        return self._use_vq() and 0.0 < text_dropout_rate(self.cfg) < 1.0

    def _chunk_groups(self, images, chunks, max_items):
        """The launch groups of `forward_chunks`: yields (packed [g * B, K2, 6] -- a clone --, the group's raw counts as the program left them
        -- under graph replay the graph's static buffer: read or clone before the next group runs --, g)."""
        dev = images.tensors.device
        feats, pooled = self._features(images)
        P, cfg = self._plan, self.cfg
        dtype = P["backbone.body.patch_embed.proj.weight"].dtype
        Bn = images.tensors.shape[0]
        use_vq = self._use_vq()
        use_graph = self.use_hip_graph and not _ops.timing_active()
        im_wh = self._im_wh(images, dev)
        onehot = str(cfg.MODEL.DYHEAD.get("SCORE_AGG", "MEAN")).upper() == "ONEHOT"
        per = max(1, int(max_items) // Bn)
        for g0 in range(0, len(chunks), per):
            grp = chunks[g0:g0 + per]
            g = len(grp)
            ids, ams, kvs, fronts, pms, labs, smaps, masked = [], [], [], [], [], [], [], []
            for cap, pm in grp:
                i, a, kv = self.tokenize([cap], dev)
                pm, lab, pm_key, smap, slab, kv = prepare_positive_map(pm, i.shape[1], kv, onehot)
                i, _, mkey = self._masked_ids(i, (cap,), pm_key, lab, pm, dev, n_images=Bn)
                masked.append((i, mkey))                          # all MAX_QUERY_LEN positions: what the cached front is computed from
                ids.append(i)
                ams.append(a)
                kvs.append(kv)
                pms.append(pm)
                labs.append(lab)
                smaps.append((smap, slab))                        # what the scoring kernel takes (ONEHOT: class column j = token j, label j + 1)
            T = self._live_len(ids[0].shape[1], max(kvs) if min(kvs) > 0 else 0)          # live-row compaction (see forward): the group's longest caption
            live = lambda t_: t_[:, :T]                           # noqa: E731
            ids, ams = [live(i) for i in ids], [live(a) for a in ams]
            vision = idx = None
            if use_vq:                                            # item order: chunk-major (item = chunk * B + image)
                vision, idx = self.query_selector.select([l for l in labs for _ in range(Bn)], [pm for pm in pms for _ in range(Bn)],
                                                         T, dev, dtype)
                if vision.shape[1] == 0:
                    vision = idx = None
            for (cap, _), (i, mkey) in zip(grp, masked):
                fronts.append(self._front_for(cap, dev, vision is not None, i, mkey))
            rep = lambda t: t.repeat_interleave(Bn, 0)            # noqa: E731  [g, ...] -> [g * B, ...] chunk-major
            # (the cached fronts hold all MAX_QUERY_LEN positions of their caption: cut to the group's live length here)
            front = {"x": rep(torch.cat([live(f["x"]) for f in fronts])),
                     "x32": None if fronts[0].get("x32") is None else rep(torch.cat([live(f["x32"]) for f in fronts])),
                     "hidden": [rep(torch.cat([live(f["hidden"][k]) for f in fronts])) for k in range(len(fronts[0]["hidden"]))],
                     "key_bias": rep(torch.cat([live(f["key_bias"]) for f in fronts])), "kv_len": rep(torch.cat([f["kv_len"] for f in fronts])),
                     "next": fronts[0]["next"]}
            tok3, lab2 = build_item_token_index(smaps)
            tok3, lab2 = rep(tok3.to(dev)).contiguous(), rep(lab2.to(dev)).contiguous()
            tile = lambda f: f.permute(0, 2, 3, 1).repeat(g, 1, 1, 1).permute(0, 3, 1, 2)     # noqa: E731  NHWC memory kept
            inputs = ([tile(f) for f in feats], None if pooled is None else pooled.repeat(g, 1, 1), front, rep(torch.cat(ids)),
                      rep(torch.cat(ams)), vision, idx, tok3, lab2, im_wh.repeat(g, 1), max(kvs))
            out = self._run("_rest_program", inputs, use_graph)
            yield out["packed"].clone(), out["counts"], g


_DETECTION_META_ARCHITECTURES = {"GeneralizedVLRCNN_New": GeneralizedVLRCNN_New}


def build_detection_model(cfg, **kwargs):
    """modeling/detector/__init__.py:9-14."""
    if cfg.get("GROUNDINGDINO", {}).get("enabled", False):       # groundingdino_new.models.build_model(cfg.GROUNDINGDINO, cfg)
        from .gdino import GroundingDINO
        return GroundingDINO(cfg, **kwargs)
    return _DETECTION_META_ARCHITECTURES[cfg.MODEL.META_ARCHITECTURE](cfg, **kwargs)
