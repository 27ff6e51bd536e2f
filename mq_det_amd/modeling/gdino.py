"""MQ-GroundingDINO behind the reference's module API, on the MI355X pipeline (gdino_pipeline.py).

Drop-in for `groundingdino_new.models.GroundingDINO.groundingdino.GroundingDINO` (:98-661) as returned by
`build_detection_model(cfg)` when `cfg.GROUNDINGDINO.enabled` (modeling/detector/__init__.py:9-14): same constructor input (the
yacs cfg), same `state_dict()` names (strict `load_state_dict` of a reference checkpoint, incl. the aliased `bbox_embed.*` /
`transformer.decoder.bbox_embed.*` entries of the shared box head), `forward(samples, targets=None, captions=..., positive_map=...)`
-> list[BoxList] (`(result, srcs)` with return_backbone_features), `load_query_bank`, `extract_query`.  Inference only.
Differences by design: vision queries work for any batch size whose images share the caption (the reference asserts B == 1,
:502); a label with an empty token list silences ALL detections exactly like the reference's NaN propagation (:291-305).
"""
import os

import torch

from .. import ops as _ops
from ..structures import BoxList, to_image_list
from . import gdino_pipeline as gp, pipeline
from .detector import expand_bbox, pool_into_bank
from .device_model import DeviceModel
from .graph_runner import Memo
from .params import build_param_tree, gdino_param_specs, gdino_swin_cfg
from .query_selector import prepare_positive_map


def preprocess_caption(caption):
    """groundingdino.py:92-96."""
    result = caption.lower().strip()
    return result if result.endswith(".") else result + "."


class GroundingDINO(DeviceModel):
    _plan_memos = ("_geo_cache",)

    def __init__(self, cfg, tokenizer=None, **kwargs):
        super().__init__(cfg)
        G = cfg.GROUNDINGDINO
        self._validate_config()
        build_param_tree(self, cfg, specs=gdino_param_specs(cfg))
        self.box_threshold = G.box_threshold
        self.num_queries, self.hidden_dim, self.max_text_len = G.num_queries, G.hidden_dim, 256
        self._build_query_path()
        self.tokenizer = tokenizer if tokenizer is not None else self._load_tokenizer(G.text_encoder_type)
        self.specical_tokens = self.tokenizer.convert_tokens_to_ids(["[CLS]", "[SEP]", ".", "?"])      # (sic) groundingdino.py:194
        self._swin = gdino_swin_cfg(cfg)
        self._geo_cache, self._txt_cache, self._map_cache = Memo(16), Memo(64), Memo(64)
        self.eval()

    @staticmethod
    def _load_tokenizer(name):
        from transformers import AutoTokenizer
        if os.path.basename(name) != "bert-base-uncased":
            raise NotImplementedError("GROUNDINGDINO.text_encoder_type: only bert-base-uncased (groundingdino.py:183-184)")
        if not os.path.isdir(name):
            raise RuntimeError(f"tokenizer files for '{name}' are not on disk (no network here): point GROUNDINGDINO.text_encoder_type "
                               "at a local directory whose basename is 'bert-base-uncased' or pass tokenizer=...")
        return AutoTokenizer.from_pretrained(name)

    def _validate_config(self):
        G = self.cfg.GROUNDINGDINO
        want = dict(two_stage_type="standard", embed_init_tgt=True, use_text_enhancer=True, use_fusion_layer=True,
                    use_text_cross_attention=True, sub_sentence_present=True, dec_pred_bbox_embed_share=True, num_patterns=0,
                    query_dim=4, num_feature_levels=4, enc_n_points=4, dec_n_points=4, hidden_dim=256, nheads=8,
                    transformer_activation="relu", pre_norm=False, position_embedding="sine", max_text_len=256)
        for k, v in want.items():
            if G.get(k, v) != v:
                raise NotImplementedError(f"GROUNDINGDINO.{k} = {G[k]}: this path implements {v!r} (configs/pretrain/mq-groundingdino-t.yaml)")
        if list(G.return_interm_indices) != [1, 2, 3]:
            raise NotImplementedError("GROUNDINGDINO.return_interm_indices must be [1, 2, 3]")
        if G.pe_temperatureH != G.pe_temperatureW:
            raise NotImplementedError("GROUNDINGDINO.pe_temperatureH != pe_temperatureW")
        V = self.cfg.VISION_QUERY
        if V.get("ADD_ADAPT_LAYER", False) or V.get("QUERY_FUSION", False) or V.get("LEARNABLE_BANK", False):
            raise NotImplementedError("VISION_QUERY.ADD_ADAPT_LAYER / QUERY_FUSION / LEARNABLE_BANK are not implemented")

    def _build_plan(self, device, dtype):
        return gp.build_gdino_plan(self.state_dict(), self.cfg, device, self._swin, dtype=dtype)

    # ------------------------------------------------------------------ memoised host-side glue
    def _text(self, captions, dev):
        def make():
            tok = self.tokenizer(list(captions), padding="max_length", return_tensors="pt")          # groundingdino.py:518
            return gp.text_inputs(self.cfg, tok["input_ids"], tok["attention_mask"], self.specical_tokens, dev)
        return self._txt_cache.get((tuple(captions), str(dev)), make)

    def _class_map(self, positive_map, dev):
        """[T, C] fp32: column label-1 holds 1/len over the label's tokens (convert_grounding_to_od_logits, MEAN);
        returns (map, has_empty_label)."""
        T, C = self.max_text_len, self.cfg.MODEL.DYHEAD.NUM_CLASSES - 1
        key = (tuple((k, (v,) if isinstance(v, int) else tuple(v)) for k, v in positive_map.items()), str(dev))

        def make():
            m = torch.zeros(T, C)
            empty = False
            for lab, toks in positive_map.items():
                toks = [toks] if isinstance(toks, int) else list(toks)
                if not toks:
                    empty = True
                    continue
                m[:, lab - 1] = 0.0
                for t in toks:
                    m[t, lab - 1] += 1.0 / len(toks)
            return m.to(dev), empty
        return self._map_cache.get(key, make)

    # ------------------------------------------------------------------ device program (capturable)
    def _program(self, x, geo, txt, vision, idx, class_map, im_hw, nan_labels, max_kv=0, trace=None):
        return gp.forward_device(self._plan, self.cfg, self._swin, x, geo, txt, vision, idx, class_map, im_hw, max_kv=int(max_kv),
                                 nan_labels=bool(nan_labels), trace=trace)

    def _program_rest(self, src32, geo, txt, vision, idx, class_map, im_hw, nan_labels, max_kv=0):
        """From the cached projected levels of the same pixels (Swin + input projections skipped)."""
        return gp.forward_device(self._plan, self.cfg, self._swin, None, geo, txt, vision, idx, class_map, im_hw, max_kv=int(max_kv),
                                 nan_labels=bool(nan_labels), src32=src32)

    @torch.no_grad()
    def forward(self, samples, targets=None, return_raw=False, **kw):
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        if targets is not None:
            captions = [t.get_field("caption") for t in targets if "caption" in t.fields()]
        else:
            captions = kw["captions"]
        captions = [preprocess_caption(c) for c in captions]
        # token positions cut away by the truncation to max_text_len cannot be scored (the reference would index past the
        # [.., 256] token scores): dropped, like the MQ-GLIP class does
        positive_map, labels_in_caption, pm_key = prepare_positive_map(kw["positive_map"], self.max_text_len)[:3]
        return_backbone_features = kw.get("return_backbone_features", False)
        images = to_image_list(samples)
        dev = images.tensors.device
        P = self._ensure_plan(dev)
        dtype = P["backbone.0.patch_embed.proj.weight"].dtype
        Bn, _, H, W = images.tensors.shape
        sizes = tuple((int(h), int(w)) for h, w in images.image_sizes)
        geo = self._geo_cache.get((H, W, sizes, str(dev)), lambda: gp.geometry(P, self.cfg, H, W, sizes, dev))
        txt, max_kv = self._text(captions, dev)
        class_map, nan_labels = self._class_map(positive_map, dev)
        vision = idx = None
        if self._use_vq():
            vision, idx = self.query_selector.select_cached(pm_key, labels_in_caption, positive_map, Bn,
                                                            self.cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN, dev, dtype)
            if vision.shape[1] == 0:
                vision = idx = None
        im_hw = torch.tensor([[h, w] for (h, w) in sizes], dtype=torch.float32, device=dev)
        x = images.tensors.to(dtype).contiguous(memory_format=torch.channels_last)
        inputs = (x, geo, txt, vision, idx, class_map, im_hw, nan_labels, max_kv)
        if return_raw:
            trace = {}
            out = self._program(*inputs, trace=trace)
            trace.update(out=out, geo=geo, txt=txt)
            return trace
        use_graph = self.use_hip_graph and not _ops.timing_active()
        # f1: the pixels of the previous call (same tensor object, not modified since) -> cached projected levels (a writer that
        # refills `images.tensors` without bumping its version counter must pass reuse_backbone=False -- see
        # GeneralizedVLRCNN_New.forward)
        out = None

        def full():                                               # miss: the whole device forward; the cache keeps a clone of its levels
            nonlocal out
            out = self._run("_program", inputs, use_graph)
            return out["srcs"].clone() if self.backbone_cache else None
        src32, hit = self._cached_features(images.tensors, kw.get("reuse_backbone"), full)
        if hit:
            out = self._run("_program_rest", (src32,) + inputs[1:], use_graph)
        self.last_packed = packed = out["packed"].clone()
        nz = out["keep"].nonzero()                                 # [n, 2] (image, query) in query order: the one device -> host
        counts = torch.bincount(nz[:, 0], minlength=Bn).tolist()   # sync of the forward
        sel = packed[nz[:, 0], nz[:, 1]]
        result, s0 = [], 0
        for b, (h, w) in enumerate(sizes):
            part = sel[s0:s0 + counts[b]]
            s0 += counts[b]
            bl = BoxList(part[:, :4].clone(), (int(w), int(h)), mode="xyxy")
            bl.add_field("labels", part[:, 5].to(torch.int64))
            bl.add_field("scores", part[:, 4].clone())
            result.append(bl)
        if return_backbone_features:
            s0, feats = 0, []
            for (h, w) in geo["shapes"]:                           # `srcs` of the reference: the projected levels, NCHW
                feats.append(out["srcs"][:, s0:s0 + h * w].reshape(Bn, h, w, -1).permute(0, 3, 1, 2).clone())
                s0 += h * w
            return result, feats
        return result

    # ------------------------------------------------------------------ the training objective, forward only (mq_det_amd/set_loss.py)
    @torch.no_grad()
    def forward_losses(self, samples, targets, captions=None, positive_map=None):
        """The set criterion of the reference's training forward (groundingdino.py:608-641, loss.py, matcher.py) on the DETERMINISTIC
        EVAL-MODE forward: no autograd, no dropout, `model.train()` keeps raising.  targets: one BoxList per image (xyxy or with a
        'normed_cxcy_boxes' field; 'labels' when a query bank is loaded); captions: one string per image, default the targets' 'caption'
        fields; positive_map [sum of gts, max_text_len], default the concatenation of the targets' 'positive_map' fields (binarised, as the
        reference does).  Runs the eval program, eagerly, through the decoder with the per-layer states kept, then `SetCriterionLoss`
        instead of the detection heads.  The label -> token table the vision-query selection needs is read ON THE HOST from the labels and
        positive-map rows: pass them as the loader yields them (CPU tensors) and the call makes no device->host transfer.
        -> the reference's dict (`loss_ce`, `loss_bbox`, `loss_giou`, `loss_*_{i}` of the aux layers, `loss_gate` with vision queries) plus
        `sums` [L, 3], `num_boxes`, `match_q`, `q2g`, on the device."""
        if self.training:
            raise NotImplementedError("training forward is out of scope")
        from ..set_loss import SetCriterionLoss
        criterion = SetCriterionLoss(self.cfg)                    # refuses unsupported settings by name, before anything is launched
        V = self.cfg.VISION_QUERY
        if V.ENABLED and V.get("RETURN_ATTN_GATE_VALUE", False):
            raise NotImplementedError("VISION_QUERY.RETURN_ATTN_GATE_VALUE: the reference's gate term indexes a Python float there")
        images = to_image_list(samples)
        dev = images.tensors.device
        Bn, _, H, W = images.tensors.shape
        if captions is None:
            captions = [t.get_field("caption") for t in targets]
        captions = [captions] * Bn if isinstance(captions, str) else list(captions)
        if len(targets) != Bn or len(captions) != Bn:
            raise ValueError(f"forward_losses: {Bn} images, {len(targets)} targets, {len(captions)} captions")
        captions = [preprocess_caption(c) for c in captions]
        if positive_map is None:
            if not all("positive_map" in t.fields() for t in targets):
                raise ValueError("forward_losses: no positive_map given and the targets carry no 'positive_map' field")
            positive_map = torch.cat([t.get_field("positive_map") for t in targets], 0)
        positive_map = (positive_map > 0).float()                 # groundingdino.py:612
        P = self._ensure_plan(dev)
        dtype = P["backbone.0.patch_embed.proj.weight"].dtype
        sizes = tuple((int(h), int(w)) for h, w in images.image_sizes)
        geo = self._geo_cache.get((H, W, sizes, str(dev)), lambda: gp.geometry(P, self.cfg, H, W, sizes, dev))
        txt, max_kv = self._text(captions, dev)
        vision = idx = None
        if self._use_vq():
            table = {}                                            # {label: token positions} over the batch, for the vision queries
            labels = torch.cat([t.get_field("labels").reshape(-1) for t in targets]).tolist()
            for r, c in positive_map.nonzero().tolist():
                table.setdefault(int(labels[r]), set()).add(c)
            pm, labels_in_caption, pm_key = prepare_positive_map({k: sorted(table[k]) for k in sorted(table)}, self.max_text_len)[:3]
            vision, idx = self.query_selector.select_cached(pm_key, labels_in_caption, pm, Bn, self.cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN,
                                                            dev, dtype)
            if vision.shape[1] == 0:
                vision = idx = None
        x = images.tensors.to(dtype).contiguous(memory_format=torch.channels_last)
        out = gp.forward_device(P, self.cfg, self._swin, x, geo, txt, vision, idx, None, None, max_kv=int(max_kv), want_set=True)
        logits, boxes = out["set_logits"], out["set_boxes"]
        L = logits.shape[0]
        outputs = {"pred_logits": logits[-1], "pred_boxes": boxes[-1],
                   "aux_outputs": [{"pred_logits": logits[l], "pred_boxes": boxes[l]} for l in range(L - 1)]}
        losses = criterion(outputs, targets, txt["token_mask"], positive_map)
        losses["outputs"] = outputs
        if V.ENABLED:                                             # groundingdino.py:621-640: under CONDITION_GATE the ff_gate parameters alone
            gates = [v.reshape(-1)[0].to(dev).float() for k, v in self.state_dict().items() if ".qv_layer." in k and k.endswith(".ff_gate")]
            if gates:
                losses["loss_gate"] = float(V.get("GATE_REGULARIZATION_SCALE", 0.1)) * (1 - torch.stack(gates).abs()).sum() / len(gates)
        return losses

    @torch.no_grad()
    def extract_query(self, samples=None, targets=None, query_images=None, visual_features=None, exclude_similar=False,
                      device=None, max_query_number=None):
        """groundingdino.py:340-421: ROI-pool the (projected) feature levels under the expanded target boxes into the bank."""
        cfg = self.cfg
        device = torch.device(device) if device else (to_image_list(samples).tensors.device if samples is not None
                                                      else visual_features[0].device)
        targets = expand_bbox([t.to(device) for t in targets if t is not None], expand_ratio=cfg.VISION_QUERY.EXPAND_RATIO)
        if visual_features is None:
            images = to_image_list(samples)
            P = self._ensure_plan(images.tensors.device)
            x = images.tensors.to(P["backbone.0.patch_embed.proj.weight"].dtype).contiguous(memory_format=torch.channels_last)
            src = gp.input_projections(P, cfg, pipeline.swin_forward(P, cfg, x, p="backbone.0", SW=self._swin))
            visual_features, s0 = [], 0
            for (h, w) in gp.level_shapes(x.shape[2], x.shape[3], cfg.GROUNDINGDINO.num_feature_levels):
                visual_features.append(src[:, s0:s0 + h * w].reshape(x.shape[0], h, w, -1).permute(0, 3, 1, 2))
                s0 += h * w
        else:
            visual_features = [v.to(device) for v in visual_features]
        return pool_into_bank(cfg, self.pooler, visual_features, targets, query_images, exclude_similar, max_query_number)
