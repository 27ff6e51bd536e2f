"""DeviceModel -- the host-side shell the two detector classes (MQ-GLIP: detector.py, MQ-GroundingDINO: gdino.py) share: the inference
plan and its lifecycle, the kernel selection kept with it, the HIP-graph settings, the feature cache of the last pixel tensor and the
reference-API methods that are the same for both.  A subclass supplies `_build_plan`, `_validate_config`, `_plan_memos` (the names of
its Memo attributes whose tensors depend on the plan) and what its feature cache stores (the `make` of `_cached_features`)."""
from collections import OrderedDict

import torch
from torch import nn

from .. import ops as _ops
from . import pipeline
from .graph_runner import GraphRunner
from .poolers import CustomPooler, Pooler
from .query_selector import QuerySelector, labels_and_maps


def compute_dtype(cfg):
    """MODEL.COMPUTE_DTYPE: the operand type of every kernel on the path -- "float16" (default, BASELINE.json configs[1]),
    "bfloat16" (configs[3]: the *_bf16 entry points of include/mqdet_hip.h) or "float32" (the precise mode: the *_f32 entry points, the
    same kernel sources with fp32 operands, and fp32 library GEMMs -- a quarter of the MFMA rate, for parity at the north-star's 1e-3 end
    to end, not for throughput); accumulation and residual streams are fp32 in every mode."""
    name = str(cfg.MODEL.get("COMPUTE_DTYPE", "float16")).lower()
    if name in ("float16", "fp16", "half"):
        return torch.float16
    if name in ("bfloat16", "bf16"):
        return torch.bfloat16
    if name in ("float32", "fp32", "float"):
        return torch.float32
    raise NotImplementedError(f"MODEL.COMPUTE_DTYPE = {name}: float16, bfloat16 or float32")


class DeviceModel(GraphRunner, nn.Module):
    _plan_memos = ()

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        M = cfg.MODEL
        self._plan = self._plan_key = None
        self._kernels = None                                      # kernel selection of the plan (ops.configure), set by prepare()
        self._graphs = OrderedDict()                              # LRU of captured HIP graphs, keyed by static shapes only
        self._feat_cache = None                                   # (pixel tensor, its version counter, what the subclass keeps of it) (f1)
        self.use_hip_graph = bool(M.get("USE_HIP_GRAPH", True))
        self.graph_cache_size = int(M.get("HIP_GRAPH_CACHE", 8))
        self.graph_warm_calls = int(M.get("HIP_GRAPH_WARM_CALLS", 1))
        self.backbone_cache = bool(M.get("BACKBONE_CACHE", True))
        self.cache_stats = {"backbone_hit": 0, "backbone_miss": 0, "graph_replay": 0, "graph_capture": 0, "eager": 0, "graph_evict": 0}

    def _build_query_path(self):
        """Box pooler of the query-extraction path (generalized_vl_rcnn_new.py:107-121) and the vision-query selector."""
        cfg = self.cfg
        RB = cfg.MODEL.ROI_BOX_HEAD
        pool_cls = Pooler if cfg.VISION_QUERY.SELECT_FPN_LEVEL else CustomPooler
        self.pooler = pool_cls(output_size=(RB.POOLER_RESOLUTION, RB.POOLER_RESOLUTION), scales=RB.POOLER_SCALES,
                               sampling_ratio=RB.POOLER_SAMPLING_RATIO, use_v2=True)
        self.query_selector = None if cfg.VISION_QUERY.DISABLE_SELECTOR else QuerySelector(cfg)

    # ------------------------------------------------------------------ plan management
    def _invalidate(self):
        self._plan = None
        for name in self._plan_memos:
            getattr(self, name).clear()
        self.clear_caches()

    def clear_caches(self):
        """Drop the per-image feature cache and every captured graph."""
        self._feat_cache = None
        self._drop_graphs()

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._invalidate()
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._invalidate()
        return out

    def prepare(self, device=None):
        """(Re)build the inference plan on `device`.  Called lazily by forward."""
        device = torch.device(device) if device is not None else next(self.parameters()).device
        if device.type != "cuda":
            raise RuntimeError("mq_det_amd runs on MI355X only (HIP kernels, no CPU fallback); got device " + str(device))
        _ops.load_library()
        self._kernels = dict(_ops.configure(self.cfg))             # kernel selection: read once per plan, kept WITH the plan
        self._validate_config()
        self._plan = self._build_plan(device, compute_dtype(self.cfg))
        self._plan_key = device
        return self._plan

    def _ensure_plan(self, device):
        """The plan for `device` (built when there is none, or one for another device), with its kernel selection active."""
        if self._plan is None or self._plan_key != device:
            self.prepare(device)
        _ops.activate(self._kernels)
        return self._plan

    def _cached_features(self, src, reuse, make):
        """-> (what the feature cache holds for the pixel tensor `src`, hit).  The previous call's pixels are recognised by OBJECT IDENTITY +
        torch's version counter; the strong reference to `src` keeps its storage alive, so the two cannot alias a different batch.  A miss
        (or `reuse` False: this call recomputes whatever the cache holds) stores `make()` when MODEL.BACKBONE_CACHE is on."""
        fc = self._feat_cache if (self.backbone_cache and reuse is not False) else None
        if fc is not None and fc[0] is src and fc[1] == src._version and self._features_usable(fc[2]):
            self.cache_stats["backbone_hit"] += 1
            return fc[2], True
        rec = make()
        if self.backbone_cache:
            self.cache_stats["backbone_miss"] += 1
            self._feat_cache = (src, src._version, rec)
        return rec, False

    def _features_usable(self, rec):
        return True

    # ------------------------------------------------------------------ reference API
    def train(self, mode=True):
        if mode:
            raise NotImplementedError("mq_det_amd implements the inference forward only (north-star scope)")
        return super().train(False)

    def load_query_bank(self, query_path):
        """A bank file's path, the `{label: Tensor[n, scales, C]}` dict, or a device-resident `QueryBank` (selected from on the device)."""
        self.query_selector.load_query_bank(query_path)

    def _use_vq(self):
        return bool(self.cfg.VISION_QUERY.ENABLED and self.query_selector is not None
                    and self.query_selector.query_bank is not None)

    def flatten_fpn_features(self, features):
        return pipeline.pooled_fpn_tokens(features)

    def get_labels_and_maps_from_positive_map(self, positive_map, dtype=torch.float):
        return labels_and_maps(positive_map, self.cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN)
