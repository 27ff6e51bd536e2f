"""Vision-query selection from a device-resident bank on the MI355X (QuerySelector with a QueryBank, csrc/query_bank.hip mq_bank_select_fwd):
the selector-level equalities of tests/test_query_select_cpu.py on the device, one launch per non-deterministic `select`, the tiny MQ-GLIP
model with a resident bank against the same model with the dict bank (`model(...)`, `forward_chunks`, `forward_grounding`), and HIP-graph
replays that must take each call's own draw."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_query_select_cpu as sc  # noqa: E402
from mq_det_amd.query_bank import QueryBank  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: the HIP path has no CPU fallback")
    from mq_det_amd import ops
    ops.load_library()
    return torch.device("cuda:0")


def _equal_detections(a, b):
    """bit-equal detections: the same program on the same vision rows and index (tests/test_gpu_parity.py)"""
    return (len(a) == len(b) and torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
            and torch.equal(a.get_field("labels"), b.get_field("labels")))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("S", [1, 5])
def test_select_on_the_device_equals_the_dict_path_in_one_launch(dev, S, dtype):
    from mq_det_amd import ops
    for C in (256, 6):
        bank = QueryBank.from_dict(sc.make_dict(C, S), dev)
        res, ref = sc.selectors(bank)
        for n_items in (1, 2):
            v, i = sc.same_select(res, ref, [sc.LABELS] * n_items, [sc.PMAP] * n_items, dtype=dtype, device=dev)
            assert v.is_cuda and i.is_cuda
        sc.same_select(res, ref, *sc.RAGGED, dtype=dtype, device=dev)
        items = 62
        sc.same_select(res, ref, [sc.LABELS] * items, [sc.PMAP] * items, dtype=dtype, device=dev, seed=9)
        assert not res.deterministic(sc.LABELS)
        ops.start_timing()
        try:
            res.select([sc.LABELS] * 2, [sc.PMAP] * 2, sc.T, dev, dtype)
        finally:
            rec = ops.stop_timing()
        assert set(rec) == {"bank_select"} and rec["bank_select"][0] == 1, rec


def test_snapshot_and_memo_on_the_device(dev):
    bank = QueryBank.from_dict(sc.make_dict(256, 1, {1: 2, 2: 3}), dev)
    res, ref = sc.selectors(bank)
    pm = {1: [0, 2], 2: [2]}
    a = res.select_cached("key", [1, 2], pm, 2, sc.T, dev, torch.float16)
    assert res.select_cached("key", [1, 2], pm, 2, sc.T, dev, torch.float16) is a
    v0, i0 = ref.select_cached("key", [1, 2], pm, 2, sc.T, dev, torch.float16)
    assert torch.equal(a[0], v0) and torch.equal(a[1], i0)
    g = torch.Generator().manual_seed(4)
    pool0 = bank.pool
    bank.update(torch.randn(200, 1, 256, generator=g), torch.tensor([1] * 100 + [30] * 100), 100)
    assert bank.pool is not pool0
    sc.same_select(res, ref, [[1, 2, 30]] * 2, [{1: [0], 2: [1], 30: [2]}] * 2, device=dev)      # `ref` holds the bank as it was at the load
    res.load_query_bank(bank)
    ref.load_query_bank({l: t.cpu() for l, t in bank.to_dict().items()})
    v, _ = sc.same_select(res, ref, [[1, 2, 30]] * 2, [{1: [0], 2: [1], 30: [2]}] * 2, device=dev)
    assert v.shape[1] == 3 * sc.K


class _Tiny:
    """the tiny MQ-GLIP model of tests/parity_checks.py with a bank of 12 rows per label, as a dict on the host and as a QueryBank"""

    def __init__(self, dev):
        import parity_checks as pc
        from mq_det_amd.structures import ImageList
        self.spec, _, self.cfg, self.model, _ = pc.tiny(dev)
        images, sizes, ids, am, self.pm, bank0 = pc.make_inputs(self.spec)
        g = torch.Generator().manual_seed(12)
        self.bank_dict = {l: torch.randn(12, *v.shape[1:], generator=g).to(v.dtype) for l, v in bank0.items()}
        self.bank = QueryBank.from_dict({l: v.float() for l, v in self.bank_dict.items()}, dev)
        self.bank_dict = {l: v.cpu() for l, v in self.bank.to_dict().items()}
        assert 12 > self.cfg.VISION_QUERY.NUM_QUERY_PER_CLASS
        self.il = lambda: ImageList(images.to(dev), sizes)
        self.kw = dict(captions=None, positive_map=self.pm, input_ids=ids.to(dev), attention_mask=am.to(dev))
        kv = int(am[0].sum())
        self.tokenize = lambda caps, d: (ids[:1].expand(len(caps), -1).contiguous().to(d), am[:1].expand(len(caps), -1).contiguous().to(d), kv)
        self.saved = (self.model.use_hip_graph, self.model.backbone_cache)

    def restore(self):
        self.model.use_hip_graph, self.model.backbone_cache = self.saved
        self.model.__dict__.pop("tokenize", None)
        self.model.clear_caches()


def test_tiny_model_with_a_resident_bank_equals_the_dict_bank_runs(dev):
    s = _Tiny(dev)
    model = s.model
    labs = list(s.pm)
    chunks = [("caption a", s.pm), ("caption b", {l: s.pm[l] for l in labs[:3]}), ("caption c", {l: s.pm[l] for l in labs[2:]})]
    caps, maps = ["caption a", "caption b"], [{l: s.pm[l] for l in labs[:4]}, {l: s.pm[l] for l in labs[3:]}]
    try:
        model.tokenize = s.tokenize
        model.use_hip_graph = False
        runs = []
        for bank in (s.bank_dict, s.bank):
            model.load_query_bank(bank)
            outs = []
            for call in (lambda: model(s.il(), **s.kw), lambda: model.forward_chunks(s.il(), chunks), lambda: model.forward_grounding(s.il(), caps, maps)):
                model.clear_caches()
                np.random.seed(21)
                outs.append(call())
            runs.append(outs)
        (fd, cd, gd), (fr, cr, gr) = runs
        assert sum(len(o) for o in fd) > 0
        for a, b in zip(fr, fd):
            assert _equal_detections(a, b)
        assert len(cr) == len(cd) == 3
        for chunk_r, chunk_d in zip(cr, cd):
            for a, b in zip(chunk_r, chunk_d):
                assert _equal_detections(a, b)
        for a, b in zip(gr, gd):
            assert _equal_detections(a, b)
    finally:
        s.restore()


def test_hip_graph_replays_take_each_calls_own_draw(dev):
    s = _Tiny(dev)
    model = s.model
    try:
        model.load_query_bank(s.bank)
        model.use_hip_graph = False
        refs = {}
        for seed in (31, 32):
            model.clear_caches()
            np.random.seed(seed)
            refs[seed] = model(s.il(), **s.kw)
        assert not all(_equal_detections(a, b) for a, b in zip(refs[31], refs[32]))              # other draws, other detections
        model.use_hip_graph = True
        model.clear_caches()
        il = s.il()
        replays = model.cache_stats["graph_replay"]
        for seed in (31, 32, 31, 32, 32, 31):                                                     # eager, capture + replay, replays
            np.random.seed(seed)
            out = model(il, **s.kw)
            for a, b in zip(out, refs[seed]):
                assert _equal_detections(a, b), seed
        assert any(e.get("stage") == 2 for e in model._graphs.values()), "HIP graph was not captured"
        assert model.cache_stats["graph_replay"] >= replays + 3
    finally:
        s.restore()
