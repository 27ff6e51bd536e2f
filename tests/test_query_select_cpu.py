"""Vision-query selection from a device-resident bank (QuerySelector with a QueryBank, csrc/query_bank.hip mq_bank_select_fwd) without a GPU:
the kernel SOURCE through the host emulation (tests/simt), under the buffer-overrun guard and both fibre schedules.  The yardstick is the dict
path of the same selector class on `bank.to_dict()`: after the same `np.random.seed` both give the same `vision` and `idx`, bit for bit, and
leave numpy's global generator in the same state.  Also: the snapshot rule, the dict-like queries, `forward()`, and
`online_update(resident=True)` on the stand-in model of tests/test_query_bank_cpu.py."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import query_bank_ref as qr  # noqa: E402
import test_query_bank_cpu as tc  # noqa: E402
from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.modeling.query_selector import QuerySelector, prepare_positive_map  # noqa: E402
from mq_det_amd.query_bank import QueryBank, online_update  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")

K = 3                                                       # NUM_QUERY_PER_CLASS of these tests
# rows per label: fewer than k, exactly k, more than k (twice), none (label 3 is inside the table, 1000 beyond it)
COUNTS = {1: 7, 2: 2, 4: 3, 6: 11}
T = 40


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def make_dict(C, S, counts=COUNTS, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + S)
    d = {lab: torch.randn(n, S, C, generator=g) for lab, n in counts.items()}
    d[1][0, 0, 0] = 1.0e5                                    # above the fp16 range: +inf in fp16 on both paths
    d[1][1, S - 1, C - 1] = -7.0e4
    return d


def selectors(bank, k=K, reference_rng=False):
    """(resident, dict): two selectors of one configuration, one holding the QueryBank, one `bank.to_dict()` on the CPU"""
    cfg = get_cfg()
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS = k
    cfg.VISION_QUERY.REFERENCE_RNG_STREAM = reference_rng
    res, ref = QuerySelector(cfg), QuerySelector(cfg)
    res.load_query_bank(bank)
    ref.load_query_bank({l: v.cpu() for l, v in bank.to_dict().items()})
    return res, ref


def seeded(fn, seed):
    np.random.seed(seed)
    out = fn()
    st = np.random.get_state()
    return out, (st[1].tolist(), st[2])


def same_select(res, ref, labels, maps, T=T, dtype=torch.float16, seed=5, device="cpu"):
    """`select` of both selectors after the same seed: equal outputs (shape, dtype, bits) and equal generator state afterwards"""
    (v, i), st = seeded(lambda: res.select(labels, maps, T, device, dtype), seed)
    (v0, i0), st0 = seeded(lambda: ref.select(labels, maps, T, device, dtype), seed)
    assert v.dtype == v0.dtype == dtype and v.shape == v0.shape and i.dtype == i0.dtype == torch.int32 and i.shape == i0.shape, \
        (v.shape, v0.shape, i.shape, i0.shape)
    assert torch.equal(v.cpu(), v0.cpu()) and torch.equal(i.cpu(), i0.cpu())
    assert st == st0
    return v, i


# one caption's labels in the caller's order; token 1 is shared by labels 1 and 2, label 2 lists token 5 twice, label 3 has no rows
LABELS = [6, 1, 2, 3, 4, 1000]
PMAP = {6: [9, 10, 11], 1: [0, 1], 2: [1, 5, 5], 3: [2], 4: [T - 1], 1000: [3]}
# the forward_grounding shape: another label list, another map and other lengths per item, one item without any query
RAGGED = ([[1, 2], [4, 6, 1, 2], [3, 1000], [], [6]],
          [{1: [0], 2: [0, 3]}, {4: [7], 6: [7, 8], 1: [8], 2: [1]}, {3: [1], 1000: [2]}, {}, {6: [5, 5, 6]}])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("C", [4, 6, 256])
def test_select_equals_the_dict_path(emu, C, S, dtype):
    bank = QueryBank.from_dict(make_dict(C, S), "cpu")
    res, ref = selectors(bank)
    for n_items in (1, 2):                                   # one caption for the whole batch: what `forward` / `forward_chunks` pass
        v, i = same_select(res, ref, [LABELS] * n_items, [PMAP] * n_items, dtype=dtype)
        assert v.shape == (n_items, (3 + 3 + 2 + 3) * S, C) and i.shape == (n_items, T, 5 * S)       # token 1: labels 1 (3 rows) and 2 (2 rows)
    same_select(res, ref, *RAGGED, dtype=dtype)


def test_the_row_above_the_fp16_range_is_selected_and_rounds_to_infinity(emu):
    bank = QueryBank.from_dict(make_dict(6, 1, {1: 2}), "cpu")
    res, ref = selectors(bank)
    v, _ = same_select(res, ref, [[1]], [{1: [0]}])
    assert v[0, 0, 0] == float("inf") and v[0, 1, 5] == float("-inf")
    v, _ = same_select(res, ref, [[1]], [{1: [0]}], dtype=torch.bfloat16)
    assert torch.isfinite(v).all()


def test_62_items_and_items_without_queries(emu):
    bank = QueryBank.from_dict(make_dict(6, 1), "cpu")
    res, ref = selectors(bank)
    rng = np.random.default_rng(1)
    labels, maps = [], []
    for it in range(62):                                     # 31 chunks x 2 images, chunk-major, every chunk with its own labels
        if it % 2 == 0:
            labs = [int(l) for l in rng.permutation([1, 2, 3, 4, 6, 1000])[:rng.integers(0, 7)]]
            pm = {l: sorted(int(t) for t in rng.integers(0, T, rng.integers(1, 4))) for l in labs}
        labels.append(labs)
        maps.append(pm)
    assert any(not l for l in labels)
    v, i = same_select(res, ref, labels, maps)
    assert v.shape[0] == i.shape[0] == 62


def test_long_captions_more_than_one_index_block_and_a_token_table_cut_in_the_middle_of_a_row(emu):
    """T = 300 (two blocks of 256 token positions per item) and 33 labels x 5 rows x 15 token positions = 2475 table entries per item: the
    kernel stages them in pieces of 2048, and 2048 is no multiple of 15"""
    counts = {l: 5 + l % 3 for l in range(33)}
    bank = QueryBank.from_dict(make_dict(8, 1, counts), "cpu")
    res, ref = selectors(bank, k=5)
    rng = np.random.default_rng(2)
    pm = {l: [int(t) for t in rng.integers(0, 300, 15 if l % 2 else 4)] for l in counts}
    pm[7] = [299] * 15                                       # one token 15 times: every row of label 7 fifteen times
    v, i = same_select(res, ref, [list(counts)] * 2, [pm] * 2, T=300)
    assert v.shape[1] == 33 * 5 and i.shape[2] >= 75


def test_reference_rng_stream_and_labels_within_k(emu):
    bank = QueryBank.from_dict(make_dict(4, 1, {1: 2, 2: 3}), "cpu")
    for rng_stream in (False, True):
        res, ref = selectors(bank, reference_rng=rng_stream)
        assert res.deterministic([1, 2, 9]) == ref.deterministic([1, 2, 9]) == (not rng_stream)
        before = seeded(lambda: None, 11)[1]
        (_, _), after = seeded(lambda: res.select([[1, 2, 9]], [{1: [0], 2: [1], 9: [2]}], T, "cpu", torch.float32), 11)
        assert (after != before) == rng_stream               # identity draws are consumed only with REFERENCE_RNG_STREAM
        same_select(res, ref, [[1, 2, 9]] * 2, [{1: [0], 2: [1], 9: [2]}] * 2)
    res, ref = selectors(QueryBank.from_dict(make_dict(6, 5), "cpu"), reference_rng=True)
    same_select(res, ref, [LABELS] * 2, [PMAP] * 2)
    same_select(res, ref, *RAGGED)


def test_deterministic_selection_is_memoised_and_a_zero_query_result_stays_empty(emu):
    bank = QueryBank.from_dict(make_dict(4, 1, {1: 2, 2: 3}), "cpu")
    res, ref = selectors(bank)
    pm = {1: [0, 2], 2: [2]}
    from mq_det_amd import ops
    calls = []
    real = ops.bank_select
    ops.bank_select = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        a = res.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16)
        b = res.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16)
        assert a is b and len(calls) == 1                    # the kernel ran once for the key
        v0, i0 = ref.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16)
        assert torch.equal(a[0], v0) and torch.equal(a[1], i0)
        v, i = res.select_cached("none", [5, 1000], {5: [0], 1000: [1]}, 2, T, "cpu", torch.float16)
        v0, i0 = ref.select_cached("none", [5, 1000], {5: [0], 1000: [1]}, 2, T, "cpu", torch.float16)
        assert v.shape == v0.shape == (2, 0, 4) and v.dtype == v0.dtype and torch.equal(i, i0) and len(calls) == 1
    finally:
        ops.bank_select = real


def test_a_token_position_beyond_the_caption_is_refused_like_the_dict_path(emu):
    bank = QueryBank.from_dict(make_dict(4, 1, {1: 2}), "cpu")
    res, ref = selectors(bank)
    for sel in (res, ref):
        with pytest.raises(IndexError):
            sel.select([[1]], [{1: [T]}], T, "cpu", torch.float16)
    same_select(res, ref, [[1]], [{1: [-1]}])                # (a negative position counts from the end on both paths)


def test_snapshot_rows_admitted_after_the_load_stay_invisible_until_the_next_load(emu):
    d = make_dict(8, 1, {1: 7, 2: 2})
    bank = QueryBank.from_dict(d, "cpu")
    res, ref = selectors(bank)
    labels, maps = [[1, 2, 40, 3]] * 2, [{1: [0], 2: [0, 1], 40: [2], 3: [3]}] * 2
    first = same_select(res, ref, labels, maps)
    pool0, slots0 = bank.pool, bank.slots
    g = torch.Generator().manual_seed(9)
    # 120 more rows: labels 1 and 2 grow, label 40 is new (beyond the 16-label table) and takes 60 rows (beyond the table's width)
    new_labels = torch.tensor([1] * 30 + [2] * 30 + [40] * 60)
    assert bank.update(torch.randn(120, 1, 8, generator=g), new_labels, 100) == 120
    assert bank.pool is not pool0 and len(bank.pool) > len(pool0)
    assert bank.slots is not slots0 and bank.slots.shape[0] > slots0.shape[0] and bank.slots.shape[1] > slots0.shape[1]
    again = same_select(res, ref, labels, maps)              # `ref` still holds the dict taken before the update
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert not res.has_vision_query(40) and res.has_vision_query(1) and res.deterministic([2]) and res._width() == 8
    assert bank.merge({3: torch.randn(4, 1, 8, generator=g)}, 100) == 4
    again = same_select(res, ref, labels, maps)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1]) and not res.has_vision_query(3)
    # the next load sees everything
    res.load_query_bank(bank)
    ref.load_query_bank({l: v.cpu() for l, v in bank.to_dict().items()})
    assert res.has_vision_query(40) and res.has_vision_query(3) and not res.deterministic([2])
    v, _ = same_select(res, ref, labels, maps)
    assert v.shape[1] == 4 * K and not torch.equal(v[:, :first[0].shape[1]], first[0])


def test_dict_like_queries_and_the_vision_only_masking_set_follow_the_snapshot(emu):
    from mq_det_amd.modeling.detector import GeneralizedVLRCNN_New
    from mq_det_amd.modeling.graph_runner import Memo
    bank = QueryBank.from_dict(make_dict(8, 1, {1: 7, 3: 2}), "cpu")
    res, ref = selectors(bank)
    for lab in (0, 1, 2, 3, 15, 16, 1000, -1, "cat"):
        assert res.has_vision_query(lab) == ref.has_vision_query(lab) == (lab in (1, 3)), lab
    for labs in ([1], [3], [2, 1000], [], [3, 1]):
        assert res.deterministic(labs) == ref.deterministic(labs), labs
    assert res._width() == ref._width() == 8
    empty = QuerySelector(res.cfg)
    empty.load_query_bank(QueryBank("cpu"))
    assert empty._width() == 1 and not empty.has_vision_query(1) and empty.deterministic([1])
    v, i = empty.select([[1], []], [{1: [0]}, {}], T, "cpu", torch.float16)
    assert v.shape == (2, 0, 1) and i.shape == (2, T, 1) and bool((i == -1).all())

    # the detector's masking set (detector._masked_ids) on a stand-in that carries what the method reads
    cfg = get_cfg()
    cfg.VISION_QUERY.MASK_DURING_INFERENCE, cfg.VISION_QUERY.TEXT_DROPOUT = True, 1.0
    pmap = {1: [1, 2], 2: [4], 3: [6, 7, 8]}
    pm, labels, pm_key, *_ = prepare_positive_map(pmap, 16)
    ids = torch.arange(1000, 1032).view(2, 16)

    def masked(sel):
        host = types.SimpleNamespace(cfg=cfg, query_selector=sel, tokenizer=types.SimpleNamespace(mask_token_id=103),
                                     _mask_cache=Memo(8, memoise=True), _use_vq=lambda: True)
        out, _, mkey = GeneralizedVLRCNN_New._masked_ids(host, ids, ("a", "a"), pm_key, labels, pm, torch.device("cpu"))
        return out, mkey
    (a, ka), (b, kb) = masked(res), masked(ref)
    assert torch.equal(a, b) and ka == kb and ka[1] == (1, 3)
    assert (a == 103).nonzero()[:, 1].tolist() == [1, 2, 6, 7, 8] * 2
    bank.update(torch.ones(1, 1, 8), torch.tensor([2]), 10)  # label 2 gains a row: masked only after the next load
    assert masked(res)[1] == ka
    res.load_query_bank(bank)
    assert masked(res)[1][1] == (1, 2, 3)


@pytest.mark.parametrize("S", [1, 5])
def test_forward_equals_the_dict_paths_triple(emu, S):
    bank = QueryBank.from_dict(make_dict(6, S), "cpu")
    res, ref = selectors(bank)
    labels = [[6, 1, 2, 3, 4], [2, 1000, 4]]
    g = torch.Generator().manual_seed(3)
    maps = [torch.rand(len(l), T, generator=g) * (torch.rand(len(l), T, generator=g) > 0.7) for l in labels]
    (q, m, has), st = seeded(lambda: res(labels, maps), 8)
    (q0, m0, has0), st0 = seeded(lambda: ref(labels, maps), 8)
    assert torch.equal(q, q0) and torch.equal(m, m0) and has == has0 == [[1, 1, 1, 0, 1], [1, 0, 1]] and st == st0
    assert q.shape == (2, (3 + 3 + 2 + 3) * S, 6)


@pytest.mark.parametrize("schedule", [("ascending", 0), ("random", 3)])
def test_under_the_guard_and_both_fibre_schedules(emu, schedule):
    import simt
    from simt import guard
    simt.set_schedule(*schedule)
    try:
        for mode in ("end", "start"):
            with guard.pointer_guard(mode), guard.guarded_ops(mode):
                for C, S, dtype in ((4, 1, torch.float16), (6, 5, torch.bfloat16), (256, 1, torch.float16), (256, 5, torch.float32),
                                    (6, 1, torch.float32), (4, 5, torch.bfloat16)):
                    bank = QueryBank.from_dict(make_dict(C, S), "cpu")
                    res, ref = selectors(bank)
                    same_select(res, ref, [LABELS] * 2, [PMAP] * 2, dtype=dtype)
                    same_select(res, ref, *RAGGED, dtype=dtype)
    finally:
        simt.set_schedule("ascending")


# ---------------------------------------------------------------------------------------------- online_update(resident=True)
class SelectingStandIn(qr.StandInModel):
    """The stand-in model of tests/test_query_bank_cpu.py with a real QuerySelector behind `load_query_bank`: a path, a dict or a QueryBank.
    `state` (what its seeded detections depend on) = the rows of the bank loaded last, as in the parent class."""

    def __init__(self, cfg, boxlist_cls, extract):
        super().__init__(cfg, boxlist_cls, extract)
        self.query_selector = QuerySelector(cfg)

    def load_query_bank(self, bank):
        sel = self.query_selector
        sel.load_query_bank(bank)
        if isinstance(bank, QueryBank):
            self.state = sum(sel._resident())
        else:
            self.state = sum(len(v) for v in sel.query_bank.values() if torch.is_tensor(v))
        self.loads.append(("bank" if isinstance(bank, QueryBank) else bank, self.state))


def run_online(js, batch, path, resident):
    cfg = tc.online_cfg(js)
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS = 2
    base = tc.standin(cfg)
    model = SelectingStandIn(cfg, BoxList, base._extract)
    o = js["online"]
    maps = [{int(k): v for k, v in m.items()} for m in o["maps"]]
    out = online_update(model, qr.loader(o["image_ids"], batch), device="cpu", cfg=cfg, num_turns=2, save_name=path,
                        queries_and_maps=(o["queries"], maps), resident=resident)
    assert out is model
    return model


@pytest.mark.parametrize("batch", [1, 2])
def test_online_update_resident_writes_the_same_files_and_selects_the_same_rows(emu, tmp_path, batch):
    js, a = tc.load_fixture()
    o = js["online"]
    want = {int(l): torch.from_numpy(a[f"online_turn1_label{l}"]) for l in o["turns"][1]}
    js = json.loads(json.dumps(js))
    if batch == 2:                                           # SUBSET counts batches (tests/test_query_bank_cpu.py)
        js["online"]["image_ids"] = o["image_ids"][:o["subset"]]
    pa, pb = str(tmp_path / "file" / "bank.pth"), str(tmp_path / "resident" / "bank.pth")
    A, B = run_online(js, batch, pa, False), run_online(js, batch, pb, True)
    tc.same_bank(torch.load(pa, map_location="cpu"), want)
    tc.same_bank(torch.load(pb, map_location="cpu"), want)
    # turn 1 saw the bank of turn 0 on both paths; the resident run is handed the final bank as well
    assert A.loads == [(pa, o["loaded_rows"])]
    assert B.loads[0] == ("bank", o["loaded_rows"]) and B.loads[1] == ("bank", sum(len(v) for v in want.values())) and len(B.loads) == 2
    assert isinstance(B.query_selector.query_bank, QueryBank) and isinstance(A.query_selector.query_bank, dict)
    # what a caller does with the file after `online_update(resident=False)`: load it.  Both models then select the same rows.
    A.load_query_bank(pa)
    labels = sorted(want) + [99]
    pm = {l: [j, j + 1] for j, l in enumerate(labels)}
    assert not B.query_selector.deterministic(labels)
    same_select(B.query_selector, A.query_selector, [labels] * 2, [pm] * 2, T=16, dtype=torch.float16)
    same_select(B.query_selector, A.query_selector, [labels] * 2, [pm] * 2, T=16, dtype=torch.float32, seed=6)


def test_the_keyword_defaults_to_off(emu):
    import inspect
    p = inspect.signature(online_update).parameters["resident"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
