"""The device-resident vision-query bank (mq_det_amd.query_bank, csrc/query_bank.hip) without a GPU: the kernel SOURCE through the host emulation
(tests/simt) against tests/golden/query_bank, which tools/gen_golden_query_bank.py records by running the reference's own extract_query and
online_update in place; against the dict path of `pool_into_bank`; the exact cases of the strict comparison, NaN and all-zero rows; the file
round trips, merge, the refusals, growth, both fibre schedules under the buffer-overrun guard, and the two driver loops on a stand-in model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import query_bank_ref as qr  # noqa: E402
from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.modeling.detector import expand_bbox, pool_into_bank  # noqa: E402
from mq_det_amd.query_bank import QueryBank, extract_query_bank, online_update  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

GOLD = os.path.join(HERE, "golden", "query_bank")
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


def load_fixture():
    with open(GOLD + ".json") as f:
        return json.load(f), dict(np.load(GOLD + ".npz"))


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def same_bank(got, want):
    """two {label: Tensor} banks: same labels, counts, row order and row BITS"""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for l in want:
        g, w = got[l].cpu(), want[l].cpu()
        assert g.dtype == w.dtype == torch.float32 and g.shape == w.shape, (l, g.shape, w.shape)
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), l


def dict_path(feats, labels, bank, exclude, maxq, thr):
    """today's `pool_into_bank` loop on prepared rows: a pooler that hands the rows over, SELECT_FPN_LEVEL by the number of scales"""
    cfg = get_cfg()
    S = feats.shape[1]
    cfg.VISION_QUERY.SELECT_FPN_LEVEL = S == 1
    cfg.VISION_QUERY.SIMILARITY_THRESHOLD = thr
    t = BoxList(torch.zeros(len(labels), 4, device=feats.device), (10, 10))
    t.add_field("labels", labels)
    pooler = lambda vf, targets, reduce_mean: feats[:, 0] if S == 1 else feats.permute(1, 0, 2)      # noqa: E731
    return pool_into_bank(cfg, pooler, [None] * 5, [t], bank, exclude, maxq)


def check_fixture_case(name, device="cpu"):
    """every call of a fixture case on a QueryBank (through pool_into_bank's dispatch) and on a dict: both equal the reference's bank"""
    js, a = load_fixture()
    case = js["cases"][name]
    cands, labels = torch.from_numpy(a[name + "_cands"]).to(device), torch.from_numpy(a[name + "_labels"]).to(device)
    # the condition the fixture was recorded under, asserted again on the data as it is here
    want, dmin, above, below = qr.replay(cands.cpu(), labels.cpu(), case["calls"], case["thr"])
    assert dmin >= qr.MARGIN and (above, below) == (case["above"], case["below"])
    assert [{str(l): v for l, v in w.items()} for w in want] == case["banks"]
    bank, plain = QueryBank(device), {}
    for call, ref in zip(case["calls"], case["banks"]):
        f, l = cands[call["lo"]:call["hi"]], labels[call["lo"]:call["hi"]]
        out = dict_path(f, l, bank, call["exclude"], call["maxq"], case["thr"])
        assert out is bank
        plain = dict_path(f, l, plain, call["exclude"], call["maxq"], case["thr"])
        expect = {int(k): cands[ids] for k, ids in ref.items()}
        same_bank(bank.to_dict(), expect)
        same_bank(plain, expect)
        assert len(bank) == len(expect) and all(k in bank for k in expect) and 1000 not in bank
    return bank


@pytest.mark.parametrize("name", ["sel_exclude", "sel_plain", "all_plain", "sel_mixed"])
def test_fixture_calls_equal_the_reference_and_the_dict_path(emu, name):
    check_fixture_case(name)


@pytest.mark.parametrize("schedule", [("ascending", 0), ("random", 3), ("random", 11)])
def test_fixture_under_the_guard_and_both_fibre_schedules(emu, schedule):
    import simt
    from simt import guard
    simt.set_schedule(*schedule)
    try:
        for mode in ("end", "start"):
            with guard.pointer_guard(mode):
                for name in ("sel_exclude", "all_plain", "sel_mixed"):
                    check_fixture_case(name)
    finally:
        simt.set_schedule("ascending")


def exact_cases(device):
    """thr = 1.0 and similarities of exactly 1.0: `>` is strict, the duplicate is admitted (as in the reference); a NaN row compares false
    against everything and is admitted, and everything is admitted against it; an all-zero row (the eps path) has similarity 0."""
    for C in (256, 64, 6):
        e1 = torch.zeros(1, 1, C, device=device)
        e1[0, 0, 0] = 1.0
        half = torch.zeros(1, 1, C, device=device)
        half[0, 0, :4] = 0.5
        for row in (e1, half):
            bank, plain = QueryBank(device), {}
            feats, labels = torch.cat([row, row, 2 * row]), torch.tensor([5, 5, 5], device=device)
            assert bank.update(feats, labels, 10, True, 1.0) == 3
            plain = dict_path(feats, labels, plain, True, 10, 1.0)
            assert len(plain[5]) == 3
            same_bank(bank.to_dict(), plain)
            # just below 1.0 the duplicates are dropped
            bank2 = QueryBank(device)
            assert bank2.update(feats, labels, 10, True, 0.999) == 1
            same_bank(bank2.to_dict(), dict_path(feats, labels, {}, True, 10, 0.999))
        g = torch.Generator().manual_seed(C)
        x = torch.randn(1, 1, C, generator=g).to(device)
        nan = x.clone()
        nan[0, 0, 1] = float("nan")
        zero = torch.zeros(1, 1, C, device=device)
        feats = torch.cat([x, nan, x, zero, zero, nan, 3 * x])
        labels = torch.full((7,), 2, device=device)
        bank = QueryBank(device)
        n = bank.update(feats, labels, 10, True, 0.85)
        plain = dict_path(feats, labels, {}, True, 10, 0.85)
        # x, nan (NaN > thr is false), [x dropped: equal to row 0 ... but the NaN row compares false, row 0 hits], zero, zero (0 > thr false), nan, [3x dropped]
        assert n == len(plain[2]) == 5
        got, want = bank.to_dict()[2].cpu(), plain[2].cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_strict_comparison_nan_and_zero_rows(emu):
    exact_cases("cpu")


def test_round_trips_and_file_read_by_the_query_selector(emu, tmp_path):
    from mq_det_amd.modeling.query_selector import QuerySelector
    bank = check_fixture_case("sel_exclude")
    d = bank.to_dict()
    assert all(isinstance(k, int) for k in d) and all(v.shape[1:] == (1, 256) for v in d.values())
    same_bank(QueryBank.from_dict(d, "cpu").to_dict(), d)
    from collections import defaultdict
    dd = defaultdict(list, d)
    dd[99]                                                   # an empty entry, as the reference's defaultdict grows them
    same_bank(QueryBank.from_dict(dd, "cpu").to_dict(), d)
    path = str(tmp_path / "sub" / "bank.pth")
    bank.save(path)
    same_bank(QueryBank.load(path, "cpu").to_dict(), d)
    same_bank(torch.load(path, map_location="cpu"), d)       # the reference's loader: torch.load of a label -> tensor dict
    cfg = get_cfg()
    sel = QuerySelector(cfg)
    sel.load_query_bank(path)
    same_bank({k: v for k, v in sel.query_bank.items()}, d)
    rows = sel._rows(3, "cpu", torch.float32)
    assert torch.equal(rows, d[3][:cfg.VISION_QUERY.NUM_QUERY_PER_CLASS].flatten(0, 1))
    same_bank({3: bank[3]}, {3: d[3]})
    with pytest.raises(KeyError):
        bank[1000]


def test_merge_truncates_in_label_then_slot_order(emu):
    g = torch.Generator().manual_seed(1)
    a = {1: torch.randn(3, 1, 64, generator=g), 4: torch.randn(2, 1, 64, generator=g)}
    b = {4: torch.randn(4, 1, 64, generator=g), 0: torch.randn(6, 1, 64, generator=g), 1: torch.randn(1, 1, 64, generator=g)}
    bank = QueryBank.from_dict(a, "cpu")
    n = bank.merge(QueryBank.from_dict(b, "cpu"), 5)
    want = {0: b[0][:5], 1: torch.cat([a[1], b[1]]), 4: torch.cat([a[4], b[4][:3]])}
    assert n == 5 + 1 + 3
    same_bank(bank.to_dict(), want)
    assert bank.merge(b, 5) == 1                             # (a dict is accepted too) labels 0 and 4 are full, label 1 has room for one more row
    same_bank(bank.to_dict(), {0: b[0][:5], 1: torch.cat([a[1], b[1], b[1]])[:5], 4: want[4]})


def test_refusals(emu):
    bank = QueryBank("cpu")
    with pytest.raises(ValueError, match="one scale"):
        bank.update(torch.zeros(2, 5, 8), torch.tensor([1, 1]), 4, True)
    with pytest.raises(ValueError, match="negative label"):
        bank.update(torch.zeros(2, 1, 8), torch.tensor([1, -3]), 4)
    with pytest.raises(TypeError):
        bank.update(torch.zeros(2, 1, 8, dtype=torch.float16), torch.tensor([1, 1]), 4)
    with pytest.raises(TypeError):
        bank.update(torch.zeros(2, 1, 8), torch.tensor([1.0, 1.0]), 4)
    assert len(bank) == 0 and bank.to_dict() == {} and bank.update(torch.zeros(0, 1, 8), torch.zeros(0, dtype=torch.int64), 4) == 0
    bank.update(torch.ones(1, 1, 8), torch.tensor([0]), 4)
    with pytest.raises(ValueError, match="rows of shape"):
        bank.update(torch.ones(1, 1, 16), torch.tensor([0]), 4)


def test_pool_and_label_table_grow_across_many_small_updates(emu):
    rng = np.random.default_rng(2)
    bank, plain = QueryBank("cpu"), {}
    grew = set()
    for step in range(60):
        n = int(rng.integers(1, 6))
        feats = torch.from_numpy(rng.standard_normal((n, 1, 32)).astype(np.float32))
        labels = torch.from_numpy(rng.integers(0, 4 + 2 * step, n))
        maxq = 3 + step // 10                                  # the capacity grows too
        before = (len(bank.pool), tuple(bank.slots.shape)) if bank.pool is not None else None
        got = bank.update(feats, labels, maxq, True, 0.85)
        size0 = sum(len(v) for v in plain.values())
        plain = dict_path(feats, labels, plain, True, maxq, 0.85)
        assert got == sum(len(v) for v in plain.values()) - size0
        after = (len(bank.pool), tuple(bank.slots.shape))
        if before and before != after:
            grew.update(i for i in range(3) if (before[0], *before[1])[i] != (after[0], *after[1])[i])
    assert grew == {0, 1, 2}, grew                             # pool rows, labels and capacity all grew on the way
    same_bank(bank.to_dict(), plain)
    assert bank.rows == sum(len(v) for v in plain.values())


# ---------------------------------------------------------------------------------------------- the driver loops on a stand-in model
def standin(cfg):
    def extract(self, images=None, targets=None, query_images=None, visual_features=None, exclude_similar=False, device=None, max_query_number=None):
        targets = expand_bbox([t.to(device or "cpu") for t in targets if t is not None], expand_ratio=cfg.VISION_QUERY.EXPAND_RATIO)
        return pool_into_bank(cfg, self.pooler, visual_features, targets, query_images, exclude_similar, max_query_number)
    return qr.StandInModel(cfg, BoxList, extract)


def online_cfg(js):
    cfg = get_cfg()
    for k, v in js["online"]["cfg"].items():
        cfg.VISION_QUERY[k] = v
    cfg.TEST.SUBSET = js["online"]["subset"]
    return cfg


def run_online(js, batch, path, device="cpu", turns=2):
    cfg = online_cfg(js)
    model = standin(cfg)
    o = js["online"]
    maps = [{int(k): v for k, v in m.items()} for m in o["maps"]]
    out = online_update(model, qr.loader(o["image_ids"], batch), device=device, cfg=cfg, num_turns=turns, save_name=path,
                        queries_and_maps=(o["queries"], maps))
    assert out is model
    return model


def test_online_update_equals_the_reference_run_at_batch_1_and_2(emu, tmp_path):
    js, a = load_fixture()
    o = js["online"]
    want = [{int(l): torch.from_numpy(a[f"online_turn{t}_label{l}"]) for l in turn} for t, turn in enumerate(o["turns"])]
    for batch in (1, 2):
        path = str(tmp_path / f"b{batch}" / "bank.pth")
        # SUBSET counts batches: at batch 2 the loader gets the images the batch-1 run saw before its cut
        js_b = json.loads(json.dumps(js))
        if batch == 2:
            js_b["online"]["image_ids"] = o["image_ids"][:o["subset"]]
        first = run_online(js_b, batch, path, turns=1)
        same_bank(torch.load(path, map_location="cpu"), want[0])
        model = run_online(js_b, batch, path, turns=2)
        same_bank(torch.load(path, map_location="cpu"), want[1])
        assert model.loads == [(path, o["loaded_rows"])] and first.loads == []          # turn 1 reloaded the file turn 0 saved
        _, _, dmin, above, below = qr.log_replay(model.log, o["cfg"]["MAX_TEST_QUERY_NUMBER"], o["thr"])
        assert dmin >= qr.MARGIN and above > 0 and below > 0


def test_online_update_starts_from_the_bank_file_and_refuses_what_the_reference_refuses(emu, tmp_path):
    js, a = load_fixture()
    start = str(tmp_path / "start.pth")
    seed_rows = {2: torch.from_numpy(a["online_turn0_label2"][:2])}
    QueryBank.from_dict(seed_rows, "cpu").save(start)
    js["online"]["cfg"]["QUERY_BANK_PATH"] = start
    path = str(tmp_path / "out.pth")
    run_online(js, 1, path, turns=1)
    got = torch.load(path, map_location="cpu")
    assert torch.equal(got[2][:2], seed_rows[2]) and len(got[2]) <= js["online"]["cfg"]["MAX_TEST_QUERY_NUMBER"]
    cfg = online_cfg(js)
    cfg.TEST.USE_MULTISCALE = True
    with pytest.raises(NotImplementedError):
        online_update(standin(cfg), [], device="cpu", cfg=cfg, save_name=path, queries_and_maps=([], []))
    cfg.TEST.USE_MULTISCALE, cfg.TEST.EVAL_TASK = False, "grounding"
    with pytest.raises(NotImplementedError):
        online_update(standin(cfg), [], device="cpu", cfg=cfg, save_name=path, queries_and_maps=([], []))


def test_extract_query_bank_loop_and_default_file_name(emu, tmp_path, monkeypatch):
    js, a = load_fixture()
    case = js["cases"]["sel_plain"]
    cands, labels = torch.from_numpy(a["sel_plain_cands"]), torch.from_numpy(a["sel_plain_labels"])
    cfg = get_cfg()
    cfg.VISION_QUERY.MAX_QUERY_NUMBER = case["calls"][0]["maxq"]
    cfg.VISION_QUERY.DATASET_NAME, cfg.VISION_QUERY.QUERY_ADDITION_NAME = "tiny", "_x"

    class Model:
        def __init__(self):
            self.cfg = cfg

        def eval(self):
            return self

        def extract_query(self, images, targets, query_images, max_query_number=None):
            lo, hi = targets
            return dict_path(cands[lo:hi], labels[lo:hi], query_images, False, max_query_number or cfg.VISION_QUERY.MAX_QUERY_NUMBER, 0.85)
    batches = [(qr.Images([n]), (c["lo"], c["hi"]), None) for n, c in enumerate(case["calls"])]
    monkeypatch.chdir(tmp_path)
    bank = extract_query_bank(Model(), batches)
    want = {int(k): cands[ids] for k, ids in case["banks"][-1].items()}
    same_bank(bank.to_dict(), want)
    name = os.path.join("MODEL", "tiny_query_{}_pool7_sel_x.pth".format(cfg.VISION_QUERY.MAX_QUERY_NUMBER))
    same_bank(torch.load(name, map_location="cpu"), want)
    cfg.VISION_QUERY.QUERY_BANK_SAVE_PATH = str(tmp_path / "named.pth")
    extract_query_bank(Model(), batches, max_query_number=2)
    assert all(len(v) == 2 for v in torch.load(cfg.VISION_QUERY.QUERY_BANK_SAVE_PATH, map_location="cpu").values())
    cfg.VISION_QUERY.QUERY_BANK_SAVE_PATH, cfg.VISION_QUERY.DATASET_NAME = "", ""
    with pytest.raises(ValueError, match="DATASET_NAME"):
        extract_query_bank(Model(), batches)
