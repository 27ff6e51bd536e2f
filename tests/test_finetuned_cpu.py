"""Fine-tuned checkpoints without a GPU (DESIGN.md "Fine-tuned checkpoints"): the three switches a few-shot run of the reference sets --
MODEL.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER, VISION_QUERY.LEARNABLE_BANK, VISION_QUERY.ADD_VISION_LAYER --, the state they add to the state
dict, `load_reference_checkpoint`, and the selector against what the reference's own `QuerySelector` returned
(tests/golden/finetuned_selector.*, tools/gen_golden_finetuned.py).  The resident path runs the kernel SOURCE (csrc/query_bank.hip
mq_bank_select_add_fwd) through the host emulation (tests/simt), under the buffer-overrun guard and both fibre schedules."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_query_select_cpu as ts  # noqa: E402
from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.modeling.query_selector import QuerySelector  # noqa: E402
from mq_det_amd.query_bank import QueryBank  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_emu = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
T, K = ts.T, ts.K


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "finetuned_selector.json")) as f:
        js = json.load(f)
    return js, np.load(os.path.join(HERE, "golden", "finetuned_selector.npz"))


# ---------------------------------------------------------------------------------------------- a small MQ-GLIP (parameters only, nothing runs)
def small_cfg(linear=False, learnable=False, vision=False, bank_path=""):
    cfg = get_cfg()
    M = cfg.MODEL
    M.SWINT.EMBED_DIM, M.SWINT.NUM_HEADS, M.SWINT.DEPTHS = 8, (1, 1, 1, 1), (1, 1, 1, 1)
    M.SWINT.OUT_CHANNELS = (8, 16, 32, 64)
    M.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS, M.LANGUAGE_BACKBONE.QV_START = 2, 1
    M.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE, M.LANGUAGE_BACKBONE.LANG_DIM = 32, 64
    M.DYHEAD.NUM_CONVS = 1
    M.DYHEAD.FUSE_CONFIG.ADD_LINEAR_LAYER = linear
    cfg.VISION_QUERY.LEARNABLE_BANK, cfg.VISION_QUERY.ADD_VISION_LAYER = learnable, vision
    cfg.VISION_QUERY.QUERY_BANK_PATH = bank_path
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS = K
    return cfg


def small_model(**kw):
    from mq_det_amd.modeling.detector import GeneralizedVLRCNN_New
    return GeneralizedVLRCNN_New(small_cfg(**kw), tokenizer=object())


def bank_file(tmp_path, S=1, C=8, name="bank.pth"):
    d = ts.make_dict(C, S)
    path = str(tmp_path / name)
    torch.save(d, path)
    return d, path


def test_state_dict_names_follow_the_switches(tmp_path):
    from mq_det_amd.modeling.params import param_specs
    d, path = bank_file(tmp_path, S=5)
    base = small_model()
    keys0 = set(base.state_dict())
    assert keys0 == {n for n, _, _ in param_specs(base.cfg)}                      # all off: today's key set, nothing from the selector
    assert not any("tunable" in k or k.startswith("query_selector.") for k in keys0)
    assert set(small_model(bank_path=path).state_dict()) == keys0                   # a plain bank is no state

    sd = small_model(linear=True).state_dict()
    assert set(sd) - keys0 == {"rpn.tunable_linear.weight"} and keys0 <= set(sd)
    w = sd["rpn.tunable_linear.weight"]
    assert w.shape == (1000, 64) and w.dtype == torch.float32 and not w.any()

    sd = small_model(learnable=True, bank_path=path).state_dict()
    assert set(sd) - keys0 == {f"query_selector.query_bank.{lab}" for lab in d} and keys0 <= set(sd)
    for lab, v in d.items():
        p = sd[f"query_selector.query_bank.{lab}"]
        assert p.shape == (len(v), 5, 8) and torch.equal(p, v) and not p.requires_grad

    sd = small_model(vision=True, bank_path=path).state_dict()
    assert set(sd) - keys0 == {"query_selector.tunable_vision_linear.weight"} and keys0 <= set(sd)
    w = sd["query_selector.tunable_vision_linear.weight"]
    assert w.shape == (1000, 8) and w.dtype == torch.float32 and not w.any()

    # without a bank file the selector's parameters do not exist yet (a checkpoint or the first load_query_bank brings them)
    m = small_model(linear=True, learnable=True, vision=True)
    assert set(m.state_dict()) - keys0 == {"rpn.tunable_linear.weight"}
    m.load_query_bank(d)
    assert set(m.state_dict()) - keys0 == {"rpn.tunable_linear.weight", "query_selector.tunable_vision_linear.weight"}
    assert m.query_selector.tunable_vision_linear.weight.shape == (1000, 8)


def test_max_query_len_beyond_the_prompt_offset_is_refused_by_name():
    m = small_model(linear=True)
    m._validate_config()
    m.cfg.MODEL.LANGUAGE_BACKBONE.MAX_QUERY_LEN = 1008
    with pytest.raises(NotImplementedError, match="ADD_LINEAR_LAYER"):
        m._validate_config()


@pytest.mark.parametrize("kinds", [("linear", "learnable", "vision"), ("linear",), ("learnable",), ("vision",)])
def test_load_reference_checkpoint_round_trip(tmp_path, kinds):
    from mq_det_amd.utils.checkpoint import load_reference_checkpoint
    on = {k: True for k in kinds}
    d, path = bank_file(tmp_path)
    src = small_model(bank_path=path, **on)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in src.parameters():                                                  # every parameter seeded and non-zero, the tuned ones too
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    sd = src.state_dict()
    tuned = [k for k in sd if "tunable" in k or k.startswith("query_selector.")]
    assert len(tuned) == ("linear" in kinds) + ("vision" in kinds) + len(d) * ("learnable" in kinds)
    file = str(tmp_path / "model_final.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}, "iteration": 3}, file)     # DetectronCheckpointer.save under DDP

    fresh = small_model(**on)                                                       # built from the config alone: no bank file
    res = load_reference_checkpoint(fresh, file, strict=True)
    assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
    got = fresh.state_dict()
    assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    sel = fresh.query_selector
    if "learnable" in kinds:
        assert isinstance(sel.query_bank, nn.ParameterDict) and fresh._use_vq()
        assert sorted(sel._source()) == sorted(d) and all(torch.equal(sel._source()[l], sd[f"query_selector.query_bank.{l}"]) for l in d)
        assert all(sel.has_vision_query(l) for l in d) and not sel.has_vision_query(3)
    else:
        assert sel.query_bank is None
    # a bare state dict, and one already stripped, load the same way
    again = small_model(**on)
    res = load_reference_checkpoint(again, {k: v for k, v in sd.items()}, strict=True)
    assert list(res.missing_keys) == [] and list(res.unexpected_keys) == []
    assert all(torch.equal(again.state_dict()[k], sd[k]) for k in tuned)

    off = small_model()
    with pytest.raises(RuntimeError, match="Unexpected key"):
        load_reference_checkpoint(off, file, strict=True)
    res = load_reference_checkpoint(small_model(), file, strict=False)
    assert sorted(res.unexpected_keys) == sorted(tuned) and list(res.missing_keys) == []


def test_the_checkpoint_file_goes_through_the_weights_only_unpickler(tmp_path):
    from mq_det_amd.utils.checkpoint import load_reference_checkpoint
    import pickle
    file = str(tmp_path / "evil.pth")
    torch.save({"model": {"a": torch.zeros(1)}, "hook": os.getcwd}, file)          # a global the weights-only unpickler does not know
    with pytest.raises(pickle.UnpicklingError):
        load_reference_checkpoint(nn.Linear(1, 1), file)


# ---------------------------------------------------------------------------------------------- the selector against the reference's
def golden_bank(a, js, S, with_empty=False):
    d = {int(l): torch.from_numpy(a[f"bank_S{S}_label{l}"]) for l in js["counts"]}
    if with_empty:
        d.update({int(l): torch.zeros(0, S, js["C"]) for l in js["no_query"]})
    return d


def golden_selector(tmp_path, a, js, S, learnable, add, resident):
    """A selector configured like the reference's of the fixture; resident: selecting from a QueryBank (built from the state dict when the
    bank is learnable)."""
    cfg = get_cfg()
    VQ = cfg.VISION_QUERY
    VQ.NUM_QUERY_PER_CLASS, VQ.LEARNABLE_BANK, VQ.ADD_VISION_LAYER = js["K"], learnable, add
    path = str(tmp_path / f"bank_S{S}_{int(learnable)}.pth")
    torch.save(golden_bank(a, js, S, with_empty=learnable), path)
    VQ.QUERY_BANK_PATH = path
    sel = QuerySelector(cfg)
    if add:
        sel.load_state_dict({**sel.state_dict(), "tunable_vision_linear.weight": torch.from_numpy(a[f"wv_S{S}"])}, strict=True)
    if resident:
        if learnable:
            sel.load_query_bank(QueryBank.from_state_dict(sel.state_dict(), "cpu", prefix="query_bank."))
            assert isinstance(sel.query_bank, nn.ParameterDict)                     # the parameters stay
        else:
            sel.load_query_bank(QueryBank.from_dict(sel.query_bank, "cpu"))
    return sel


def case_inputs(js, case):
    inp = js["inputs"][case["input"]]
    return inp["labels"], [{int(k): v for k, v in m.items()} for m in inp["maps"]]


def rng_state():
    st = np.random.get_state()
    return st[1].tolist(), int(st[2])


def check_case(sel, js, a, case, dtypes=DTYPES):
    labels, maps = case_inputs(js, case)
    tag = case["tag"]
    want32 = torch.from_numpy(a[tag + "_queries"])
    mask = torch.from_numpy(a[tag + "_masks"])
    want_rng = (a[tag + "_rng_key"].tolist(), case["rng_pos"])
    out = {}
    for dtype in dtypes:
        np.random.seed(case["seed"])
        v, idx = sel.select(labels, maps, js["T"], "cpu", dtype)
        assert rng_state() == want_rng, tag                                         # the reference's draws, in its order
        want = want32.to(dtype)                                                     # ONE rounding of the reference's fp32 rows
        assert v.dtype == dtype and v.shape == want.shape, (tag, v.shape, want.shape)
        assert torch.equal(v, want), (tag, dtype, (v.float() - want.float()).abs().max())
        # padding rows are exact zeros (bit pattern: no -0.0, no offset): the rows no token of the reference's mask attends from
        real = mask.bool().any(-1)
        pad = v[~real]
        assert pad.numel() == 0 or not pad.view(torch.int16 if dtype != torch.float32 else torch.int32).any(), tag
        # the gather index names, per token, exactly the rows whose mask column the reference set
        for i in range(len(labels)):
            for t in range(js["T"]):
                got = sorted(set(idx[i, t][idx[i, t] >= 0].tolist()))
                assert got == mask[i, :, t].nonzero().flatten().tolist(), (tag, i, t)
        out[dtype] = (v, idx)
    return out


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("learnable", [False, True])
@pytest.mark.parametrize("add", [False, True])
def test_dict_path_equals_the_reference(tmp_path, golden, S, learnable, add):
    js, a = golden
    sel = golden_selector(tmp_path, a, js, S, learnable, add, resident=False)
    cases = [c for c in js["cases"] if (c["S"], c["learnable"], c["add"]) == (S, learnable, add)]
    assert len(cases) == 3
    for case in cases:
        check_case(sel, js, a, case)
        # the reference-shaped triple of forward()
        labels, maps = case_inputs(js, case)
        loc = []
        for l, pm in zip(labels, maps):
            m = torch.zeros(len(l), js["T"])
            for j, lab in enumerate(l):
                m[j, list(pm[lab])] = 1
            loc.append(m / (m.sum(-1)[:, None] + 1e-6))
        np.random.seed(case["seed"])
        q, m, has = sel(labels, loc)
        assert torch.equal(q, torch.from_numpy(a[case["tag"] + "_queries"])) and has == case["has_vision_query"]
        assert torch.equal(m, torch.from_numpy(a[case["tag"] + "_masks"]).float())
        assert rng_state() == (a[case["tag"] + "_rng_key"].tolist(), case["rng_pos"])


@needs_emu
@pytest.mark.parametrize("schedule", [("ascending", 0), ("random", 3)])
def test_resident_path_equals_the_reference_under_the_guard(emu, tmp_path, golden, schedule):
    import simt
    from simt import guard
    js, a = golden
    simt.set_schedule(*schedule)
    try:
        for mode in ("end", "start"):
            with guard.pointer_guard(mode), guard.guarded_ops(mode):
                for S in (1, 5):
                    for learnable in (False, True):
                        for add in (False, True):
                            res = golden_selector(tmp_path, a, js, S, learnable, add, resident=True)
                            ref = golden_selector(tmp_path, a, js, S, learnable, add, resident=False)
                            assert res._resident() is not None and ref._resident() is None
                            for case in js["cases"]:
                                if (case["S"], case["learnable"], case["add"]) != (S, learnable, add):
                                    continue
                                got = check_case(res, js, a, case)
                                for dtype in DTYPES:                                 # ... and the index of the dict path, bit for bit
                                    np.random.seed(case["seed"])
                                    v0, i0 = ref.select(*case_inputs(js, case), js["T"], "cpu", dtype)
                                    assert torch.equal(got[dtype][0], v0) and torch.equal(got[dtype][1], i0), case["tag"]
    finally:
        simt.set_schedule("ascending")


# ---------------------------------------------------------------------------------------------- resident path = dict path
def offset_selectors(bank, wv, k=K):
    """(resident, dict) selectors with VISION_QUERY.ADD_VISION_LAYER and the offset `wv` (None: the zero it is created with)"""
    cfg = get_cfg()
    cfg.VISION_QUERY.NUM_QUERY_PER_CLASS, cfg.VISION_QUERY.ADD_VISION_LAYER = k, True
    res, ref = QuerySelector(cfg), QuerySelector(cfg)
    res.load_query_bank(bank)
    ref.load_query_bank({l: v.cpu() for l, v in bank.to_dict().items()})
    for sel in (res, ref):
        assert sel.tunable_vision_linear.weight.shape == (1000, bank.pool.shape[-1]) and not sel.tunable_vision_linear.weight.any()
        if wv is not None:
            sel.load_state_dict({"tunable_vision_linear.weight": wv}, strict=True)
    return res, ref


def seeded_wv(C, seed=3):
    return torch.randn(1000, C, generator=torch.Generator().manual_seed(seed + C))


@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("C", [4, 6, 256])
def test_resident_equals_dict_with_a_vision_offset(emu, C, S, dtype):
    bank = QueryBank.from_dict(ts.make_dict(C, S), "cpu")
    res, ref = offset_selectors(bank, seeded_wv(C))
    plain = ts.selectors(bank)[1]
    for n_items in (1, 2):
        v, _ = ts.same_select(res, ref, [ts.LABELS] * n_items, [ts.PMAP] * n_items, dtype=dtype)
        v0, _ = ts.seeded(lambda: plain.select([ts.LABELS] * n_items, [ts.PMAP] * n_items, T, "cpu", dtype), 5)[0]
        assert v.shape == v0.shape and not torch.equal(v, v0)                       # the offset is in the rows
    v, _ = ts.same_select(res, ref, *ts.RAGGED, dtype=dtype)
    # an item's rows get W[0 ..] whatever its place in the batch; its padding rows stay exact zeros
    lens = [sum(min(ts.COUNTS.get(l, 0), K) for l in labs) * S for labs in ts.RAGGED[0]]
    for i, n in enumerate(lens):
        assert not v[i, n:].view(torch.int32 if dtype == torch.float32 else torch.int16).any()
        assert n == 0 or v[i, :n].float().abs().sum() > 0


@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
def test_an_offset_at_8_bytes_takes_the_scalar_path_and_is_equal(emu, dtype):
    C = 4
    bank = QueryBank.from_dict(ts.make_dict(C, 5), "cpu")
    res, ref = offset_selectors(bank, seeded_wv(C))
    buf = torch.zeros(2 + 1000 * C)
    view = buf[2:].view(1000, C)
    view.copy_(seeded_wv(C))
    res.tunable_vision_linear.weight = nn.Parameter(view, requires_grad=False)
    res._drop_memos()
    assert res._row_add(1, "cpu").data_ptr() == view.data_ptr() and view.data_ptr() % 16 == 8 and bank.pool.data_ptr() % 16 == 0
    ts.same_select(res, ref, [ts.LABELS] * 2, [ts.PMAP] * 2, dtype=dtype)
    ts.same_select(res, ref, *ts.RAGGED, dtype=dtype)


@needs_emu
def test_the_addend_is_read_up_to_its_last_row_and_no_further(emu):
    """add_rows == Q * S exactly, a guard page directly behind (and, second mode, in front of) the addend: the launch passes.  One row more
    in an item is a ValueError on the host, before any launch."""
    from simt import guard
    from mq_det_amd import ops
    for C, S in ((4, 5), (6, 1), (256, 5)):
        bank = QueryBank.from_dict(ts.make_dict(C, S), "cpu")
        res, ref = offset_selectors(bank, seeded_wv(C))
        n = (3 + 3 + 2 + 3) * S                                                     # rows of the LABELS item: the longest of both inputs
        for mode in ("end", "start"):
            g = guard.guarded(seeded_wv(C)[:n], mode)
            res.tunable_vision_linear.weight = nn.Parameter(g, requires_grad=False)
            res._drop_memos()
            assert res._row_add(n, "cpu").data_ptr() == g.data_ptr()
            with guard.guarded_ops(mode):
                ts.same_select(res, ref, [ts.LABELS] * 2, [ts.PMAP] * 2, dtype=torch.float16)
                ts.same_select(res, ref, *ts.RAGGED, dtype=torch.bfloat16)
        # the wrapper itself, with tables that name Q * S rows
        res.tunable_vision_linear.weight = nn.Parameter(guard.guarded(seeded_wv(C)[:n - 1], "end"), requires_grad=False)
        res._drop_memos()
        calls = []
        real = ops.bank_select
        ops.bank_select = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        try:
            with pytest.raises(ValueError, match="ADD_VISION_LAYER"):
                res.select([ts.LABELS], [ts.PMAP], T, "cpu", torch.float16)
            res.select([[1, 2]], [{1: [0], 2: [1]}], T, "cpu", torch.float16)        # 5 S rows: fits
        finally:
            ops.bank_select = real
        assert len(calls) == 1
        short = QuerySelector(ref.cfg)
        short.load_query_bank(ref._source())
        short.tunable_vision_linear.weight = nn.Parameter(seeded_wv(C)[:n - 1].clone(), requires_grad=False)
        with pytest.raises(ValueError, match="ADD_VISION_LAYER"):
            short.select([ts.LABELS], [ts.PMAP], T, "cpu", torch.float16)


@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,S", [(4, 1), (6, 5), (256, 1)])
def test_the_old_export_is_what_it_was(emu, C, S, dtype):
    """mq_bank_select_fwd through the shared body: equal to the dict path (the yardstick of tests/test_query_select_cpu.py), equal to the
    symbol called directly, and equal to mq_bank_select_add_fwd with a zero addend."""
    from mq_det_amd import ops
    bank = QueryBank.from_dict(ts.make_dict(C, S), "cpu")
    res, ref = ts.selectors(bank)
    ts.same_select(res, ref, [ts.LABELS] * 2, [ts.PMAP] * 2, dtype=dtype)
    ts.same_select(res, ref, *ts.RAGGED, dtype=dtype)
    seen = []
    real = ops.bank_select
    ops.bank_select = lambda *a, **k: (seen.append((a, k)), real(*a, **k))[1]
    try:
        np.random.seed(5)
        v, idx = res.select(*ts.RAGGED, T, "cpu", dtype)
    finally:
        ops.bank_select = real
    (pool, slots, qsrc, qtok, T_, smax, dt), kw = seen[0]
    assert not kw and dt == dtype                                                   # switches off: the call is today's, no row_add
    v1, i1 = ops.bank_select(pool, slots, qsrc, qtok, T_, smax, dtype, row_add=None)
    lib = ops.load_library()
    v2, i2 = torch.full_like(v1, 7), torch.full_like(i1, 7)
    I, Q, MT = qtok.shape
    rc = lib.mq_bank_select_fwd(*(ctypes.c_void_p(t.data_ptr()) for t in (pool, slots, qsrc, qtok, v2, i2)), pool.shape[0], slots.shape[0],
                                slots.shape[1], I, Q, MT, S, C, T_, smax, ops._SELECT_OUT[dtype], ctypes.c_void_p(0))
    assert rc == 0
    v3, i3 = ops.bank_select(pool, slots, qsrc, qtok, T_, smax, dtype, row_add=torch.zeros(Q * S, C))
    for vv, ii in ((v1, i1), (v2, i2), (v3, i3)):
        assert torch.equal(vv, v) and torch.equal(ii, idx)


# ---------------------------------------------------------------------------------------------- the initial values change nothing
@needs_emu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_vision_offset_is_the_switch_off(emu, dtype):
    bank = QueryBank.from_dict(ts.make_dict(6, 5), "cpu")
    res, ref = offset_selectors(bank, None)                                         # zero, as created
    res0, ref0 = ts.selectors(bank)
    for labels, maps in (([ts.LABELS] * 2, [ts.PMAP] * 2), ts.RAGGED):
        v, i = ts.same_select(res, ref, labels, maps, dtype=dtype)
        v0, i0 = ts.same_select(res0, ref0, labels, maps, dtype=dtype)
        assert torch.equal(v, v0) and torch.equal(i, i0)


def test_prompt_offset_adds_in_fp32_and_rounds_once_and_zero_changes_nothing():
    from mq_det_amd.modeling import pipeline
    g = torch.Generator().manual_seed(1)
    B, Tl, H = 2, 32, 64
    h32 = torch.randn(B, Tl, H, generator=g)
    w = torch.randn(1000, H, generator=g) * 0.1
    emb = torch.randn(B, Tl, H, generator=g)
    for dtype in (torch.float16, torch.bfloat16):
        for split in (True, False):                                                 # with / without the unrounded text stream
            def lang():
                return {"hidden": h32.to(dtype), "hidden32": h32.clone() if split else None, "embedded": emb.clone(), "masks": None}
            same = pipeline.prompt_offset({}, lang())                               # switch off: the plan holds no addend
            assert torch.equal(same["hidden"], h32.to(dtype)) and torch.equal(same["embedded"], emb)
            zero = pipeline.prompt_offset({"rpn.tunable_linear.w32": torch.zeros(1000, H)}, lang())
            assert torch.equal(zero["hidden"], h32.to(dtype)) and torch.equal(zero["embedded"], emb)
            assert not split or torch.equal(zero["hidden32"], h32)
            out = pipeline.prompt_offset({"rpn.tunable_linear.w32": w}, lang())
            src = h32 if split else h32.to(dtype).float()
            assert torch.equal(out["hidden"], (src + w[:Tl]).to(dtype))             # row t of W at token position t, one rounding
            assert torch.equal(out["embedded"], emb + w[:Tl])
            assert (out["hidden32"] is None) if not split else torch.equal(out["hidden32"], h32 + w[:Tl])


# ---------------------------------------------------------------------------------------------- memos follow the parameters
@needs_emu
@pytest.mark.parametrize("resident", [False, True])
def test_load_state_dict_drops_the_memoised_selection(emu, resident):
    d = ts.make_dict(4, 1, {1: 2, 2: 3})
    bank = QueryBank.from_dict(d, "cpu")
    res, ref = offset_selectors(bank, seeded_wv(4, seed=1))
    sel = res if resident else ref
    pm = {1: [0, 2], 2: [2]}
    a = sel.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16)
    assert sel.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16) is a     # memoised
    w2 = seeded_wv(4, seed=2)
    sel.load_state_dict({"tunable_vision_linear.weight": w2}, strict=True)
    b = sel.select_cached("key", [1, 2], pm, 2, T, "cpu", torch.float16)
    rows = torch.cat([d[1][:2, 0], d[2][:3, 0]])
    assert b is not a and not torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(b[0], (rows + w2[:5]).to(torch.float16)[None].expand(2, -1, -1))
    assert torch.equal(a[0], (rows + seeded_wv(4, seed=1)[:5]).to(torch.float16)[None].expand(2, -1, -1))


def test_a_models_load_state_dict_reaches_the_selectors_memos(tmp_path):
    d, path = bank_file(tmp_path, C=4)
    m = small_model(learnable=True, vision=True, bank_path=path)
    sel = m.query_selector
    pm = {2: [1], 4: [3]}
    a = sel.select_cached("key", [2, 4], pm, 1, T, "cpu", torch.float32)
    assert sel.select_cached("key", [2, 4], pm, 1, T, "cpu", torch.float32) is a
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd["query_selector.tunable_vision_linear.weight"] = seeded_wv(4)
    sd["query_selector.query_bank.2"] = sd["query_selector.query_bank.2"] + 1.0
    m.load_state_dict(sd, strict=True)
    b = sel.select_cached("key", [2, 4], pm, 1, T, "cpu", torch.float32)
    want = torch.cat([d[2][:K, 0] + 1.0, d[4][:K, 0]]) + seeded_wv(4)[:5]
    assert torch.equal(b[0][0], want) and not torch.equal(a[0], b[0])
    # load_query_bank replaces what is selected FROM; the parameters stay in the state dict (the reference asserts the key off instead)
    m.load_query_bank({2: torch.ones(1, 1, 4)})
    c = sel.select_cached("key", [2, 4], pm, 1, T, "cpu", torch.float32)
    assert torch.equal(c[0][0], torch.ones(1, 4) + seeded_wv(4)[:1])
    assert torch.equal(m.state_dict()["query_selector.query_bank.2"], sd["query_selector.query_bank.2"])
