"""The forward-only set criterion of MQ-GroundingDINO (mq_det_amd.set_loss, csrc/set_loss.hip) without a GPU: the kernel SOURCES through the
host emulation (tests/simt) against tests/golden/set_loss, which tools/gen_golden_set_loss.py records by running the reference's own
HungarianMatcher / SetCriterion in place; both fibre schedules under the buffer-overrun guard; solver draws against the restatement
(tests/set_loss_ref.py, itself checked against scipy here); worst-case, tied and non-finite problems; the refusals; `hungarian_match`'s return
format; targets without 'normed_cxcy_boxes'; the normaliser under a gloo world of 2."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import set_loss_cases as sc  # noqa: E402
import set_loss_ref as sr  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


@pytest.fixture(scope="module")
def cases():
    return {n: sc.Case(n) for n in sc.NAMES}


# ---------------------------------------------------------------------------------------------- the yardsticks themselves
def test_restatement_solver_equals_scipy():
    """the YARDSTICK against scipy (it runs no code of the package: it does not count as coverage of the kernels)"""
    pytest.importorskip("scipy")
    for nq, G in sc.SOLVER_SHAPES:
        if G:
            C = sc.solver_draw(nq, G, 0)
            assert np.array_equal(sr.lsap(C), sc.scipy_solve(C)), (nq, G)
    i = np.arange(64)
    C = ((i[:, None] + 1) * (i[None, :] + 1)).astype(np.float32)
    assert sr.total(C, sr.lsap(C)) == sr.total(C, sc.scipy_solve(C))


@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_conditions_and_restatement(cases, name):
    """every stored matrix has a unique optimum (positive gap, `small`: >= 2 G eps); the restatement reproduces the reference's cost,
    indices and losses"""
    pytest.importorskip("scipy")
    case = cases[name]
    c64 = case.cost64()
    gaps = []
    for l in range(case.L):
        for b, c in enumerate(case.counts):
            if c == 0:
                continue
            ref = case.ref_cost[l, case.offs[b]:case.offs[b + 1]]
            gap = sr.gap_to_second_best(ref.numpy(), sc.scipy_solve)
            gaps.append(gap)
            assert gap > (2 * c * sc.eps_of(ref) if case.spec.get("wide_gap") else 0.0), (l, b, gap)
            assert np.array_equal(sr.lsap(ref.numpy()), case.ref_match[l, case.offs[b]:case.offs[b + 1]].numpy())
            err = (c64[l][case.offs[b]:case.offs[b + 1]] - ref.double()).abs()
            assert float(err.max()) <= 1e-5 * max(1.0, float(ref.abs().max())), float(err.max())     # the reference's own fp32 error
    assert min(gaps) == pytest.approx(case.meta["min_gap"], rel=1e-9)
    h = case.host
    sums = [sr.sums_ref(h["logits"][l], h["boxes"][l], case.per_image(h["gt"]), case.per_image(h["pm"]), h["mask"], case.ref_indices()[l],
                        sc.ALPHA, sc.GAMMA) for l in range(case.L)]
    mine = sr.losses_from_sums(sums, max(case.G, 1), sc.COEF)
    assert set(mine) == set(case.ref_losses)
    for k, v in case.ref_losses.items():
        assert mine[k] == pytest.approx(v, rel=1e-5), k


# ---------------------------------------------------------------------------------------------- the kernels on the fixtures
@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_cost(emu, cases, name):
    sc.check_cost(cases[name], emu)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_solver_on_the_reference_cost(emu, cases, name):
    sc.check_solver_on_reference_cost(cases[name], emu)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_solver_on_own_cost(emu, cases, name):
    sc.check_solver_on_own_cost(cases[name], emu)


@pytest.mark.parametrize("name", sc.NAMES)
def test_fixture_losses(emu, cases, name):
    from mq_det_amd import SetCriterionLoss
    sc.check_losses(cases[name], SetCriterionLoss)


@pytest.mark.parametrize("name", ["small", "main"])
def test_hungarian_match_returns_the_reference_indices(emu, cases, name):
    from mq_det_amd import hungarian_match
    case = cases[name]
    got = hungarian_match(case.outputs(), case.targets, case.dev["pm"], sc.cfg())
    assert isinstance(got, list) and len(got) == case.L
    for l, per_image in enumerate(got):
        assert len(per_image) == case.B
        for b, (qi, gj) in enumerate(per_image):
            assert qi.dtype == gj.dtype == torch.int64 and qi.shape == gj.shape == (case.counts[b],)
            assert bool((qi[1:] > qi[:-1]).all())                 # sorted by query, as scipy returns them
            if name == "small":                                   # the gap makes the device's own cost yield the reference's indices
                ri, rj = case.ref_indices()[l][b]
                assert torch.equal(qi, ri) and torch.equal(gj, rj)
    host = hungarian_match(case.outputs(), case.targets, case.dev["pm"], sc.cfg(), host=True)
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for x, y in zip(got, host) for a, b in zip(x, y))


@pytest.mark.parametrize("schedule", [("ascending", 0), ("random", 3), ("random", 11)])
def test_fixture_under_the_guard_and_both_fibre_schedules(emu, cases, schedule):
    import simt
    from mq_det_amd import SetCriterionLoss
    from simt import guard
    simt.set_schedule(*schedule)
    try:
        for mode in ("end", "start"):
            with guard.pointer_guard(mode):
                # `full` / `main`: more than one query tile, the 66.5 KB cost tile, the background column (`main` under one schedule)
                for name in ("small", "empty", "square", "full") + (("main",) if schedule[0] == "ascending" and mode == "end" else ()):
                    sc.check_cost(cases[name], emu)
                    sc.check_solver_on_reference_cost(cases[name], emu)
                    sc.check_solver_on_own_cost(cases[name], emu)
                    sc.check_losses(cases[name], SetCriterionLoss)
                sc.check_solver_draw(emu, 65, 33, 0)
    finally:
        simt.set_schedule("ascending")


# ---------------------------------------------------------------------------------------------- the solver alone
@pytest.mark.parametrize("nq,G", sc.SOLVER_SHAPES)
def test_solver_draws(emu, nq, G):
    sc.check_solver_draw(emu, nq, G, 0)


def _solve(emu, C):
    G, nq = C.shape
    m, q = emu.hungarian(torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32))[None], torch.tensor([0, G], dtype=torch.int32), [G])
    return m[0], q[0]


def test_solver_multiplicative_worst_case(emu):
    """C[i][j] = (i + 1)(j + 1): long augmenting paths"""
    i = np.arange(64)
    C = ((i[:, None] + 1) * (i[None, :] + 1)).astype(np.float32)
    m, q = _solve(emu, C)
    sc.assert_valid_matching(m, q, [64], 64)
    assert sr.total(C, m.numpy()) == sr.total(C, sr.lsap(C)) == float(sum((k + 1) * (64 - k) for k in range(64)))


def test_solver_integer_ties_and_duplicate_gts(emu):
    """ties: the assignment is not unique, the total is -- compared in fp64, exactly"""
    rng = np.random.default_rng(5)
    for G, nq in ((9, 9), (20, 70), (33, 130)):
        C = rng.integers(0, 4, (G, nq)).astype(np.float32)
        C[1] = C[0]                                               # duplicate gt boxes: equal rows
        C[G - 1] = C[0]
        m, q = _solve(emu, C)
        sc.assert_valid_matching(m, q, [G], nq)
        assert sr.total(C, m.numpy()) == sr.total(C, sr.lsap(C))
        m2, _ = _solve(emu, C)
        assert torch.equal(m, m2)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_entry_gives_up_and_shows_in_the_sums(emu, cases, bad):
    """emulation only: the solver returns, the problem's gts are -1, the layer's sums NaN, no guard trips; the other problems are solved"""
    from simt import guard
    case = cases["small"]
    d = case.dev
    cost = case.ref_cost.clone()
    cost[1, case.offs[2] + 1, 17] = bad                          # layer 1, image 2
    with guard.pointer_guard("end"):
        match_q, q2g = emu.hungarian(cost, case.gt_off, case.counts)
        sums = emu.set_loss(d["logits"], d["boxes"], d["gt"], d["pm"], case.gt_off, d["mask"], q2g, match_q, sc.ALPHA, sc.GAMMA)
    want = case.ref_match.clone().int()
    want[1, case.offs[2]:] = -1
    assert torch.equal(match_q, want) and bool((q2g[1, 2] == -1).all()) and bool((q2g[1, 0] >= 0).any())
    assert bool(torch.isnan(sums[1]).all()) and bool(torch.isfinite(sums[0]).all())


# ---------------------------------------------------------------------------------------------- the host side
def test_refusals(emu, cases):
    from mq_det_amd import SetCriterionLoss, hungarian_match, validate_set_loss_config
    cfg = sc.cfg()
    validate_set_loss_config(cfg)
    cfg.GROUNDINGDINO.matcher.matcher_type = "SimpleMinsumMatcher"
    with pytest.raises(NotImplementedError, match="matcher_type"):
        SetCriterionLoss(cfg)
    cfg = sc.cfg()
    cfg.VISION_QUERY.CONDITION_GATE = False
    with pytest.raises(NotImplementedError, match="CONDITION_GATE"):
        validate_set_loss_config(cfg)
    cfg.VISION_QUERY.ENABLED = False                              # no gates at all: nothing to restate
    validate_set_loss_config(cfg)
    cfg = sc.cfg()
    cfg.VISION_QUERY.FIX_ATTN_GATE = 0.5                          # no ff_gate parameters: the reference's gate term raises
    with pytest.raises(NotImplementedError, match="FIX_ATTN_GATE"):
        validate_set_loss_config(cfg)
    # a setting edited after construction is refused at the call, before anything is launched
    case = cases["small"]
    crit = SetCriterionLoss(sc.cfg())
    crit.cfg.GROUNDINGDINO.matcher.matcher_type = "SimpleMinsumMatcher"
    with pytest.raises(NotImplementedError, match="matcher_type"):
        crit(case.outputs(), case.targets, case.dev["mask"], case.dev["pm"])
    # more gts than queries / more queries than the solver takes: by count, before any launch
    launched = []
    real = emu.set_cost
    emu.set_cost = lambda *a, **k: launched.append(1) or real(*a, **k)
    try:
        gt = sc._boxes(np.random.default_rng(0), (5,))
        out = {"pred_logits": torch.zeros(1, 4, 8), "pred_boxes": torch.full((1, 4, 4), 0.5)}
        pm = torch.zeros(5, 8)
        pm[:, 1] = 1
        with pytest.raises(ValueError, match="5 gt boxes for 4 queries"):
            hungarian_match(out, sc.targets_of(gt, [5]), pm, sc.cfg())
        out = {"pred_logits": torch.zeros(1, 1025, 8), "pred_boxes": torch.full((1, 1025, 4), 0.5)}
        with pytest.raises(NotImplementedError, match="1025 queries"):
            hungarian_match(out, sc.targets_of(gt, [5]), pm, sc.cfg())
    finally:
        emu.set_cost = real
    assert not launched
    with pytest.raises(ValueError, match="5 gt boxes for 4 queries"):
        emu.hungarian(torch.zeros(1, 5, 4), torch.tensor([0, 5], dtype=torch.int32), [5])
    with pytest.raises(NotImplementedError, match="1025"):
        emu.hungarian(torch.zeros(1, 1, 1025), torch.tensor([0, 1], dtype=torch.int32), [1])
    lib = emu.load_library()
    assert lib.mq_hungarian_fwd(None, None, None, None, 1, 1, 1025, 1, 1, None) == -2
    assert lib.mq_hungarian_fwd(None, None, None, None, 1, 1, 4, 5, 5, None) == -3
    with pytest.raises(ValueError, match="positive_map"):
        hungarian_match(case.outputs(), case.targets, case.dev["pm"][:-1], sc.cfg())
    with pytest.raises(ValueError, match="BoxLists"):
        hungarian_match(case.outputs(), [case.host["gt"]], case.dev["pm"], sc.cfg())


def test_targets_without_normed_boxes(emu, cases):
    """the field is derived from the xyxy boxes and the image size, as the reference's dataset does"""
    from mq_det_amd import SetCriterionLoss
    from mq_det_amd.set_loss import _normed_cxcywh
    case = cases["small"]
    plain = sc.targets_of(case.host["gt"], case.counts, normed=False)
    for t, g in zip(plain, case.per_image(case.host["gt"])):
        assert "normed_cxcy_boxes" not in t.fields()
        assert float((_normed_cxcywh(t) - g).abs().max()) <= 2e-7
    crit = SetCriterionLoss(sc.cfg())
    a = crit(case.outputs(), case.targets, case.dev["mask"], case.dev["pm"])
    b = crit(case.outputs(), plain, case.dev["mask"], case.dev["pm"])
    assert torch.equal(a["match_q"], b["match_q"])                # the gap of `small` covers a last-bit change of the gt boxes
    assert torch.allclose(a["sums"], b["sums"], rtol=1e-5)
    assert a["num_boxes"] == case.G and set(sc.Case("small").ref_losses) <= set(a)


def test_evaluate_loss_dispatches_and_sums_before_it_normalises(emu, cases):
    """mq_det_amd.evaluate_loss on an MQ-GroundingDINO model: raw sums of all batches first, one normalisation by the total gt count"""
    from mq_det_amd import SetCriterionLoss, evaluate_loss
    cfg = sc.cfg()
    batch = [cases["small"], cases["empty"]]

    class Model:
        def __init__(self):
            self.cfg = cfg

        def eval(self):
            return self

        def forward_losses(self, images, targets):
            case = batch[images]
            out = SetCriterionLoss(cfg)(case.outputs(), targets, case.dev["mask"], case.dev["pm"])
            out["loss_gate"] = torch.tensor(0.05)
            return out
    got = evaluate_loss(Model(), [(i, c.targets, None) for i, c in enumerate(batch)], device="cpu")
    outs = [SetCriterionLoss(cfg)(c.outputs(), c.targets, c.dev["mask"], c.dev["pm"])["sums"].double() for c in batch]
    s, n = outs[0] + outs[1], batch[0].G + batch[1].G
    assert got["num_boxes"] == n and got["batches"] == 2 and got["loss_gate"] == pytest.approx(0.05)
    for l, sfx in ((0, "_0"), (1, "")):
        for j, name in enumerate(("loss_ce", "loss_bbox", "loss_giou")):
            assert got[name + sfx] == pytest.approx(float(s[l, j]) / n * sc.COEF[j], rel=1e-12)
    with pytest.raises(ValueError, match="no batch"):
        evaluate_loss(Model(), [], device="cpu")


def test_model_keeps_refusing_training_and_forward_losses_refuses_by_name():
    import gdino_checks as gc
    from oracle.spec import tiny_gdino_spec
    _, cfg, model = gc.gdino_model(torch.device("cpu"), tiny_gdino_spec())
    with pytest.raises(NotImplementedError):
        model.train()
    cfg.GROUNDINGDINO.matcher.matcher_type = "SimpleMinsumMatcher"
    try:
        with pytest.raises(NotImplementedError, match="matcher_type"):           # by name, before the device is touched
            model.forward_losses(torch.zeros(1, 3, 64, 64), [], ["a"])
    finally:
        cfg.GROUNDINGDINO.matcher.matcher_type = "HungarianMatcher"


def test_num_boxes_under_a_gloo_world_of_two():
    """num_boxes = max(all-reduced gt count / world, 1): 2 gloo processes with different batches"""
    script = os.path.join(ROOT, "tests", "_gloo_set_loss_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29548")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29548", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("SET_LOSS_NUM_BOXES_OK") == 2
