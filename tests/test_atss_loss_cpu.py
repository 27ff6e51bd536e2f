"""The forward-only ATSS objective (mq_det_amd.losses, csrc/atss_loss.hip) without a GPU: the kernel SOURCES through the host emulation
(tests/simt) against tests/golden/atss_loss, which tools/gen_golden_atss_loss.py records by running the reference's own
ATSSLossComputation.prepare_targets / __call__ in place; the three operand builds; both fibre schedules under the buffer-overrun guard; an
image without gts; a batch without positives; the refusals; shapes and dtypes of `prepare_targets`; the normalisers under a gloo world of 2.

`forward_losses` end to end on the tiny model through the emulation: tests/test_atss_forward_losses_cpu.py (the fp32-operand fixture); its
host-side argument checks are covered below."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import atss_loss_cases as ac  # noqa: E402
import atss_loss_ref as ar  # noqa: E402
from mq_det_amd.config import get_cfg  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
pytestmark = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


@pytest.mark.parametrize("name", ac.NAMES)
def test_fixture_targets_equal_the_reference(emu, name):
    from mq_det_amd import prepare_targets
    ac.check_targets(ac.Case(name), prepare_targets)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", ac.NAMES)
def test_fixture_losses_16bit(emu, name, dtype):
    ac.check_losses(ac.Case(name, dtype=dtype), compact=name != "alpha_neg")


@pytest.mark.parametrize("name", ac.NAMES)
def test_fixture_losses_precise(name):
    import simt
    with simt.installed(f32=1):
        ac.check_losses(ac.Case(name, dtype=torch.float32))


@pytest.mark.parametrize("schedule", [("ascending", 0), ("random", 3), ("random", 11)])
def test_fixture_under_the_guard_and_both_fibre_schedules(emu, schedule):
    import simt
    from mq_det_amd import prepare_targets
    from simt import guard
    simt.set_schedule(*schedule)
    try:
        for mode in ("end", "start"):
            with guard.pointer_guard(mode):
                case = ac.Case("tiny")
                ac.check_targets(case, prepare_targets)
                ac.check_losses(case)
    finally:
        simt.set_schedule("ascending")


def _restated(case_levels, gts, labels, pms, d, mask, alpha=0.25, gamma=2.0):
    logits = ar.logits_of(d["tok"].double(), d["tk"].double(), d["tbias"].double(), torch.float64)
    return ar.losses_ref([l.double() for l in case_levels], [g.double() for g in gts], labels, [p.double() for p in pms], d["reg"].double(),
                         d["ctr"].double(), logits, mask, alpha, gamma)


def test_image_without_gts_is_all_background(emu):
    """Deliberate difference from the reference (whose max over an empty dimension raises): an image without gt boxes is all background."""
    from mq_det_amd import ATSSLoss, prepare_targets
    case = ac.Case("alpha_neg")
    empty = BoxList(torch.zeros(0, 4), case.targets[0].size)
    empty.add_field("labels", torch.zeros(0, dtype=torch.int64))
    targets = [empty, case.targets[1]]
    pm = case.pms[1]
    cls, reg, tok = prepare_targets(targets, case.levels, pm)
    assert not cls[0].any() and not reg[0].any() and torch.equal(tok[0][:, -1], torch.ones(case.A)) and not tok[0][:, :-1].any()
    assert torch.equal(cls[1], case.ref_cls[1]) and torch.equal(tok[1], case.token_labels(case.ref_matched)[1])
    out = ATSSLoss(case.cfg())(case.head(), case.levels, targets, pm, case.mask)
    assert bool((out["matched"][0] == -1).all()) and torch.equal(out["matched"][1], case.ref_matched[1])
    want = _restated(case.levels, [empty.bbox, case.gts[1]], [empty.get_field("labels"), case.labels[1]], [pm[:0], pm], case.draws, case.mask,
                     alpha=case.meta["alpha"])
    assert int(out["sums"][0]) == want["num_pos"] > 0
    for k in ("loss_reg", "loss_centerness", "loss_dot_product_token"):
        assert abs(float(out[k]) - want[k]) <= 1e-5 * abs(want[k]), (k, float(out[k]), want[k])


def test_batch_without_positives(emu):
    """zero positives: loss_reg and loss_centerness are the reference's degenerate (empty) sums, the token loss is divided by max(0, 1)"""
    from mq_det_amd import ATSSLoss
    case = ac.Case("full")
    empty = BoxList(torch.zeros(0, 4), case.targets[0].size)
    empty.add_field("labels", torch.zeros(0, dtype=torch.int64))
    out = ATSSLoss(case.cfg())(case.head(), case.levels, [empty, empty], case.pm[:0], case.mask)
    assert bool((out["matched"] == -1).all()) and out["sums"][:5].tolist() == [0.0] * 5
    assert float(out["loss_reg"]) == 0.0 and float(out["loss_centerness"]) == 0.0 and float(out["loss_cls"]) == 0.0
    want = _restated(case.levels, [empty.bbox] * 2, [empty.get_field("labels")] * 2, [case.pm[:0]] * 2, case.draws, case.mask)
    assert want["num_pos"] == 0 and want["loss_dot_product_token"] > 0          # a caption of full length: the background column counts
    assert abs(float(out["loss_dot_product_token"]) - want["loss_dot_product_token"]) <= 1e-5 * want["loss_dot_product_token"]


def test_two_runs_are_bit_identical(emu):
    from mq_det_amd import ATSSLoss
    case = ac.Case("main")
    a = ATSSLoss(case.cfg())(case.head(), case.levels, case.targets, case.pm, case.mask)
    b = ATSSLoss(case.cfg())(case.head(), case.levels, case.targets, case.pm, case.mask)
    assert torch.equal(a["sums"].view(torch.int32), b["sums"].view(torch.int32)) and torch.equal(a["matched"], b["matched"])


def test_plain_path_of_the_gemm_fallback_head(emu):
    """a head that carries materialised dot products instead of the fused operands: same losses from the plain torch path"""
    from mq_det_amd import ATSSLoss
    case = ac.Case("tiny")
    fused = ATSSLoss(case.cfg())(case.head(), case.levels, case.targets, case.pm, case.mask)
    d = case.draws
    T = case.head()["tbias"].shape[1]
    dot = torch.bmm(d["tok"], d["tk"][:, :T].transpose(1, 2))
    offs, dots, regs, ctrs = 0, [], [], []
    for (h, w) in case.sizes:
        n = h * w
        dots.append(dot[:, offs:offs + n])
        regs.append(d["reg"][:, offs:offs + n].reshape(case.B, h, w, 4).permute(0, 3, 1, 2))
        ctrs.append(d["ctr"][:, offs:offs + n].reshape(case.B, h, w, 1).permute(0, 3, 1, 2))
        offs += n
    plain = ATSSLoss(case.cfg())({"dot": dots, "bbox_reg": regs, "centerness": ctrs, "tbias": d["tbias"][:, :T].contiguous()}, case.levels,
                                 case.targets, case.pm, case.mask)
    assert torch.equal(plain["sums"][:5], fused["sums"][:5])
    assert abs(float(plain["sums"][5]) - float(fused["sums"][5])) <= 1e-5 * float(fused["sums"][5])


def test_refusals(emu):
    from mq_det_amd import ATSSLoss, prepare_targets
    fc_keys = {"USE_DOT_PRODUCT_TOKEN_LOSS": False, "USE_CLASSIFICATION_LOSS": True, "USE_TOKEN_LOSS": True, "USE_CONTRASTIVE_ALIGN_LOSS": True,
               "USE_SHALLOW_CONTRASTIVE_LOSS": True, "USE_BACKBONE_SHALLOW_CONTRASTIVE_LOSS": True, "MLM_LOSS": True}
    for key, bad in fc_keys.items():
        cfg = get_cfg()
        ATSSLoss(cfg)
        cfg.MODEL.DYHEAD.FUSE_CONFIG[key] = bad
        with pytest.raises(NotImplementedError, match=key):
            ATSSLoss(cfg)
    cfg = get_cfg()
    cfg.MODEL.RPN.ASPECT_RATIOS = (0.5, 1.0, 2.0)
    with pytest.raises(NotImplementedError, match="ASPECT_RATIOS"):
        ATSSLoss(cfg)
    cfg = get_cfg()
    cfg.MODEL.RPN.SCALES_PER_OCTAVE = 3
    with pytest.raises(NotImplementedError, match="SCALES_PER_OCTAVE"):
        ATSSLoss(cfg)
    cfg = get_cfg()
    cfg.MODEL.ATSS.TOPK = 65
    with pytest.raises(NotImplementedError, match="TOPK"):
        ATSSLoss(cfg)
    # a setting edited after construction is refused at the call, before anything is launched
    case = ac.Case("tiny")
    crit = ATSSLoss(case.cfg())
    crit.cfg.MODEL.DYHEAD.FUSE_CONFIG.USE_TOKEN_LOSS = True
    with pytest.raises(NotImplementedError, match="USE_TOKEN_LOSS"):
        crit(case.head(), case.levels, case.targets, case.pm, case.mask)
    # targets
    good = case.targets[0]
    xywh = good.convert("xywh")
    xywh.add_field("labels", good.get_field("labels"))
    nolabels = BoxList(good.bbox, good.size)
    for bad in ([xywh, case.targets[1]], [nolabels, case.targets[1]], [good.bbox, case.targets[1]], [], good):
        with pytest.raises(ValueError):
            prepare_targets(bad, case.levels, None)
    with pytest.raises(ValueError, match="positive_map"):
        prepare_targets(case.targets, case.levels, case.pm[:-1])
    with pytest.raises(ValueError, match="anchors"):
        prepare_targets(case.targets, [torch.zeros(3, 5)], None)
    with pytest.raises(ValueError, match="TOPK"):
        prepare_targets(case.targets, case.levels, None, topk=100)
    assert get_cfg().MODEL.ATSS.TOPK == 9 and get_cfg().MODEL.ATSS.REG_LOSS_WEIGHT == 2.0
    fc = get_cfg().MODEL.DYHEAD.FUSE_CONFIG
    assert (fc.TOKEN_ALPHA, fc.TOKEN_GAMMA, fc.DOT_PRODUCT_TOKEN_LOSS_WEIGHT) == (0.25, 2.0, 1.0)


def test_model_keeps_refusing_training_and_forward_losses_checks_its_arguments():
    from mq_det_amd import build_detection_model
    cfg = get_cfg()
    cfg.MODEL.SWINT.DEPTHS = (2, 2, 2, 2)
    cfg.MODEL.LANGUAGE_BACKBONE.NUM_HIDDEN_LAYERS, cfg.MODEL.LANGUAGE_BACKBONE.QV_START = 2, 1
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = 1100
    cfg.MODEL.DYHEAD.NUM_CONVS = 1
    model = build_detection_model(cfg, tokenizer=object())
    with pytest.raises(NotImplementedError):
        model.train()
    cfg.MODEL.DYHEAD.FUSE_CONFIG.USE_CONTRASTIVE_ALIGN_LOSS = True
    with pytest.raises(NotImplementedError, match="USE_CONTRASTIVE_ALIGN_LOSS"):     # by name, before the device is touched
        model.forward_losses(torch.zeros(1, 3, 64, 64), [], ["a"])
    cfg.MODEL.DYHEAD.FUSE_CONFIG.USE_CONTRASTIVE_ALIGN_LOSS = False
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.forward_losses(torch.zeros(1, 3, 64, 64), [], ["a"])


def test_prepare_targets_accepts_the_reference_anchor_layout(emu):
    """per image a list of per-level BoxLists, as the reference's anchor generator returns them"""
    from mq_det_amd import prepare_targets
    case = ac.Case("tiny")
    per_image = [[BoxList(l, case.targets[0].size) for l in case.levels] for _ in range(case.B)]
    cls, reg, tok = prepare_targets(case.targets, per_image)
    assert tok == [] and all(torch.equal(c, r) for c, r in zip(cls, case.ref_cls))


def test_evaluate_loss_sums_before_it_normalises(emu):
    """dataset means come from the raw sums of all batches (not from the mean of per-batch losses), with one list transfer at the end"""
    from mq_det_amd import ATSSLoss, evaluate_loss
    cases = [ac.Case("tiny"), ac.Case("alpha_neg")]
    cfg = cases[0].cfg()

    class Model:
        def __init__(self):
            self.cfg = cfg

        def eval(self):
            return self

        def forward_losses(self, images, targets, captions):
            case = cases[images]
            assert captions == ["c%d" % b for b in range(case.B)]
            return ATSSLoss(cfg)(case.head(), case.levels, targets, case.pm, case.mask)
    batches = []
    for i, c in enumerate(cases):
        for b, t in enumerate(c.targets):
            t.add_field("caption", "c%d" % b)
        batches.append((i, c.targets, None))
    got = evaluate_loss(Model(), batches, device="cpu")
    outs = [ATSSLoss(cfg)(c.head(), c.levels, c.targets, c.pm, c.mask)["sums"].double() for c in cases]
    s = (outs[0] + outs[1]).tolist()
    assert got["num_pos"] == int(s[0]) and got["batches"] == 2
    assert got["loss_reg"] == pytest.approx(2.0 * s[2] / s[1], rel=1e-12) and got["loss_centerness"] == pytest.approx(s[3] / s[0], rel=1e-12)
    assert got["loss_dot_product_token"] == pytest.approx(s[5] / s[0], rel=1e-12)
    with pytest.raises(ValueError, match="no batch"):
        evaluate_loss(Model(), [], device="cpu")


def test_normalisers_under_a_gloo_world_of_two():
    """max(num_pos / world, 1) and S centerness / world with both all-reduced, as the reference's reduce_sum does: 2 gloo processes"""
    script = os.path.join(ROOT, "tests", "_gloo_atss_loss_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29547", script], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ATSS_NORMALISERS_OK") == 2
