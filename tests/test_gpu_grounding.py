"""`GeneralizedVLRCNN_New.forward_grounding` on the MI355X: the tiny model of parity_checks.tiny on the 160 x 192 canvas, B = 3, three different
captions (12, 30 and 21 tokens) with positive maps of 2, 5 and 3 phrases, once with a query bank and once without.  Item i is compared with
the per-item `model(...)` call of the same build (split-precise mode: element gate 1e-3 + 1e-3 |ref| on the head outputs, zero elements
outside) and with the fp32 oracle called per item (the detection gate of parity_checks.check_full_model as it stands); in the default fp16
build the labels, the counts and the HIP-graph replay are checked."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

from mq_det_amd.structures import ImageList  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")
HW = ((150, 190), (160, 170), (140, 192))
NVALID = (12, 30, 21)
MAPS = [{1: [1, 2], 2: [4]}, {1: [1], 2: [3, 4], 3: [6], 4: [8, 9, 10], 5: [12]}, {1: [2], 2: [5, 6], 3: [9]}]
CAPS = ["first caption", "second caption . longer", "third caption"]


class Setup:
    """the tiny model of the current parity_checks dtype + the inputs; the oracle's per-item detections are computed once per bank setting"""
    _oracle = {}

    def __init__(self, with_bank):
        import parity_checks as pc
        from oracle.weights import make_query_bank
        self.pc = pc
        self.spec, self.sd, self.cfg, self.model, _ = pc.tiny(DEV)
        images, self.sizes, _, _, _, _ = pc.make_inputs(self.spec, B=3, hw=HW)
        self.images = images
        g = torch.Generator().manual_seed(17)
        T = self.spec.max_query_len
        self.ids = torch.zeros(3, T, dtype=torch.long)
        self.am = torch.zeros(3, T, dtype=torch.long)
        for i, n in enumerate(NVALID):
            self.ids[i, :n] = torch.randint(1, self.spec.vocab, (n,), generator=g)
            self.am[i, :n] = 1
        self.bank = make_query_bank(range(1, 6), self.spec) if with_bank else None
        self.with_bank = with_bank
        rows = {c: i for i, c in enumerate(CAPS)}

        def tokenize(caps, dev):
            r = [rows[c] for c in caps]
            return self.ids[r].to(dev), self.am[r].to(dev), max(NVALID[i] for i in r)
        self.model.tokenize = tokenize
        self.model.load_query_bank(self.bank)
        self.model.clear_caches()

    def il(self, i=None):
        if i is None:
            return ImageList(self.images.to(DEV), self.sizes)
        return ImageList(self.images[i:i + 1].to(DEV), self.sizes[i:i + 1])

    def oracle(self, i):
        key = (self.with_bank, i)
        if key not in Setup._oracle:
            from oracle import detector as od
            with torch.no_grad():
                Setup._oracle[key] = od.forward(self.sd, self.spec, self.images[i:i + 1], self.sizes[i:i + 1], self.ids[i:i + 1], self.am[i:i + 1],
                                                MAPS[i], self.bank)[0]
        return Setup._oracle[key]


def detection_gate(pc, post, b, ref):
    """parity_checks.check_full_model's gate on the final detections: of the oracle's top-50, the fraction matched by a detection of the same
    label with IoU > 0.9 (legacy + 1) and |ds| < 0.02 must reach 0.8 (bf16: IoU > 0.8, 8 x the score distance)"""
    n = int(post["counts"][b])
    gb, gs, gl = post["boxes"][b, :n].cpu(), post["scores"][b, :n].cpu(), post["labels"][b, :n].cpu()
    rb, rs, rl = ref["boxes"], ref["scores"], ref["labels"]
    top = torch.argsort(rs, descending=True)[:50]
    matched = 0
    for i in top.tolist():
        same = (gl == rl[i])
        if not same.any():
            continue
        lt = torch.max(gb[:, :2], rb[i, :2])
        br = torch.min(gb[:, 2:], rb[i, 2:])
        inter_a = (br - lt + 1).clamp(min=0).prod(1)
        a1 = (gb[:, 2] - gb[:, 0] + 1) * (gb[:, 3] - gb[:, 1] + 1)
        a2 = (rb[i, 2] - rb[i, 0] + 1) * (rb[i, 3] - rb[i, 1] + 1)
        iou = torch.where(same, inter_a / (a1 + a2 - inter_a), torch.zeros_like(a1))
        j = int(iou.argmax())
        if iou[j] > (0.9 if pc.TOL_SCALE == 1.0 else 0.8) and abs(float(gs[j] - rs[i])) < 0.02 * pc.TOL_SCALE:
            matched += 1
    frac = matched / max(1, len(top))
    print(f"item {b}: n_hip={n} n_ref={len(rb)} matched {matched}/{len(top)}", flush=True)
    return frac, n, len(rb)


@pytest.mark.parametrize("with_bank", [True, False], ids=["bank", "text_only"])
def test_default_build_labels_counts_oracle_and_graph_replay(with_bank):
    s = Setup(with_bank)
    m = s.model
    with torch.no_grad():
        raw = m.forward_grounding(s.il(), CAPS, MAPS, return_raw=True)
        for i in range(3):                                                         # the fp32 oracle called per item
            frac, n, n_ref = detection_gate(s.pc, raw["post"], i, s.oracle(i))
            assert frac >= 0.8, (i, frac)
        replays = m.cache_stats["graph_replay"]
        outs = [m.forward_grounding(s.il(), CAPS, MAPS) for _ in range(3)]         # eager, capture + replay, replay
    assert m.cache_stats["graph_replay"] >= replays + 2
    assert m.last_packed.shape[0] == 3
    for i, bl in enumerate(outs[0]):
        labels = bl.get_field("labels").tolist()
        assert 0 < len(bl) <= m.last_packed.shape[1] and set(labels) <= set(MAPS[i]), (i, sorted(set(labels)))
        assert bl.size == (HW[i][1], HW[i][0]) and bl.bbox.is_cuda
        n_ref = len(s.oracle(i)["boxes"])                                          # plausible: within half of the oracle's count
        assert abs(len(bl) - n_ref) <= max(5, n_ref // 2), (i, len(bl), n_ref)
        for later in outs[1:]:
            assert torch.equal(later[i].bbox, bl.bbox) and torch.equal(later[i].get_field("scores"), bl.get_field("scores"))
            assert torch.equal(later[i].get_field("labels"), bl.get_field("labels"))
    # forward keeps its behaviour: the per-item call gives the same labels and about as many detections
    with torch.no_grad():
        one = m(s.il(1), captions=[CAPS[1]], positive_map=MAPS[1])[0]
    assert set(one.get_field("labels").tolist()) <= set(MAPS[1]) and abs(len(one) - len(outs[0][1])) <= max(3, len(one) // 20)


@pytest.fixture(scope="module")
def f32():
    """the split-precise mode (as tests/test_gpu_parity.py selects it)"""
    import parity_checks as pc
    from mq_det_amd import ops
    prev = os.environ.get("MQ_F32_OPERANDS")
    os.environ["MQ_F32_OPERANDS"] = "1"
    ops.configure()
    pc.use_dtype(torch.float32)
    yield pc
    pc.use_dtype(torch.float16)
    if prev is None:
        os.environ.pop("MQ_F32_OPERANDS", None)
    else:
        os.environ["MQ_F32_OPERANDS"] = prev
    ops.configure()


@pytest.mark.parametrize("with_bank", [True, False], ids=["bank", "text_only"])
def test_split_precise_item_equals_the_per_item_call(f32, with_bank):
    s = Setup(with_bank)
    m = s.model
    worst = 0.0
    with torch.no_grad():
        raw = m.forward_grounding(s.il(), CAPS, MAPS, return_raw=True)
        for i in range(3):
            ref = m(s.il(i), captions=[CAPS[i]], positive_map=MAPS[i], return_raw=True)
            nv = NVALID[i]
            for lvl in range(5):
                pairs = [("dot", (raw["head"]["dot"][lvl][i].float() + raw["head"]["tbias"][i][None, :])[:, :nv],
                          (ref["head"]["dot"][lvl][0].float() + ref["head"]["tbias"][0][None, :])[:, :nv]),
                         ("bbox_reg", raw["head"]["bbox_reg"][lvl][i].float(), ref["head"]["bbox_reg"][lvl][0].float()),
                         ("centerness", raw["head"]["centerness"][lvl][i].float(), ref["head"]["centerness"][lvl][0].float())]
                for name, got, want in pairs:
                    assert got.shape == want.shape and want.numel() > 0, (name, got.shape, want.shape)
                    diff = (got - want).abs()
                    excess = (diff - (1e-3 + 1e-3 * want.abs())).max().item()
                    worst = max(worst, diff.max().item())
                    print(f"item {i} lvl {lvl} {name}: max |diff| {diff.max().item():.3e}", flush=True)
                    assert torch.isfinite(got).all() and excess <= 0, (i, lvl, name, diff.max().item())
            frac, n, n_ref = detection_gate(f32, raw["post"], i, s.oracle(i))    # the fp32 oracle called per item
            assert frac >= 0.8, (i, frac)
    print(f"worst |diff| {worst:.3e}", flush=True)
