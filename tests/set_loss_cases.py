"""TEST INFRASTRUCTURE shared by tests/test_set_loss_cpu.py (kernel sources through tests/simt) and tests/test_gpu_set_loss.py (the device):
the integer draws and fixture cases of tests/golden/set_loss (tools/gen_golden_set_loss.py: the reference's own matcher and criterion, run in
place) and the gates.

Gates.  Cost: every finite entry within 1e-4 + 1e-4 |ref| of the reference's (fp32 element-wise math on bounded inputs: logits k / 8 with
|k| <= 32 keep 1 - p >= 0.018, so no logarithm is amplified; ten times inside the project's 1e-3 gate).  Solver: on the reference's stored
matrix, bit for bit, the indices equal the reference's (the optimum of every stored matrix is unique by a positive gap, asserted).  Solver on
the device's own cost: an entry-wise error eps moves the total of any assignment by at most G eps, so the device's assignment, priced on the
fp64 cost, is within 2 G eps of the optimum; for `small` the gap to the second best exceeds that, so the indices are the reference's.  Losses,
with the reference's indices fed in: 1e-3 + 1e-3 |ref|, the project's standing gate; two runs give the same bits."""
import hashlib
import json
import os

import numpy as np
import torch

import set_loss_ref as sr
from mq_det_amd.config import get_gdino_cfg
from mq_det_amd.structures import BoxList

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "set_loss", "cases")
T_FULL = 256
SIZE = (640, 480)                                            # (width, height) of every target BoxList
COST = (1.0, 5.0, 2.0)                                       # set_cost_class, set_cost_bbox, set_cost_giou
COEF = (2.0, 5.0, 2.0)                                       # loss_ce_coef, loss_bbox_coef, loss_giou_coef
ALPHA, GAMMA = 0.25, 2.0
SPECS = {
    # counts: gts per image; live: live text tokens; pad: -inf columns the device's logits keep behind them; stray: a positive token of gt 0
    # at a column the device's logits do not have (>= T); stray_pad: a positive token of the last gt at a -inf logit INSIDE the T columns
    "main": dict(seed=1, L=2, nq=900, counts=(1, 7, 40), live=60, pad=4, stray=True),
    "full": dict(seed=2, L=2, nq=100, counts=(2, 5), live=256, pad=0, stray=False),
    "square": dict(seed=3, L=2, nq=12, counts=(12, 12), live=40, pad=3, stray=False, stray_pad=True),
    "empty": dict(seed=4, L=2, nq=32, counts=(3, 0, 4), live=33, pad=0, stray=True),
    "small": dict(seed=5, L=2, nq=32, counts=(6, 2, 5), live=24, pad=8, stray=False, stray_pad=True, wide_gap=True),
}
NAMES = tuple(SPECS)
COST_ATOL = COST_RTOL = 1e-4
LOSS_ATOL = LOSS_RTOL = 1e-3
_FIX = None


def _boxes(rng, shape, cluster=False):
    """cxcywh in 1/1024 steps (exact in fp32), inside the unit square"""
    if cluster:
        c = rng.integers(460, 564, (*shape, 2))
        wh = rng.integers(150, 260, (*shape, 2))
    else:
        c = rng.integers(205, 820, (*shape, 2))
        wh = rng.integers(40, 400, (*shape, 2))
    return torch.from_numpy(np.concatenate([c, wh], -1) / 1024.0).float()


def draw(spec, seed):
    """Everything a case holds but the reference's results, from integer draws."""
    rng = np.random.default_rng(seed)
    L, nq, counts, live = spec["L"], spec["nq"], spec["counts"], spec["live"]
    B, G = len(counts), sum(counts)
    k = rng.integers(-32, 33, (L, B, nq, live))
    full = torch.full((L, B, nq, T_FULL), -float("inf"))
    full[..., :live] = torch.from_numpy(k / 8.0).float()
    boxes = _boxes(rng, (L, B, nq))
    gt = torch.cat([_boxes(rng, (c,), cluster=c >= 30) for c in counts]) if G else torch.zeros(0, 4)
    pm = torch.zeros(G, T_FULL)
    for g in range(G):
        span = int(rng.integers(1, 4))
        start = int(rng.integers(1, max(2, live - span)))
        pm[g, start:start + span] = 1.0
    if spec["stray"] and live + 10 < T_FULL:
        pm[0, live + 10] = 1.0
    if spec.get("stray_pad"):
        assert spec["pad"] > 1
        pm[G - 1, live + 1] = 1.0
    mask = torch.zeros(B, T_FULL, dtype=torch.int32)
    mask[:, :live] = 1
    T = min(T_FULL, live + spec["pad"])
    return {"logits_full": full, "logits": full[..., :T].contiguous(), "boxes": boxes, "gt": gt, "pm": pm, "mask_full": mask,
            "mask": mask[:, :T].contiguous()}


def checksum(d):
    h = hashlib.sha256()
    for key in ("logits_full", "boxes", "gt", "pm"):
        h.update(d[key].numpy().tobytes())
    return h.hexdigest()[:16]


def match_of(index_i, index_j, count):
    """(index_i, index_j) of one image -> the query of each gt [count]"""
    out = np.full(count, -1, dtype=np.int64)
    out[np.asarray(index_j)] = np.asarray(index_i)
    return out


def scipy_solve(cost):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(np.asarray(cost, dtype=np.float64))[1]


def fixture():
    global _FIX
    if _FIX is None:
        with open(GOLD + ".json") as f:
            _FIX = (json.load(f), dict(np.load(GOLD + ".npz")))
    return _FIX


def targets_of(gt, counts, device="cpu", normed=True):
    out, off = [], 0
    for c in counts:
        g = gt[off:off + c]
        t = BoxList((sr.xyxy(g) * torch.tensor([[SIZE[0], SIZE[1]] * 2], dtype=torch.float32)).to(device), SIZE, mode="xyxy")
        if normed:
            t.add_field("normed_cxcy_boxes", g.to(device))
        out.append(t)
        off += c
    return out


def cfg():
    c = get_gdino_cfg()
    assert (c.GROUNDINGDINO.loss_ce_coef, c.GROUNDINGDINO.loss_bbox_coef, c.GROUNDINGDINO.loss_giou_coef) == COEF
    m = c.GROUNDINGDINO.matcher
    assert (m.set_cost_class, m.set_cost_bbox, m.set_cost_giou, m.focal_alpha) == (*COST, ALPHA)
    return c


class Case:
    """One fixture case on `device`: the draws, the reference's cost [L, G, nq], its matching [L, G] and its losses."""

    def __init__(self, name, device="cpu"):
        js, a = fixture()
        self.name, self.spec, self.meta = name, SPECS[name], js["cases"][name]
        d = draw(self.spec, self.meta["seed"])
        assert checksum(d) == self.meta["checksum"], "the integer draws drifted"
        self.counts = list(self.spec["counts"])
        self.L, self.B, self.nq, self.T = d["logits"].shape
        self.G = sum(self.counts)
        self.host = d
        self.dev = {k: v.to(device) for k, v in d.items()}
        self.device = device
        self.offs = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.gt_off = torch.tensor(self.offs, dtype=torch.int32, device=device)
        self.ref_cost = torch.from_numpy(a[name + "_cost"]).reshape(self.L, self.G, self.nq)
        self.ref_match = torch.from_numpy(a[name + "_match"]).reshape(self.L, self.G)
        self.targets = targets_of(d["gt"], self.counts, device)
        self.ref_losses = self.meta["losses"]

    def outputs(self):
        lg, bx = self.dev["logits"], self.dev["boxes"]
        return {"pred_logits": lg[-1], "pred_boxes": bx[-1],
                "aux_outputs": [{"pred_logits": lg[l], "pred_boxes": bx[l]} for l in range(self.L - 1)]}

    def per_image(self, t):
        return [t[self.offs[b]:self.offs[b + 1]] for b in range(self.B)]

    def ref_indices(self):
        return [[sr.indices_of(m.numpy()) for m in self.per_image(self.ref_match[l])] for l in range(self.L)]

    def cost64(self):
        """the restatement's fp64 cost, per layer a [G, nq] tensor"""
        h = self.host
        return [torch.cat(sr.cost_ref(h["logits"][l], h["boxes"][l], self.per_image(h["gt"]), self.per_image(h["pm"]), *COST, ALPHA))
                if self.G else torch.zeros(0, self.nq, dtype=torch.float64) for l in range(self.L)]


def eps_of(cost):
    return COST_ATOL + COST_RTOL * float(cost.abs().max()) if cost.numel() else COST_ATOL


def assert_valid_matching(match_q, q2g, counts, nq):
    """every gt matched once, to distinct queries; q2g is the inverse map.  match_q [G], q2g [B, nq] of one layer (host tensors)"""
    off = 0
    for b, c in enumerate(counts):
        m = match_q[off:off + c].long()
        assert bool(((m >= 0) & (m < nq)).all()) and len(torch.unique(m)) == c, (b, m)
        inv = torch.full((nq,), -1, dtype=torch.int64)
        inv[m] = torch.arange(c)
        assert torch.equal(q2g[b].long(), inv), b
        off += c


def check_cost(case, ops):
    d = case.dev
    got = ops.set_cost(d["logits"], d["boxes"], d["gt"], d["pm"], case.gt_off, *COST, ALPHA).cpu()
    ref = case.ref_cost
    assert got.shape == ref.shape and bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all())
    err = (got.double() - ref.double()).abs()
    bound = COST_ATOL + COST_RTOL * ref.double().abs()
    print(f"set_cost {case.name}: max |dev - ref| = {float(err.max()) if err.numel() else 0.0:.3e}")
    assert bool((err <= bound).all()), float((err - bound).max())
    return got


def check_solver_on_reference_cost(case, ops):
    match_q, q2g = ops.hungarian(case.ref_cost.to(case.device).contiguous(), case.gt_off, case.counts)
    match_q, q2g = match_q.cpu(), q2g.cpu()
    assert torch.equal(match_q.long(), case.ref_match.long()), case.name
    for l in range(case.L):
        assert_valid_matching(match_q[l], q2g[l], case.counts, case.nq)


def check_solver_on_own_cost(case, ops):
    d = case.dev
    cost = ops.set_cost(d["logits"], d["boxes"], d["gt"], d["pm"], case.gt_off, *COST, ALPHA)
    match_q, q2g = ops.hungarian(cost, case.gt_off, case.counts)
    match_q, q2g = match_q.cpu(), q2g.cpu()
    c64 = case.cost64()
    for l in range(case.L):
        assert_valid_matching(match_q[l], q2g[l], case.counts, case.nq)
        for b, c in enumerate(case.counts):
            if c == 0:
                continue
            C = c64[l][case.offs[b]:case.offs[b + 1]].numpy()
            mine = sr.total(C, match_q[l, case.offs[b]:case.offs[b + 1]].numpy())
            best = sr.total(C, sr.lsap(C))
            assert mine - best <= 2 * c * eps_of(torch.from_numpy(C)), (case.name, l, b, mine - best)
    if case.spec.get("wide_gap"):
        assert torch.equal(match_q.long(), case.ref_match.long())


def check_losses(case, SetCriterionLoss):
    crit = SetCriterionLoss(cfg())
    args = (case.outputs(), case.targets, case.dev["mask"], case.dev["pm"])
    out = crit(*args, indices=case.ref_indices())
    again = crit(*args, indices=case.ref_indices())
    assert torch.equal(out["sums"].view(torch.int32), again["sums"].view(torch.int32))
    assert set(case.ref_losses) == {k for k in out if k.startswith("loss_")}, set(case.ref_losses) ^ set(out)
    for k, ref in case.ref_losses.items():
        got = float(out[k])
        print(f"set_loss {case.name} {k}: dev {got:.6f} ref {ref:.6f}")
        assert abs(got - ref) <= LOSS_ATOL + LOSS_RTOL * abs(ref), (k, got, ref)
    # the 3 L raw sums against the reference's losses un-normalised (num_boxes = max(G, 1))
    n = max(case.G, 1)
    sums = out["sums"].cpu()
    for l in range(case.L):
        sfx = "" if l == case.L - 1 else f"_{l}"
        for j, name in enumerate(("loss_ce", "loss_bbox", "loss_giou")):
            ref = case.ref_losses[name + sfx] * n / COEF[j]
            assert abs(float(sums[l, j]) - ref) <= LOSS_ATOL + LOSS_RTOL * abs(ref), (l, name, float(sums[l, j]), ref)
    return out


def solver_draw(nq, G, seed):
    """a random [G, nq] fp32 problem: the restatement's optimum is unique with probability 1; compared by indices"""
    rng = np.random.default_rng(1000 * seed + 7 * nq + G)
    return rng.standard_normal((G, nq)).astype(np.float32)


SOLVER_SHAPES = [(nq, G) for nq in (1, 7, 63, 64, 65, 257, 1024) for G in sorted({0, 1, nq // 2, *((nq,) if nq <= 64 else ()), *((100,) if nq >= 257 else ())})
                 if G <= nq] + [(900, 300)]


def check_solver_draw(ops, nq, G, seed, device="cpu"):
    C = solver_draw(nq, G, seed)
    cost = torch.from_numpy(C)[None].contiguous().to(device)
    off = torch.tensor([0, G], dtype=torch.int32, device=device)
    match_q, q2g = ops.hungarian(cost, off, [G])
    match_q, q2g = match_q.cpu(), q2g.cpu()
    assert_valid_matching(match_q[0], q2g[0], [G], nq)
    ref = sr.lsap(C)
    assert sr.total(C, match_q[0].numpy()) == sr.total(C, ref) and np.array_equal(match_q[0].numpy(), ref), (nq, G, seed)


# ---------------------------------------------------------------------------------------------- forward_losses on the tiny MQ-GroundingDINO
def end_to_end(dev):
    """`forward_losses` of the shallow MQ-GroundingDINO of the parity ladders (vision queries, one image) in parity_checks' current operand
    type -> (device dict, oracle logits [L, B, nq, T] / boxes [L, B, nq, 4] built from the `hs` / `refs` of oracle/gdino.py's trace on the
    device's two-stage selection, per-image gts, per-image positive maps, text mask).  The tiny spec shares one `bbox_embed` over the
    decoder layers (dec_pred_bbox_embed_share), so this comparison pins the pairing of `hs[l]` with `refs[l]` but cannot notice a wrong
    layer index on the box head itself."""
    from dataclasses import replace

    import gdino_checks as gc
    import parity_checks as pc
    from oracle import gdino as og
    from oracle.spec import tiny_gdino_spec
    from oracle.weights import make_query_bank
    from mq_det_amd.structures import to_image_list
    from mq_det_amd.utils.tokenizer import positive_map_from_spans
    spec = replace(tiny_gdino_spec(), vision_query=True)
    sd, cfg, model = gc.gdino_model(dev, spec)
    if not cfg.VISION_QUERY.ENABLED:
        model._plan = None
    cfg.VISION_QUERY.ENABLED = True
    n_classes = 10
    caption, spans = gc._caption(n_classes)
    labels = list(range(1, n_classes + 1))
    pmap = positive_map_from_spans(model.tokenizer, caption + ".", spans, labels)
    bank = make_query_bank(labels, spec, seed=1, scales=1)
    model.query_selector.query_bank = {k: v.to(dev) for k, v in bank.items()}
    g = torch.Generator().manual_seed(11)
    img = torch.randn(3, 120, 150, generator=g).to(pc.H16).float()
    il = to_image_list([img], 32)
    sizes = [tuple(s) for s in il.image_sizes]
    tok = model.tokenizer([caption + "."], padding="max_length", return_tensors="pt")
    rng = np.random.default_rng(21)
    G = n_classes                                             # every label of the caption has a gt: the same vision queries as the eval forward
    gt = _boxes(rng, (G,))
    gl = torch.from_numpy(rng.permutation(n_classes)[:G] + 1).long()
    pm = torch.zeros(G, T_FULL)
    for r, lab in enumerate(gl.tolist()):
        pm[r, pmap[lab]] = 1.0
    t = BoxList(sr.xyxy(gt) * torch.tensor([[150.0, 120.0, 150.0, 120.0]]), (150, 120), mode="xyxy")
    t.add_field("normed_cxcy_boxes", gt)
    t.add_field("labels", gl)
    t.add_field("caption", caption)
    t.add_field("positive_map", pm)
    with torch.no_grad():
        ild = to_image_list([img.to(dev)], 32)
        tr = model(ild, captions=[caption], positive_map=pmap, return_raw=True)       # the device's two-stage selection (deterministic)
        out = model.forward_losses(ild, [t])
        o = og.forward({k: (v.to(pc.H16).float() if v.dtype.is_floating_point else v) for k, v in sd.items()}, spec, il.tensors, sizes,
                       tok["input_ids"], tok["attention_mask"], pmap, model.specical_tokens, bank, topk_override=tr["topk"].cpu())
    tmask = tok["attention_mask"][:, :spec.max_text_len].bool()
    L = spec.dec_layers
    ref_logits = torch.stack([og.contrastive_embed(o["hs"][l], o["memory_text"], tmask, spec.max_text_len) for l in range(L)])
    ref_boxes = torch.stack([(og._mlp(sd_f(sd, pc), f"bbox_embed.{l}", o["hs"][l], 3) + og.inverse_sigmoid(o["refs"][l])).sigmoid() for l in range(L)])
    gates = [v.float().reshape(-1)[0] for k, v in sd.items() if ".qv_layer." in k and k.endswith(".ff_gate")]
    want_gate = float(cfg.VISION_QUERY.GATE_REGULARIZATION_SCALE) * float(sum(1 - abs(float(x)) for x in gates)) / len(gates)
    return out, {"logits": ref_logits, "boxes": ref_boxes, "gt": [gt], "pm": [pm], "mask": tmask.int(), "loss_gate": want_gate}


def sd_f(sd, pc):
    return {k: (v.to(pc.H16).float() if v.dtype.is_floating_point else v) for k, v in sd.items()}


def check_end_to_end(out, want, gate=True):
    """`gate`: per-layer logits / boxes within 1e-3 + 1e-3 |ref| of the oracle (finite entries; -inf positions equal) and the device's losses
    within the same gate of the restatement's FOR THE DEVICE'S ASSIGNMENT on the oracle's outputs.  Always: finite losses, a valid assignment,
    optimal within 2 G eps on the device's own outputs.  -> the measured deviations"""
    lg = torch.stack([o["pred_logits"] for o in out["outputs"]["aux_outputs"]] + [out["outputs"]["pred_logits"]]).float().cpu()
    bx = torch.stack([o["pred_boxes"] for o in out["outputs"]["aux_outputs"]] + [out["outputs"]["pred_boxes"]]).float().cpu()
    L, B, nq, T = lg.shape
    fin = torch.isfinite(want["logits"])
    assert torch.equal(torch.isfinite(lg), fin)
    dev = {"logits": float(((lg - want["logits"])[fin].abs() / (1 + want["logits"][fin].abs())).max()),
           "boxes": float(((bx - want["boxes"]).abs() / (1 + want["boxes"].abs())).max())}
    counts = [len(g) for g in want["gt"]]
    match_q, q2g = out["match_q"].cpu(), out["q2g"].cpu()
    n = max(sum(counts), 1)
    for l in range(L):
        assert_valid_matching(match_q[l], q2g[l], counts, nq)
        own = torch.cat(sr.cost_ref(lg[l], bx[l], want["gt"], want["pm"], *COST, ALPHA)).numpy()
        mine, best = sr.total(own, match_q[l].numpy()), sr.total(own, sr.lsap(own))
        assert mine - best <= 2 * counts[0] * eps_of(torch.from_numpy(own)), (l, mine - best)
        idx = [indices_of_image(match_q[l], counts, b) for b in range(B)]
        sums = sr.sums_ref(want["logits"][l], want["boxes"][l], want["gt"], want["pm"], want["mask"], idx, ALPHA, GAMMA)
        sfx = "" if l == L - 1 else f"_{l}"
        for j, name in enumerate(("loss_ce", "loss_bbox", "loss_giou")):
            ref, got = sums[j] / n * COEF[j], float(out[name + sfx])
            dev[name + sfx] = abs(got - ref) / (1 + abs(ref))
            print(f"set_loss end_to_end {name + sfx}: dev {got:.6f} oracle {ref:.6f}")
            assert got == got and abs(got) != float("inf")
    assert abs(float(out["loss_gate"]) - want["loss_gate"]) <= 1e-6
    print("set_loss end_to_end deviations (|dev - ref| / (1 + |ref|)):", {k: f"{v:.2e}" for k, v in dev.items()})
    if gate:
        bad = {k: v for k, v in dev.items() if v > 1e-3}
        assert not bad, bad
    return dev


def indices_of_image(match_q_layer, counts, b):
    off = int(np.sum(counts[:b]))
    return sr.indices_of(match_q_layer[off:off + counts[b]].numpy())
