"""TEST INFRASTRUCTURE shared by tests/test_atss_loss_cpu.py (kernel sources through tests/simt) and tests/test_gpu_atss_loss.py (the device):
the fixture cases of tests/golden/atss_loss (tools/gen_golden_atss_loss.py: the reference's own loss code, run in place), rebuilt into the
arguments of mq_det_amd.losses, and the gates the issue sets.

Gates.  Box and centerness losses: within 1e-5 relative of the reference's fp32 value (sums of at most a few thousand well-conditioned
positive terms; a tree sum adds log2(n) 2^-24).  Token loss: with L64 = the formula in fp64 on fp64 products of the SAME rounded operands and
Lref = the reference's function on a torch fp32 bmm, |Ldev - L64| <= max(4 |Lref - L64|, 1e-5 L64) -- the floor is a few-ulp exp / log plus
the tree sum over non-negative terms, the factor 4 allows for another accumulation order in the 256-term dot products."""
import json
import os

import numpy as np
import torch

import atss_loss_ref as ar
from mq_det_amd.config import get_cfg
from mq_det_amd.structures import BoxList

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "atss_loss", "cases")
NAMES = ("main", "tiny", "full", "alpha_neg")
BOX_RTOL = 1e-5
_FIX = None


def fixture():
    global _FIX
    if _FIX is None:
        with open(GOLD + ".json") as f:
            _FIX = (json.load(f), dict(np.load(GOLD + ".npz")))
    return _FIX


class Case:
    """One fixture case on `device` with its operands in `dtype` (the kernels' operand type: fp16 / bf16, or fp32 in the precise mode)."""

    def __init__(self, name, device="cpu", dtype=torch.float16):
        js, a = fixture()
        self.name, self.meta = name, js["cases"][name]
        self.sizes = [tuple(s) for s in js["sizes"]]
        self.t_full = js["t_full"]
        H, W = js["canvas"]
        m = self.meta
        self.B = len(m["counts"])
        self.levels = ar.grid_anchors(self.sizes, torch.from_numpy(a[name + "_cells"]), device=device)
        self.A = sum(h * w for h, w in self.sizes)
        gt, labels = torch.from_numpy(a[name + "_gt"]), torch.from_numpy(a[name + "_labels"])
        pm = torch.zeros(len(gt), self.t_full)
        idx = torch.from_numpy(a[name + "_pm_idx"]).long()
        pm[idx[:, 0], idx[:, 1]] = torch.from_numpy(a[name + "_pm_val"])
        self.pm = pm.to(device)
        self.gts, self.labels, self.pms, self.targets = [], [], [], []
        off = 0
        for n in m["counts"]:
            self.gts.append(gt[off:off + n].to(device))
            self.labels.append(labels[off:off + n].to(device))
            self.pms.append(self.pm[off:off + n])
            t = BoxList(self.gts[-1], (W, H), mode="xyxy")
            t.add_field("labels", self.labels[-1])
            self.targets.append(t)
            off += n
        self.mask = torch.from_numpy(a[name + "_mask"]).long().to(device)
        draws = ar.head_draws(m["head_seed"], self.B, self.A, self.t_full)
        assert ar.checksum(draws) == m["checksum"], "the integer draws of the head outputs drifted"
        self.draws = {k: torch.from_numpy(v).to(device) for k, v in draws.items()}
        for k in ("tok", "tk"):                                 # exact in every operand type: small integers over powers of two
            assert torch.equal(self.draws[k].to(dtype).float(), self.draws[k])
        self.dtype = dtype
        self.ref_matched = torch.from_numpy(a[name + "_matched"]).to(device)
        self.ref_cls = torch.from_numpy(a[name + "_cls"]).long().to(device)
        self.ref_reg = torch.from_numpy(a[name + "_reg"]).to(device)

    def assert_conditions(self):
        """the four conditions, recomputed in fp64 on the data as it is here"""
        ok, worst = ar.conditions_hold([l.cpu() for l in self.levels], [g.cpu() for g in self.gts], self.meta["topk"])
        assert ok, (self.name, worst)
        for k, v in worst.items():
            rec = self.meta["margins"][k]
            assert v == rec or abs(v - rec) <= 1e-9 * max(1.0, abs(rec)), (k, v, rec)

    def cfg(self):
        cfg = get_cfg()
        cfg.MODEL.DYHEAD.FUSE_CONFIG.TOKEN_ALPHA = self.meta["alpha"]
        cfg.MODEL.DYHEAD.FUSE_CONFIG.TOKEN_GAMMA = self.meta["gamma"]
        cfg.MODEL.ATSS.TOPK, cfg.MODEL.ATSS.REG_LOSS_WEIGHT = self.meta["topk"], self.meta["reg_weight"]
        return cfg

    def head(self, compact=True):
        """the head dict ATSSLoss takes: fused operands + the box outputs; compact: only the first 16 ceil(live / 16) text positions, as the
        live-token compaction of the model hands them over (the positive map keeps its full width)"""
        live = self.meta["live"]
        T = min(self.t_full, -(-live // 16) * 16) if compact else self.t_full
        d = self.draws
        return {"tok": d["tok"].to(self.dtype).contiguous(), "tk16": d["tk"][:, :T].to(self.dtype).contiguous(), "tbias": d["tbias"][:, :T].contiguous(),
                "max_kv": live, "reg": d["reg"], "ctr": d["ctr"], "sizes": self.sizes}

    def token_labels(self, matched):
        """dense [B, A, T] token labels from row indices: the positive-map row of the matched gt, the background row for -1"""
        return torch.stack([ar.token_targets_image(matched[b].long(), self.pms[b], self.t_full) for b in range(self.B)])

    def l64(self):
        """the normalised token loss in fp64 on fp64 products of the operands, with the reference's assignment"""
        d = self.draws
        logits = ar.logits_of(d["tok"].double(), d["tk"].double(), d["tbias"].double(), torch.float64)
        tot = 0.0
        for b in range(self.B):
            tgt = ar.token_targets_image(self.ref_matched[b].long(), self.pms[b].double(), self.t_full)
            tot += float(ar.token_loss_image(logits[b], tgt, self.mask[b], self.meta["alpha"], self.meta["gamma"]))
        return tot / max(self.meta["num_pos"], 1)


def check_targets(case, prepare_targets):
    """assignment, labels and token-label rows EQUAL to the reference's; regression targets within 1e-6 + 1e-6 |ref|"""
    from mq_det_amd import losses
    case.assert_conditions()
    matched, _ = losses.assign(case.targets, case.levels, case.meta["topk"])
    assert matched.dtype == torch.int32 and torch.equal(matched, case.ref_matched), (case.name, int((matched != case.ref_matched).sum()))
    cls, reg, tok = prepare_targets(case.targets, case.levels, case.pm, topk=case.meta["topk"])
    assert len(cls) == len(reg) == len(tok) == case.B
    want_tok = case.token_labels(case.ref_matched)
    for b in range(case.B):
        assert cls[b].dtype == torch.int64 and cls[b].shape == (case.A,) and torch.equal(cls[b], case.ref_cls[b])
        assert reg[b].dtype == torch.float32 and reg[b].shape == (case.A, 4)
        err = (reg[b] - case.ref_reg[b]).abs()
        assert bool((err <= 1e-6 + 1e-6 * case.ref_reg[b].abs()).all()), (case.name, b, float(err.max()))
        assert tok[b].dtype == torch.float32 and tok[b].shape == (case.A, case.t_full) and torch.equal(tok[b], want_tok[b])
    return matched


def check_losses(case, compact=True, report=None):
    """ATSSLoss on the case against the reference's returned losses, at the gates above -> the output dict (tensors on the device)"""
    from mq_det_amd.losses import ATSSLoss
    out = ATSSLoss(case.cfg())(case.head(compact), case.levels, case.targets, case.pm, case.mask)
    ref = case.meta["losses"]
    assert torch.equal(out["matched"], case.ref_matched)
    sums = out["sums"].tolist()
    assert int(sums[0]) == case.meta["num_pos"] and float(out["loss_cls"]) == 0.0
    l64 = case.l64()
    dev_tok, ref_tok = float(out["loss_dot_product_token"]), ref["loss_dot_product_token"]
    fig = {"case": case.name, "dtype": str(case.dtype), "loss_reg": (float(out["loss_reg"]), ref["loss_reg"]),
           "loss_centerness": (float(out["loss_centerness"]), ref["loss_centerness"]), "token_dev_rel": abs(dev_tok - l64) / l64,
           "token_ref_rel": abs(ref_tok - l64) / l64}
    print("atss_loss", json.dumps(fig))
    if report is not None:
        report.append(fig)
    for k in ("loss_reg", "loss_centerness"):
        assert abs(float(out[k]) - ref[k]) <= BOX_RTOL * abs(ref[k]), (case.name, k, float(out[k]), ref[k])
    assert abs(dev_tok - l64) <= max(4 * abs(ref_tok - l64), 1e-5 * l64), (case.name, dev_tok, ref_tok, l64)
    return out


# ------------------------------------------------------------------------------------------------ random shapes beyond the fixtures
# (canvas, text positions T, positive-map width, live tokens, box seed): the levels of a 256 x 320 and of an 800 x 1333 canvas, per batch four
# images of G = 0, 1, 33 and 200 boxes.  T = 8: a whole caption shorter than one 16-column block (the background column is live);
# T = 136 under a 256-wide map: live-token compaction with a partial last block; T = 256: two LDS chunks of text rows.
# The box seeds are the first (seed, seed + 1000, ...) at which the four conditions hold in fp64 with every drawn box kept (RandomCase asserts them).
RANDOM_COUNTS = (0, 1, 33, 200)
RANDOM_CASES = {"256x320-T8": ((256, 320), 8, 8, 8, 11), "256x320-T136": ((256, 320), 136, 256, 130, 12), "256x320-T256": ((256, 320), 256, 256, 256, 13),
                "800x1333-T136": ((800, 1333), 136, 256, 130, 14), "800x1333-T256": ((800, 1333), 256, 256, 256, 1015)}


class RandomCase:
    def __init__(self, name, device="cpu", dtype=torch.float16, check=True):
        (H, W), T, Tpm, live, seed = RANDOM_CASES[name]
        self.name, self.T, self.t_full, self.live, self.dtype = name, T, Tpm, live, dtype
        self.sizes = ar.level_sizes(H, W)
        self.levels = ar.grid_anchors(self.sizes, ar.cell_anchors(), device=device)
        self.A = sum(h * w for h, w in self.sizes)
        self.B = len(RANDOM_COUNTS)
        rng = np.random.default_rng(seed)
        self.gts, self.labels, self.pms, self.targets = [], [], [], []
        for n in RANDOM_COUNTS:
            box = torch.from_numpy(ar.draw_boxes(rng, n, W, H, lo=10.0, hi=0.7))
            lab = torch.from_numpy(rng.integers(1, 41, n).astype(np.int64))
            pm = torch.zeros(n, Tpm)
            for j in range(n):
                span = int(rng.integers(1, 4))
                start = int(rng.integers(0, max(1, live - span)))
                pm[j, start:start + span] = 1.0 / span
            self.gts.append(box.to(device))
            self.labels.append(lab.to(device))
            self.pms.append(pm.to(device))
            t = BoxList(self.gts[-1], (W, H), mode="xyxy")
            t.add_field("labels", self.labels[-1])
            self.targets.append(t)
        self.pm = torch.cat(self.pms)
        if check:
            ok, worst = ar.conditions_hold([l.cpu() for l in self.levels], [g.cpu() for g in self.gts])
            assert ok, (name, worst)
        self.mask = torch.zeros(self.B, T, dtype=torch.int64, device=device)
        self.mask[:, :live] = 1
        self.mask[1, live // 2:] = 0                            # one image with a shorter caption
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
        # operands rounded ONCE to the kernel's operand type; everything downstream (fp64, fp32 bmm, kernel) starts from these values
        self.tok = (0.6 * rnd(self.B, self.A, 256)).to(dtype).to(device)
        self.tk = (0.12 * rnd(self.B, T, 256)).to(dtype).to(device)
        self.tbias = (-1.5 + 0.5 * rnd(self.B, T)).to(device)
        self.reg = (0.8 * rnd(self.B, self.A, 4)).to(device)
        self.ctr = (1.5 * rnd(self.B, self.A)).to(device)

    def head(self):
        return {"tok": self.tok.contiguous(), "tk16": self.tk.contiguous(), "tbias": self.tbias.contiguous(), "max_kv": self.live, "reg": self.reg,
                "ctr": self.ctr, "sizes": self.sizes}

    def restated(self, dtype, matched=None):
        logits = ar.logits_of(self.tok, self.tk, self.tbias, dtype)
        return ar.losses_ref([l.to(dtype) for l in self.levels], [g.to(dtype) for g in self.gts], self.labels, [p.to(dtype) for p in self.pms],
                             self.reg.to(dtype), self.ctr.to(dtype), logits, self.mask, 0.25, 2.0, matched=matched)


def check_random(case, report=None):
    """ATSSLoss on a random case against the from-scratch restatement run on the same device: assignment and positives equal, box terms
    within 1e-5 of the restatement's fp32 value, the token loss at the three-number gate"""
    from mq_det_amd.losses import ATSSLoss
    out = ATSSLoss(get_cfg())(case.head(), case.levels, case.targets, case.pm, case.mask)
    ref = case.restated(torch.float32)
    for b in range(case.B):
        assert torch.equal(out["matched"][b].long(), ref["matched"][b]), (case.name, b)
    assert bool((out["matched"][0] == -1).all())
    r64 = case.restated(torch.float64, matched=ref["matched"])
    assert int(out["sums"][0]) == ref["num_pos"] == r64["num_pos"] > 0
    l64, lref, ldev = r64["loss_dot_product_token"], ref["loss_dot_product_token"], float(out["loss_dot_product_token"])
    fig = {"case": case.name, "dtype": str(case.dtype), "num_pos": ref["num_pos"], "loss_reg": (float(out["loss_reg"]), ref["loss_reg"]),
           "loss_centerness": (float(out["loss_centerness"]), ref["loss_centerness"]), "token_dev_rel": abs(ldev - l64) / l64,
           "token_ref_rel": abs(lref - l64) / l64}
    print("atss_loss", json.dumps(fig))
    if report is not None:
        report.append(fig)
    for k in ("loss_reg", "loss_centerness"):
        assert abs(float(out[k]) - ref[k]) <= BOX_RTOL * abs(ref[k]), (case.name, k, float(out[k]), ref[k], r64[k])
    assert abs(ldev - l64) <= max(4 * abs(lref - l64), 1e-5 * l64), (case.name, ldev, lref, l64)
    return out


# ------------------------------------------------------------------------------------------------ end to end on the tiny model of the parity ladders
def targets_for(sizes, pm, seed=0):
    """one gt box per label of the caption's positive map `pm` ({label: token positions}: the vision queries of the forward are then the
    oracle's) per image, with generic fractional corners, and their positive-map rows over MAX_QUERY_LEN = 256"""
    targets, rows = [], []
    rng = np.random.default_rng(seed)
    for (h, w) in sizes:
        box = torch.from_numpy(ar.draw_boxes(rng, len(pm), w, h, lo=20.0, hi=0.6))
        t = BoxList(box, (w, h), mode="xyxy")
        t.add_field("labels", torch.tensor(list(pm)))
        targets.append(t)
        for lab in pm:
            r = torch.zeros(256)
            r[pm[lab]] = 1.0 / len(pm[lab])
            rows.append(r)
    return targets, torch.stack(rows)


def end_to_end(dev, dtype, switch=True):
    """forward_losses of the tiny model in `dtype` and the restatement on the fp32 oracle's head outputs -> (device dict, expected dict).
    switch False: parity_checks is in `dtype` already and stays there (the emulation fixture of tests/test_simt_fp32_operands_cpu.py)"""
    import parity_checks as pc
    from oracle import detector as od
    from mq_det_amd.structures import ImageList
    if switch:
        pc.use_dtype(dtype)
    try:
        spec, sd, cfg, model, P = pc.tiny(dev)
        images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
        model.load_query_bank(bank)
        targets, pmt = targets_for(sizes, pm)
        with torch.no_grad():
            _, inter = od.forward(sd, spec, images, sizes, ids, am, pm, bank, return_intermediates=True)
            out = model.forward_losses(ImageList(images.to(dev), sizes), targets, positive_map=pmt, input_ids=ids.to(dev), attention_mask=am.to(dev))
        h = inter["head"]
        B = images.shape[0]
        fsz = [tuple(r.shape[-2:]) for r in h["bbox_reg"]]
        levels = [a.cpu() for a in model._anchors([torch.zeros(1, 1, *s, device=dev) for s in fsz])]
        reg = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, 4) for r in h["bbox_reg"]], 1).float()
        ctr = torch.cat([c.permute(0, 2, 3, 1).reshape(B, -1) for c in h["centerness"]], 1).float()
        logits = torch.cat(list(h["dot_product_logits"]), 1).float()
        ok, worst = ar.conditions_hold(levels, [t.bbox for t in targets])
        assert ok, worst
        want = ar.losses_ref(levels, [t.bbox for t in targets], [t.get_field("labels") for t in targets], [pmt[len(pm) * b:len(pm) * (b + 1)] for b in range(B)],
                             reg, ctr, logits, am, 0.25, 2.0)
        return out, want
    finally:
        if switch:
            pc.use_dtype(torch.float16)
