"""Test-time augmentation (mq_det_amd/tta.py, csrc/tta.hip) without a GPU.

The host pieces (config defaults, Resize.get_size, format resolution, BoxList.transpose) against tests/golden/tta_merge.json / .npz, which
tools/gen_golden_tta.py records by executing the reference's box_aug.py in place; the two kernels' SOURCES through the host emulation
(tests/simt): the ingest bit-exact to Pillow's resize + the reference's ToTensor / Normalize / to_image_list, the merge bit-exact to the
reference's merge of the same detections."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mq_det_amd import get_cfg, tta  # noqa: E402
from mq_det_amd.structures import BoxList  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta_merge")
_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD + ".json") as f:
        js = json.load(f)
    return js, dict(np.load(GOLD + ".npz"))


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def test_config_defaults_equal_the_reference(gold):
    js, _ = gold
    cfg = get_cfg()
    for k, v in js["defaults"].items():
        node, key = (cfg.INPUT, k.split(".")[1]) if k.startswith("INPUT.") else (cfg.TEST, k)
        got = node[key]
        got = [list(r) for r in got] if k == "RANGES" else list(got) if isinstance(got, tuple) else got
        assert got == v, k
    assert cfg.TEST.USE_MULTISCALE is False
    from mq_det_amd.config import get_gdino_cfg
    assert get_gdino_cfg().INPUT.FORMAT == "rgb"


def test_get_size_matches_the_reference(gold):
    js, _ = gold
    for w, h, s, m, oh, ow in js["get_size"]:
        assert tta.get_size((w, h), s, None if m < 0 else m) == (oh, ow), (w, h, s, m)


def test_input_format_resolution():
    cfg = get_cfg()
    assert tta.input_format(cfg) == "bgr255"
    cfg.INPUT.FORMAT = "RGB255"
    assert tta.input_format(cfg) == "rgb255"
    cfg.INPUT.FORMAT, cfg.INPUT.TO_BGR255 = "", False
    with pytest.raises(ValueError):
        tta.input_format(cfg)


def test_boxlist_transpose_and_resize_match_the_reference(gold):
    _, a = gold
    bl = BoxList(torch.from_numpy(a["box"]), tuple(int(v) for v in a["size"]))
    assert torch.equal(bl.transpose(0).bbox, torch.from_numpy(a["flip_lr"]))
    assert torch.equal(bl.transpose(1).bbox, torch.from_numpy(a["flip_tb"]))
    assert torch.equal(bl.resize((262, 194)).bbox, torch.from_numpy(a["resize_eq"]))
    assert torch.equal(bl.resize((200, 50)).bbox, torch.from_numpy(a["resize_ne"]))
    with pytest.raises(NotImplementedError):
        bl.transpose(2)


class _CountingModel:
    def __init__(self, cfg):
        self.cfg, self.calls = cfg, 0

    def __call__(self, *a, **k):
        self.calls += 1
        raise AssertionError("no forward may run")


@pytest.mark.parametrize("mode", ["soft-nms", "vote", "soft-vote"])
def test_unsupported_special_nms_is_refused_before_any_forward(mode):
    cfg = get_cfg()
    cfg.TEST.SPECIAL_NMS = mode
    m = _CountingModel(cfg)
    with pytest.raises(NotImplementedError, match="TEST.SPECIAL_NMS"):
        tta.im_detect_bbox_aug(m, [np.zeros((8, 8, 3), np.uint8)], "cpu")
    assert m.calls == 0


def test_groundingdino_is_refused():
    from mq_det_amd.config import get_gdino_cfg
    m = _CountingModel(get_gdino_cfg())
    with pytest.raises(NotImplementedError, match="GroundingDINO"):
        tta.im_detect_bbox_aug(m, [np.zeros((8, 8, 3), np.uint8)], "cpu")
    assert m.calls == 0


def test_pil_coefficients_match_pillow_one_axis():
    """pil_coeffs restated against Pillow itself on single-row / single-column images (one pass each)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for n_in, n_out in ((7, 56), (640, 400), (427, 1668), (100, 99), (13, 1), (1, 9), (2500, 333)):
        row = rng.integers(0, 256, (1, n_in, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(row).resize((n_out, 1), Image.BILINEAR))
        b, k = tta.pil_coeffs(n_in, n_out)
        acc = np.full((n_out, 3), 1 << 21, np.int64)
        for j in range(k.shape[1]):
            idx = np.minimum(b[:, 0] + j, n_in - 1)
            acc += row[0, idx].astype(np.int64) * np.where(j < b[:, 1], k[:, j], 0)[:, None]
        got = np.clip(acc >> 22, 0, 255).astype(np.uint8)
        assert np.array_equal(got, want[0]), (n_in, n_out)


def _pil_canvas(a, scale, max_size, flip, fmt, mean, std):
    """The reference's ingest of one image with Pillow: T.Resize (PIL BILINEAR), hflip, ToTensor, Normalize (torchvision's fp32 ops)."""
    from PIL import Image
    im = Image.fromarray(a)
    oh, ow = tta.get_size(im.size, scale, max_size)
    r = im.resize((ow, oh), Image.BILINEAR)
    if flip:
        r = r.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.array(r)).permute(2, 0, 1).contiguous().float().div(255)
    if "bgr" in fmt:
        t = t[[2, 1, 0]]
    if "255" in fmt:
        t = t * 255
    m, s = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
    return t.sub(m[:, None, None]).div(s[:, None, None])


@needs_simt
@pytest.mark.parametrize("fmt", ["bgr255", "rgb"])
def test_ingest_kernel_is_bit_exact_to_pillow(emu, fmt):
    """Ragged batch of odd sizes; up-scale x4, down-scale, a same-width and a same-size image (skipped passes); plain and flipped; zero
    padding up to /32; both formats."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(7)
    shapes = [(37, 53), (61, 29), (40, 40), (23, 71)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    imgs[2][:20] = 255                                      # saturated rows: the clamp
    cfg = get_cfg()
    if fmt == "rgb":
        cfg.INPUT.FORMAT, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD = "rgb", [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    up = tta.Upload(imgs, torch.device("cpu"))
    for scale, max_size in ((150, 2500), (23, 2500), (40, 2500), (29, 100), (61, 300)):
        plain, flipped, sizes = tta.ingest(up, scale, max_size, cfg, True)
        assert plain.shape[2] % 32 == 0 and plain.shape[3] % 32 == 0
        for b, a in enumerate(imgs):
            for fl, canvas in ((False, plain), (True, flipped)):
                want = _pil_canvas(a, scale, max_size, fl, tta.input_format(cfg), cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD)
                h, w = want.shape[1:]
                assert sizes[b] == (h, w)
                assert torch.equal(canvas[b, :, :h, :w], want), (scale, b, fl)
                assert not canvas[b, :, h:].any() and not canvas[b, :, :, w:].any()
    plain, none, _ = tta.ingest(up, 40, 2500, cfg, False)
    assert none is None


def _fixture_dets(js, a, name):
    case = js["cases"][name]
    packed = torch.from_numpy(a[f"{name}_packed"])
    n_scales = len(case["cfg"]["SCALES"])
    rngs = case["cfg"]["RANGES"] if len(case["cfg"]["RANGES"]) == n_scales else [None] * n_scales
    dets = []
    for t in range(packed.shape[0]):
        wh = [(w, h) for (h, w) in case["calls"][t]]
        dets.append((packed[t], case["counts"][t], wh, t % 2 == 1, rngs[t // 2]))
    cfg = get_cfg()
    for k, v in case["cfg"].items():
        cfg.TEST[k] = tuple(v) if isinstance(v, list) else v
    return cfg, dets, [tuple(wh) for wh in case["image_wh"]]


def nms_restated(boxes, scores, thresh):
    """_C.nms (csrc/cuda/nms.cu): score order, greedy, IoU > thresh with the legacy +1, kept indices ascending (nms.cu:138-142)."""
    n = boxes.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order]
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    lt = torch.max(b[:, None, :2], b[None, :, :2])
    rb = torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > thresh).numpy()
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= over[i, i + 1:]
    return torch.sort(order[torch.tensor(keep, dtype=torch.long)])[0]


def merge_restated(dets, orig_wh, cfg):
    """box_aug.py's merge, restated on host tensors in its own order (tests/golden pins this against the reference's code)."""
    out = []
    for b, (w, h) in enumerate(orig_wh):
        B_, S_, L_ = [], [], []
        for packed, counts, wh, fl, rng in dets:
            p = packed[b, :counts[b]]
            bx, sc, lb = p[:, :4].clone(), p[:, 4].clone(), p[:, 5].to(torch.int64)
            ws, hs = wh[b]
            if fl:
                bx = torch.stack([ws - bx[:, 2] - 1, bx[:, 1], ws - bx[:, 0] - 1, bx[:, 3]], 1)
            if rng is not None:
                ar = (bx[:, 2] - bx[:, 0] + 1) * (bx[:, 3] - bx[:, 1] + 1)
                k = (ar > rng[0] * rng[0]) & (ar < rng[1] * rng[1])
                bx, sc, lb = bx[k], sc[k], lb[k]
            rw, rh = float(w) / float(ws), float(h) / float(hs)
            bx = bx * torch.tensor([rw, rh, rw, rh], dtype=torch.float32)
            B_.append(bx), S_.append(sc), L_.append(lb)
        bx, sc, lb = torch.cat(B_), torch.cat(S_), torch.cat(L_)
        rb, rs, rl = [], [], []
        for j in tta.class_list(cfg):
            i = (lb == j).nonzero().view(-1)
            keep = nms_restated(bx[i], sc[i], cfg.TEST.TH) if cfg.TEST.TH > 0 else torch.arange(len(i))
            rb.append(bx[i][keep]), rs.append(sc[i][keep]), rl.append(torch.full((len(keep),), j, dtype=torch.int64))
        rb, rs, rl = torch.cat(rb), torch.cat(rs), torch.cat(rl)
        n, top = len(rs), cfg.TEST.PRE_NMS_TOP_N
        if n > top > 0:
            thr, _ = torch.kthvalue(rs, n - top + 1)
            k = rs >= thr.item()
            rb, rs, rl = rb[k], rs[k], rl[k]
        out.append((rb, rs, rl))
    return out


@needs_simt
@pytest.mark.parametrize("name", ["band", "noband", "unsorted"])
def test_merge_kernels_match_the_reference_merge(emu, gold, name):
    js, a = gold
    cfg, dets, orig_wh = _fixture_dets(js, a, name)
    with pytest.warns(UserWarning, match="outside TEST.SELECT_CLASSES"):
        tta._WARNED_CLASSES = False
        res = tta.merge(dets, orig_wh, cfg, torch.device("cpu"))
    assert [len(r) for r in res] == js["cases"][name]["out_counts"]
    for b, r in enumerate(res):
        assert r.size == orig_wh[b] and r.mode == "xyxy" and r.fields() == ["scores", "labels"]
        assert torch.equal(r.bbox, torch.from_numpy(a[f"{name}_boxes{b}"]))
        assert torch.equal(r.get_field("scores"), torch.from_numpy(a[f"{name}_scores{b}"]))
        assert torch.equal(r.get_field("labels"), torch.from_numpy(a[f"{name}_labels{b}"]))
    for b, (rb, rs, rl) in enumerate(merge_restated(dets, orig_wh, cfg)):       # the restatement the GPU test uses, pinned here
        assert torch.equal(rb, res[b].bbox) and torch.equal(rs, res[b].get_field("scores")) and torch.equal(rl, res[b].get_field("labels"))


def random_dets(seed, T, B, K, wh_orig, n_cls=12, dense=False):
    """Seeded per-transform detections with distinct scores (score-sorted rows like the model's) for the restated-merge checks."""
    g = np.random.default_rng(seed)
    dets = []
    pool = g.permutation(np.arange(1, T * B * K + 1)).astype(np.float32) / np.float32(1 << 20)
    for t in range(T):
        packed = np.zeros((B, K, 6), np.float32)
        counts, wh = [], []
        for b, (w, h) in enumerate(wh_orig):
            s = [1.0, 1.5, 0.75, 2.0][t // 2 % 4]
            ws, hs = int(w * s), int(h * s)
            n = K if dense else int(g.integers(K // 2, K + 1))
            x1, y1 = g.uniform(0, 0.8 * ws, n), g.uniform(0, 0.8 * hs, n)
            rows = np.stack([x1, y1, x1 + g.uniform(2, 0.3 * ws, n), y1 + g.uniform(2, 0.3 * hs, n)], 1)
            sc = pool[(t * B + b) * K:(t * B + b) * K + n]
            lab = g.integers(0, n_cls, n)
            o = np.argsort(-sc, kind="stable")
            packed[b, :n] = np.concatenate([rows[o], sc[o, None], lab[o, None]], 1)
            counts.append(n)
            wh.append((ws, hs))
        dets.append((torch.from_numpy(packed), counts, wh, t % 2 == 1, [(0, 10000), (32, 10000), (0, 300), (16, 500)][t // 2 % 4]))
    return dets


@needs_simt
def test_merge_kernels_match_the_restated_merge_on_random_rows(emu):
    cfg = get_cfg()
    cfg.TEST.PRE_NMS_TOP_N, cfg.TEST.NUM_CLASSES = 150, 9
    wh = [(640, 480), (375, 500), (200, 333)]
    dets = random_dets(21, 8, len(wh), 120, wh)
    res = tta.merge(dets, wh, cfg, torch.device("cpu"))
    for b, (rb, rs, rl) in enumerate(merge_restated(dets, wh, cfg)):
        assert len(rs) == len(res[b]) > 0
        assert torch.equal(rb, res[b].bbox) and torch.equal(rs, res[b].get_field("scores")) and torch.equal(rl, res[b].get_field("labels"))


def test_repeated_classes_and_too_many_rows_are_refused_before_any_forward():
    cfg = get_cfg()
    cfg.TEST.SELECT_CLASSES = (3, 1, 3)
    m = _CountingModel(cfg)
    with pytest.raises(NotImplementedError, match="repeats a class"):
        tta.im_detect_bbox_aug(m, [np.zeros((8, 8, 3), np.uint8)], "cpu")
    cfg = get_cfg()
    cfg.MODEL.ATSS.DETECTIONS_PER_IMG = 700                 # 24 transforms x (700 + 16) rows > 16 384
    m = _CountingModel(cfg)
    with pytest.raises(ValueError, match="exceed"):
        tta.im_detect_bbox_aug(m, [np.zeros((8, 8, 3), np.uint8)], "cpu")
    assert m.calls == 0
