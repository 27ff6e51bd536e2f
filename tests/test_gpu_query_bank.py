"""The device-resident vision-query bank on the MI355X (mq_det_amd.query_bank, csrc/query_bank.hip): the reference fixture, two large shapes
against the dict path of `pool_into_bank` on the same device tensors, NaN halos around every buffer, `extract_query(query_images=QueryBank)`
from pixels on the tiny MQ-GLIP and MQ-GroundingDINO models, and one `online_update` turn on the tiny model.  Every test runs its body in a
process of its own under a time limit (a fault or a hang fails that test, not the session)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))

import query_bank_ref as qr  # noqa: E402
import test_query_bank_cpu as tc  # noqa: E402
from mq_det_amd.query_bank import QueryBank, online_update  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]
DEV = torch.device("cuda:0")


def clustered_fast(seed, n, C, n_labels, centres=8, skew=0):
    """n candidates [n, 1, C] around per-label centres, small or large noise, 10 % exact copies of the previous candidate of the label's
    cluster (vectorised tests/query_bank_ref.py clustered); skew: this many extra candidates of label 0 in front of the rest"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, n_labels, n)
    if skew:
        labels[rng.choice(n, skew, replace=False)] = 0
    which = rng.integers(0, centres, n)
    cen = rng.standard_normal((n_labels, centres, C))
    cen /= np.linalg.norm(cen, axis=-1, keepdims=True)
    sigma = np.where(rng.random(n) < 0.6, 0.18, 1.3) / np.sqrt(C)
    x = (cen[labels, which] + rng.standard_normal((n, C)) * sigma[:, None]) * rng.uniform(0.5, 4.0, n)[:, None]
    x = x.astype(np.float32)
    dup = np.nonzero(rng.random(n) < 0.1)[0]
    dup = dup[dup > 0]
    x[dup], labels[dup] = x[dup - 1], labels[dup - 1]
    return torch.from_numpy(x[:, None]), torch.from_numpy(labels.astype(np.int64))


def against_dict_path(feats, labels, chunk, maxq, exclude, thr=0.85, check_margin=True):
    """`chunk` candidates per call on a QueryBank and on a dict, same device tensors -> (bank, admitted)"""
    if check_margin and exclude:
        calls = [{"lo": lo, "hi": min(lo + chunk, len(feats)), "exclude": True, "maxq": maxq} for lo in range(0, len(feats), chunk)]
        _, dmin, above, below = qr.replay(feats, labels, calls, thr)
        print(f"margin condition: {above} comparisons above, {below} below the threshold, smallest distance {dmin:.3g}", flush=True)
        assert dmin >= qr.MARGIN and above > 0 and below > 0
    f, l = feats.to(DEV), labels.to(DEV)
    bank, plain, admitted = QueryBank(DEV), {}, 0
    for lo in range(0, len(f), chunk):
        admitted += bank.update(f[lo:lo + chunk], l[lo:lo + chunk], maxq, exclude, thr)
        plain = tc.dict_path(f[lo:lo + chunk], l[lo:lo + chunk], plain, exclude, maxq, thr)
    got = bank.to_dict()
    assert all(v.is_cuda for v in got.values())
    tc.same_bank(got, plain)
    assert admitted == sum(len(v) for v in plain.values()) == bank.rows
    return bank, plain


def _body_fixture():
    for name in ("sel_exclude", "sel_plain", "all_plain", "sel_mixed"):
        bank = tc.check_fixture_case(name, DEV)
        assert bank.pool.is_cuda
    tc.exact_cases(DEV)
    print("OK fixture cases and exact cases on the device", flush=True)


def _body_large_exclude():
    feats, labels = clustered_fast(21, 4096, 256, 64)
    bank, plain = against_dict_path(feats, labels, 512, 100, True)
    n = [len(v) for v in plain.values()]
    print(f"OK 4096 candidates x 64 labels x capacity 100 with exclusion: {sum(n)} rows admitted, {min(n)} .. {max(n)} per label", flush=True)


def _body_large_plain():
    feats, labels = clustered_fast(22, 60000, 256, 365, skew=6000)
    bank, plain = against_dict_path(feats, labels, 15000, 5000, False)
    n = [len(v) for v in plain.values()]
    assert max(n) == 5000 and len(plain) == 365                 # label 0 reached the capacity in the middle of a call
    print(f"OK 60000 candidates x 365 labels x capacity 5000 without exclusion: {sum(n)} rows, {min(n)} .. {max(n)} per label", flush=True)


def _body_halo():
    from halo import poisoned_args
    with poisoned_args("nan"):
        for name in ("sel_exclude", "all_plain", "sel_mixed"):
            tc.check_fixture_case(name, DEV)
        tc.exact_cases(DEV)
        feats, labels = clustered_fast(23, 1024, 256, 16)
        against_dict_path(feats, labels, 256, 40, True)
        feats, labels = clustered_fast(24, 600, 36, 7)           # 36 floats per row: the 16-byte path with a partial wave
        against_dict_path(feats, labels, 200, 30, True)
    print("OK under NaN halos", flush=True)


def _extract_both(model, kwargs, exclude):
    from collections import defaultdict
    plain = model.extract_query(query_images=defaultdict(list), **kwargs)
    bank = model.extract_query(query_images=QueryBank(DEV), **kwargs)
    assert isinstance(bank, QueryBank)
    tc.same_bank(bank.to_dict(), {k: v for k, v in plain.items() if torch.is_tensor(v)})
    # a second pass over the same boxes with exclusion: the same decisions on both paths
    plain2 = model.extract_query(query_images={k: v.clone() for k, v in plain.items()}, exclude_similar=exclude, **kwargs)
    bank2 = model.extract_query(query_images=bank, exclude_similar=exclude, **kwargs)
    tc.same_bank(bank2.to_dict(), plain2)
    return plain2


def _body_extract_glip():
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    spec, sd, cfg, model, P = pc.tiny(DEV)
    images, sizes, ids, am, pm, bank = pc.make_inputs(spec)
    bl, _ = pc._query_targets(sizes, DEV)
    out = _extract_both(model, dict(images=ImageList(images.to(DEV), sizes), targets=bl), True)
    assert sorted(out) == [1, 2, 3]
    print("OK extract_query from pixels, tiny MQ-GLIP:", {k: tuple(v.shape) for k, v in out.items()}, flush=True)


def _body_extract_gdino():
    import gdino_checks as gc
    from oracle.spec import tiny_gdino_spec
    from mq_det_amd.structures import BoxList, to_image_list
    sd, cfg, model = gc.gdino_model(DEV, tiny_gdino_spec())
    g = torch.Generator().manual_seed(11)
    il = to_image_list([torch.randn(3, 120, 150, generator=g).to(DEV)], 32)
    t = BoxList(torch.tensor([[10.0, 12.0, 80.0, 90.0], [30.0, 20.0, 140.0, 110.0], [12.0, 11.0, 82.0, 91.0]], device=DEV), (150, 120), mode="xyxy")
    t.add_field("labels", torch.tensor([2, 5, 2], device=DEV))
    out = _extract_both(model, dict(samples=il, targets=[t]), True)
    assert sorted(out) == [2, 5]
    print("OK extract_query from pixels, tiny MQ-GroundingDINO:", {k: tuple(v.shape) for k, v in out.items()}, flush=True)


def _body_online():
    """one online_update turn on the tiny MQ-GLIP model: the saved file loads, and the next forward selects its vision queries from it"""
    import tempfile
    import parity_checks as pc
    from mq_det_amd.structures import ImageList
    spec, sd, cfg, model, P = pc.tiny(DEV)
    images, sizes, ids, am, pm, bank0 = pc.make_inputs(spec)
    kv = int(am[0].sum())
    model.tokenize = lambda caps, dev: (ids[:1].expand(len(caps), -1).contiguous().to(dev), am[:1].expand(len(caps), -1).contiguous().to(dev), kv)
    model.load_query_bank(bank0)
    il = ImageList(images.to(DEV), sizes)
    with torch.no_grad():
        before = model(il, captions=["caption a"] * len(sizes), positive_map=pm)
    scores = torch.cat([o.get_field("scores") for o in before])
    assert len(scores) > 4
    saved = (cfg.VISION_QUERY.get("SCORE_THRESHOLD"), cfg.VISION_QUERY.get("MAX_TEST_QUERY_NUMBER"), cfg.TEST.get("SUBSET"), cfg.VISION_QUERY.QUERY_BANK_PATH)
    cfg.VISION_QUERY.SCORE_THRESHOLD = float(scores.sort().values[len(scores) // 2])          # the better half is kept (strict)
    cfg.VISION_QUERY.MAX_TEST_QUERY_NUMBER, cfg.TEST.SUBSET, cfg.VISION_QUERY.QUERY_BANK_PATH = 3, -1, ""
    try:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "online.pth")
            loader = [(il, [None] * len(sizes), list(range(len(sizes))))]
            out = online_update(model, loader, device=DEV, cfg=cfg, num_turns=1, save_name=path,
                                queries_and_maps=(["caption a", "caption b"], [pm, pm]))
            assert out is model
            new = torch.load(path, map_location="cpu")
            n_kept = int((scores > cfg.VISION_QUERY.SCORE_THRESHOLD).sum())
            assert 0 < sum(len(v) for v in new.values()) <= 2 * n_kept and all(len(v) <= 3 and v.shape[1:] == (1, 256) for v in new.values())
            assert set(new) <= set(torch.cat([o.get_field("labels") for o in before]).tolist())
            model.load_query_bank(path)
            lab = sorted(new)[0]
            rows = model.query_selector._rows(lab, DEV, torch.float32)
            assert torch.equal(rows.cpu(), new[lab][:cfg.VISION_QUERY.NUM_QUERY_PER_CLASS].flatten(0, 1))
            assert not torch.equal(rows.cpu()[:1], bank0[lab][:1].flatten(0, 1).float())
            with torch.no_grad():
                after = model(il, captions=["caption a"] * len(sizes), positive_map=pm)
            changed = any(len(a) != len(b) or not torch.equal(a.get_field("scores"), b.get_field("scores")) for a, b in zip(after, before))
            assert changed                                         # other vision queries, other detections
    finally:
        cfg.VISION_QUERY.SCORE_THRESHOLD, cfg.VISION_QUERY.MAX_TEST_QUERY_NUMBER, cfg.TEST.SUBSET, cfg.VISION_QUERY.QUERY_BANK_PATH = saved
    print("OK online_update turn on the tiny model:", {k: len(v) for k, v in new.items()}, flush=True)


def _run(body, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), body], capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    assert r.returncode == 0, f"{body}: rc {r.returncode}\n{out[-4000:]}"
    return out


def test_fixture_and_exact_cases_on_device():
    _run("fixture", 300)


def test_4096_candidates_64_labels_with_exclusion_equal_the_dict_path():
    print(_run("large_exclude", 600)[-1500:])


def test_365_labels_capacity_5000_without_exclusion_equal_the_dict_path():
    print(_run("large_plain", 900)[-1500:])


def test_under_nan_halos():
    _run("halo", 600)


def test_extract_query_from_pixels_tiny_mq_glip_equals_the_dict_call():
    _run("extract_glip", 600)


def test_extract_query_from_pixels_tiny_mq_groundingdino_equals_the_dict_call():
    _run("extract_gdino", 600)


def test_online_update_turn_on_the_tiny_model():
    _run("online", 600)


if __name__ == "__main__":
    globals()["_body_" + sys.argv[1]]()
