"""The random-shape sweep of the TEST.SPECIAL_NMS = 'soft-nms' / 'vote' / 'soft-vote' merges without a GPU: one round of
tests/tta_special_draws.py per mode through the host emulation of the kernel SOURCES (tests/simt) against the numpy restatement
(tests/tta_special_ref.py) by the rules of tta_special_cases.compare -- classes past one wave (65 .. 255 rows) and past one 256-row trip
(257, 300, 513), images of more than one and more than two 256-row tiles, the workspace behind a large class, every position of the
top-N cut.  tests/test_gpu_tta_special_sweep.py runs the same draws, and more rounds behind them, on the MI355X.

Mutation check (on a scratch copy of csrc/tta.hip, never committed; the suite before this file passed under all four):
  soft-NMS cross-wave pick reads red_k[0] for red_k[w]      fails soft-nms draw 0 (the 300-row class: the pick of a wave other than 0 is lost)
  red_d[q][3] dropped from the voted sum                    fails vote and soft-vote draw 0 (a cluster of the 300-row class with a member in wave 3)
  tta_cut_rank_kernel: total > top_n  ->  total >= top_n    changes NO output row: with exactly top_n rows kept the threshold becomes the lowest
                                                            kept score, which keeps them all.  Only thr itself tells ("-inf: no cut"), and
                                                            test_cut_threshold_contract_over_several_tiles reads it: fails at top_n == total
  staging prefix starts at 0 instead of `run`               fails draw 0 of every mode (rows of the second 256-row trip land on the first's slots)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tta_special_draws as sd  # noqa: E402
import tta_special_ref as ref  # noqa: E402
from mq_det_amd import tta  # noqa: E402

_CXX = os.environ.get("SIMT_CXX", "/opt/rocm/lib/llvm/bin/clang++")
needs_simt = pytest.mark.skipif(not os.path.exists(_CXX), reason=f"{_CXX} not found: the kernel-source emulation cannot be built here")
CPU = torch.device("cpu")
_ROUND = {}


def round0(mode):
    """the first round of `mode`, drawn once (and counted once in sd.STATS) and never modified"""
    if mode not in _ROUND:
        _ROUND[mode] = list(sd.cases(mode, 1))
    return _ROUND[mode]


@pytest.fixture(scope="module")
def emu():
    import simt
    with simt.installed() as ops:
        yield ops


def _sizes(case):
    """live rows per (image, class-list position), counted from the restated rows"""
    out = []
    for bx, s, lb in case["rows"]:
        ok = ~np.isnan(s)
        out.append(tuple(int((lb[ok] == c).sum()) for c in case["classes"]))
    return out


def round_features(mode, cases):
    """What tta_special_draws promises of every round, read from the restated rows and the restated reference alone."""
    sizes_seen, n_seen, cuts, ws, behind, ties = set(), [], set(), set(), False, 0
    flips, bands, Ts, Bs, members = set(), set(), set(), set(), {"r": 0, "o": 0, "a": 0}
    for c in cases:
        sizes = _sizes(c)
        assert sizes == [tuple(s) for s in c["sizes"]], c["what"]
        cl = c["classes"]
        assert list(cl) != sorted(cl) and len(set(cl)) == len(cl), c["what"]
        assert any(all(s[p] == 0 for s in sizes) for p in range(len(cl))), f"{c['what']}: no label without rows"
        for (bx, s, lb), sz in zip(c["rows"], sizes):
            assert int(np.isnan(s).sum()) == 1, c["what"]
            out = lb[~np.isin(lb, cl)]
            assert (out < max(cl)).any() and (out > max(cl)).any(), f"{c['what']}: labels outside the list, below and above its largest"
            for k in np.unique(lb):
                assert ref._distinct(s[(lb == k) & ~np.isnan(s)])
            n_seen.append(sum(sz))
            if c["plan"] in (1, 2, 3, 4, 5):                       # (no 300-row class: the image ends at or next to a multiple of 256)
                assert min(sum(sz) % 256, -sum(sz) % 256) <= 1, (c["what"], sum(sz))
            sizes_seen.update(sz)
        assert sizes_seen <= set(sd.SIZES)
        # the transforms: ragged counts, one of them full
        counts = np.array([d[1] for d in c["dets"]])
        K = c["dets"][0][0].shape[1]
        assert counts.max() == K and (len(c["dets"]) == 1 or len({tuple(r) for r in counts}) > 1), c["what"]
        flips.update(d[3] for d in c["dets"])
        bands.update(d[4] for d in c["dets"])
        Ts.add(len(c["dets"]))
        Bs.add(len(c["orig_wh"]))
        # the cut, against the reference's un-cut count of the image it was placed on
        count, top_n = c["uncut_count"], c["top_n"]
        assert count == len(ref.merge_special(*c["rows"][c["cut_image"]], cl, mode, c["th"], sd.INFERENCE_TH, 0)["scores"]) > 2
        w0 = c["want"][c["cut_image"]]
        if top_n >= sd.NO_CUT:
            cuts.add("none")
        elif top_n in (count, count - 1, 1):
            cuts.add({count: "count", count - 1: "count-1", 1: "one"}[top_n])
            assert len(w0["scores"]) == min(top_n, count)
        elif len(w0["scores"]) == top_n + 1:                       # kthvalue kept one row more than top_n: a tie exactly at the cut
            low = np.argsort(w0["scores"], kind="stable")[:2]
            assert w0["scores"][low[0]] == w0["scores"][low[1]] and w0["labels"][low[0]] != w0["labels"][low[1]], c["what"]
            assert w0["margins"]["in_distinct"] and w0["margins"]["out_distinct"]
            ties += 1
        else:
            assert 1 < top_n < count - 1 and len(w0["scores"]) == top_n, c["what"]
            cuts.add("middle")
        # the workspace
        cap = sd.DEFAULT_CAP if c["row_cap"] is None else c["row_cap"]
        assert c["workspace_classes"] == sum(m > cap for sz in sizes for m in sz)
        ws.add(min(c["workspace_classes"], 2))
        for sz in sizes:
            for p, m in enumerate(sz):
                behind |= m > cap and any(q > cap and q >= 257 for q in sz[:p]) and sum(sz[:p]) >= 257
        # the boxes
        for b, sz in enumerate(sizes):
            w = c["want"][b] if top_n >= sd.NO_CUT else ref.merge_special(*c["rows"][b], cl, mode, c["th"], sd.INFERENCE_TH, 0)
            for p, m in enumerate(sz):
                rows_p = w["labels"] == cl[p]
                if mode == "soft-nms" or m <= 2:
                    continue
                members[c["kinds"][p]] = max(members[c["kinds"][p]], int(w["avg"][rows_p].max()))
                if c["kinds"][p] == "o":
                    # one cluster of the whole class (soft-vote: beside it, the members whose softened score stays above INFERENCE_TH)
                    assert (w["avg"][rows_p] > 0).sum() == 1 and w["avg"][rows_p].max() == m and (mode == "soft-vote" or rows_p.sum() == 1), (c["what"], p)
                if c["kinds"][p] == "a":
                    assert rows_p.sum() == m and not w["avg"][rows_p].any(), (c["what"], p)            # no overlaps: untouched
    assert max(sizes_seen) >= 257 and any(65 <= m <= 255 for m in sizes_seen) and {0, 1, 2} <= sizes_seen, sizes_seen
    assert any(n > 512 for n in n_seen) and any(256 < n <= 512 for n in n_seen) and 0 in n_seen, n_seen
    assert cuts == {"none", "count", "count-1", "one", "middle"}, cuts
    assert ties == (0 if mode == "soft-nms" else 1)
    assert ws == {0, 1, 2}, ws
    assert behind, "no class behind a large class in the workspace"
    assert flips == {False, True} and None in bands and sd.BAND in bands and {1, 2, 3} <= Ts and {1, 2, 3} <= Bs
    if mode == "soft-nms":                                         # survivors that were decayed more than once
        assert max(int(w["eff"].max()) for c in cases for w in c["want"] if len(w["eff"])) >= 2
    else:
        kinds = {c["kinds"][p] for c in cases for sz in _sizes(c) for p, m in enumerate(sz) if m > 2}
        assert kinds == {"r", "o", "a"}
        assert members["r"] >= 8 and members["o"] >= 256 and members["a"] == 0, members      # random boxes: many members; one cluster: all four waves


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_draws_hold_what_they_claim(mode):
    cases = round0(mode)
    assert len(cases) == len(sd.PLANS) and [c["k"] for c in cases] == list(range(len(cases)))
    round_features(mode, [c for c in cases])
    again = sd.draw(mode, 5, 0)                                    # draw k is the same case whatever was drawn before it
    sd.STATS[mode]["drawn"] -= 1
    sd.STATS[mode]["rejected"] -= again["rejected"] is not None
    for (p, *_), (q, *_) in zip(again["dets"], cases[5]["dets"]):
        assert np.array_equal(p.numpy(), q.numpy(), equal_nan=True)
    assert again["top_n"] == cases[5]["top_n"] and again["classes"] == cases[5]["classes"]


@pytest.mark.parametrize("mode", ref.MODES)
def test_the_reference_rejects_few_draws(mode):
    round0(mode)
    sd.check_rejections(mode)


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_sweep_matches_the_restated_reference(emu, mode):
    ran = 0
    for c in round0(mode):
        if c["rejected"] is None:
            sd.run(c, CPU)
            ran += 1
    assert ran >= 0.9 * len(sd.PLANS)
    sd.check_rejections(mode)


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_large_classes_do_not_depend_on_the_schedule(emu, mode):
    import simt
    import tta_special_cases as sc
    ran = 0
    for c in round0(mode):
        if c["rejected"] is not None or max(max(s) for s in c["sizes"]) < 257:
            continue
        outs = []
        try:
            for sched, seed in (("ascending", 0), ("descending", 0), ("random", 7)):
                simt.set_schedule(sched, seed)
                outs.append(sc.host(tta.merge(c["dets"], c["orig_wh"], sd.make_cfg(c), CPU, row_cap=c["row_cap"])))
        finally:
            simt.set_schedule("ascending")
        for o in outs[1:]:
            for x, y in zip(outs[0], o):
                assert torch.equal(x.bbox, y.bbox) and torch.equal(x.get_field("scores"), y.get_field("scores")), c["what"]
                assert torch.equal(x.get_field("labels"), y.get_field("labels")), c["what"]
        ran += 1
    assert ran >= 5


@needs_simt
@pytest.mark.parametrize("mode", ref.MODES)
def test_equal_scores_across_waves_go_to_the_lower_original_row(emu, mode):
    sd.run_ties(mode, CPU)


@needs_simt
def test_cut_threshold_contract_over_several_tiles(emu):
    sd.run_cut_contract(CPU)
