#!/usr/bin/env python3
"""Write tests/golden/finetuned_selector.npz + finetuned_selector.json: what the reference's own `QuerySelector`
(modeling/query_selector/query_selector.py), loaded by file from where it lies and run in eval mode, returns with
VISION_QUERY.LEARNABLE_BANK on / off x VISION_QUERY.ADD_VISION_LAYER on / off.

The bank is seeded: labels {1: 7, 2: 2, 4: 3, 6: 11} rows, S in {1, 5} scales, C = 6; `tunable_vision_linear.weight` is seeded and non-zero;
NUM_QUERY_PER_CLASS = 3; numpy's global generator is seeded before every call.  The inputs are those of tests/test_query_select_cpu.py: its
single-caption label list (LABELS / PMAP, for one and for two images) and its ragged batch (RAGGED) without the two items that select no
row at all -- the empty one and [3, 1000] --, which the reference cannot concatenate (`torch.cat([])`, :95).  Labels 3 and 1000 have no
vision query: the reference's bank is a `defaultdict(list)` (engine/inference.py:401) and reads them as `[]`; its `nn.ParameterDict` cannot
hold a list, so with LEARNABLE_BANK the bank file carries a [0, S, C] entry for each (the same draws are consumed, no row comes out).

Per case the fixture holds `queries`, `masks`, `has_vision_query` and numpy's generator state after the call.

    python tools/gen_golden_finetuned.py          (needs the reference checkout; test infrastructure, never run on the GPU box)
"""
import importlib.util
import json
import os
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "finetuned_selector")

import test_query_select_cpu as ts  # noqa: E402

C, K, T = 6, 3, ts.T
NO_QUERY = (3, 1000)


def reference_selector_class():
    from oracle import _refload
    path = os.path.join(_refload.REF, "maskrcnn_benchmark", "modeling", "query_selector", "query_selector.py")
    spec = importlib.util.spec_from_file_location("reference_query_selector", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.QuerySelector


def make_cfg(path, learnable, add):
    VQ = types.SimpleNamespace(QUERY_BANK_PATH=path, LEARNABLE_BANK=learnable, ADD_VISION_LAYER=add, PURE_TEXT_RATE=0.0,
                               NUM_QUERY_PER_CLASS=K, RANDOM_KSHOT=False)
    return types.SimpleNamespace(MODEL=types.SimpleNamespace(DEVICE="cpu"), VISION_QUERY=VQ)


def location_maps(labels, pmap):
    """generalized_vl_rcnn_new.py:295-305 for the labels of one image"""
    m = torch.zeros(len(labels), T)
    for j, lab in enumerate(labels):
        m[j, list(pmap[lab])] = 1
    return m / (m.sum(-1)[:, None] + 1e-6)


def inputs():
    ragged = [(l, m) for l, m in zip(*ts.RAGGED) if any(lab in ts.COUNTS for lab in l)]
    return {"single1": ([ts.LABELS], [ts.PMAP]), "single2": ([ts.LABELS] * 2, [ts.PMAP] * 2),
            "ragged": ([l for l, _ in ragged], [m for _, m in ragged])}


def main():
    Ref = reference_selector_class()
    arrays, meta = {}, {"C": C, "K": K, "T": T, "counts": {str(k): v for k, v in ts.COUNTS.items()}, "no_query": list(NO_QUERY), "cases": [],
                        "inputs": {n: {"labels": ls, "maps": [{str(k): v for k, v in m.items()} for m in ms]} for n, (ls, ms) in inputs().items()}}
    real_load = torch.load
    with tempfile.TemporaryDirectory() as tmp:
        for S in (1, 5):
            g = torch.Generator().manual_seed(77 + S)
            bank = {lab: torch.randn(n, S, C, generator=g) for lab, n in ts.COUNTS.items()}
            wv = torch.randn(1000, C, generator=g)
            for lab, v in bank.items():
                arrays[f"bank_S{S}_label{lab}"] = v.numpy()
            arrays[f"wv_S{S}"] = wv.numpy()
            plain, with_empty = os.path.join(tmp, f"plain{S}.pth"), os.path.join(tmp, f"empty{S}.pth")
            torch.save(bank, plain)
            torch.save({**bank, **{lab: torch.zeros(0, S, C) for lab in NO_QUERY}}, with_empty)
            for learnable in (False, True):
                for add in (False, True):
                    torch.load = lambda p, map_location=None: real_load(p, map_location=map_location, weights_only=True)
                    try:
                        sel = Ref(make_cfg(with_empty if learnable else plain, learnable, add))
                    finally:
                        torch.load = real_load
                    if not learnable:                        # the reference's banks are defaultdict(list): a label without queries reads as []
                        sel.query_bank = defaultdict(list, sel.query_bank)
                    if add:
                        assert sel.tunable_vision_linear.weight.shape == (1000, C) and not sel.tunable_vision_linear.weight.any()
                        sel.tunable_vision_linear.weight.data.copy_(wv)
                    sel.eval()
                    for seed, (name, (labels, maps)) in enumerate(inputs().items()):
                        seed = 5 + seed
                        np.random.seed(seed)
                        with torch.no_grad():
                            q, m, has = sel(labels, [location_maps(l, pm) for l, pm in zip(labels, maps)])
                        st = np.random.get_state()
                        tag = f"S{S}_L{int(learnable)}_A{int(add)}_{name}"
                        assert q.dtype == torch.float32 and q.shape[0] == len(labels) and q.shape[2] == C, (tag, q.shape, q.dtype)
                        arrays[tag + "_queries"], arrays[tag + "_masks"] = q.numpy(), m.numpy().astype(np.uint8)
                        arrays[tag + "_rng_key"] = st[1]
                        meta["cases"].append({"tag": tag, "S": S, "learnable": learnable, "add": add, "input": name, "seed": seed,
                                              "has_vision_query": has, "rng_pos": int(st[2])})
                        print(tag, tuple(q.shape), has)
    # the offset is visible: with and without it the recorded rows differ, and learnable on / off agree
    for S in (1, 5):
        for name in inputs():
            a, b = arrays[f"S{S}_L0_A0_{name}_queries"], arrays[f"S{S}_L0_A1_{name}_queries"]
            assert a.shape == b.shape and np.abs(a - b).max() > 0.1
            for A in (0, 1):
                assert np.array_equal(arrays[f"S{S}_L0_A{A}_{name}_queries"], arrays[f"S{S}_L1_A{A}_{name}_queries"])
    with open(OUT + ".json", "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    np.savez_compressed(OUT + ".npz", **arrays)
    print("wrote", OUT + ".json", OUT + ".npz", os.path.getsize(OUT + ".npz"), "bytes")


if __name__ == "__main__":
    main()
