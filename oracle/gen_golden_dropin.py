"""What the reference's own code returns for the drop-in / caller-sequence / evaluator tests, stored as DATA so that those tests run
from the repository alone:

    python -m oracle.gen_golden_dropin      -> tests/golden/dropin_reference.json   (needs the reference checkout that oracle/_refload.py reads)

Recorded, each by executing the reference's code in place (oracle/_refload.py; nothing of its source is written out):
  * cfg:       the reference's config trees (config/defaults.py merged with the YAMLs the tests name), as plain values
  * queries:   engine/inference.py create_queries_and_maps_from_dataset -> captions and positive maps, for the category lists and
               synthetic tokenizers of tests/test_dropin_reference_cfg.py
  * glipdemo:  engine/predictor_glip.py GLIPDemo -- the caption and label -> token map compute_prediction hands to the model, and the
               kept order of _post_process_fixed_thresh / _post_process on a seeded synthetic prediction
  * resize_box: engine/inference.py resize_box on a seeded BoxList
  * evaluator: lvis_eval.py LvisEvaluatorFixedAP.by_cat after update() (tests/test_host_cpu.py) and after a world-2
               synchronize_between_processes (tests/_gloo_eval_worker.py; the all_gather of the two ranks done in this one process)
"""
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TESTS = os.path.join(ROOT, "tests")
OUT = os.path.join(TESTS, "golden", "dropin_reference.json")


def encode(v, root):
    """Config values -> JSON (tuples tagged, so that the tests get back exactly the types the reference's tree holds; paths the tree
    derives from the checkout's location, e.g. PATHS_CATALOG, relative to the checkout)."""
    if isinstance(v, dict):
        return {k: encode(x, root) for k, x in v.items()}
    if isinstance(v, tuple):
        return {"__tuple__": [encode(x, root) for x in v]}
    if isinstance(v, list):
        return [encode(x, root) for x in v]
    if isinstance(v, str) and v.startswith(root + "/"):
        return os.path.relpath(v, root)
    return v


def _maps(maps):
    return [{str(k): list(v) for k, v in m.items()} for m in maps]


def _by_cat(by_cat):
    return {str(int(c)): [[int(a["image_id"]), float(a["score"]), [float(v) for v in a["bbox"]]] for a in anns] for c, anns in by_cat.items()}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, TESTS)
    from oracle import _refload
    from oracle.spec import tiny_gdino_spec
    from mq_det_amd.structures import BoxList, to_image_list
    from mq_det_amd.utils.tokenizer import build_synthetic_tokenizer
    import test_dropin_reference_cfg as td
    import test_host_cpu as th
    import _gloo_eval_worker as gw

    out = {"cfg": {}, "queries": {}}
    out["cfg"]["mq-glip-t+lvis_minival"] = encode(_refload.reference_cfg("configs/pretrain/mq-glip-t.yaml",
                                                                          "configs/vision_query_5shot/lvis_minival.yaml"), _refload.REF)
    out["cfg"]["mq-glip-t"] = encode(_refload.reference_cfg("configs/pretrain/mq-glip-t.yaml"), _refload.REF)
    out["cfg"]["mq-groundingdino-t"] = encode(_refload.reference_cfg("configs/pretrain/mq-groundingdino-t.yaml"), _refload.REF)

    fns = _refload.reference_functions("maskrcnn_benchmark/engine/inference.py",
                                       ["clean_name", "create_positive_dict", "chunks", "create_queries_and_maps",
                                        "create_queries_and_maps_from_dataset", "resize_box"],
                                       {"load_from_yaml_file": None})

    # captions / positive maps with the overrides the tests apply (local synthetic tokenizer, chunking of the lvis_minival YAML)
    cfg = _refload.reference_cfg("configs/pretrain/mq-glip-t.yaml", "configs/vision_query_5shot/lvis_minival.yaml")
    tok_dir = build_synthetic_tokenizer(tempfile.mkdtemp(), size=4000, extra_words=td.words_of(td.LVIS_LIKE))
    cfg.MODEL.LANGUAGE_BACKBONE.TOKENIZER_TYPE = cfg.MODEL.LANGUAGE_BACKBONE.MODEL_TYPE = tok_dir
    dataset = types.SimpleNamespace(categories=lambda: {i + 1: n for i, n in enumerate(td.LVIS_LIKE)})
    q, m = fns["create_queries_and_maps_from_dataset"](dataset, cfg, disable_print=True)
    out["queries"]["glip_lvis_like"] = {"queries": list(q), "maps": _maps(m)}

    cfg = _refload.reference_cfg("configs/pretrain/mq-groundingdino-t.yaml")
    names = td.LVIS_LIKE[:12]
    spec = tiny_gdino_spec(vocab=4000)
    tok_dir = build_synthetic_tokenizer(tempfile.mkdtemp(), size=spec.vocab, extra_words=td.words_of(names))
    cfg.GROUNDINGDINO.text_encoder_type = tok_dir
    cfg.MODEL.LANGUAGE_BACKBONE.TOKENIZER_TYPE = cfg.MODEL.LANGUAGE_BACKBONE.MODEL_TYPE = tok_dir
    cfg.MODEL.LANGUAGE_BACKBONE.BERT_VOCAB_SIZE = spec.vocab
    dataset = types.SimpleNamespace(categories=lambda: {i + 1: n for i, n in enumerate(names)})
    q, m = fns["create_queries_and_maps_from_dataset"](dataset, cfg, disable_print=True)
    out["queries"]["gdino_lvis_like12"] = {"queries": list(q), "maps": _maps(m)}

    # resize_box on a seeded BoxList
    bl, targets = td.resize_box_case()
    r = fns["resize_box"](bl, targets)
    out["resize_box"] = {"bbox": r.bbox.tolist(), "size": [int(v) for v in r.size]}

    # GLIPDemo: what compute_prediction hands to the model, and the post-processing order
    from transformers import AutoTokenizer
    ref = _refload.reference_classes("maskrcnn_benchmark/engine/predictor_glip.py", ["GLIPDemo"],
                                     ["create_positive_map", "create_positive_map_label_to_token_from_positive_map"],
                                     {"to_image_list": to_image_list, "timeit": __import__("timeit"), "print": lambda *a, **k: None})
    cfg = _refload.reference_cfg("configs/pretrain/mq-glip-t.yaml")
    tok_dir = build_synthetic_tokenizer(tempfile.mkdtemp(), size=4000, extra_words=[w for n in td.GLIPDEMO_NAMES for w in n.split()])
    demo = ref["GLIPDemo"].__new__(ref["GLIPDemo"])
    demo.cfg = cfg
    demo.device = demo.cpu_device = torch.device("cpu")
    demo.tokenizer = AutoTokenizer.from_pretrained(tok_dir)
    demo.transforms = lambda img: torch.zeros(3, 32, 32)
    demo.confidence_threshold = td.GLIPDEMO_THRESHOLD
    seen = []

    class Model:
        def __call__(self, image_list, captions=None, positive_map=None):
            seen.append({"captions": list(captions), "positive_map": {str(k): list(v) for k, v in positive_map.items()}})
            b = BoxList(torch.zeros(0, 4), (32, 32))
            b.add_field("scores", torch.zeros(0))
            b.add_field("labels", torch.zeros(0, dtype=torch.long))
            return [b]
    demo.model = Model()
    image = torch.zeros(150, 190, 3).numpy()
    demo.compute_prediction(image, td.GLIPDEMO_NAMES)
    caption, spans = td.glipdemo_caption()
    demo.run_ner = lambda text: spans
    demo.compute_prediction(image, caption)
    pred = td.glipdemo_prediction_case()
    keep_fixed = demo._post_process_fixed_thresh(pred)
    keep_thr = demo._post_process(pred, threshold=td.GLIPDEMO_THRESHOLD)
    out["glipdemo"] = {"plus": demo.plus, "calls": seen,
                       "post_process_fixed_thresh": {"scores": keep_fixed.get_field("scores").tolist(), "labels": keep_fixed.get_field("labels").tolist(),
                                                     "bbox": keep_fixed.bbox.tolist()},
                       "post_process": {"scores": keep_thr.get_field("scores").tolist(), "labels": keep_thr.get_field("labels").tolist(),
                                        "bbox": keep_thr.bbox.tolist()}}

    # the evaluator: update() of (image id, dict) pairs; world-2 synchronize (all_gather of both ranks' by_cat, rank order)
    ev = _refload.reference_classes("maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis_eval.py", ["LvisEvaluatorFixedAP"],
                                    ["_merge_lists", "convert_to_xywh"], {"LVIS": object})
    e = ev["LvisEvaluatorFixedAP"](gt=None, topk=50)
    e.update(th.evaluator_update_preds())
    out["evaluator"] = {"update_topk50": _by_cat(e.by_cat)}
    ranks = []
    for rank in range(2):
        gathered = types.SimpleNamespace(all_gather=lambda obj: [r.by_cat for r in ranks])
        ev = _refload.reference_classes("maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis_eval.py", ["LvisEvaluatorFixedAP"],
                                        ["_merge_lists"], {"LVIS": object, "dist": gathered})
        e = ev["LvisEvaluatorFixedAP"](gt=None, topk=gw.TOPK)
        for anns in gw.rank_annotations(rank):
            e.update(anns, is_cur_results=True)
        ranks.append(e)
    ranks[0].synchronize_between_processes()
    out["evaluator"]["world2_synchronized"] = _by_cat(ranks[0].by_cat)

    import json
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
