"""Phrase-grounding evaluation: the `TEST.EVAL_TASK = "grounding"` branch of the reference's `inference()` (engine/inference.py:583-641 the
loop, :701-724 the evaluator calls) on a Flickr30k Entities style loader.

Batches are `(images, targets, image_ids, ...)`; every target is a BoxList with the fields `caption`, `positive_map_eval` ([phrases, tokens]
0/1), `original_img_id`, `sentence_id` and `orig_size` ((height, width)).  Difference by design: the reference asserts one image per batch
(:622); here a batch of any size goes through `GeneralizedVLRCNN_New.forward_grounding` in one launch sequence (MQ-GroundingDINO models
take one `model(...)` call per item), and `flickr_post_process` is `FlickrRecallEvaluator.update_boxlist` on the device."""
import torch

from .structures import ImageList, to_image_list


def create_positive_map_label_to_token_from_positive_map(positive_map, plus=0):
    """engine/inference.py:285-289: row i of the [phrases, tokens] map -> {i + plus: [positions of its non-zero entries]}."""
    return {i + plus: torch.nonzero(positive_map[i], as_tuple=True)[0].tolist() for i in range(len(positive_map))}


def label_offset(cfg):
    """`plus` (:618-621): VLDyHead labels start at 1."""
    return 1 if cfg.MODEL.RPN_ARCHITECTURE == "VLDYHEAD" else 0


@torch.no_grad()
def evaluate_grounding(model, data_loader, evaluator, device="cuda", output_file=None):
    """-> the evaluator's `score` dict ({"Recall@1_all": ..}); written to `output_file` (bbox.csv) when given."""
    device = torch.device(device)
    plus = label_offset(model.cfg)
    batched = hasattr(model, "forward_grounding")
    for batch in data_loader:
        images, targets, image_ids, *_ = batch
        images = to_image_list(images).to(device)
        captions = [t.get_field("caption") for t in targets]
        maps = [create_positive_map_label_to_token_from_positive_map(t.get_field("positive_map_eval"), plus=plus) for t in targets]
        if batched:
            outputs = model.forward_grounding(images, captions, maps)
            outputs = outputs[0] if isinstance(outputs, tuple) else outputs
        else:
            outputs = []
            for i, (cap, pm) in enumerate(zip(captions, maps)):
                out = model(ImageList(images.tensors[i:i + 1], images.image_sizes[i:i + 1]), captions=[cap], positive_map=pm)
                outputs.append((out[0] if isinstance(out, tuple) else out)[0])
        for t, pm, out in zip(targets, maps, outputs):
            evaluator.update_boxlist(t.get_field("original_img_id"), t.get_field("sentence_id"), out, len(pm), plus, t.get_field("orig_size"))
    evaluator.synchronize_between_processes()
    score = evaluator.summarize()
    main = not (torch.distributed.is_available() and torch.distributed.is_initialized()) or torch.distributed.get_rank() == 0
    if output_file is not None and main:                      # (every rank holds the score; the main process writes, :722-724)
        evaluator.write_results(score, output_file)
    return score
