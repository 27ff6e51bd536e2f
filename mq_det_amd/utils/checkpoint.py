"""Loading what the reference's fine-tuning saved.

`DetectronCheckpointer.save` (utils/checkpoint.py:33-53) writes `{"model": state_dict, "optimizer": ..., "scheduler": ..., "iteration": ...}`
with the keys of a DistributedDataParallel model prefixed `module.`.  A few-shot run of tools/finetune.py adds up to three kinds of state to
that dict (DESIGN.md "Fine-tuned checkpoints"): `rpn.tunable_linear.weight`, `query_selector.query_bank.<label>` and
`query_selector.tunable_vision_linear.weight`; a model built from the run's config owns (or, for the selector's, creates on load) exactly
those names, so the load below is strict-clean."""
import os

import torch


def load_reference_checkpoint(model, path_or_dict, strict=True):
    """Load a checkpoint file in the reference's layout, or a bare state dict, into `model`; returns `load_state_dict`'s
    `(missing_keys, unexpected_keys)` result.  The file is read through torch's weights-only unpickler, like the bank files.  One leading
    `module.` is stripped from every key.  Nothing else: no URL handling, no key remapping."""
    ckpt = path_or_dict
    if isinstance(ckpt, (str, os.PathLike)):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=True)
    sd = ckpt["model"] if isinstance(ckpt, dict) and "model" in ckpt and isinstance(ckpt["model"], dict) else ckpt
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    return model.load_state_dict(sd, strict=strict)
