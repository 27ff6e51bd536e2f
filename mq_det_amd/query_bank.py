"""The vision-query bank on the device, and the two loops that drive it.

`QueryBank` holds what the reference keeps in a `defaultdict(list)` of `{label: Tensor[n, scales, C]}` (generalized_vl_rcnn_new.py:232-288,
groundingdino.py:397-421) as four device tensors: an append-only row pool [R, S, C], a slot table [labels, capacity] int32 of pool rows in
admission order, counts [labels] and the cached 1 / max(|row|, 1e-12) of every row.  `update` runs the reference's admission loop for a whole
batch of candidates in ONE kernel launch (csrc/query_bank.hip mq_bank_admit) with the reference's sequential semantics; `to_dict` / `save`
give back exactly what the dict path would hold.  `pool_into_bank` (modeling/detector.py) takes this path when `extract_query` is handed a
`QueryBank` as `query_images`, for MQ-GLIP and MQ-GroundingDINO alike; a dict takes the Python loop it always took.
`model.load_query_bank(bank)` hands the bank to the forward as it is: the selector (modeling/query_selector.py) snapshots its counts and selects
the vision queries of every call from `pool` / `slots` with one launch (mq_bank_select_fwd).

`extract_query_bank` is the extraction loop of tools/train_net.py:294-336 and `online_update` the test-time refinement of
engine/inference.py:383-499 (called from tools/test_grounding_net.py:181-227)."""
import os

import torch

from . import ops as _ops
from .structures import cat_boxlist


class QueryBank:
    """Device-resident vision-query bank.  Rows are fp32 (what the poolers return and the dict path stores).  The pool and the label table
    grow geometrically; there is no dense [labels, capacity, S, C] tensor."""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        self.pool = None                                   # [R, S, C] fp32, rows [0, self.rows) in use
        self.inv_norm = None                               # [R] fp32: 1 / max(|row|, 1e-12) (read with S == 1 only)
        self.slots = None                                  # [labels, capacity] int32: pool rows of a label, in admission order
        self.counts = None                                 # [labels] int32
        self._state = None                                 # [2] int32: pool rows in use, overflow flag
        self.rows = 0                                      # host copy of _state[0] (exact after every update)
        self._host_counts = None                           # counts on the host, fetched on demand

    # ------------------------------------------------------------------ storage
    @property
    def row_shape(self):
        return None if self.pool is None else tuple(self.pool.shape[1:])

    def _reserve(self, n_new, n_labels, cap, S, C):
        """Room for n_new more pool rows, n_labels labels and `cap` rows per label."""
        dev = self.device
        if self.pool is None:
            self.pool = torch.empty(max(64, n_new), S, C, dtype=torch.float32, device=dev)
            self.inv_norm = torch.zeros(len(self.pool), dtype=torch.float32, device=dev)
            self.slots = torch.zeros(max(16, n_labels), max(1, cap), dtype=torch.int32, device=dev)
            self.counts = torch.zeros(len(self.slots), dtype=torch.int32, device=dev)
            self._state = torch.zeros(2, dtype=torch.int32, device=dev)
            return
        if self.row_shape != (S, C):
            raise ValueError(f"this bank holds rows of shape {self.row_shape}, not {(S, C)}")
        R = len(self.pool)
        if self.rows + n_new > R:
            R = max(self.rows + n_new, 2 * R)
            pool = torch.empty(R, S, C, dtype=torch.float32, device=dev)
            inv = torch.zeros(R, dtype=torch.float32, device=dev)
            pool[:self.rows] = self.pool[:self.rows]
            inv[:self.rows] = self.inv_norm[:self.rows]
            self.pool, self.inv_norm = pool, inv
        L, W = self.slots.shape
        if n_labels > L or cap > W:
            L2 = L if n_labels <= L else max(n_labels, 2 * L)
            W2 = W if cap <= W else max(cap, 2 * W)
            slots = torch.zeros(L2, W2, dtype=torch.int32, device=dev)
            counts = torch.zeros(L2, dtype=torch.int32, device=dev)
            slots[:L, :W] = self.slots
            counts[:L] = self.counts
            self.slots, self.counts = slots, counts

    def _counts(self):
        if self._host_counts is None:
            self._host_counts = [] if self.counts is None else self.counts.tolist()
        return self._host_counts

    # ------------------------------------------------------------------ the admission loop
    @torch.no_grad()
    def update(self, feats, labels, max_query_number, exclude_similar=False, thr=0.85):
        """Run the candidates `feats` [N, S, C] (fp32) with `labels` [N] through the reference's admission loop, in row order; returns the
        number admitted.  A candidate is skipped when its label holds `max_query_number` rows or -- `exclude_similar`, label not empty -- a
        row of its label has cosine similarity > `thr`; a candidate admitted earlier in the call counts as part of the bank.

        Host synchronisations: TWO per call, whatever N is -- the smallest and largest label (to refuse negative ones and size the label
        table) before the launch, the number of pool rows in use (the return value) after it.  Launches: one stable sort, one kernel."""
        feats = torch.as_tensor(feats)
        if feats.dim() != 3:
            raise ValueError(f"feats must be [N, scales, channels], got {tuple(feats.shape)}")
        N, S, C = feats.shape
        if exclude_similar and S != 1:
            # the reference asserts feat.shape[0] == 1 at the point of comparison (generalized_vl_rcnn_new.py:276)
            raise ValueError(f"exclude_similar needs one scale per row (VISION_QUERY.SELECT_FPN_LEVEL), got {S}")
        if feats.dtype != torch.float32:
            raise TypeError(f"the bank holds float32 rows (what the poolers return), got {feats.dtype}")
        labels = torch.as_tensor(labels)
        if labels.dim() != 1 or len(labels) != N:
            raise ValueError(f"labels must be [N] with N = {N}, got {tuple(labels.shape)}")
        if labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise TypeError(f"labels must be integers, got {labels.dtype}")
        max_query_number = int(max_query_number)
        if N == 0 or max_query_number <= 0:
            return 0
        feats = feats.to(self.device).contiguous()
        sorted_labels, order = torch.sort(labels.to(self.device, torch.int64), stable=True)
        lo, hi = torch.stack([sorted_labels[0], sorted_labels[-1]]).tolist()           # sync 1
        if lo < 0:
            raise ValueError(f"negative label {lo}")
        # no label can hold more rows than the bank has after this call: the table is never wider than that
        cap = min(max_query_number, self.rows + N)
        self._reserve(N, hi + 1, cap, S, C)
        self._host_counts = None
        _ops.bank_admit(feats.view(N, S * C), sorted_labels, order, self.pool, self.inv_norm, self.slots, self.counts, self._state,
                        lo, hi - lo + 1, min(max_query_number, self.slots.shape[1]), exclude_similar, thr)
        used, overflow = self._state.tolist()                                           # sync 2
        if overflow:
            raise RuntimeError("mq_bank_admit ran out of pool rows")
        admitted, self.rows = used - self.rows, used
        return admitted

    def merge(self, other, max_query_number):
        """Append another bank's rows (e.g. the per-rank files the reference writes and never merges, tools/train_net.py:305-329) in label
        order, then slot order, up to `max_query_number` rows per label, through the same kernel.  Returns the number admitted."""
        if not isinstance(other, QueryBank):
            other = QueryBank.from_dict(other, self.device)
        feats, labels = other._rows_in_label_order()
        if feats is None:
            return 0
        return self.update(feats, labels, max_query_number, exclude_similar=False)

    def _rows_in_label_order(self):
        counts = self._counts()
        if not any(counts):
            return None, None
        labs = [l for l, n in enumerate(counts) if n]
        idx = torch.cat([self.slots[l, :counts[l]] for l in labs]).long()
        labels = torch.repeat_interleave(torch.tensor(labs, dtype=torch.int64), torch.tensor([counts[l] for l in labs]))
        return self.pool[idx], labels.to(self.device)

    # ------------------------------------------------------------------ the dict view
    def __len__(self):
        """Number of labels that hold rows (the length of the dict the reference keeps)."""
        return sum(1 for n in self._counts() if n)

    def __contains__(self, label):
        counts = self._counts()
        return isinstance(label, int) and 0 <= label < len(counts) and counts[label] > 0

    def __getitem__(self, label):
        if label not in self:
            raise KeyError(label)
        return self.pool[self.slots[label, :self._counts()[label]].long()]

    def labels(self):
        return [l for l, n in enumerate(self._counts()) if n]

    def to_dict(self):
        """{int label: Tensor[n, S, C]} -- the tensors the dict path of `pool_into_bank` would hold after the same calls."""
        return {l: self[l] for l in self.labels()}

    @classmethod
    def from_dict(cls, d, device="cuda"):
        """A bank with the rows of `{label: Tensor[n, S, C]}` (entries that are empty lists, as in a `defaultdict(list)`, are skipped)."""
        bank = cls(device)
        items = [(int(k), v) for k, v in d.items() if torch.is_tensor(v) and len(v)]
        if items:
            feats = torch.cat([v.to(bank.device) for _, v in items])
            labels = torch.repeat_interleave(torch.tensor([k for k, _ in items], dtype=torch.int64), torch.tensor([len(v) for _, v in items]))
            bank.update(feats, labels, max(len(v) for _, v in items), exclude_similar=False)
        return bank

    @classmethod
    def from_state_dict(cls, sd, device="cuda", prefix="query_selector.query_bank."):
        """A resident bank from the learnable bank of a fine-tuned checkpoint (VISION_QUERY.LEARNABLE_BANK): the entries
        `<prefix><label>` of the state dict `sd`, in its order."""
        return cls.from_dict({int(k[len(prefix):]): v.detach().float() for k, v in sd.items() if k.startswith(prefix)}, device)

    @classmethod
    def load(cls, path, device="cuda"):
        return cls.from_dict(load_bank_file(path, device), device)

    def save(self, path):
        """Write the bank as the reference does (`torch.save` of the label -> tensor dict): `QuerySelector.load_query_bank` of this project
        and of the reference read the file."""
        folder = os.path.dirname(os.path.abspath(path))
        os.makedirs(folder, exist_ok=True)
        torch.save({l: t.cpu() for l, t in self.to_dict().items()}, path)


def load_bank_file(path, device="cpu"):
    """The label -> tensor dict of a bank file, through torch's weights-only unpickler (as `QuerySelector.load_query_bank`).  `QueryBank.save`
    writes a plain dict of tensors, which it reads; a file the reference wrote with `torch.save` of its `defaultdict(list)` is refused by that
    unpickler on torch >= 2.6 and has to be re-saved as a plain dict where it came from."""
    return torch.load(path, map_location=torch.device(device))


def _pool_tag(cfg):
    return "sel" if cfg.VISION_QUERY.SELECT_FPN_LEVEL else "all"


def _dataset_name(cfg, split):
    name = cfg.VISION_QUERY.get("DATASET_NAME", "")
    if name:
        return name
    sets = cfg.DATASETS.get(split, ())
    if not sets:
        raise ValueError(f"the default file name needs VISION_QUERY.DATASET_NAME or DATASETS.{split}; or pass the file name")
    return sets[0].split("_")[0]


def _model_device(model):
    try:
        return next(model.parameters()).device
    except (AttributeError, StopIteration):
        return torch.device("cpu")


@torch.no_grad()
def extract_query_bank(model, batches, max_query_number=None, save_path=None):
    """The bank-building loop of tools/train_net.py:294-336: `model.extract_query(images, targets, bank)` for every `(images, targets, *_)`
    of `batches`, on a device-resident bank; the bank is saved to `save_path`, else VISION_QUERY.QUERY_BANK_SAVE_PATH, else the
    reference's file name `MODEL/{dataset}_query_{MAX_QUERY_NUMBER}_pool{resolution}_{sel|all}{QUERY_ADDITION_NAME}.pth`.  Returns the
    `QueryBank`."""
    cfg = model.cfg
    device = _model_device(model)
    bank = QueryBank(device)
    model.eval()
    for images, targets, *_ in batches:
        bank = model.extract_query(images.to(device), targets, bank, max_query_number=max_query_number)
    save_name = save_path or cfg.VISION_QUERY.get("QUERY_BANK_SAVE_PATH", "")
    if not save_name:
        save_name = "MODEL/{}_query_{}_pool{}_{}{}.pth".format(_dataset_name(cfg, "TRAIN"), cfg.VISION_QUERY.MAX_QUERY_NUMBER,
                                                               cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION, _pool_tag(cfg),
                                                               cfg.VISION_QUERY.get("QUERY_ADDITION_NAME", ""))
    bank.save(save_name)
    return bank


@torch.no_grad()
def online_update(model, data_loader, device="cuda", cfg=None, num_turns=1, save_name=None, *, queries_and_maps, resident=False):
    """Test-time refinement of the bank (engine/inference.py:383-499): per turn, every batch of `data_loader` is detected with every chunk
    caption, the detections of an image are concatenated in chunk order, those with score > VISION_QUERY.SCORE_THRESHOLD (strict) are
    pooled from the backbone features and admitted with `exclude_similar=True` up to VISION_QUERY.MAX_TEST_QUERY_NUMBER per label; the
    bank is saved to `save_name` after the turn and loaded into the model before the next one.  Returns the model.

    `queries_and_maps` = `(all_queries, all_positive_map_label_to_token)` of the caller's `create_queries_and_maps_from_dataset` (the data
    layer is not part of this package).  Only TEST.EVAL_TASK = "detection"; TEST.USE_MULTISCALE raises NotImplementedError, as in the
    reference.  The bank starts from VISION_QUERY.QUERY_BANK_PATH when that file exists, else empty.
    The detections come from `model(...)`: with VISION_QUERY.MASK_DURING_INFERENCE (vision-only evaluation, detector._masked_ids) the words of
    the labels the model's bank has rows for are masked, and `model.load_query_bank` between turns changes that set with the bank.
    `resident=True`: the model is handed the `QueryBank` itself between turns and after the last one (`QuerySelector.load_query_bank` keeps
    it with a snapshot of its counts and selects from it on the device) instead of reading the file back as a CPU dict; the file is written
    every turn all the same, and the rows admitted during a turn still enter the forward only at the next load.

    Two deliberate differences from the reference:
      * batches of more than one image are accepted (the reference asserts 1, "TODO: support batched outputs").  The bank only enters the
        forward between turns, so the result equals the batch-1 run over the same image order;
      * the reference's "lvis" branch reads `all_output` before anything was appended to it and cannot run; every dataset takes the generic
        branch here."""
    device = torch.device(device)
    cfg = model.cfg if cfg is None else cfg
    if cfg.TEST.EVAL_TASK != "detection":
        raise NotImplementedError(f"TEST.EVAL_TASK = {cfg.TEST.EVAL_TASK}: only detection")
    if cfg.TEST.USE_MULTISCALE:
        raise NotImplementedError("online_update with TEST.USE_MULTISCALE")
    VQ = cfg.VISION_QUERY
    all_queries, all_maps = queries_and_maps
    bank = QueryBank.load(VQ.QUERY_BANK_PATH, device) if VQ.QUERY_BANK_PATH and os.path.exists(VQ.QUERY_BANK_PATH) else QueryBank(device)
    if save_name is None:
        save_name = "MODEL/{}_val_query_{}_pool{}_loop{}_{}.pth".format(_dataset_name(cfg, "TEST"), VQ.MAX_TEST_QUERY_NUMBER,
                                                                         cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION, num_turns, _pool_tag(cfg))
    subset = cfg.TEST.get("SUBSET", -1)
    for turn in range(num_turns):
        if turn > 0:
            model.load_query_bank(bank if resident else save_name)
        model.eval()
        for i, batch in enumerate(data_loader):
            if i == subset:
                break
            images, targets, *_ = batch
            images = images.to(device)
            per_chunk, feats = [], None
            for caption, positive_map in zip(all_queries, all_maps):
                output, feats = model(images, captions=[caption] * len(targets), positive_map=positive_map, return_backbone_features=True)
                per_chunk.append(output)
            kept = []
            for b in range(len(per_chunk[0])):
                o = cat_boxlist([chunk[b] for chunk in per_chunk])
                kept.append(o[o.get_field("scores") > VQ.SCORE_THRESHOLD])
            if any(len(k) for k in kept):                                              # (no box kept: nothing to pool, the bank stays as it is)
                bank = model.extract_query(targets=kept, query_images=bank, visual_features=feats, exclude_similar=True, device=device,
                                           max_query_number=VQ.MAX_TEST_QUERY_NUMBER)
        bank.save(save_name)
    if resident:
        model.load_query_bank(bank)
    return model
