"""Vision-query selection (host-side glue, tiny compute).

Reference: modeling/query_selector/query_selector.py:8-116 (bank `{label: Tensor[n, scales, C]}`, <= k rows per
label, `[V, T]` 0/1 attention mask, `pad_sequence`) and generalized_vl_rcnn_new.py:295-305 (label -> token map).
MI355X-first difference: besides the dense mask the selector emits the gather index `idx[b, t, :]` (the
vision rows each text token may attend to) that the reference re-derives from the mask with a top-k trick in
EACH of the 6 GCP layers (modeling_bert_new.py:40-63,162-184); it is built once, on the host, from the
positive_map the caller already holds -- no device work, no sync.
With a device-resident `QueryBank` (mq_det_amd.query_bank) instead of the dict, the draws stay on the host and the rows and the index come
from one kernel launch (`_select_resident`, csrc/query_bank.hip mq_bank_select_fwd).
Fine-tuned checkpoints (DESIGN.md "Fine-tuned checkpoints"): VISION_QUERY.LEARNABLE_BANK keeps the bank as the reference's `nn.ParameterDict`
`query_bank.<label>` (:17-21, 59-60) and VISION_QUERY.ADD_VISION_LAYER owns `tunable_vision_linear.weight` [1000, C], added to an image's
concatenated query rows before the padding (:98-99) -- on the resident path inside the same launch (mq_bank_select_add_fwd).
"""
import os
import random

import numpy as np
import torch
from torch import nn

from .. import ops as _ops
from ..query_bank import QueryBank
from .params import Container

VISION_LAYER_ROWS = 1000                                       # rows of `tunable_vision_linear.weight` (query_selector.py:27)


def labels_and_maps(positive_map, T, device="cpu", dtype=torch.float32):
    labels = [k for k, v in positive_map.items() if len(v) != 0]
    m = torch.zeros(len(labels), T, dtype=dtype, device=device)
    for j, lab in enumerate(labels):
        m[j, list(positive_map[lab])] = 1
    return labels, m / (m.sum(-1)[:, None] + 1e-6)


def build_token_index(positive_map, labels, device):
    """[L, MT] int32 token positions per label (-1 padded) + [L] int32 label ids, for the scoring kernel."""
    mt = max(1, max((len(positive_map[l]) for l in labels), default=1))
    idx = torch.full((max(len(labels), 1), mt), -1, dtype=torch.int32)
    for j, l in enumerate(labels):
        toks = positive_map[l] if not isinstance(positive_map[l], int) else [positive_map[l]]
        idx[j, :len(toks)] = torch.tensor(toks, dtype=torch.int32)
    ids = torch.tensor(list(labels) if labels else [0], dtype=torch.int32)
    return idx.to(device, non_blocking=True), ids.to(device, non_blocking=True)


def build_item_token_index(score_maps):
    """`build_token_index` for items that each score their own map (forward_chunks: one per chunk; forward_grounding: one per image):
    score_maps = [(map, labels)] -> host tensors tok3 [items, L, MT] int32 token positions (-1 padded, also the rows of an item with fewer
    than L labels) and lab2 [items, L] int32 label ids (0 padded), L / MT = the largest label count / token count."""
    L = max(1, max(len(l) for _, l in score_maps))
    MT = max(1, max((len(pm[k]) for pm, l in score_maps for k in l), default=1))
    tok3 = torch.full((len(score_maps), L, MT), -1, dtype=torch.int32)
    lab2 = torch.zeros(len(score_maps), L, dtype=torch.int32)
    for c, (pm, l) in enumerate(score_maps):
        for j, k in enumerate(l):
            tok3[c, j, :len(pm[k])] = torch.tensor(pm[k], dtype=torch.int32)
            lab2[c, j] = k
    return tok3, lab2


def prepare_positive_map(positive_map, T, max_kv=0, onehot=False):
    """What a forward needs from the caller's `{label: [token positions]}` for a caption of T positions; returns
    (positive_map, labels_in_caption, pm_key, score_map, score_labels, max_kv):
    - the map with `int` entries listed and positions >= T dropped (the tokenizer's truncation cut them away; the reference would index a
      [L, T] map with them, generalized_vl_rcnn_new.py:295-305), the labels that keep a token, and a hashable key of the two;
    - the map and labels the scoring kernel takes: the map itself, or for SCORE_AGG = ONEHOT class column j = token j, label j + 1
      (`logits[:, :, :len(positive_map)]`, rpn/inference.py:789-791: at most T columns exist);
    - the key-length bound.  `max_kv <= 0` (unknown) passes through; otherwise it is widened to cover every column that will be scored (the
      alignment kernel only computes columns below 16 ceil(max_kv / 16): a map that names a token behind the caption's last live one --
      abnormal, but legal for the reference, which scores all T columns -- must not be scored as 0 inside a MEAN) and clamped to T.
      Scored columns are 0 .. len(positive_map) - 1 with ONEHOT, else up to the cleaned map's highest token.  A ONEHOT map whose TOKENS lie
      beyond both the caption's live length and len(positive_map) does not widen the bound: those columns are never scored."""
    pm = {k: [t for t in ([v] if isinstance(v, int) else v) if t < T] for k, v in positive_map.items()}
    labels = [k for k, v in pm.items() if len(v) != 0]
    pm_key = tuple((k, tuple(pm[k])) for k in labels)
    if onehot:
        scored = min(len(pm), T)
        score_map, score_labels = {j + 1: [j] for j in range(scored)}, list(range(1, scored + 1))
    else:
        scored = 1 + max((max(pm[k]) for k in labels), default=-1)
        score_map, score_labels = pm, labels
    if max_kv > 0:
        max_kv = min(max(max_kv, scored), T)
    return pm, labels, pm_key, score_map, score_labels, max_kv


def text_dropout_rate(cfg):
    """VISION_QUERY.TEXT_DROPOUT when the eval forward masks category words (generalized_vl_rcnn_new.py:397-400), else 0.0: the words of
    every category that has vision queries become [MASK] before the language backbone -- the README's vision-only evaluation
    (`VISION_QUERY.MASK_DURING_INFERENCE True VISION_QUERY.TEXT_DROPOUT 1.0`).  Masking runs with ENABLED, TEXT_DROPOUT > 0,
    MASK_DURING_INFERENCE and NOT NEW_MASK_TOKEN (the learned mask token exists in training only: the reference does nothing with it at
    inference).  The reference asserts PURE_TEXT_RATE == 0 then (:399); any other value is refused here, by name."""
    VQ = cfg.VISION_QUERY
    p = float(VQ.get("TEXT_DROPOUT", 0.0))
    if not (VQ.ENABLED and p > 0.0 and VQ.get("MASK_DURING_INFERENCE", False)):
        return 0.0
    if VQ.get("PURE_TEXT_RATE", 0.0) != 0.0:
        raise NotImplementedError(f"VISION_QUERY.PURE_TEXT_RATE = {VQ.PURE_TEXT_RATE}: must be 0 with VISION_QUERY.MASK_DURING_INFERENCE "
                                  "(the reference asserts it: part text, part vision is not implemented there either)")
    return 0.0 if VQ.get("NEW_MASK_TOKEN", False) else p


def consume_text_dropout_draws(B, n_labels):
    """The draws of `text_dropout_mask` without the mask: one `random.random()` per (image, label)."""
    for _ in range(B * n_labels):
        random.random()


def text_dropout_mask(labels, positive_map, has_query, T, p, B, reference_rng=False):
    """[B, T] bool, True where `input_ids` become the tokenizer's [MASK] id (generalized_vl_rcnn_new.py:401-407, eval), or None when no
    position is masked.  For every image i and, within it, every label j of `labels` (the caption's labels in positive-map order) one
    `random.random()` of Python's global generator is drawn FIRST -- also for labels without vision queries --; label j is masked in image i
    when the draw is < p AND `has_query(label)`: all of `positive_map[label]`.
    p >= 1: every draw succeeds, so the mask is a function of the bank alone and the same for every image; the draws are then skipped
    unless `reference_rng` (VISION_QUERY.REFERENCE_RNG_STREAM: consume the generator exactly like the reference, QuerySelector.__init__).
    Host only: the caller moves the mask to the device."""
    has = [bool(has_query(lab)) for lab in labels]
    if p >= 1.0:
        if reference_rng:
            consume_text_dropout_draws(B, len(labels))
        hit = [has] * B
    else:
        hit = [[(random.random() < p) and h for h in has] for _ in range(B)]       # the draw comes first: `and` must not skip it
    if not any(any(row) for row in hit):
        return None
    mask = torch.zeros(B, T, dtype=torch.bool)
    for i, row in enumerate(hit if p < 1.0 else hit[:1]):
        for lab, h in zip(labels, row):
            if h:
                mask[i, list(positive_map[lab])] = True
    if p >= 1.0:
        mask[1:] = mask[0]
    return mask


class QuerySelector(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.num_query_per_class = cfg.VISION_QUERY.NUM_QUERY_PER_CLASS
        # VISION_QUERY.REFERENCE_RNG_STREAM (not a reference key; default False): consume numpy's global generator once per label
        # on EVERY forward exactly like the reference (query_selector.py:74) -- also when every draw is the identity -- so that a
        # run seeded like a reference run keeps the SAME generator state call for call.  Off: identity draws are
        # skipped and memoised (same selections, no per-forward host work), and the generator state then differs from a
        # reference run's as soon as one caption did not need a real draw.
        self.reference_rng = bool(cfg.VISION_QUERY.get("REFERENCE_RNG_STREAM", False))
        # fine-tuned state (both off in every shipped yaml: nothing below exists then and the selector is what it was)
        self.learnable_bank = bool(cfg.VISION_QUERY.get("LEARNABLE_BANK", False))
        self.add_vision_layer = bool(cfg.VISION_QUERY.get("ADD_VISION_LAYER", False))
        self.query_bank = None
        self._loaded = None                                    # what `load_query_bank` handed over while the bank is a ParameterDict
        self._param_bank = None                                # {int(label): tensor} view of the ParameterDict (dropped with the memos)
        self._snapshot = None                                  # host counts of a resident QueryBank at load time (None: dict bank)
        self._dev_bank = {}
        self._sel_cache = {}
        if self.learnable_bank or self.add_vision_layer:
            self._register_load_state_dict_pre_hook(self._adopt_checkpoint_state)
        path = cfg.VISION_QUERY.QUERY_BANK_PATH
        if path:
            if not os.path.exists(path):
                raise FileNotFoundError(f"query bank path {path} not exists")
            if self.learnable_bank:
                self._make_learnable_bank(torch.load(path, map_location="cpu"))
                self._make_vision_layer()
            else:
                self.load_query_bank(path)

    # ------------------------------------------------------------------ fine-tuned state
    def _make_learnable_bank(self, tensors):
        """The bank as parameters, named like the reference's (:20): `query_bank.<label>` [n, scales, C], frozen."""
        prev = self.__dict__.get("query_bank")
        bank = nn.ParameterDict({str(k): nn.Parameter(v.detach().clone(), requires_grad=False) for k, v in tensors.items()
                                 if torch.is_tensor(v)})       # (an entry without rows stays a key of the state dict; it selects nothing)
        self.query_bank = bank                                  # (nn.Module.__setattr__ takes the plain attribute away)
        if prev is not None:                                    # a bank loaded before the parameters existed stays what is selected from
            self._loaded = prev
        self._drop_memos()

    def _make_vision_layer(self, width=None):
        """`tunable_vision_linear.weight` [1000, C], zero like the reference's (:27-28); C from the bank unless given.  Does nothing without
        the key, when the parameter exists, or while no width is known."""
        if not self.add_vision_layer or "tunable_vision_linear" in self._modules:
            return
        if width is None:
            if not self._has_rows():
                return
            width = self._width()
        self.tunable_vision_linear = Container()
        self.tunable_vision_linear.register_parameter(
            "weight", nn.Parameter(torch.zeros(VISION_LAYER_ROWS, int(width), dtype=torch.float32), requires_grad=False))

    def _has_rows(self):
        bank = self._source()
        if isinstance(bank, QueryBank):
            return bank.pool is not None
        return bank is not None and any(torch.is_tensor(v) and v.numel() for v in bank.values())

    def _adopt_checkpoint_state(self, state_dict, prefix, *_):
        """load_state_dict pre-hook: a checkpoint alone is enough.  The parameters this selector does not own yet are created from the
        incoming keys `query_bank.<label>` / `tunable_vision_linear.weight` with their shapes (the reference needs the original bank
        file for that, :17-28); they are filled by the load that follows.  The memos of rows that depend on parameters are dropped."""
        if self.learnable_bank and not isinstance(self._modules.get("query_bank"), nn.ParameterDict):
            p = prefix + "query_bank."
            found = {k[len(p):]: v for k, v in state_dict.items() if k.startswith(p) and torch.is_tensor(v)}
            if found:
                self._make_learnable_bank(found)
        key = prefix + "tunable_vision_linear.weight"
        if key in state_dict and torch.is_tensor(state_dict[key]) and state_dict[key].dim() == 2:
            self._make_vision_layer(state_dict[key].shape[1])
        self._drop_memos()

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._drop_memos()
        return out

    def _drop_memos(self):
        self._param_bank = None
        self._dev_bank = {}
        self._sel_cache = {}

    def _source(self):
        """The bank the selection reads: what `load_query_bank` handed over last; else the learnable parameters as the plain dict
        `{int(label): tensor}` (same draws, same order, a label without an entry is text-only); else `query_bank` as it is."""
        if self._loaded is not None:
            return self._loaded
        bank = self.query_bank
        if isinstance(bank, nn.ParameterDict):
            if self._param_bank is None:
                self._param_bank = {int(k): v.detach() for k, v in bank.items()}
            return self._param_bank
        return bank

    def _row_add(self, n_rows, device):
        """`tunable_vision_linear.weight` (fp32, on `device`) for items of up to `n_rows` real vision rows; None without the key.  Row v of
        the weight belongs to position v of an item's concatenated rows, v = q * scales + s (query_selector.py:98-99)."""
        if not self.add_vision_layer or "tunable_vision_linear" not in self._modules:
            return None
        w = self.tunable_vision_linear.weight
        if n_rows > w.shape[0]:
            # the reference fails on the shape mismatch of the sum at this point
            raise ValueError(f"VISION_QUERY.ADD_VISION_LAYER: an item holds {n_rows} vision-query rows, tunable_vision_linear has {w.shape[0]}")
        key = ("row_add", str(device))
        if key not in self._dev_bank:
            self._dev_bank[key] = w.detach().to(device=device, dtype=torch.float32).contiguous()
        return self._dev_bank[key]

    def load_query_bank(self, bank):
        """`bank`: path to a torch-saved dict or the dict itself: {label: Tensor[n, scales, C]}, or a device-resident `QueryBank`.
        A `QueryBank` is kept as it is, with a host SNAPSHOT of its counts: its pool and slot table are append-only, so the rows the
        snapshot names stay where they are whatever is admitted later (also across a reallocation: the bank's current tensors are read at
        every call), and rows admitted after this call stay invisible until the bank is loaded again.
        With VISION_QUERY.LEARNABLE_BANK / ADD_VISION_LAYER the reference asserts that this is never called (:34-35).  Here it stays allowed
        and replaces what the selector selects FROM; the parameters `query_bank.<label>` stay in the state dict as they are, and
        `tunable_vision_linear.weight` is created at the first call when no checkpoint or bank file gave its width before."""
        if not isinstance(bank, QueryBank):
            bank = torch.load(bank, map_location="cpu") if isinstance(bank, (str, os.PathLike)) else bank
        if isinstance(self._modules.get("query_bank"), nn.ParameterDict):
            self._loaded = bank
        else:
            self.query_bank = bank
        self._snapshot = (bank, list(bank._counts())) if isinstance(bank, QueryBank) else None
        self._dev_bank = {}
        self._sel_cache = {}
        self._make_vision_layer()

    def _resident(self):
        """The counts snapshot of a resident `QueryBank`; None with a dict bank or none.  (A `QueryBank` assigned to `query_bank` without
        `load_query_bank` is snapshotted at its first use.)"""
        bank = self._source()
        if not isinstance(bank, QueryBank):
            return None
        if self._snapshot is None or self._snapshot[0] is not bank:
            self._snapshot = (bank, list(bank._counts()))
        return self._snapshot[1]

    def _count(self, label):
        """Rows of a label in the resident bank's snapshot (0: none, not an integer label, or beyond the table)."""
        snap = self._resident()
        return snap[label] if isinstance(label, (int, np.integer)) and 0 <= label < len(snap) else 0

    def _candidates(self, label):
        """Bank entry of a label; None when the label has no vision query.  Reference banks are `defaultdict(list)`
        (engine/inference.py:401): a label without queries reads as `[]` and contributes no vision rows
        (query_selector.py:77-78, `isinstance(candidate_queries, list)`); a plain dict without the key is treated alike."""
        bank = self._source()
        cand = bank[label] if (label in bank or hasattr(bank, "default_factory")) else None
        if cand is None or isinstance(cand, (list, tuple)) or len(cand) == 0:
            return None
        return cand

    def has_vision_query(self, label):
        """The reference's `has_vision_query` flag of a label (query_selector.py:77-78): the bank holds at least one row for it."""
        if self._resident() is not None:
            return self._count(label) > 0
        return self._candidates(label) is not None

    def deterministic(self, labels):
        """True when no label of `labels` holds more bank rows than NUM_QUERY_PER_CLASS: the reference's eval-mode draw
        `sorted(np.random.choice(len, n, replace=False))` (query_selector.py:74-76) is then the identity, and the
        selection may be memoised.  Otherwise every forward draws again, from numpy's global generator like the reference.
        (With VISION_QUERY.REFERENCE_RNG_STREAM nothing is memoised: every label of every forward consumes its draw.)"""
        if self.reference_rng:
            return False
        if self._resident() is not None:
            return all(self._count(lab) <= self.num_query_per_class for lab in labels)
        for lab in labels:
            cand = self._candidates(lab)
            if cand is not None and len(cand) > self.num_query_per_class:
                return False
        return True

    def _rows(self, label, device, dtype, draw=False):
        """[n * scales, C] vision rows of one label (n = min(len, k)); None when the label has none.
        draw: consume numpy's global generator exactly like the reference does for EVERY label (:74), also when the draw is
        the identity -- used when some label of the caption holds more than k rows, so that the same seed gives the same
        selection as the reference."""
        if self._resident() is not None:                            # resident bank (only `forward`, the reference-shaped output, comes here)
            pos = self._draw(self._count(label), draw)
            if len(pos) == 0:
                return None
            bank = self._source()
            rows = bank.slots[label].index_select(0, torch.from_numpy(pos).to(bank.slots.device)).long()
            return bank.pool[rows].flatten(0, 1).to(device=device, dtype=dtype)
        cand = self._candidates(label)
        k = self.num_query_per_class
        if draw:
            n_tot = 0 if cand is None else len(cand)
            idx = sorted(np.random.choice(n_tot, min(n_tot, k), replace=False).tolist())
            if cand is None:
                return None
            if n_tot > k:
                return cand[idx].flatten(0, 1).to(device=device, dtype=dtype)
        if cand is None:
            return None
        key = (label, device, dtype)
        if key not in self._dev_bank:
            self._dev_bank[key] = cand[:k].flatten(0, 1).to(device=device, dtype=dtype)
        return self._dev_bank[key]

    def _draw(self, n_tot, draw):
        """Positions in a label's slot row that enter a forward, ascending (int64 array): the reference's draw (:74) when `draw`, consumed
        also when the label has no rows or the draw is the identity; else the first min(n, k)."""
        k = self.num_query_per_class
        if draw:
            return np.sort(np.random.choice(n_tot, min(n_tot, k), replace=False)).astype(np.int64)
        return np.arange(min(n_tot, k), dtype=np.int64)

    def _width(self):
        if self._resident() is not None:
            return 1 if self._source().pool is None else self._source().pool.shape[-1]
        for v in self._source().values():
            if torch.is_tensor(v) and v.numel():
                return v.shape[-1]
        return 1

    def select(self, batched_labels, batched_positive_maps, T, device, dtype):
        """-> vision [B, V, C] (zero padded), idx [B, T, S] int32 (-1 padded).  Labels without bank rows are skipped
        (text-only for that label, like the reference)."""
        if self._resident() is not None:
            return self._select_resident(batched_labels, batched_positive_maps, T, device, dtype)
        per_image, tok_lists = [], []
        # ADD_VISION_LAYER: the rows are assembled in fp32, the offset is added, and the sum is rounded ONCE (the per-label cache in `dtype`
        # would round twice)
        add = self.add_vision_layer and "tunable_vision_linear" in self._modules
        row_dtype = torch.float32 if add else dtype
        for labels, pmap in zip(batched_labels, batched_positive_maps):
            rows, owners = [], [[] for _ in range(T)]
            base = 0
            draw = not self.deterministic(labels)
            for lab in labels:
                r = self._rows(lab, device, row_dtype, draw)
                if r is None:
                    continue
                rows.append(r)
                for t in pmap[lab]:
                    owners[t].extend(range(base, base + r.shape[0]))
                base += r.shape[0]
            if add and rows:
                per_image.append((torch.cat(rows) + self._row_add(base, device)[:base]).to(dtype))
            else:
                per_image.append(torch.cat(rows) if rows else torch.zeros(0, self._width(), device=device, dtype=dtype))
            tok_lists.append(owners)
        vision = torch.nn.utils.rnn.pad_sequence(per_image, batch_first=True)
        S = max(1, max(len(o) for owners in tok_lists for o in owners))
        idx = torch.full((len(tok_lists), T, S), -1, dtype=torch.int32)
        for b, owners in enumerate(tok_lists):
            for t, o in enumerate(owners):
                if o:
                    idx[b, t, :len(o)] = torch.tensor(sorted(o), dtype=torch.int32)
        return vision.contiguous(), idx.to(device, non_blocking=True)

    def _select_resident(self, batched_labels, batched_positive_maps, T, device, dtype):
        """`select` from a resident `QueryBank`: the draws of the dict path in its order (numpy's global generator ends in the same state),
        two integer tables built with numpy -- qsrc [I, Q, 2] = (label, position in the label's slot row) and qtok [I, Q, MT] = the label's
        token positions per selected query, -1 padded --, ONE upload and ONE launch (ops.bank_select) that writes the padded vision rows in
        `dtype` and the gather index.  No per-label copies, no torch.cat / pad_sequence, no loop over the T token positions."""
        bank, I = self._source(), len(batched_labels)
        e_item, e_lab, e_tok, e_pos = [], [], [], []              # one entry per (item, label with rows)
        toks, tok_of = [], {}                                     # distinct token lists of this call: (id(map), label) -> row of tokU
        snap, k = self._resident(), self.num_query_per_class
        first = [np.arange(n, dtype=np.int64) for n in range(k + 1)]          # the identity selections (read only)
        for i, (labels, pmap) in enumerate(zip(batched_labels, batched_positive_maps)):
            ns = [snap[lab] if isinstance(lab, (int, np.integer)) and 0 <= lab < len(snap) else 0 for lab in labels]
            draw = self.reference_rng or max(ns, default=0) > k                # not self.deterministic(labels)
            for lab, n in zip(labels, ns):
                if draw:                                                       # (also for a label without rows: the draw is consumed)
                    pos = self._draw(n, True)
                if n == 0:
                    continue
                if not draw:
                    pos = first[min(n, k)]
                u = tok_of.get((id(pmap), lab))
                if u is None:
                    t = np.asarray(pmap[lab], dtype=np.int64).reshape(-1)
                    if len(t) and (t.min() < -T or t.max() >= T):
                        raise IndexError(f"label {lab}: token position out of range for {T} positions")
                    u = tok_of[(id(pmap), lab)] = len(toks)
                    toks.append(np.where(t < 0, t + T, t))
                e_item.append(i)
                e_lab.append(lab)
                e_tok.append(u)
                e_pos.append(pos)
        if not e_pos:                                             # what pad_sequence makes of I empty images: callers fall back to text only
            return (torch.zeros(I, 0, self._width(), device=device, dtype=dtype),
                    torch.full((I, T, 1), -1, dtype=torch.int32).to(device, non_blocking=True))
        S = bank.pool.shape[1]
        e_item, e_lab, e_tok = np.asarray(e_item), np.asarray(e_lab), np.asarray(e_tok)
        e_n = np.asarray([len(p) for p in e_pos])
        per_item = np.bincount(e_item, weights=e_n, minlength=I).astype(np.int64)
        Q, MT = int(per_item.max()), max(1, max(len(t) for t in toks))
        row_add = self._row_add(Q * S, bank.pool.device)          # (refuses an item with more rows than the offset has, before the launch)
        tokU = np.full((len(toks), MT), -1, dtype=np.int32)
        for u, t in enumerate(toks):
            tokU[u, :len(t)] = t
        # every selected query: its entry, its item and its place q inside the item (entries are in item order already)
        q_e = np.repeat(np.arange(len(e_n)), e_n)
        q_item = e_item[q_e]
        q_in = np.arange(len(q_e)) - (np.cumsum(per_item) - per_item)[q_item]
        tab = np.full(I * Q * (2 + MT), -1, dtype=np.int32)       # qsrc and qtok in one buffer: one upload
        qsrc, qtok = tab[:I * Q * 2].reshape(I, Q, 2), tab[I * Q * 2:].reshape(I, Q, MT)
        qsrc[q_item, q_in, 0] = e_lab[q_e]
        qsrc[q_item, q_in, 1] = np.concatenate(e_pos)
        qtok[q_item, q_in] = tokU[e_tok[q_e]]
        # the longest owner list: rows per (item, token) = sum over the entries that list the token of n * S, counted with multiplicity
        tokE = tokU[e_tok]
        live = tokE >= 0
        owners = np.zeros(I * T, dtype=np.int64)
        np.add.at(owners, (e_item[:, None] * T + tokE)[live], np.broadcast_to((e_n * S)[:, None], tokE.shape)[live])
        smax = max(1, int(owners.max()))
        dev_tab = torch.from_numpy(tab).to(bank.pool.device, non_blocking=True)
        if row_add is None:
            vision, idx = _ops.bank_select(bank.pool, bank.slots, dev_tab[:I * Q * 2].view(I, Q, 2), dev_tab[I * Q * 2:].view(I, Q, MT), T, smax, dtype)
        else:
            vision, idx = _ops.bank_select(bank.pool, bank.slots, dev_tab[:I * Q * 2].view(I, Q, 2), dev_tab[I * Q * 2:].view(I, Q, MT), T, smax, dtype,
                                           row_add=row_add)
        return vision.to(device), idx.to(device)

    def select_cached(self, key, labels, positive_map, B, T, device, dtype):
        """Memoised `select` for B images sharing one caption (eval protocol): no per-call host or device work."""
        if not self.deterministic(labels):
            return self.select([labels] * B, [positive_map] * B, T, device, dtype)
        k = (key, B, T, str(device), dtype)
        hit = self._sel_cache.get(k)
        if hit is None:
            if len(self._sel_cache) > 128:
                self._sel_cache.clear()
            from .graph_runner import memoised
            hit = self._sel_cache[k] = memoised(self.select([labels] * B, [positive_map] * B, T, device, dtype))
        return hit

    def forward(self, batched_label_list, batched_location_map, batched_pos_labels=None):
        """Reference-compatible output (queries, 0/1 attention masks [B,V,T], has_vision_query)."""
        if self._source() is None:
            return None, None, None
        qs, ms, has = [], [], []
        for labels, maps in zip(batched_label_list, batched_location_map):
            q_img, m_img = [], []
            flags = []
            draw = not self.deterministic(labels)
            add = self.add_vision_layer and "tunable_vision_linear" in self._modules
            for lab, loc in zip(labels, maps):
                r = self._rows(lab, loc.device, torch.float32 if add else loc.dtype, draw)
                flags.append(0 if r is None else 1)
                if r is None:
                    continue
                q_img.append(r)
                m_img.append(loc[None].expand(r.shape[0], -1))
            if add and q_img:
                q = torch.cat(q_img)
                qs.append((q + self._row_add(len(q), q.device)[:len(q)]).to(m_img[0].dtype))
            else:
                qs.append(torch.cat(q_img))
            ms.append(torch.cat(m_img))
            has.append(flags)
        q = torch.nn.utils.rnn.pad_sequence(qs, batch_first=True)
        m = torch.nn.utils.rnn.pad_sequence(ms, batch_first=True).clone()
        m[m != 0] = 1
        return q, m, has


def build_query_selector(cfg):
    return QuerySelector(cfg)
