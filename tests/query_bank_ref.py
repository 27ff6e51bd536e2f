"""TEST INFRASTRUCTURE ONLY.  Shared by tools/gen_golden_query_bank.py (which drives the REFERENCE's extract_query / online_update with it) and
by the query-bank tests (which drive this project's): the fp64 replay of the admission loop that measures how far every similarity lies from
the threshold, the seeded candidate generator, and the stand-in model / data of the online-update runs."""
import numpy as np
import torch

MARGIN = 1e-4      # every similarity the reference computes lies at least this far from the threshold (fp32 dot of 256 normalised terms: ~1.5e-5)


def replay(cands, labels, calls, thr):
    """The admission loop restated in fp64.  cands [M, S, C], labels [M] (all candidates of all calls, in order); calls = [{"lo", "hi",
    "exclude", "maxq"}].  -> (banks after every call as {label: [candidate ids]}, smallest |similarity - thr| over every comparison made,
    number of comparisons above / below the threshold)."""
    c64 = torch.as_tensor(cands).double().flatten(1)
    n64 = c64 / c64.norm(dim=1).clamp_min(1e-12)[:, None]
    labels = [int(l) for l in labels]
    bank, out, dmin, above, below = {}, [], float("inf"), 0, 0
    for call in calls:
        for i in range(call["lo"], call["hi"]):
            cur = bank.setdefault(labels[i], [])
            if len(cur) >= call["maxq"]:
                continue
            if call["exclude"] and cur:
                sims = n64[cur] @ n64[i]
                dmin = min(dmin, float((sims - thr).abs().min()))
                above += int((sims > thr).sum())
                below += int((sims <= thr).sum())
                if bool((sims > thr).any()):
                    continue
            cur.append(i)
        out.append({l: list(v) for l, v in bank.items() if v})
    return out, dmin, above, below


def clustered(rng, n, S, C, labels, centres_per_label=3, dup=0.15):
    """n candidates [n, S, C] fp32 around per-label cluster centres: small noise (cosine to the centre ~0.97), large noise (~0.6) or an exact
    copy of an earlier candidate of the same label -- both branches of the similarity test are taken, none near the threshold."""
    labs = rng.choice(labels, n)
    out = np.zeros((n, S, C), np.float32)
    for i in range(n):
        same = [j for j in range(i) if labs[j] == labs[i]]
        if same and rng.random() < dup:
            out[i] = out[rng.choice(same)]
            continue
        crng = np.random.default_rng([7, int(labs[i]), int(rng.integers(centres_per_label))])
        centre = crng.standard_normal((S, C))
        centre /= np.linalg.norm(centre, axis=-1, keepdims=True)
        sigma = (0.18 if rng.random() < 0.6 else 1.3) / np.sqrt(C)
        out[i] = ((centre + rng.standard_normal((S, C)) * sigma) * rng.uniform(0.5, 4.0)).astype(np.float32)
    return out, labs.astype(np.int64)


# ---------------------------------------------------------------------------------------------- online update: stand-in data and model
class Images:
    """What the loops see of an image batch: `.to(device)` and the image ids the stand-in model seeds its detections with."""

    def __init__(self, ids):
        self.ids = list(ids)

    def to(self, device):
        return self


def loader(image_ids, batch):
    """batches (images, targets, image_ids) like the reference's data loader; targets are dicts (never moved, never read)"""
    return [(Images(image_ids[n:n + batch]), [{} for _ in image_ids[n:n + batch]], image_ids[n:n + batch]) for n in range(0, len(image_ids), batch)]


class Loader(list):
    dataset = None


K_DET, C_FEAT, N_CHUNKS, IMG_SIZE = 12, 64, 2, (400, 300)
SCORES = np.array([0.25, 0.5, 0.5, 0.75, 0.875], np.float32)      # SCORE_THRESHOLD of the runs is 0.5: a score of exactly 0.5 is dropped


class StandInModel:
    """Seeded detections and 'backbone features' per (state, image id): state = rows of the bank file loaded last (0 before any load), so
    a turn that reloads the saved file sees other detections than the first.  Detection k of an image has x1 = 10 + 2 k (20 x 30 boxes well
    inside the image: expand_bbox drops none), and `pooler` maps a box back to k and returns row k of the image's feature table."""

    def __init__(self, cfg, boxlist_cls, extract):
        self.cfg, self.BoxList, self._extract, self.state, self.loads, self.log = cfg, boxlist_cls, extract, 0, [], []

    def eval(self):
        return self

    def load_query_bank(self, path):
        from mq_det_amd.query_bank import load_bank_file
        bank = load_bank_file(path)
        self.state = sum(len(v) for v in bank.values() if torch.is_tensor(v))
        self.loads.append((path, self.state))

    def table(self, image_id):
        rng = np.random.default_rng([11, self.state, image_id])
        out = np.zeros((K_DET, C_FEAT), np.float32)
        for k in range(K_DET):
            centre = np.random.default_rng([13, int(rng.integers(4))]).standard_normal(C_FEAT)
            centre /= np.linalg.norm(centre)
            sigma = (0.18 if rng.random() < 0.6 else 1.3) / np.sqrt(C_FEAT)
            out[k] = (centre + rng.standard_normal(C_FEAT) * sigma) * rng.uniform(0.5, 4.0)
        return out

    def __call__(self, images, captions=None, positive_map=None, return_backbone_features=False):
        assert return_backbone_features and len(captions) == len(images.ids)
        c = int(captions[0].split("#")[1])
        per = K_DET // N_CHUNKS
        out = []
        for i in images.ids:
            rng = np.random.default_rng([17, self.state, i, c])
            k = np.arange(c * per, (c + 1) * per)
            x1 = 10.0 + 2.0 * k
            bl = self.BoxList(torch.tensor(np.stack([x1, np.full(per, 20.0), x1 + 20, np.full(per, 50.0)], 1), dtype=torch.float32), IMG_SIZE,
                              mode="xyxy")
            bl.add_field("scores", torch.from_numpy(rng.choice(SCORES, per)))
            bl.add_field("labels", torch.from_numpy(rng.integers(1, 4, per).astype(np.int64)))
            out.append(bl)
        return out, [torch.from_numpy(np.stack([self.table(i) for i in images.ids]))]

    def pooler(self, visual_features, boxlists, reduce_mean=False):
        rows, labels = [], []
        for b, bl in enumerate(boxlists):
            k = torch.round((bl.bbox[:, 0] + 5 - 10) / 2).long()
            rows.append(visual_features[0][b, k])
            labels.append(bl.get_field("labels"))
        rows = torch.cat(rows)
        self.log.append((rows.clone(), torch.cat(labels).clone()))
        return rows if reduce_mean else rows[:, :, None, None]

    def extract_query(self, *a, **k):
        return self._extract(self, *a, **k)


def log_replay(log, maxq, thr):
    """replay() over the candidates the pooler saw, one call per extract_query"""
    cands = torch.cat([r for r, _ in log])[:, None]
    labels = torch.cat([l for _, l in log]).tolist()
    calls, lo = [], 0
    for r, _ in log:
        calls.append({"lo": lo, "hi": lo + len(r), "exclude": True, "maxq": maxq})
        lo += len(r)
    banks, dmin, above, below = replay(cands, labels, calls, thr)
    return cands, banks, dmin, above, below
