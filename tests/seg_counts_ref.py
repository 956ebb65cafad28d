"""NumPy model of the segmentation counts (mccnn_seg_counts_add, segmentation_counts) and of the two scoring rules on top of
them (segmentation_scores, part_iou): a plain loop over the rows, written from the definition in include/mccnn.h, plus the
inputs the CPU and GPU tests share."""
import functools

import numpy as np


def counts(pred, labels, C, batch_ids=None, B=1, weights=None, ignore=-1, start=None):
    """-> int64 [B, C, 3] (intersection, union, ground truth), added to a copy of `start` when given."""
    out = np.zeros((B, C, 3), np.int64) if start is None else np.array(start, np.int64).reshape(B, C, 3).copy()
    pred, labels = np.asarray(pred).reshape(-1), np.asarray(labels).reshape(-1)
    for i in range(len(labels)):
        l, p = int(labels[i]), int(pred[i])
        b = 0 if batch_ids is None else int(batch_ids[i])
        if not 0 <= l < C or (ignore >= 0 and l == ignore) or not 0 <= b < B:
            continue
        if weights is not None and weights[i] == 0:    # (-0.0 == 0; a NaN is not)
            continue
        out[b, l, 2] += 1
        out[b, l, 1] += 1
        if p == l:
            out[b, l, 0] += 1
        elif 0 <= p < C:
            out[b, p, 1] += 1
    return out


def _ratio(num, den):
    return float(num) / float(den) if den > 0 else 1.0


def scores(cnt, ignore=-1):
    """The ScanNet rule -> dict(iou [C], acc [C], meanIoU, meanAcc, totalAcc), float64."""
    c = np.asarray(cnt, np.int64).sum(0)
    C = c.shape[0]
    iou = np.array([_ratio(c[k, 0], c[k, 1]) for k in range(C)])
    acc = np.array([_ratio(c[k, 0], c[k, 2]) for k in range(C)])
    keep = [k for k in range(C) if k != ignore]
    mean = lambda v: float(np.sum([v[k] for k in keep])) / len(keep) if keep else 1.0   # noqa: E731
    return dict(iou=iou, acc=acc, meanIoU=mean(iou), meanAcc=mean(acc),
                totalAcc=_ratio(sum(int(c[k, 0]) for k in keep), sum(int(c[k, 2]) for k in keep)))


def part_iou(cnt, mask):
    """The ShapeNet rule -> float64 [B]: the mean over a cloud's masked classes of I / U (1.0 where U is 0; 1.0 for an empty
    mask)."""
    cnt = np.asarray(cnt, np.int64)
    out = np.ones(cnt.shape[0])
    for b in range(cnt.shape[0]):
        parts = [k for k in range(cnt.shape[1]) if mask[b][k]]
        if parts:
            out[b] = float(np.sum([_ratio(cnt[b, k, 0], cnt[b, k, 1]) for k in parts])) / len(parts)
    return out


# ------------------------------------------------------------------------------------------------- shared inputs
def draw(n, B, C, seed, clouds="contiguous", weights=True, ignore=-1):
    """Labels in [-1, C] and predictions that hit about half the rows, the others anywhere in [-2, C + 1]: some of either fall
    outside [0, C) on both sides. Batch ids in contiguous clouds of unequal size ("contiguous"), shuffled row by row
    ("shuffled") or absent (None); about 2 % of them are -1 or B. Weights: 1 / 0 / 0.5 / 2, or None."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(-1, C + 1, n).astype(np.int32)
    pred = np.where(rng.random(n) < 0.5, labels, rng.integers(-2, C + 2, n)).astype(np.int32)
    bid = None
    if clouds is not None:
        cuts = np.sort(rng.integers(0, n + 1, B - 1))
        bid = np.searchsorted(cuts, np.arange(n), side="right").astype(np.int32)   # (unequal sizes, some perhaps empty)
        if clouds == "shuffled":
            bid = rng.permutation(bid)
        bad = rng.random(n) < 0.02
        bid[bad] = rng.choice(np.array([-1, B], np.int32), int(bad.sum()))
    rw = rng.choice(np.array([1.0, 0.0, 0.5, 2.0], np.float32), n, p=[0.6, 0.2, 0.1, 0.1]) if weights else None
    return dict(pred=pred, labels=labels, bid=bid, rw=rw, B=B, C=C, ignore=ignore, n=n)


def scannet_case(n=20000, C=21):
    """The ScanNet form: one cloud, no batch ids, label 0 ignored, weights with 0, -0.0f, NaN and negative values."""
    d = draw(n, 1, C, 77, clouds=None, weights=False, ignore=0)
    rng = np.random.default_rng(78)
    d["rw"] = rng.choice(np.array([1.0, 0.0, -0.0, np.nan, -1.5, 0.25], np.float32), n).astype(np.float32)
    assert np.signbit(d["rw"][d["rw"] == 0]).any() and np.isnan(d["rw"]).any()
    return d


TAILS = (63, 64, 65, 255, 257, 1000)
CASES = {
    "one-hit": lambda: dict(pred=np.array([1], np.int32), labels=np.array([1], np.int32), bid=None, rw=None, B=1, C=2, ignore=-1, n=1),
    "one-miss": lambda: dict(pred=np.array([0], np.int32), labels=np.array([1], np.int32), bid=None, rw=None, B=1, C=2, ignore=-1, n=1),
    "many": lambda: draw(70001, 32, 50, 5),
    "interleaved": lambda: draw(4099, 7, 6, 6, clouds="shuffled"),
    "no-table": lambda: draw(5000, 64, 400, 7),
    "scannet": scannet_case,
}
for _n in TAILS:
    CASES["tail-%d" % _n] = functools.partial(draw, _n, 3, 5, 100 + _n)
SMALL = ["one-hit", "one-miss"] + ["tail-%d" % n for n in TAILS] + ["interleaved", "no-table", "scannet"]   # (quick on the CPU)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs, counts of the model from zeros). Computed once and shared: treat both as read-only."""
    d = CASES[name]()
    want = counts(d["pred"], d["labels"], d["C"], d["bid"], d["B"], d["rw"], d["ignore"])
    for a in list(d.values()) + [want]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d, want
