"""What the per-slot buffers of a batch in flight share (resample.ResizeSlot, metrics.ScoreSlot, niqe.NiqeSlot, clipiqa.ClipIqaSlot,
musiq.MusiqSlot, maniqa.ManiqaSlot; metrics.DistsColumn stands last in a batch's scorers and reads the DISTS values ScoreSlot holds): the pool
they are kept in, the final size of every image of a batch, and the grouping of a batch's images into device calls. Host code only.

The scorer slots have one life cycle, which pipeline._Batch drives without knowing which is which: fill() / plan() on the host says what
the batch's rows are (the predictions first, then - with copies=2 - the stage-1 images), reserve() grows the scratch, queue(first, images,
results=None) puts the calls for rows first .. first + n - 1 on the current stream, download() queues the copy to the host, and scores(first,
count) reads a tuple per row once that copy has completed.
"""
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np


class Pooled:
    """A class whose instances are kept on the context, one per (tag, staging slot): get() makes it at the first use. The slots of "sync"
    (process) and "stream" (process_stream, two of them) never share buffers, so a batch in flight is not overwritten."""

    @classmethod
    def get(cls, ctx, slot=0, tag="sync"):
        pool = ctx.__dict__.setdefault("_slots", {})
        key = (cls.__name__, tag, slot)
        if key not in pool:
            pool[key] = cls(ctx)
        return pool[key]


def record_sizes(records) -> List[Tuple[int, int]]:
    """The final size (h, w) of every image of a resize batch: the LANCZOS target, else the valid rectangle of the network's output."""
    return [tuple(rec.geo.lanczos[::-1]) if rec.geo.lanczos else tuple(rec.geo.valid_hw) for rec in records]


def final_sizes(what: str, n: int, h: int, w: int, records=None, rects=None, sizes=None, gts=None, min_edge: Optional[int] = None) -> List[Tuple[int, int]]:
    """The size (h, w) every image of a batch of n images is scored at, the network's output being h x w.
    what="gt", the paired scores: the final sizes of the resize records, else the png rectangles `rects`, else the ground truths' own sizes when
    there is one per image, else the whole output. Every ground truth is then checked against its size (metrics.check_ground_truth; min_edge is
    the smallest edge the scorers take), so a mismatch raises ValueError with both sizes before anything is launched for the batch.
    what="niqe" / "clipiqa" / "musiq" / "maniqa", the no-reference scores: the resize records, the png rectangles, `sizes` (niqe_rects), the ground truths' sizes, the
    whole output. Only a resized result may be larger than the network's output."""
    def ints(rr):
        return [tuple(int(v) for v in r) for r in rr]

    paired = what == "gt"
    if records is not None:
        finals = record_sizes(records)
    elif rects is not None:
        finals = ints(rects)
    elif sizes is not None and not paired:
        finals = ints(sizes)
    elif gts is not None and (len(gts) == n or not paired):
        finals = [tuple(np.shape(g)[:2]) for g in gts]
    else:
        finals = [(h, w)] * n
    if paired:
        from .metrics import check_ground_truth
        check_ground_truth(gts, finals, **({"min_edge": min_edge} if min_edge is not None else {}))
        for i, (gh, gw) in enumerate(finals):
            if gh > h or gw > w:
                raise ValueError(f"gt: ground truth {i} is {gh} x {gw}, the network's output is {h} x {w}")
        return finals
    if len(finals) != n:
        raise ValueError(f"{what}: {len(finals)} sizes for a batch of {n} images")
    for i, (fh, fw) in enumerate(finals):
        if fh < 1 or fw < 1 or (records is None and (fh > h or fw > w)):
            raise ValueError(f"{what}: image {i} is scored at {fh} x {fw}, the network's output is {h} x {w}")
    return finals


def spans(shapes: Sequence[Tuple[int, int]], results: Optional[Sequence], n: int) -> Iterator[Tuple[int, int, object]]:
    """The device calls of n images whose sizes are shapes[0 .. n - 1]: (i, k, result) for the images i .. k - 1. Consecutive plain crops of one
    size share a call (result is None); an image with a resized result - results[i] is not None - is a call of its own."""
    i = 0
    while i < n:
        r = results[i] if results is not None else None
        k = i + 1
        while r is None and k < n and shapes[k] == shapes[i] and (results is None or results[k] is None):
            k += 1
        yield i, k, r
        i = k
