"""CPU float64 reference of ``scoring.score_rank``'s contract, stated literally:

    beats(j)  = (s_j > s_h and j != h) or (s_j == s_h and j < h)
    place[r]  = #{ j in the catalogue, j not in seen(r) : beats(j) }          (0-based)

the (score desc, item id asc) order of ``score_topk``.  ``places`` takes the logits as given (any
float dtype; compared as they are), so a test decides what the scores are."""
import numpy as np


def beats(s_j, j, s_h, h) -> bool:
    return bool((s_j > s_h and j != h) or (s_j == s_h and j < h))


def places(logits, held, seen_rows=None) -> np.ndarray:
    """``logits [n, I]``, ``held [n]`` item ids, ``seen_rows``: per row, the item ids left out
    (None: nothing is).  Returns int64 ``[n]``."""
    logits = np.asarray(logits)
    held = np.asarray(held).astype(np.int64)
    n, I = logits.shape
    ids = np.arange(I)
    out = np.zeros(n, dtype=np.int64)
    for r in range(n):
        h = int(held[r])
        s, sh = logits[r], logits[r, h]
        b = ((s > sh) & (ids != h)) | ((s == sh) & (ids < h))
        if seen_rows is not None and len(seen_rows[r]):
            b[np.asarray(seen_rows[r], dtype=np.int64)] = False
        out[r] = int(b.sum())
    return out


def places_literal(logits, held, seen_rows=None) -> np.ndarray:
    """The same count item by item through ``beats`` (the slow form the vectorised one is
    checked against)."""
    logits = np.asarray(logits)
    n, I = logits.shape
    out = np.zeros(n, dtype=np.int64)
    for r in range(n):
        h = int(held[r])
        gone = set() if seen_rows is None else {int(x) for x in seen_rows[r]}
        out[r] = sum(1 for j in range(I)
                     if j not in gone and beats(logits[r, j], j, logits[r, h], h))
    return out
