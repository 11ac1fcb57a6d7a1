"""The bf16 k-NN segmentation golden (tests/golden/seg_knn_bf16.npz): the rules the maker and the tests share.  Pure numpy.

The problem is seg_knn_cases.py's (400 keys, 160 queries, D = 64), drawn the same way from its own seed.  The reference at
``dtype="bfloat16"`` casts keys and queries to bf16 and ranks bf16 DISTANCES; those carry 8 significant bits, tie in bulk, and
``torch.topk`` leaves ties open, so its neighbour lists are one arbitrary member of a set of valid answers.  The golden
therefore stores the reference's bf16 distance matrices (as uint16 bit patterns) and the tests check membership of that set:

VALIDITY.  A list of k neighbours is a valid top-k of the reference's distances, with ``slack`` bf16 steps, when the largest
reference distance among the k listed keys does not exceed the reference's k-th smallest distance (over the keys that are not
skipped) by more than ``slack`` steps.  One step is one unit in the last place of a bf16 value: the distance between the two
neighbouring bf16 numbers, 2^-8 at values in [0.5, 1).  Steps are counted on the bit patterns (``ordinal``), which are monotone.

CLEAR BOUNDARY.  (query, k, distance) is clear when the reference's k-th and (k+1)-th smallest distances differ by MORE than
one step.  Then the reference's neighbour SET is unique and any answer valid within one step has exactly that set, hence -
the vote being a function of the set - exactly the reference's per-pixel prediction.

``f64_lists`` is the float64 ordering of the bf16-ROUNDED operands under the (distance, key row index) rule: the definition
the engine implements in f32, written here in numpy, not the code under test.  What the maker measured at the stored seed
(MAX_SLACK is its acceptance condition, not a result of the engine): L2 valid with 0 steps, cosine within 1 step - the price
of rounding the operands once instead of normalising in bf16."""
import numpy as np

import seg_knn_cases as KC

MAX_SLACK = {"L2": 0, "cosine": 1}        # steps the maker accepts for the f64 ordering (condition (b))
MIN_CLEAR_FRACTION, MIN_CLEAR_PER_CELL = 0.40, 8   # condition (a)


def round_bf16(x):
    """f32 array -> the f32 values of its round-to-nearest-even bf16 cast (torch's ``.to(torch.bfloat16)``; no NaN here)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16
    return r.view(np.float32)


def ordinal(bits):
    """uint16 bf16 bit patterns -> int32, monotone in the value (a difference is a number of bf16 steps)."""
    b = bits.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def f64_distances(q, k):
    """{"L2": squared distance, "cosine": distance} in float64 of the bf16-rounded rows (KC.oracle_distances' expressions)."""
    return {name: d for name, (d, _) in KC.oracle_distances(round_bf16(q), round_bf16(k)).items()}


def f64_lists(q, k, keep, kmax):
    """{distance: int64 [n, kmax]} key row indices by (f64 distance of the rounded operands, index) over the kept keys."""
    rows = np.nonzero(keep)[0]
    out = {}
    for name, d in f64_distances(q, k).items():
        out[name] = np.stack([rows[np.lexsort((rows, d[i, rows]))[:kmax]] for i in range(d.shape[0])])
    return out


def boundaries(ref_bits, keep, ks=KC.KS):
    """The reference's sorted ordinals over the kept keys -> {k: (k-th smallest ordinal [n], clear [n] bool)}."""
    s = np.sort(ordinal(ref_bits)[:, keep], axis=1)
    return {k: (s[:, k - 1], s[:, k] - s[:, k - 1] > 1) for k in ks}


def slack_steps(ref_bits, keep, lists, ks=KC.KS):
    """The largest excess, in bf16 steps and over all queries and k, of the worst reference distance among lists[:, :k]
    over the reference's k-th smallest (<= 0: valid with zero slack)."""
    o = ordinal(ref_bits)
    b = boundaries(ref_bits, keep, ks)
    assert keep[lists].all()
    return max(int((np.take_along_axis(o, lists[:, :k], 1).max(1) - b[k][0]).max()) for k in ks)


def clear_counts(ref, keep, ks=KC.KS):
    """{(distance, k): number of clear queries} for ref = {distance: bits}."""
    return {(name, k): int(boundaries(bits, keep, ks)[k][1].sum()) for name, bits in ref.items() for k in ks}


def condition_a(counts, n_queries):
    return (sum(counts.values()) >= MIN_CLEAR_FRACTION * n_queries * len(counts)
            and min(counts.values()) >= MIN_CLEAR_PER_CELL)


def kept(key_labels):
    """Keys whose mode label (the smallest value on a tie, torch.mode) is not ignored."""
    modes = np.asarray([np.bincount(row, minlength=256).argmax() for row in key_labels])
    return ~np.isin(modes, KC.IGNORE)
