"""Writes tests/golden/kat_topk.json: hand-derived known answers for the top-k search (knnMatch with k up to 32).

As for make_golden.py, nothing here is captured from a program: every expected value follows in closed form from OpenCV's
knnMatch order (distance ascending, then train index ascending; missing neighbours are (-1, INT32_MAX)) and is written out
below.  No oracle or product code is imported.  Each case: the name of its train set (in "trains"), query rows, k, and the
expected [N, k] tables."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
INT_MAX = 2**31 - 1


def prefix_ones(i):
    """32-byte descriptor whose first i bits (MSB-first within bytes) are 1: d(prefix_ones(a), prefix_ones(b)) = |a - b|."""
    bits = np.zeros(256, np.uint8)
    bits[:i] = 1
    return np.packbits(bits).tolist()


ZEROS, ONES = prefix_ones(0), prefix_ones(256)
PATTERN = [0xA5, 0x3C] * 16                     # an arbitrary row; its complement is at distance 256
COMPLEMENT = [255 - b for b in PATTERN]
cases = []

# 1. ladder: train row i = prefix_ones(i), i = 0..40.  Query prefix_ones(20): row 20 at 0, then (19, 21) at 1, (18, 22) at 2 ...
#    so the k-th place ties between 20 - j and 20 + j and the lower index comes first.
ladder = [prefix_ones(i) for i in range(41)]
for k in (1, 2, 3, 4, 5, 8, 9):
    order = [20] + [r for j in range(1, 21) for r in (20 - j, 20 + j)]
    cases.append({"name": f"ladder_k{k}", "k": k, "train": ladder, "query": [prefix_ones(20)],
                  "idx": [order[:k]], "dist": [[abs(r - 20) for r in order[:k]]]})
# zeros against the ladder: rows in index order at distance = index; ones: from row 40 down, at 256 - index
cases.append({"name": "ladder_ends_k32", "k": 32, "train": ladder, "query": [ZEROS, ONES],
              "idx": [list(range(32)), list(range(40, 8, -1))],
              "dist": [list(range(32)), [256 - r for r in range(40, 8, -1)]]})

# 2. all-equal train rows: every row ties, so the k lowest indices; the complement is at distance 256 from every row
same = [PATTERN] * 50
for k in (3, 7, 16, 32):
    cases.append({"name": f"all_equal_k{k}", "k": k, "train": same, "query": [PATTERN, COMPLEMENT],
                  "idx": [list(range(k)), list(range(k))], "dist": [[0] * k, [256] * k]})

# 3. fewer train rows than k: every row, then (-1, INT32_MAX)
short = [prefix_ones(i) for i in (5, 1, 3)]
for k in (4, 5, 32):
    cases.append({"name": f"short_train_k{k}", "k": k, "train": short, "query": [ZEROS],
                  "idx": [[1, 2, 0] + [-1] * (k - 3)], "dist": [[1, 3, 5] + [INT_MAX] * (k - 3)]})
cases.append({"name": "empty_train_k6", "k": 6, "train": [], "query": [ZEROS, ONES],
              "idx": [[-1] * 6] * 2, "dist": [[INT_MAX] * 6] * 2})

# 4. k = 32 against four distinct distances: row i = prefix_ones(i % 4), i = 0..39 -> ten rows at each of 0, 1, 2, 3 from zeros.
#    The 32 nearest are the ten rows of distance 0, of 1, of 2, then the two lowest rows of distance 3 (3 and 7).
mod4 = [prefix_ones(i % 4) for i in range(40)]
want = list(range(0, 40, 4)) + list(range(1, 40, 4)) + list(range(2, 40, 4)) + [3, 7]
cases.append({"name": "four_distances_k32", "k": 32, "train": mod4, "query": [ZEROS],
              "idx": [want], "dist": [[0] * 10 + [1] * 10 + [2] * 10 + [3, 3]]})
# and k = 12 from prefix_ones(3): distance 0 for i % 4 == 3 (ten rows), then the two lowest rows of distance 1 (i % 4 == 2: rows 2, 6)
cases.append({"name": "four_distances_k12", "k": 12, "train": mod4, "query": [prefix_ones(3)],
              "idx": [list(range(3, 40, 4)) + [2, 6]], "dist": [[0] * 10 + [1, 1]]})

if __name__ == "__main__":
    trains = {}
    for c in cases:                               # each distinct train set once
        name = next((n for n, rows in trains.items() if rows == c["train"]), None)
        if name is None:
            name = c["name"].rsplit("_k", 1)[0]
            trains[name] = c["train"]
        c["train"] = name
    with open(os.path.join(HERE, "kat_topk.json"), "w") as f:
        json.dump({"doc": __doc__.splitlines()[0], "trains": trains, "cases": cases}, f, indent=None)
        f.write("\n")
