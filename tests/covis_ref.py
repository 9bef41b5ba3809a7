"""The covisibility tables by brute force, on another route than slamhip.covisibility (which sorts) and csrc/covis.hip (which
sorts twice): per point the set of free observers, and a dict keyed by (k1, k2) that collects the common points in ascending
order.  With ``fixed=None`` nothing is fixed: the graph as ORB-SLAM keeps it, which slamhip.covisibility refuses."""
import numpy as np


def covisibility_ref(obs_pose, obs_point, K, fixed=None):
    """-> (edges int32 [E,2], weights int32 [E], pair_ptr int32 [E+1], pair_a int32 [P], pair_b int32 [P]).  The input must be
    valid: indices in range and no (pose, point) pair twice."""
    op, ol = np.asarray(obs_pose).reshape(-1).tolist(), np.asarray(obs_point).reshape(-1).tolist()
    free = [True] * int(K) if fixed is None else [not bool(f) for f in np.asarray(fixed).reshape(-1)]
    assert len(free) == K and len(op) == len(ol)
    seen = {}
    for o, (k, l) in enumerate(zip(op, ol)):
        assert 0 <= k < K and l >= 0
        if free[k]:
            assert k not in seen.setdefault(l, {}), "a (pose, point) pair twice"
            seen[l][k] = o
    common = {}
    for l in sorted(seen):
        poses = sorted(seen[l])
        for i, k1 in enumerate(poses):
            for k2 in poses[i + 1:]:
                common.setdefault((k1, k2), []).append((seen[l][k1], seen[l][k2]))
    keys = sorted(common)
    edges = np.array(keys, np.int32).reshape(-1, 2)
    weights = np.array([len(common[k]) for k in keys], np.int32)
    pair_ptr = np.r_[0, np.cumsum(weights)].astype(np.int32)
    flat = [ab for k in keys for ab in common[k]]
    pa, pb = (np.array([ab[i] for ab in flat], np.int32) for i in (0, 1))
    return edges, weights, pair_ptr, pa, pb


def same_tables(got, want):
    """Every one of the five arrays equal in dtype, shape and value."""
    return len(got) == len(want) == 5 and all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
