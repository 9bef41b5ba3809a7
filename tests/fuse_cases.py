"""Scenes the fusion tests share, built so that the expected answer is known by construction: a small map seen
by a few keyframes a short baseline apart, every landmark with one feature in every frame, some landmarks held twice (a
duplicate map point that one keyframe made on its own), and hand-built frames for the cases that tell Fuse from
SearchByProjection."""
import numpy as np

import proj_match_ref as R

CAMERA = (256.0, 256.0, 320.0, 240.0)
SIZE = (640, 480)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SCALE, SCALE2 = R.scale_tables(8, 1.2)
I34 = np.eye(4)[:3]


def flip_bits(rng, desc, k):
    out = desc.copy()
    for i in range(len(out)):
        for b in rng.choice(256, k, replace=False):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def project(T, X, camera=CAMERA):
    c = X @ T[:, :3].T + T[:, 3]
    return np.stack([camera[0] * c[:, 0] / c[:, 2] + camera[2], camera[1] * c[:, 1] / c[:, 2] + camera[3]], 1)


def world(seed, n_land, n_frames=3, n_dup=0, n_clutter=20, p_seen=0.5, noise=0.3, flips=6):
    """``n_land`` landmarks in front of ``n_frames`` cameras (centres 0.15 apart, no rotation).  Every frame has one feature
    per landmark - at its projection plus ``noise``, on the level the landmark's range predicts, its descriptor ``flips`` bits
    from the landmark's - and ``n_clutter`` random features, rows shuffled.  Map point m < n_land is landmark m, observed in
    frame 0 always (the first ``n_dup``: never) and in each other frame with probability ``p_seen`` (the first ``n_dup``: in
    all of them); map point n_land + k is a DUPLICATE of landmark k < n_dup, observed in frame 0 only.  Returns a dict: pts
    (xyz, desc, range, normal over all M map points), frames (list of dict desc, xy, level, point), lists, poses, centres,
    row_of int [n_frames, n_land], land int [M] the landmark of each map point."""
    rng = np.random.default_rng(seed)
    centres = np.stack([np.array([0.15 * b, 0.05 * b, 0.0]) for b in range(n_frames)])
    poses = np.stack([np.c_[np.eye(3), -c] for c in centres])
    u, v = rng.uniform(60, SIZE[0] - 60, n_land), rng.uniform(60, SIZE[1] - 60, n_land)
    z = rng.uniform(4.0, 10.0, n_land)
    X = np.stack([(u - CAMERA[2]) / CAMERA[0] * z, (v - CAMERA[3]) / CAMERA[1] * z, z], 1)
    d0 = np.linalg.norm(X, axis=1)
    level = rng.integers(0, 6, n_land)
    dmax = d0 * SCALE[level] * 0.93                      # s[l-1] d < dmax < s[l] d from every camera: the predicted level is l
    dmin = dmax / SCALE[-1]
    normal = X / d0[:, None]
    desc = rng.integers(0, 256, (n_land, 32), dtype=np.uint8)
    land = np.concatenate([np.arange(n_land), np.arange(n_dup)])
    M = len(land)
    seen = rng.uniform(size=(n_land, n_frames)) < p_seen
    seen[:, 0] = True
    seen[:n_dup, 0] = False
    seen[:n_dup, 1:] = True
    frames, row_of = [], np.zeros((n_frames, n_land), np.int64)
    for b in range(n_frames):
        xy = np.concatenate([project(poses[b], X) + rng.normal(0, noise, (n_land, 2)),
                             np.stack([rng.uniform(0, SIZE[0], n_clutter), rng.uniform(0, SIZE[1], n_clutter)], 1)]).astype(np.float32)
        fd = np.concatenate([flip_bits(rng, desc, flips), rng.integers(0, 256, (n_clutter, 32), dtype=np.uint8)])
        fl = np.concatenate([level, rng.integers(0, 8, n_clutter)]).astype(np.int32)
        perm = rng.permutation(n_land + n_clutter)
        row_of[b] = np.argsort(perm)[:n_land]
        point = np.full(n_land + n_clutter, -1, np.int32)
        point[row_of[b][seen[:, b]]] = np.flatnonzero(seen[:, b])
        if b == 0:
            point[row_of[0][:n_dup]] = n_land + np.arange(n_dup)
        frames.append(dict(desc=np.ascontiguousarray(fd[perm]), xy=np.ascontiguousarray(xy[perm]), level=fl[perm], point=point))
    lists = [[(b, int(row_of[b][m])) for b in range(n_frames) if seen[m, b]] for m in range(n_land)]
    lists += [[(0, int(row_of[0][k]))] for k in range(n_dup)]
    pts = dict(xyz=X[land] + 0.0, desc=np.concatenate([desc, flip_bits(rng, desc[:n_dup], 3)]), range=np.stack([dmin * dmin, dmax * dmax], 1)[land],
               normal=normal[land])
    return dict(pts=pts, frames=frames, lists=lists, poses=poses, centres=centres, row_of=row_of, land=land, n_land=n_land)


def subset(pts, idx):
    """The point-set dict of the map points ``idx`` (with their ids)."""
    idx = np.asarray(idx, np.int64).reshape(-1)
    d = {k: np.ascontiguousarray(v[idx]) for k, v in pts.items() if v is not None}
    d["id"] = idx.astype(np.int32)
    return d


def keyframe_sets(W):
    """One point set per frame: the map points it observes, ascending."""
    B = len(W["frames"])
    return [np.array(sorted(m for m, l in enumerate(W["lists"]) if any(f == b for f, _ in l)), np.int64) for b in range(B)]


def expected(W, idx, b):
    """By construction, for the map points ``idx`` fused into frame b: (status, row, other) - 5 where the point is observed
    there, else linked (0) to its landmark's feature, whose holder is ``other``."""
    st, row, ot = [], [], []
    for m in idx:
        r = int(W["row_of"][b][W["land"][m]])
        if any(f == b for f, _ in W["lists"][m]):
            st.append(5), row.append(-1), ot.append(-1)
        else:
            st.append(0), row.append(r), ot.append(int(W["frames"][b]["point"][r]))
    return np.array(st, np.int32), np.array(row, np.int32), np.array(ot, np.int32)


def ref_pair(F, W, sets, a, b, **kw):
    """tests/fuse_ref.search for the pair (set a, frame b) of the world W."""
    return F.search(subset(W["pts"], sets[a]), W["frames"][b], b, W["lists"], W["poses"][b], W["centres"][b], kw.pop("th", 3.0), CAMERA,
                    kw.pop("bounds", BOUNDS), SCALE, SCALE2, **kw)


def flat_frame(xy, level, desc, point=None):
    """A hand-built frame for the points of ``flat_points``."""
    n = len(level)
    return dict(desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32), xy=np.asarray(xy, np.float32).reshape(n, 2),
                level=np.asarray(level, np.int32), point=np.full(n, -1, np.int32) if point is None else np.asarray(point, np.int32))


def flat_points(uv, desc, ids=None):
    """Points at depth 1 under the identity pose and the unit camera: they project onto ``uv`` exactly.  No range, no normal,
    level 0: the predicted level is 0 and the radius ``th``."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    n = len(uv)
    return dict(xyz=np.c_[uv, np.ones(n)], desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
                id=np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids, np.int32), level=np.zeros(n, np.int32))


def ones(k):
    """A descriptor with its first k bits set."""
    d = np.zeros(32, np.uint8)
    d[:k // 8] = 255
    if k % 8:
        d[k // 8] = (1 << (k % 8)) - 1
    return d
