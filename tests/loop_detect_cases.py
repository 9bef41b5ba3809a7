"""The scenes of the loop-candidate tests: small integer tables written directly (no vocabulary), the sizes taken from
slam_loop_limits.  A designed scene carries the answer it exists for in ``expect`` (worked out by hand in the comment beside
it); a random scene has none and is held to tests/loop_detect_ref.py."""
import functools

import numpy as np

DERIVE = 0xFFFFFFFF
N_SIZES = 9
DESIGNED = ("padding", "repeat-and-self", "out-of-range", "all-excluded", "cmax-zero", "limits", "derived", "ties", "one-gbest",
            "exactly-three-quarters", "wide-acc", "neighbour-below-min", "word-filter", "reloc")


def limits():
    from slamhip import loop_detect

    return loop_detect.limits()


class Scene:
    def __init__(self, name, s, common, best, connected=None, own=None, limit=None, min_s=None, mode="loop", expect=None):
        self.name, self.mode, self.expect = name, mode, expect or {}
        self.s = np.atleast_2d(np.asarray(s, np.uint32))
        self.common = np.atleast_2d(np.asarray(common, np.int32))
        self.Q, self.E = self.s.shape
        self.best = np.asarray(best, np.int64).reshape(self.E, -1)
        self.nb = self.best.shape[1]
        self.connected, self.own, self.limit, self.min_s = connected, own, limit, min_s

    def kwargs(self):
        return dict(best_table=self.best, connected=self.connected, own_ids=self.own, limit=self.limit, min_s=self.min_s, nb=self.nb, mode=self.mode)

    def reference(self):
        """The answer of tests/loop_detect_ref.py per query, with the excluded lists as the product builds them."""
        import loop_detect_ref as R

        out = []
        for q in range(self.Q):
            own = -1 if self.own is None else int(np.broadcast_to(self.own, (self.Q,))[q])
            excluded = [] if self.connected is None else [int(x) for x in self.connected[q]]
            if own >= 0:
                excluded.append(own)
            limit = self.E if self.limit is None else int(np.broadcast_to(self.limit, (self.Q,))[q])
            min_s = DERIVE if self.min_s is None else int(np.broadcast_to(self.min_s, (self.Q,))[q])
            out.append(R.candidates_ref([int(x) for x in self.s[q]], [int(x) for x in self.common[q]], self.best.tolist(), excluded, own, limit, min_s,
                                        0 if self.mode == "loop" else 1))
        return out


def sizes():
    T = limits()["tile_entries"]
    return [1, 2, 31, 32, 33, T - 1, T, T + 1, 2 * T + 1]


SHAPES = ((1, 0), (3, 1), (1, 10), (3, 16))             # (Q, nb): every E meets both Q and every nb


def random_scene(name, E, Q, nb, seed, mode="loop"):
    rng = np.random.default_rng(seed)
    common = rng.integers(0, 13, (Q, E)) * (rng.random((Q, E)) < 0.7)
    s = rng.integers(0, 1000, (Q, E)) * (common > 0)
    best = rng.integers(0, E, (E, nb))
    best[rng.random((E, nb)) < 0.3] = -1
    if mode != "loop":
        return Scene(name, s, common, best, mode=mode)
    connected = [rng.integers(0, E, rng.integers(0, 6)).tolist() for _ in range(Q)]
    own = [int(rng.integers(0, E)) if q % 2 == 0 else -1 for q in range(Q)]
    limit = None if seed % 2 else [int(rng.integers(0, E + 1)) for _ in range(Q)]
    min_s = None if seed % 3 == 0 else [DERIVE if q % 2 else int(rng.integers(0, 600)) for q in range(Q)]
    return Scene(name, s, common, best, connected, own, limit, min_s)


def random_scenes():
    out = []
    for n, E in enumerate(sizes()):
        for m, (Q, nb) in enumerate(SHAPES):
            out.append(random_scene(f"random-{n}-{m}", E, Q, nb, 100 + 4 * n + m))
    T = limits()["tile_entries"]
    out += [random_scene("random-reloc-0", 33, 3, 10, 7, "relocalization"), random_scene("random-reloc-1", T + 1, 1, 16, 8, "relocalization")]
    return out


def designed_scenes():
    five = lambda E: [5] * E  # noqa: E731
    none = lambda E, nb: np.full((E, nb), -1)  # noqa: E731
    out = []
    # rows that are all padding: acc = s, gbest = i; acc_max = 30 keeps 4 acc > 90, entry 0 alone
    out.append(Scene("padding", [30, 20, 10], five(3), none(3, 2), min_s=0, expect=dict(ids=[[0]], acc=[[30, 20, 10]], gbest=[[0, 1, 2]])))
    # row 0 repeats 1 and names itself, summed as written: 100 + 50 + 50 + 100
    best = none(4, 3)
    best[0] = [1, 1, 0]
    out.append(Scene("repeat-and-self", [100, 50, 60, 10], five(4), best, min_s=0, expect=dict(ids=[[0]], acc=[[300, 50, 60, 10]], gbest=[[0, 1, 2, 3]])))
    # excluded 7 and -3 and the neighbours 4, 1000 and 2^31 - 1 are outside: five skipped; 2 is excluded; row 3 names itself
    out.append(Scene("out-of-range", [40, 30, 20, 10], five(4), [[4, 1], [1000, -1], [-1, -1], [2 ** 31 - 1, 3]], [[7, -3, 2]], min_s=0,
                     expect=dict(ids=[[0]], acc=[[70, 30, 0, 20]], gbest=[[0, 1, -1, 3]], skipped=5)))
    out.append(Scene("all-excluded", [3, 2, 1], five(3), none(3, 1), [[0, 1, 2]], expect=dict(ids=[[]], acc=[[0, 0, 0]], gbest=[[-1, -1, -1]])))
    out.append(Scene("cmax-zero", [3, 2, 1], [0, 0, 0], none(3, 1), min_s=0, expect=dict(ids=[[]], acc=[[0, 0, 0]])))
    # limit 0: nothing; 1: entry 0 alone, its neighbour 1 is past the limit; E: every group sums to 50, the best of {0,1} is 1, of {2,3} is 2
    out.append(Scene("limits", [[10, 40, 30, 20]] * 3, [five(4)] * 3, [[1], [0], [3], [2]], limit=[0, 1, 4], min_s=0,
                     expect=dict(ids=[[], [0], [1, 2]], acc=[[0, 0, 0, 0], [10, 0, 0, 0], [50, 50, 50, 50]], gbest=[[-1] * 4, [0, -1, -1, -1], [1, 1, 2, 2]])))
    # derived min_s: no connected entry -> 2^31, nothing passes; a connected entry without a shared word -> 0; the query's own entry
    # (s = 1) is not looked at -> 150, and entry 0 (s = 100) fails it
    out.append(Scene("derived", [[100, 200, 300], [100, 200, 0], [100, 1, 150]], [[5, 5, 5], [5, 5, 0], [5, 5, 5]], none(3, 0), [[], [2], [2]], [-1, -1, 1],
                     expect=dict(ids=[[], [1], []], acc=[[0, 0, 0], [100, 200, 0], [0, 0, 0]])))
    # ties: candidate 0 and its neighbour 1 both 50 -> 0; the neighbours 1 and 0 of candidate 3 both 50 -> 1, the earlier position
    best = none(5, 2)
    best[0], best[3] = [1, -1], [1, 0]
    out.append(Scene("ties", [50, 50, 40, 40, 10], five(5), best, min_s=0, expect=dict(ids=[[1]], acc=[[100, 50, 40, 140, 10]], gbest=[[0, 1, 2, 1, 4]])))
    # three retained candidates with one gbest: one member
    out.append(Scene("one-gbest", [10, 10, 90, 5], five(4), [[2], [2], [-1], [-1]], min_s=0, expect=dict(ids=[[2]], acc=[[100, 100, 90, 5]], gbest=[[2, 2, 2, 3]])))
    # 4 x 300 = 3 x 400 exactly is not retained, 301 is
    out.append(Scene("exactly-three-quarters", [400, 300, 301], five(3), none(3, 0), min_s=0, expect=dict(ids=[[0, 2]])))
    # seventeen scores just below 2^31: acc needs 36 bits
    s = [2 ** 31 - 1 - i for i in range(20)]
    best = none(20, 16)
    best[0] = np.arange(1, 17)
    out.append(Scene("wide-acc", s, five(20), best, min_s=0, expect=dict(ids=[[0]], acc=[[sum(s[:17])] + s[1:]], gbest=[list(range(20))])))
    # neighbour 1 lies below min_s = 50 and is no candidate, yet adds its 40
    out.append(Scene("neighbour-below-min", [60, 40, 55], five(3), [[1], [-1], [-1]], min_s=50, expect=dict(ids=[[0]], acc=[[100, 0, 55]], gbest=[[0, -1, 2]])))
    # the word filter: 5 c > 4 x 10 keeps 10 and 9, not 8 and 1; the neighbours that fail it add nothing
    out.append(Scene("word-filter", [10, 99, 20, 99], [10, 8, 9, 1], [[1], [0], [3], [2]], min_s=0, expect=dict(ids=[[2]], acc=[[10, 0, 20, 0]], gbest=[[0, -1, 2, -1]])))
    # relocalisation: no threshold, acc = s, 4 acc > 9 keeps entry 2
    out.append(Scene("reloc", [1, 2, 3], five(3), none(3, 0), mode="relocalization", expect=dict(ids=[[2]], acc=[[1, 2, 3]])))
    return out


def names():
    """The names of every scene; needs no library (the sizes behind ``random-n-m`` are ``sizes()[n]`` and ``SHAPES[m]``)."""
    return list(DESIGNED) + [f"random-{n}-{m}" for n in range(N_SIZES) for m in range(len(SHAPES))] + ["random-reloc-0", "random-reloc-1"]


@functools.lru_cache(None)
def scenes():
    out = {s.name: s for s in designed_scenes() + random_scenes()}
    assert list(out) == names() and len(sizes()) == N_SIZES
    return out
