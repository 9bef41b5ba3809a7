"""Exactly-stated Sim(3) graphs for the zero-tolerance tests.  Nothing here is imported by the product.

Every vertex and measurement has R = I, a translation with integer coordinates and a scale in {1/2, 1, 2, 4}; the vertex
translations are multiples of 8 and each measurement's scale is s_j / s_i, so every s_D = 1 exactly, log s_D = 0, the
rotation angle is 0, r = [0, t_D, 0] with integer t_D, Jl^-1 = [[I, 0], [-t_D^ / 2, I]], and with integer information every
number of the linearisation is a multiple of 2^-14 far below 2^53: any order of f64 additions gives the same bits.  The
expected values are computed in int64: J_j times 128, J_i = -J_j Ad times 128, the blocks times 128^2."""
from __future__ import annotations

import numpy as np

SCALE = 128
SCALES = (0.5, 1.0, 2.0, 4.0)


def _hat_int(w):
    W = np.zeros(w.shape[:-1] + (3, 3), np.int64)
    W[..., 0, 1], W[..., 0, 2] = -w[..., 2], w[..., 1]
    W[..., 1, 0], W[..., 1, 2] = w[..., 2], -w[..., 0]
    W[..., 2, 0], W[..., 2, 1] = -w[..., 1], w[..., 0]
    return W


class ExactGraph:
    def __init__(self, name, V, edges, seed, masks=()):
        rng = np.random.default_rng(seed)
        self.name, self.V = name, V
        self.edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        E = self.E = len(self.edges)
        self.s = rng.choice(SCALES, V)
        self.t = 8 * rng.integers(-1, 2, (V, 3))
        self.tz = rng.integers(-2, 3, (E, 3))
        i, j = self.edges[:, 0], self.edges[:, 1]
        self.sz = self.s[j] / self.s[i]
        eye = np.tile(np.eye(3), (V, 1, 1))
        self.sims = np.concatenate([np.concatenate([eye, self.t[:, :, None].astype(float)], 2).reshape(V, 12), self.s[:, None]], 1)
        self.meas = np.concatenate([np.concatenate([eye[:1].repeat(E, 0), self.tz[:, :, None].astype(float)], 2).reshape(E, 12),
                                    self.sz[:, None]], 1)
        off = rng.integers(-1, 2, (E, 7, 7))
        self.info_int = np.triu(off, 1) + np.swapaxes(np.triu(off, 1), 1, 2) + np.eye(7, dtype=np.int64) * rng.integers(1, 6, (E, 7, 1))
        self.info = self.info_int.astype(float)
        self.masks = [np.zeros(V, np.uint8)] + [np.ascontiguousarray(m, np.uint8) for m in masks]

    def jacobians_int(self):
        """(v = t_D [E,3], 128 J_i, 128 J_j) in int64"""
        i, j = self.edges[:, 0], self.edges[:, 1]
        sA8 = np.round(8 * self.s[j] / self.s[i]).astype(np.int64)            # s_A in eighths: {1 .. 64}
        assert np.array_equal(sA8 / 8.0, self.s[j] / self.s[i])
        tA = self.t[j] - (sA8[:, None] * self.t[i]) // 8                        # t_i is a multiple of 8
        v = tA - self.tz                                                        # t_D = s_A (-t_Z / s_Z) + t_A, s_A / s_Z = 1
        E = self.E
        Jj = np.zeros((E, 7, 7), np.int64)                                      # times 16
        Jj[:, np.arange(7), np.arange(7)] = 16
        Jj[:, 3:6, 0:3] = -8 * _hat_int(v)
        Jj[:, 3:6, 6] = 16 * v
        Ad = np.zeros((E, 7, 7), np.int64)                                      # times 8
        Ad[:, np.arange(3), np.arange(3)] = 8
        Ad[:, 3:6, 0:3] = 8 * _hat_int(tA)
        Ad[:, np.arange(3, 6), np.arange(3, 6)] = sA8[:, None]
        Ad[:, 3:6, 6] = -8 * tA
        Ad[:, 6, 6] = 8
        return v, -(Jj @ Ad), 8 * Jj

    def linearize_int(self):
        """(cost, b [V,7], Hd [V,7,7], W [E,7,7]) as f64, from int64 arithmetic"""
        v, Ji, Jj = self.jacobians_int()
        r = np.zeros((self.E, 7), np.int64)
        r[:, 3:6] = v
        Om = self.info_int
        Or = np.einsum("eab,eb->ea", Om, r)
        T_ = lambda A: np.swapaxes(A, 1, 2)
        W = T_(Ji) @ Om @ Jj
        Hd = np.zeros((self.V, 7, 7), np.int64)
        b = np.zeros((self.V, 7), np.int64)
        np.add.at(Hd, self.edges[:, 0], T_(Ji) @ Om @ Ji)
        np.add.at(Hd, self.edges[:, 1], T_(Jj) @ Om @ Jj)
        np.add.at(b, self.edges[:, 0], np.einsum("eba,eb->ea", Ji, Or))
        np.add.at(b, self.edges[:, 1], np.einsum("eba,eb->ea", Jj, Or))
        for A in (W, Hd):
            assert np.abs(A).max() < 2 ** 53
        cost = int(np.einsum("ea,ea->", r, Or))
        return float(cost), b / float(SCALE), Hd / float(SCALE ** 2), W / float(SCALE ** 2)

    def hmul_int(self, fixed, lam, x):
        """(H + lam I) x over the free vertices for integer lam and x [V,7], from int64 arithmetic"""
        v, Ji, Jj = self.jacobians_int()
        Om = self.info_int
        T_ = lambda A: np.swapaxes(A, 1, 2)
        x = np.asarray(x, np.int64)
        i, j = self.edges[:, 0], self.edges[:, 1]
        free = np.asarray(fixed) == 0
        y = np.zeros((self.V, 7), np.int64)
        np.add.at(y, i, np.einsum("eab,eb->ea", T_(Ji) @ Om @ Ji, x[i]))
        np.add.at(y, j, np.einsum("eab,eb->ea", T_(Jj) @ Om @ Jj, x[j]))
        W = T_(Ji) @ Om @ Jj
        both = (free[i] & free[j])[:, None]
        np.add.at(y, i, np.where(both, np.einsum("eab,eb->ea", W, x[j]), 0))
        np.add.at(y, j, np.where(both, np.einsum("eba,eb->ea", W, x[i]), 0))
        y += int(lam) * SCALE ** 2 * x
        y[~free] = 0
        assert np.abs(y).max() < 2 ** 53
        return y / float(SCALE ** 2)


def _chain(V):
    k = np.arange(V - 1)
    return np.stack([k, k + 1], 1)


def _uneven(V, seed):
    rng = np.random.default_rng(seed)
    a = (rng.random(V) < 0.3).astype(np.uint8)
    b = np.zeros(V, np.uint8)
    b[::7] = 1
    b[3:12] = 1                      # a run that starts inside one vertex group of a wave and ends inside the next
    return [a, b]


def exact_graphs(big=True):
    out = []
    for V in (8, 9, 10, 35, 36, 37) + ((512 * 36 - 1, 512 * 36, 512 * 36 + 1) if big else ()):      # one wave, one block, the block cap
        extra = np.array([[0, V - 1], [V // 2, 0], [V - 1, V // 3]])
        out.append(ExactGraph(f"chain{V}", V, np.concatenate([_chain(V), extra]), V, _uneven(V, V)))
    # every degree 0 .. 13: vertex d has d edges into a pool of leaves, alternating direction
    deg_edges = [(d, 14 + (3 * d + q) % 20) if q % 2 else (14 + (3 * d + q) % 20, d) for d in range(14) for q in range(d)]
    out.append(ExactGraph("degrees", 34, np.array(deg_edges), 71, _uneven(34, 72)))
    for deg in (127, 128, 129, 130, 1000):                                                         # the hub threshold and a large hub
        s = np.arange(1, deg + 1)
        spokes = np.where((s % 2 == 0)[:, None], np.stack([np.zeros_like(s), s], 1), np.stack([s, np.zeros_like(s)], 1))
        hub_fixed = np.zeros(deg + 1, np.uint8)
        hub_fixed[0] = 1
        out.append(ExactGraph(f"hub{deg}", deg + 1, np.concatenate([spokes, _chain(deg + 1)[1:]]), deg, [hub_fixed, 1 - hub_fixed] + _uneven(deg + 1, deg)))
    for E in (63, 64, 65):                                                                         # the edge kernel's block
        out.append(ExactGraph(f"edges{E}", 40, np.stack([np.arange(E) % 40, (np.arange(E) * 7 + 3) % 40], 1), E, _uneven(40, E)))
    dup = np.array([[0, 1], [0, 1], [1, 0], [1, 2], [2, 1], [2, 1], [3, 0], [0, 3], [3, 0]])      # duplicate and reversed edges
    out.append(ExactGraph("duplicates", 4, dup, 5, [np.array([0, 1, 0, 0])]))
    return out
