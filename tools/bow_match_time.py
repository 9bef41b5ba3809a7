"""Time of the node-constrained search (slam_bow_match_*).  Device calls are bracketed by HIP events
(slam_timer_start/stop) around one call on device-resident arrays, after a warm-up call; the median and the spread
(min - max) over the rounds are reported.  Host-side lines are wall clock and say so.

    python tools/bow_match_time.py [--rounds R]

  * scene    256 keyframes of 2000 rows and one frame of 2000 rows: every keyframe shares 1200 rows with the frame (three bits
             flipped in each), the other rows are random; the nodes come from slam_bow_transform through a full k = 10, L = 6
             tree of random centres (1 111 111 nodes) at levels_up 4 and 2;
  * group    slam_bow_match_group of 1 and of 256 images (LDS sort by (node, row), gather of the descriptors);
  * search   slam_bow_match_search of 1 pair and of 256 pairs (each keyframe against the frame) - pair table, claims, scan,
             finish - under both scan orders (0: a lane per grouped position, 1: a lane per row), alternating in one session: the
             A/B of the scan mapping;
  * dense    what the library offered before for the same pairs: slam_bf_knn2_batch_u256 (8 launches of 32 pairs; one
             slam_bf_knn2_u256 for the lone pair) by device events, plus the read-back of the tables and the selection of 4k (b, c)
             in numpy on one host core, wall clock.
The dense search compares every row with every row, so it finds the nearest row whatever its node; the node search only looks
inside the node, which is ORB-SLAM's trade.  The matches of both are counted.  The values are a record, not a gate."""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-experiments_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import slamhip  # noqa: E402
from slamhip import bow, bow_match  # noqa: E402
from slamhip._lib import BowGroups, addr  # noqa: E402

import bow_match_ref as R  # noqa: E402
from bow_time import full_tree, opt, spread  # noqa: E402

B, N, SHARED = 256, 2000, 1200


def main():
    rounds = opt("--rounds", 9)
    ctx = slamhip.default_context()
    lib, h = ctx.lib, ctx.handle
    rng = np.random.default_rng(1907)

    def timed(fn):
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    def run(call):
        timed(call)
        return [timed(call) for _ in range(rounds)]

    print(slamhip.load().slam_version().decode())
    print(f"plan for {B} pairs of {N} rows: {bow_match.plan_describe(B, N)}")
    vocab = full_tree(rng, 10, 6)
    dv = vocab.upload(ctx)
    frame = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    kfs = rng.integers(0, 256, (B * N, 32), dtype=np.uint8)
    for b in range(B):
        rows = rng.permutation(N)[:SHARED]
        twin = frame[rng.permutation(N)[:SHARED]].copy()
        for _ in range(3):
            bit = rng.integers(0, 256, SHARED)
            twin[np.arange(SHARED), bit >> 3] ^= (128 >> (bit & 7)).astype(np.uint8)
        kfs[b * N + rows] = twin
    d_kf, d_fr = ctx.upload(kfs), ctx.upload(frame)
    off_kf, off_fr = np.arange(B + 1, dtype=np.int64) * N, np.array([0, N], np.int64)
    pairs = np.stack([np.arange(B), np.zeros(B, np.int64)], axis=1).astype(np.int32)
    d_m, d_c = ctx.malloc(4 * B * N), ctx.malloc(4 * B)

    # ---- the dense path of the parent: top-2 of every pair, then the selection on the host
    tab_i, tab_d = ctx.malloc(8 * B * N), ctx.malloc(8 * B * N)

    def dense_device(P):
        if P == 1:
            slamhip.knn2_device(ctx, d_kf.view(0, 32 * N), N, d_fr, N, tab_i.view(0, 8 * N), tab_d.view(0, 8 * N))
            return
        for g in range(0, P, 32):
            slamhip.knn2_device_batch(ctx, [(d_kf.view(32 * N * p, 32 * N), N, d_fr, N, tab_i.view(8 * N * p, 8 * N), tab_d.view(8 * N * p, 8 * N))
                                            for p in range(g, min(P, g + 32))])

    def dense_host(P):
        idx, dist = tab_i.download(np.int32, (P, N, 2)), tab_d.download(np.int32, (P, N, 2))
        return [R.one_to_one(idx[p], dist[p], R.proposed(idx[p], dist[p]), N) for p in range(P)]

    dense = {}
    for P in (1, B):
        dev = run(lambda: dense_device(P))
        dense_host(P)
        wall = []
        for _ in range(min(rounds, 5)):
            t0 = time.perf_counter()
            m12 = dense_host(P)
            wall.append((time.perf_counter() - t0) * 1e3)
        dense[P] = (np.median(dev), np.median(wall), int(sum((m >= 0).sum() for m in m12)))
        print(f"dense      {P:3d} pair(s) of {N} x {N}: top-2 {spread(dev)}  by device events ({(P + 31) // 32} launch(es)); read-back + numpy selection "
              f"{np.median(wall) * 1e3:10.1f} us  [{min(wall) * 1e3:9.1f} - {max(wall) * 1e3:9.1f}]  wall clock on one host core; "
              f"{dense[P][2] / P:.0f} matches / pair")

    for up in (4, 2):
        nodes_kf, nodes_fr = ctx.malloc(4 * B * N), ctx.malloc(4 * N)
        words = ctx.malloc(4 * B * N)
        for rows, n, out in ((d_kf, B * N, nodes_kf), (d_fr, N, nodes_fr)):
            assert lib.slam_bow_transform(h, rows.ptr, n, dv.node_desc.ptr, dv.child.ptr, dv.word_of_node.ptr, vocab.n_nodes, 6, up, 0, words.ptr,
                                          out.ptr) == 0
        n_nodes = len(np.unique(nodes_fr.download(np.int32, (N,))))
        sets = {}
        for name, rows, nodes, off in (("kf", d_kf, nodes_kf, off_kf), ("fr", d_fr, nodes_fr, off_fr)):
            n = int(off[-1])
            out = [ctx.malloc(32 * n), ctx.malloc(4 * n), ctx.malloc(4 * n), ctx.malloc(4 * n)]
            for images in sorted({1, len(off) - 1}):
                def group():
                    assert lib.slam_bow_match_group(h, rows.ptr, nodes.ptr, addr(off), images, *(o.ptr for o in out)) == 0

                v = run(group)
                if name == "kf":
                    print(f"group      levels_up {up}, {images:3d} image(s) of {N} rows: {spread(v)}  {np.median(v) * 1e3 / images:8.2f} us / image")
            sets[name] = (out, BowGroups(out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, None, addr(off), len(off) - 1))
        g1, g2 = sets["kf"][1], sets["fr"][1]
        for P in (1, B):
            med, bits = {}, {}
            for order in (0, 1, 0, 1):                  # the two scan mappings, alternating in one session
                def search():
                    assert lib.slam_bow_match_search(h, ctypes.byref(g1), ctypes.byref(g2), addr(pairs), P, bow_match.TH_LOW, bow_match.RATIO, order,
                                                     d_m.ptr, d_c.ptr, None, None) == 0

                med.setdefault(order, []).extend(run(search))
                bits.setdefault(order, d_m.download(np.int32, (P * N,)).tobytes() + d_c.download(np.int32, (P,)).tobytes())
            assert bits[0] == bits[1], "the two scan orders disagree"
            found = int(d_c.download(np.int32, (P,)).sum())
            for order in (0, 1):
                print(f"search     levels_up {up} ({n_nodes} nodes in the frame), {P:3d} pair(s), scan order {order}: {spread(med[order])}  "
                      f"{np.median(med[order]) * 1e3 / P:8.2f} us / pair, {found / P:.0f} matches / pair")
            t = np.median(med[0])
            dev, wall, _ = dense[P]
            verdict = "is faster than" if t < dev else "loses to"
            print(f"ratio      levels_up {up}, {P:3d} pair(s): the node search (scan order 0) takes {t / dev:6.3f} of the dense top-2 alone - it {verdict} "
                  f"the dense path's device part - and {t / (dev + wall):6.3f} of the dense path with its read-back and host selection")
        for o in sets["kf"][0] + sets["fr"][0] + [nodes_kf, nodes_fr, words]:
            o.free()
    for o in (d_kf, d_fr, d_m, d_c, tab_i, tab_d):
        o.free()
    vocab.free()


if __name__ == "__main__":
    main()
