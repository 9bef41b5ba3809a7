"""The CPU-side figures behind the bounds of tests/test_sim3_opt_cpu.py, from the numpy statement (tests/sim3_opt_ref.py:
central-difference Jacobians, numpy sums, np.linalg.solve) and the host twin of csrc/sim3_opt.hip (tests/sim3_opt_twin.py:
analytic Jacobians, the header's summation order, LDL^T); no GPU is used.

    python tools/sim3_opt_edges.py > profiles/sim3_opt_edges.log      (--table: the same figures as the tests' BOUNDS table)

One line per (scene, quantity): the error of numpy's and of the twin's output model, |s / s_true - 1|, |R - R_true| (Frobenius)
and |t - t_true| / (1 + |t_true|).  The truth of an 'exact' scene is the planted similarity; the truth of a 'noisy' scene is
the minimiser of the plain cost over the pairs stage 2 ran on, next to numpy's model (undamped Gauss-Newton to a standstill,
sim3_opt_ref.polished): what is measured there is how far the fixed 5 + 10 / 5 iterations stop from it.  A test bound is
16 x the larger of the two.  Then the conditions on the scenes (planted outliers kept, planted inliers kept, the Huber cost
at the start and at the end), the Jacobian against central differences, and the work per scene."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import sim3_opt_ref as ref  # noqa: E402
import sim3_opt_twin as tw  # noqa: E402

K = ref.EUROC
QUANTITIES = ("scale", "rotation", "translation")


def main():
    rows, notes = [], []
    for name, (sc, start, kind) in ref.scene_list().items():
        r = ref.optimize(sc, start)
        m, mask, chi2, st, work = tw.optimize(sc["X1"], sc["X2"], sc["px1"], sc["px2"], start, K, sc["sigma2"], with_work=True)
        assert np.array_equal(mask, r["mask"]) and st[0] == r["stats"][0] and st[2] == r["stats"][2], name
        truth = sc["model"] if kind == "exact" else ref.polished(sc, r["model"], r["fitted"])
        en, et = ref.model_errors(r["model"], truth), ref.model_errors(m, truth)
        for q, a, b in zip(QUANTITIES, en, et):
            rows.append((name, q, a, b))
        ti = sc["true_inlier"]
        h0 = ref.cost(start, sc, K, r["start_active"], np.sqrt(ref.TH2))[0]
        h1 = ref.cost(r["model"], sc, K, r["start_active"], np.sqrt(ref.TH2))[0]
        notes.append(f"scene {name:20s} inliers {st[0]:3d} nBad {st[2]:3d} planted outliers kept {int(mask[~ti].sum())} planted inliers kept "
                     f"{mask[ti].mean():.3f} huber cost {h0:.4e} -> {h1:.4e} twin steps {st[1]:2d} trials {work[0]:2d} linearisations {work[1]:2d}"
                     f" status {st[3]} | numpy steps {r['stats'][1]:2d} trials {r['work']['trials']:2d}")
    if "--table" in sys.argv:
        for f, q, a, b in rows:
            print(f'    ("{f}", "{q}"): 16 * {max(a, b):.3e},{" " * max(1, 34 - len(f) - len(q))}# numpy {a:.3e} twin {b:.3e}')
        return
    print("scene                quantity       numpy        twin")
    for f, q, a, b in rows:
        print(f"{f:20s} {q:12s} {a:12.3e} {b:12.3e}")
    print()
    for n in notes:
        print(n)
    sc, start, _ = ref.scene_list()["noisy_s1_out30"]
    worst = 0.0
    for i in range(len(sc["X1"])):
        p = np.concatenate([sc["X1"][i], sc["X2"][i], sc["px1"][i], sc["px2"][i], sc["sigma2"][i]])
        J = tw.pair(start, p, K)[3]
        Jn = np.zeros((4, 7))
        for k in range(7):
            x = np.zeros(7)
            x[k] = ref.STEP
            Jn[:, k] = (tw.pair(tw.retract(start, x), p, K)[0] - tw.pair(tw.retract(start, -x), p, K)[0]) / (2 * ref.STEP)
        worst = max(worst, float(np.abs(J - Jn).max() / np.abs(J).max()))
    print(f"\njacobian noisy_s1_out30: analytic against central differences of the twin's residual, worst |dJ| / max |J| over 200 pairs: {worst:.3e}")


if __name__ == "__main__":
    main()
