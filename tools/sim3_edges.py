"""The CPU-side figures behind the bounds of tests/test_sim3_cpu.py, from the numpy reference (tests/sim3_ref.py, Umeyama by
SVD) and the host twin of csrc/sim3.hip (tests/sim3_twin.py, Horn by Jacobi); no GPU is used.

    python tools/sim3_edges.py > profiles/sim3_edges.log          (--table: the same figures as the tests' BOUNDS table)

One line per (group, family, quantity): the worst error of numpy and of the twin.  A test bound is 16 x the larger of the two.
  * solver   the three-point solver on the 2000 samples and on 200 samples drawn from every family scene, against the planted
             similarity (on the noisy families both errors are the noise, alike; the mirror family has no planted model and
             is measured for orthonormality and determinant only): |R^T R - I|, |det R - 1|, |s / s_true - 1|, |R - R_true|,
             |t - t_true| / (1 + |t_true|);
  * exact    triples and clouds of 40 under rational similarities, against the exact Fractions;
  * refit    noisy clouds of n = 3 ... 1000 at the origin and shifted by 1e4, and the mirror-image cloud of 200 (the best
             proper rotation), against the same fit in np.longdouble;
  * ate      the ATE of a planted similarity of a 200-pose path (0 in exact arithmetic)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import sim3_ref as ref  # noqa: E402
import sim3_twin as tw  # noqa: E402

ROWS = []


def row(group, family, quantity, numpy_value, twin_value):
    ROWS.append((group, family, quantity, float(numpy_value), float(twin_value)))


def ate(model, tr):
    return float(np.sqrt(((ref.apply(model, tr["est"]) - tr["gt"]) ** 2).sum(1).mean()))


def main():
    sets = [("samples", ref.solver_samples())] + [(name, ref.family_samples(name)) for name in ref.family_scenes()]
    for name, (X1, X2, truth) in sets:
        mn, okn = ref.threepoint(X1, X2)
        mt, okt = tw.threepoint(X1, X2)
        assert okn.all() and okt.all(), name
        truth = None if name == "mirror" else truth
        qn, qt = ref.model_quantities(mn, truth), ref.model_quantities(mt, truth)
        for k in qn:
            row("solver", name, k, qn[k], qt[k])
    for n in (3, 40):
        en, et = np.zeros(3), np.zeros(3)
        for c in ref.exact_cases():
            if c["n"] != n:
                continue
            mn = ref.refit(c["X1"], c["X2"])[0]
            mt = tw.threepoint(c["X1"], c["X2"])[0][0] if n == 3 else tw.refit(c["X1"], c["X2"])[0]
            en, et = np.maximum(en, ref.exact_errors(mn, c)), np.maximum(et, ref.exact_errors(mt, c))
        for k, q in enumerate(("scale", "rotation", "translation")):
            row("exact", "triples" if n == 3 else "clouds", q, en[k], et[k])
    for off in (0.0, 1e4):
        wn, wt = {}, {}
        for n in ref.REFIT_SIZES:
            sc = ref.refit_cloud(n, off)
            truth = ref.refit_longdouble(sc["X1"], sc["X2"])
            qn = ref.model_quantities(ref.refit(sc["X1"], sc["X2"])[0], truth)
            qt = ref.model_quantities(tw.refit(sc["X1"], sc["X2"])[0], truth)
            for k in ("scale", "rotation", "translation"):
                wn[k], wt[k] = max(wn.get(k, 0.0), qn[k]), max(wt.get(k, 0.0), qt[k])
        for k in wn:
            row("refit", f"offset_{off:g}", k, wn[k], wt[k])
    mir = ref.family_scenes()["mirror"]
    truth = ref.refit_longdouble(mir["X1"], mir["X2"])
    qn = ref.model_quantities(ref.refit(mir["X1"], mir["X2"])[0], truth)
    qt = ref.model_quantities(tw.refit(mir["X1"], mir["X2"])[0], truth)
    for k in qn:
        row("refit", "mirror", k, qn[k], qt[k])
    tr = ref.trajectory()
    row("ate", "path200", "rmse", ate(ref.refit(tr["est"], tr["gt"])[0], tr), ate(tw.refit(tr["est"], tr["gt"])[0], tr))
    if "--table" in sys.argv:
        for g, f, q, a, b in ROWS:
            print(f'    ("{g}", "{f}", "{q}"): 16 * {max(a, b):.3e},{" " * max(1, 14 - len(f) - len(q))}# numpy {a:.3e} twin {b:.3e}')
        return
    print("group    family         quantity       numpy        twin         twin / numpy")
    for g, f, q, a, b in ROWS:
        ratio = b / a if a > 0 else float("inf") if b > 0 else 1.0
        print(f"{g:8s} {f:14s} {q:12s} {a:12.3e} {b:12.3e} {ratio:10.2f}{'   <-- twin more than 16 x numpy' if ratio > 16 else ''}")


if __name__ == "__main__":
    main()
