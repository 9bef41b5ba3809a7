"""The CPU-side figures behind the constants of tests/test_homography_cpu.py and of csrc/homography.hip, from the numpy
reference (tests/homography_ref.py) and the host twin (tests/hg_twin.py); no GPU is used.

    python tools/homography_edges.py > profiles/homography_edges.log

  * the numpy four-point solver's own errors on the tests' 2000 samples (the yardsticks; the twin gets 16x each), the
    twin's beside them, and the share of samples left out as ill-conditioned for numpy;
  * the spread (s1 - s3) / s2 of the best homography on pure_rotation/t0 and pure_rotation/b1e-6 (HG_ROTATION_ONLY lies
    between the two);
  * the candidates' votes and the distance of the true pose from the nearest candidate on the planar scenes;
  * R_H = S_H / (S_H + S_E) per family, noise-free, and on the planar scenes with 0.5 px noise and 30 % outliers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, p)

import hg_twin  # noqa: E402
import homography_ref as hr  # noqa: E402
import two_view_ref as ref  # noqa: E402
from oracle import oracle  # noqa: E402

ILL = 1e-4          # s7 / s0 of numpy's normalised 8x9 system below this: left out


def solver_errors(H, ok, p1, p2, Ht):
    tr = cm = fr = 0.0
    for s in np.flatnonzero(ok):
        tr = max(tr, float(np.abs(hr.transfer(H[s], p1[s]) - p2[s]).max()))
        cm = max(cm, hr.common_distance(H[s], Ht))
        fr = max(fr, abs(float(np.linalg.norm(H[s])) - 1))
    return tr, cm, fr


def main():
    p1, p2, Ht = hr.fourpoint_samples(0, 2000)
    res = [hr.fourpoint(a, b) for a, b in zip(p1, p2)]
    Hn, okn, cond = np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res])
    keep = okn & (cond >= ILL)
    Ht_, okt = hg_twin.fourpoint(p1, p2)
    print(f"samples 2000: numpy models {okn.sum()}, twin models {okt.sum()}, left out (numpy s7/s0 < {ILL:g} or no model) {(~keep).sum()}"
          f" = {(~keep).mean() * 100:.2f} %")
    print("                 transfer px    |H - H_true|    | |H| - 1 |")
    print("numpy          : %.3e      %.3e      %.3e" % solver_errors(Hn, keep, p1, p2, Ht))
    print("twin           : %.3e      %.3e      %.3e" % solver_errors(Ht_, keep & (okt != 0), p1, p2, Ht))
    scenes = dict(hr.family_scenes())
    print("rotation-only spread (s1 - s3) / s2 of the RANSAC winner (numpy svd / twin):")
    for name in ("pure_rotation/t0", "pure_rotation/b1e-6", "pure_rotation/b1e-3"):
        sc = scenes[name]
        H, mask, _ = hr.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)
        d = hr.decompose(H, sc["K"], sc["px1"], sc["px2"], mask, bound=0.0)
        sv = hg_twin.decompose(sc["px1"], sc["px2"], sc["K"], H, mask)["sv"]
        print(f"  {name:22s} {d['spread']:.3e} / {(sv[0] - sv[2]) / sv[1]:.3e}")
    print("decomposition (numpy): votes, and the true pose's distance from the nearest candidate")
    for name in ("planar/fronto", "planar/tilt60"):
        sc = scenes[name]
        H, mask, st = hr.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)
        d = hr.decompose(H, sc["K"], sc["px1"], sc["px2"], mask)
        err = min(np.linalg.norm(P - np.c_[sc["R"], sc["t"]]) for P in d["pose_all"])
        print(f"  {name:22s} inliers {st[0]} votes {d['count'].tolist()} stats {d['stats'].tolist()} nearest candidate {err:.3e}")
        # the figure NUMPY_POSE of tests/test_homography_cpu.py comes from: numpy's and the twin's decomposition of the TWIN's winner
        Ht, mt, _ = hg_twin.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)
        dn = hr.decompose(Ht, sc["K"], sc["px1"], sc["px2"], mt)
        dt = hg_twin.decompose(sc["px1"], sc["px2"], sc["K"], Ht, mt)
        en, et = (min(np.linalg.norm(P - np.c_[sc["R"], sc["t"]]) for P in d_["pose_all"]) for d_ in (dn, dt))
        print(f"  {name:22s} test figure (the twin's winner decomposed): numpy {en:.3e} twin {et:.3e}")
    print("R_H = S_H / (S_H + S_E), sigma 1, H-RANSAC threshold 3, E-RANSAC threshold 1, 256 hypotheses, seed 0 (numpy floats / twin fixed point):")
    noisy = [(f"planar_noisy/{sc['variant']}", sc) for sc in hr.scenes_planar_noisy()]
    for name, sc in list(scenes.items()) + noisy:
        H = hr.ransac(sc["px1"], sc["px2"], 256, 3.0, 0)[0]
        E = oracle.tv_twin_ransac(sc["px1"], sc["px2"], sc["K"], 256, 1.0, 0)[0]
        sh, se, r = hr.model_scores(H, E, sc["K"], sc["px1"], sc["px2"])
        score, rt = hg_twin.model_score(sc["px1"], sc["px2"], sc["K"], H, E)
        print(f"  {name:28s} S_H {sh:10.3f} S_E {se:10.3f} R_H {r:.4f} / {score[0]} {score[1]} {rt:.4f}")


if __name__ == "__main__":
    main()
