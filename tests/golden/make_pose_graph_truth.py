#!/usr/bin/env python3
"""Writes tests/golden/pose_graph_truth.npz: the inputs of the pose-graph sweep (angles 1e-12 .. 3.0999 rad and two beyond the
contract, translation parts 1e-3 .. 1e3, five families of information matrices) and, per sample and family, the 80-digit
mpmath truth of one edge's linearisation rounded to f64 (tests/pose_graph_truth.py has the definitions).  Needs mpmath; the
tests that read the fixture do not.

    python tests/golden/make_pose_graph_truth.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "slam-experiments_amd")]

import pose_graph_truth as T  # noqa: E402

if __name__ == "__main__":
    fx = T.build_fixture()
    np.savez_compressed(T.FIXTURE, **fx)
    print(f"{T.FIXTURE}: {len(fx['xi'])} samples, {os.path.getsize(T.FIXTURE)} bytes")
