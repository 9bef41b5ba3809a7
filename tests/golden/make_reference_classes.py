"""Writes tests/golden/reference_classes.json: the member names (``__slots__`` entries, ``self.x`` assigned in ``__init__``,
methods) of the reference's Frame / MapPoint / Feature / Map classes (primitives.py, backend.py), as
``tests/test_reference_overlay_cpu.py::_class_members`` reads them from the syntax trees.  Names only: the test that checks
the hand-made stand-ins against them then runs without the reference.

    python tests/golden/make_reference_classes.py REFERENCE_DIR
"""
import ast
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = ("Frame", "MapPoint", "Feature", "Map")


def reference_classes(ref_dir):
    spec = importlib.util.spec_from_file_location("overlay_test", os.path.join(HERE, "..", "test_reference_overlay_cpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    real = {}
    for fname in ("primitives.py", "backend.py"):
        with open(os.path.join(ref_dir, fname)) as f:
            for k, v in mod._class_members(ast.parse(f.read())).items():
                real.setdefault(k, set()).update(v)
    return {cls: sorted(real[cls]) for cls in CLASSES}


if __name__ == "__main__":
    with open(os.path.join(HERE, "reference_classes.json"), "w") as f:
        json.dump(reference_classes(sys.argv[1]), f, indent=1)
        f.write("\n")
