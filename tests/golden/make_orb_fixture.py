"""Writes tests/golden/orb_desk_320x240.npz: the reference's desk image (1.png, 640x480 RGB) as u8 gray data at 320x240, so the
ORB tests also see real image statistics.  Data only: gray = (77 R + 150 G + 29 B + 128) >> 8, then each 2x2 block is averaged
as (sum + 2) >> 2.  Run once where the reference is present (never on the GPU host):  python tests/golden/make_orb_fixture.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    src = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/1.png"
    rgb = np.asarray(Image.open(src).convert("RGB"), np.int64)
    gray = (77 * rgb[:, :, 0] + 150 * rgb[:, :, 1] + 29 * rgb[:, :, 2] + 128) >> 8
    h, w = gray.shape
    assert (h, w) == (480, 640), gray.shape
    small = (gray[0::2, 0::2] + gray[0::2, 1::2] + gray[1::2, 0::2] + gray[1::2, 1::2] + 2) >> 2
    out = os.path.join(HERE, "orb_desk_320x240.npz")
    np.savez_compressed(out, image=small.astype(np.uint8))
    print(out, os.path.getsize(out), "bytes")
