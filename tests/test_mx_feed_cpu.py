"""CPU suite: the prepared-image feed of the 32x32x64 matrix-core top-2 search (bf_mx32.hip: bf_mx_image_kernel and
bf_mx32_image_top2_kernel) without a GPU - the image restated in numpy (which byte of it holds which source word, by the
formula of the in-kernel staging, and that a 32x32x64 dot over it is the Hamming distance), the form of the image-fed kernel
in the built library's gfx950 code object (the MFMA form, registers, scratch and LDS of the shipped kernel; a stage is four
direct-to-LDS copies per thread that stay in flight behind the whole-stage trip, and no ds_write_b128 is left; the epilogue's
cross-workgroup hand-off as tests/test_isa_handoff_cpu.py pins it), and the routing between the two feeds against its rule."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_isa_handoff_cpu as H
import test_mx32_cpu as X                                       # the expand map, the MFMA restatement and the listing checks: one copy

STAGE = 128                                                     # SLAM_MX_STAGE
ROW_BYTES = 128                                                 # an expanded row: 8 source words x 16 bytes


# ---- the image ----------------------------------------------------------------------------------------------------------

def piece_offset(row, word):
    """Byte offset in the image of the 16 bytes that hold source word `word` (0..7) of train row `row`.  The in-kernel staging
    (bf_mx32_scan.inc) has thread tid carry half sh = tid & 1 of row srow = tid >> 1 of a stage, word 4 sh + j going to
    dst0[(j >> 1) * 64 + (j & 1) * 32] with dst0 = tile + (srow >> 5) * 256 + sh * 128 + (srow & 31), in units of 16 bytes;
    the image is those stages one after the other."""
    stage, srow = divmod(row, STAGE)
    sh, j = divmod(word, 4)
    return 16 * (stage * STAGE * 8 + (srow >> 5) * 256 + sh * 128 + (srow & 31) + (j >> 1) * 64 + (j & 1) * 32)


def image(t):
    """bf_mx_image_kernel in numpy: t [M, 8] uint32 -> the image as uint32 words, rows padded to whole stages with the row of
    zero bits."""
    m = len(t)
    rows = (m + STAGE - 1) // STAGE * STAGE
    tp = np.zeros((rows, 8), np.uint32)
    tp[:m] = t
    img = np.zeros(rows * ROW_BYTES // 4, np.uint32)
    for row in range(rows):
        for word in range(8):
            o = piece_offset(row, word) // 4
            img[o:o + 4] = X.expand(tp[row, word])
    return img


def test_the_offsets_tile_the_image_exactly_once():
    offs = np.array([piece_offset(r, w) for r in range(3 * STAGE) for w in range(8)])
    assert sorted(offs.tolist()) == list(range(0, 3 * STAGE * ROW_BYTES, 16))
    # K-quarter q = word // 2, half hk = word % 2: group of 32 rows -> [quarter][lane = (row & 31) + 32 hk] x 16 bytes
    for r in (0, 1, 31, 32, 127, 128, 200, 383):
        for w in range(8):
            assert piece_offset(r, w) == 16 * ((r // 32) * 256 + (w // 2) * 64 + (r & 31) + 32 * (w % 2))


def test_a_stage_of_the_image_is_what_a_lane_reads_as_its_operand():
    """The search reads, for group g of a stage and K-quarter kq, tile[g * 256 + kq * 64 + lane] (16 bytes): over the image
    that must be X.operand of the group's rows, and the four dots of a group must give 256 - 2 x Hamming."""
    rng = np.random.default_rng(3)
    m = 2 * STAGE + 77                                           # a ragged last stage
    t = rng.integers(0, 1 << 32, (m, 8), dtype=np.uint64).astype(np.uint32)
    t[:len(X.EDGE_ROWS)] = X.EDGE_ROWS
    t[m - len(X.EDGE_ROWS):] = X.EDGE_ROWS
    q = rng.integers(0, 1 << 32, (32, 8), dtype=np.uint64).astype(np.uint32)
    q[5], q[6], q[7] = t[0], ~t[1], t[m - 1] ^ np.uint32(1)
    img = image(t).reshape(-1, 4)                                # [16-byte piece, 4 words]
    b = X.operand(q)
    rows = len(img) * 16 // ROW_BYTES
    tp = np.zeros((rows, 8), np.uint32)
    tp[:m] = t
    for g in range(rows // 32):
        a = img[g * 256:(g + 1) * 256].reshape(4, 64, 4)         # [K-quarter][lane]
        assert np.array_equal(a, X.operand(tp[32 * g:32 * g + 32]))
        d = sum(X.mfma_32x32x64(a[kq], b[kq]) for kq in range(4))
        assert np.array_equal((256 - d) // 2, X.popcount_dist(tp[32 * g:32 * g + 32], q)) and (d % 2 == 0).all()
    # the rows past M hold the fill nibble everywhere: +1.0 in every element, the row of zero bits
    pad = np.concatenate([img[piece_offset(r, w) // 16] for r in range(m, rows) for w in range(8)])
    assert (pad == 0x22222222).all()


def test_a_thread_s_four_copies_cover_the_stage():
    """Piece j of wave w, lane l: bytes 4096 j + 1024 w + 16 l of the stage, in the image and in LDS alike."""
    got = sorted(4096 * j + 1024 * w + 16 * l for j in range(4) for w in range(4) for l in range(64))
    assert got == list(range(0, STAGE * ROW_BYTES, 16))


# ---- the built kernel ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def image_kernel(built, tmp_path_factory):
    """(disassembly of bf_mx32_image_top2_kernel, its metadata note, its mangled name) from the library the package loads."""
    if not (os.path.exists(X.OBJDUMP) and os.path.exists(X.READELF)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    from slamhip import _lib

    tmp = str(tmp_path_factory.mktemp("mx_feed_isa"))
    local = os.path.join(tmp, "lib.so")
    shutil.copy(_lib.LIB_PATH, local)
    subprocess.run([X.OBJDUMP, "--offloading", local], cwd=tmp, check=True, capture_output=True)
    for f in sorted(os.listdir(tmp)):
        if "gfx950" not in f:
            continue
        obj = os.path.join(tmp, f)
        text = subprocess.run([X.OBJDUMP, "-d", obj], check=True, capture_output=True, text=True).stdout
        m = re.search(r"^[0-9a-f]+ <(_Z\d+bf_mx32_image_top2_kernel\w*)>:$", text, re.M)
        if not m:
            continue
        assert not m.group(1)[2:].lstrip("0123456789").startswith("bf_top2_mx32_kernel")   # the shipped kernel's tests find theirs by that prefix
        body = text[m.end():].split("\n\n", 1)[0]
        notes = subprocess.run([X.READELF, "--notes", obj], check=True, capture_output=True, text=True).stdout
        meta = next(b for b in re.split(r"\n\s+- \.agpr_count", notes) if re.search(r"\.name:\s+" + m.group(1) + r"\n", b))
        return body, "\n    - .agpr_count" + meta, m.group(1)
    pytest.fail("bf_mx32_image_top2_kernel is not in the library")


def test_the_kernel_has_the_form_of_the_shipped_one(image_kernel):
    k = image_kernel[:2]
    X.test_every_mfma_is_the_fp4_32x32x64_form(k)
    X.test_accumulators_stay_in_vgprs(k)                        # no AGPR moves
    X.test_four_waves_per_simd_no_scratch_and_lds_of_four_blocks(k)   # <= 128 VGPRs, no scratch, LDS <= 40960 B
    X.test_fold_is_integer(k)


def _instructions(body):
    return [ln.split("//")[0].strip() for ln in body.splitlines() if ln.split("//")[0].strip()]


def test_a_stage_is_four_direct_copies_and_no_expanded_store(image_kernel):
    ins = _instructions(image_kernel[0])
    assert not [i for i in ins if i.startswith("ds_write_b128")]                 # nothing is expanded in this kernel
    glds = [k for k, i in enumerate(ins) if i.startswith("global_load_lds_dwordx4")]
    assert len(glds) == 8                                                        # the chunk start's four and the trip's four
    bars = [k for k, i in enumerate(ins) if i.startswith("s_barrier")]
    spans = [(a, b) for a, b in zip(bars[:-1], bars[1:]) if sum(i.startswith("v_mfma") for i in ins[a:b]) >= 64]
    assert len(spans) == 1, "the scan between two stage barriers"
    a, b = spans[0]
    trip = [k for k in glds if a < k < b]
    assert len(trip) == 4 and trip[-1] - trip[0] <= 12                           # one statement, at the trip's start
    # the copies stay in flight behind the whole trip: the 32 MFMAs of the trip follow them with no wait on vmcnt in between,
    # and a wait for all of them stands between the last copy and the stage barrier
    k, seen = trip[-1] + 1, 0
    while seen < 32:
        assert k < b and "vmcnt" not in ins[k], ins[k]
        seen += ins[k].startswith("v_mfma")
        k += 1
    assert any(i.startswith("s_waitcnt") and "vmcnt(0)" in i for i in ins[k:b])
    # and the chunk start's copies are waited for in front of the barrier that opens the chunk's first stage
    first = [k for k in glds if k < a]
    assert len(first) == 4
    nxt = min(x for x in bars if x > first[-1])
    assert any(i.startswith("s_waitcnt") and "vmcnt(0)" in i for i in ins[first[-1]:nxt])
    # every copy names a scalar base and one vector offset: no vector address arithmetic per copy
    assert all(re.fullmatch(r"global_load_lds_dwordx4 v\d+, s\[\d+:\d+\]", ins[k]) for k in glds), [ins[k] for k in glds]


def test_the_epilogue_hands_off_as_the_other_top2_kernels_do(image_kernel):
    body, _, name = image_kernel
    ins = [i for i in _instructions(body) if not re.match(r"^[0-9a-f]+ <", i)]
    kernels = {name: ins, **{f"{name}#{k}": ins for k in range(6)}}             # the pinned checks count kernels: the same one seven times
    H.test_every_merge_atomic_returns({name: ins})
    H.test_ticket_sits_behind_wait_and_barrier_and_the_last_arriver_reads_with_atomics(kernels)
    adds = [i for i in ins if i.startswith("global_atomic_add")]
    assert len(adds) >= 3 and all(" sc0" in i for i in adds), adds


# ---- routing ------------------------------------------------------------------------------------------------------------

def rule(n, m):
    """DESIGN.md 3c "Feed": the shapes that feed 0 runs from the prepared image, among those the 32x32x64 kernel runs: the box
    the measured gains span."""
    return 65536 <= n <= 131072 and 65536 <= m <= 200000


def test_auto_takes_the_image_exactly_inside_the_measured_box(built):
    import slamhip

    for n in (1, 500, 8192, 20000, 65535, 65536, 65537, 100000, 131072, 131073, 262144, 1 << 20):
        for m in (1, 16384, 40000, 65535, 65536, 65537, 100000, 131072, 199999, 200000, 200001, 1 << 20):
            assert slamhip.mx_feed_describe(n, m, 0) == (2 if rule(n, m) else 1), (n, m)
            assert slamhip.mx_feed_describe(n, m, 1) == 1
            assert slamhip.mx_feed_describe(n, m, 2) == 2


def test_only_feeds_0_1_2_exist(built):
    import slamhip
    from slamhip import _lib
    from slamhip._lib import SlamHipError

    for feed in (-1, 3, 4, 1 << 20):
        with pytest.raises(SlamHipError):
            slamhip.mx_feed_describe(4096, 4096, feed)
        assert _lib.load().slam_bf_set_mx_feed(None, feed) == _lib.SLAM_ERR_INVALID
    # the engine numbers stay as they were: the feed is no engine
    with pytest.raises(SlamHipError):
        slamhip.mx_tile_describe(4096, 4096, 4)
