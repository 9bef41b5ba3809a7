"""The draw generator of the four RANSAC calls, restated from the header comment of slam_tv_essential_ransac_f64 in Python
integers (masked to 64 bits by hand): independent of the kernels and of their host twins.  tests/two_view_ref.py, pnp_ref.py,
homography_ref.py and sim3_ref.py take their draw_sample from here; only the sample size differs between them."""
MASK64 = (1 << 64) - 1


def splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def draw_word(seed, h, d):
    return splitmix(splitmix((seed & MASK64) ^ ((h * 0xD1B54A32D192ED03) & MASK64)) ^ ((d * 0x8CB92BA72F3D8DD7) & MASK64))


def draw_sample(seed, h, n, size):
    """The ``size`` distinct indices of hypothesis h among n >= size: index(d) = ((word(seed, h, d) >> 32) * n) >> 32 for
    d = 0, 1, 2, ..., an index already drawn skipped."""
    out, d = [], 0
    while len(out) < size:
        i = ((draw_word(seed, h, d) >> 32) * n) >> 32
        d += 1
        if i not in out:
            out.append(int(i))
    return out
