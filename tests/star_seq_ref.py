"""The oracle's starfield main loop (Draw; Update, frame by frame), shared by the starfield
sequence tests.  Not a test module."""
import numpy as np

import oracle

# a session that takes both wraps of Update: long frames push every z below 0, the negative
# frame time pushes some above 1, and the 1e9 ms frame leaves every z near -5e5
SCRIPT = [0, 16, 17, 400, 1300, 16, 2000, -700, 16, 0.5, 33, 1e9, 16]

_DEN = np.frombuffer(np.uint32(3).tobytes(), np.float32)[0]      # a denormal
SPECIAL_STARS = np.array([[0, 0, 0], [1, 1, 0], [-1, 0.5, -0.0], [0.25, -0.25, _DEN], [0.5, 0.5, np.inf],
                          [0.5, 0.5, np.nan], [np.inf, 0.1, 0.5], [0.1, 0.2, 0.5], [-0.3, 0.1, 0.9]], np.float32)
SPECIAL_DTS = [0, 16, -700, np.inf, 16, np.nan, 16, 0]


def oracle_run(stars, dts, n_updates, n_frames, W, H):
    """(frames [n_frames, W*H], final stars, wraps): frame f is the oracle's Draw after f updates;
    wraps = (stars with z <= 0 before an update, stars with z > 1 after that wrap), summed."""
    s = np.array(stars, np.float32).reshape(-1, 3).copy()
    frames = np.zeros((n_frames, W * H), np.uint32)
    low = high = 0
    with np.errstate(invalid="ignore"):
        for f in range(max(n_frames, n_updates)):
            if f < n_frames:
                frames[f] = oracle.starfield_draw(s, W, H)
            if f < n_updates:
                z = s[:, 2]
                low += int((z <= 0).sum())
                high += int((np.where(z <= 0, z + np.float32(1), z) > 1).sum())
                oracle.starfield_update(s, float(np.float32(dts[f])))
    frames.setflags(write=False)
    s.setflags(write=False)
    return frames, s, (low, high)


def same_stars(got, ref):
    """bit-equal where the reference is not NaN, NaN where it is"""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    if got.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]) and np.isnan(got[nan]).all())
