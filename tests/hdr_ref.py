"""The exposure chain restated in numpy: luminance, bin, frame record, exposure with adaptation,
tone curves and PutPixelSDL, all in np.float32 and integer arithmetic, each float operation
written out on its own so that nothing can be fused or reordered.  tests/test_hdr.py pins it by
hand and compares the library's host helpers with it; tests/test_hdr_gpu.py compares the kernels
with it.  Arrays of floats are compared as bit patterns (.view(np.uint32)) throughout."""
import numpy as np

BINS = 256
BIN_BASE = 888
TONE_LINEAR, TONE_REINHARD, TONE_REINHARD_WHITE = 0, 1, 2
CHUNK = 8            # frames of one exposure step inside cg_rt_render_exposed(_device)
F = np.float32

_err = dict(all="ignore")


def f32(x):
    return np.asarray(x, dtype=np.float32)


def from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def luminance(x, y, z):
    with np.errstate(**_err):
        a = F(0.2126) * f32(x)
        b = F(0.7152) * f32(y)
        c = F(0.0722) * f32(z)
        ab = (a + b).astype(np.float32)
        return (ab + c).astype(np.float32)


def counted(L):
    with np.errstate(**_err):
        return f32(L) > F(0.0)           # False for NaN, +-0, negatives; True for +inf


def bin_of(L):
    """int32: the bin of each L, -1 where it is not counted."""
    L = f32(L)
    b = (bits(L).astype(np.int64) >> 20) - BIN_BASE
    return np.where(counted(L), np.clip(b, 0, BINS - 1), -1).astype(np.int32)


def bin_edge(b):
    return from_bits(((np.asarray(b, np.int64) + BIN_BASE + 1) << 20).astype(np.uint32))


def stats_of(pixels):
    """(hist uint32[256], record dict) of one plane float32[n, 3 or 4]."""
    px = f32(pixels)
    L = luminance(px[:, 0], px[:, 1], px[:, 2])
    if px.shape[1] == 4:
        with np.errstate(**_err):
            cov = px[:, 3] > F(0.0)
    else:
        cov = np.ones(len(px), bool)
    cnt = cov & counted(L)
    hist = np.bincount(bin_of(L)[cnt], minlength=BINS).astype(np.uint32)
    lb = bits(L)[cnt]
    rec = dict(n_counted=int(cnt.sum()), n_dark=int((cov & ~cnt).sum()), n_uncovered=int((~cov).sum()),
               max_bits=int(lb.max()) if lb.size else 0, min_bits=int(lb.min()) if lb.size else 0xFFFFFFFF)
    return hist, rec


def target_scale(hist, permille, target, scale_min, scale_max):
    """t_f of one histogram."""
    h = [int(v) for v in np.asarray(hist).reshape(BINS)]
    total = sum(h)
    if total == 0:
        t = F(1.0)
    else:
        k = max(1, (total * int(permille) + 999) // 1000)
        run, b = 0, BINS - 1
        for i, v in enumerate(h):
            run += v
            if run >= k:
                b = i
                break
        with np.errstate(**_err):
            t = F(F(target) / bin_edge(b))
    return F(np.fmin(np.fmax(t, F(scale_min)), F(scale_max)))


def exposure(hists, permille, target, scale_min, scale_max, rate, prev=None):
    """s_f of histograms uint32[n, 256]: s_0 = prev if given else t_0; s_f = s + (t_f - s) * rate."""
    hists = np.asarray(hists).reshape(-1, BINS)
    out = np.zeros(len(hists), np.float32)
    s = None if prev is None else F(prev)
    for f, h in enumerate(hists):
        t = target_scale(h, permille, target, scale_min, scale_max)
        if f == 0:
            s = t if s is None else s
        else:
            with np.errstate(**_err):
                d = F(t - s)
                m = F(d * F(rate))
                s = F(s + m)
        out[f] = s
    return out


def exposure_chunked(hists, permille, target, scale_min, scale_max, rate, prev=None, chunk=CHUNK):
    """The scales of cg_rt_render_exposed: exposure() per chunk of frames, each chunk after the
    first with the scale before it as prev."""
    hists = np.asarray(hists).reshape(-1, BINS)
    out = np.zeros(len(hists), np.float32)
    for f0 in range(0, len(hists), chunk):
        out[f0:f0 + chunk] = exposure(hists[f0:f0 + chunk], permille, target, scale_min, scale_max, rate,
                                      prev if f0 == 0 else out[f0 - 1])
    return out


def tone(op, v, white2=1.0):
    v = f32(v)
    with np.errstate(**_err):
        if op == TONE_LINEAR:
            return v
        den = (F(1.0) + v).astype(np.float32)
        if op == TONE_REINHARD:
            return (v / den).astype(np.float32)
        if op == TONE_REINHARD_WHITE:
            q = (v / F(white2)).astype(np.float32)
            n = (v * (F(1.0) + q).astype(np.float32)).astype(np.float32)
            return (n / den).astype(np.float32)
    raise ValueError(op)


def chan8(c):
    """SDLauxiliary.h's uint32_t(clamp(255 * c, 0, 255)) with glm's min / max: a NaN product gives 0."""
    with np.errstate(**_err):
        k = (F(255.0) * f32(c)).astype(np.float32)
        k = np.where(k > F(0.0), k, F(0.0)).astype(np.float32)      # max(k, 0): k > 0 ? k : 0
        k = np.where(k < F(255.0), k, F(255.0)).astype(np.float32)  # min(k, 255): k < 255 ? k : 255
    return k.astype(np.uint32)                                      # truncation of a value in [0, 255]


def put_pixels(xyz):
    xyz = f32(xyz)
    return (np.uint32(128 << 24) + (chan8(xyz[..., 0]) << np.uint32(16)) + (chan8(xyz[..., 1]) << np.uint32(8))
            + chan8(xyz[..., 2])).astype(np.uint32)


def pack(rgba, scale, op=TONE_LINEAR, white2=1.0):
    """uint32[...]: put_pixel(tone(op, c * scale)) of float32[..., 3 or 4]."""
    rgba = f32(rgba)
    with np.errstate(**_err):
        v = (rgba[..., :3] * F(scale)).astype(np.float32)
    return put_pixels(tone(op, v, white2))


# ---- inputs shared by the CPU and GPU tests ------------------------------------------------

def special_luminances():
    """float32 values around everything the bin rule distinguishes."""
    vals = [0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1.0, 0.5, 2.0 ** -16, 1e-30, 65536.0, 3.0e38, 1e-45, 1.17549435e-38]
    out = [F(v) for v in vals]
    edges = bin_edge(np.arange(BINS))
    for e in edges[[0, 1, 7, 8, 119, 120, 126, 127, 128, 254, 255]]:
        out += [e, np.nextafter(e, F(0)), np.nextafter(e, F(np.inf))]
    out += [from_bits(0x7FC0DEAD), from_bits(0xFFC00001), from_bits(0x7F800001), from_bits(0x00000001),
            from_bits(0x807FFFFF)]
    return np.array(out, np.float32)


def random_floats(rng, n):
    """n float32 drawn as bit patterns: every exponent, both signs, NaNs and infinities included."""
    return from_bits(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)).copy()


def hand_histograms():
    """(name, hist uint32[256], permille) cases; the expected bins are literals in tests/test_hdr.py."""
    def h(**kw):
        a = np.zeros(BINS, np.uint32)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    return [
        ("empty", h(), 990),
        ("one_bin", h(b128=1000), 990),
        ("permille_0", h(b10=5, b100=5, b200=5), 0),
        ("permille_1", h(b10=5, b100=5, b200=5), 1),
        ("permille_500", h(b10=5, b100=5, b200=5), 500),
        ("permille_1000", h(b10=5, b100=5, b200=5), 1000),
        ("sum_equals_k_at_boundary", h(b50=500, b60=490, b70=10), 990),
        ("one_past_boundary", h(b50=500, b60=489, b70=11), 990),
        ("huge_counts", h(b0=0xFFFFFFFF, b255=0xFFFFFFFF), 501),
    ]


def random_histograms(rng, n):
    """Histograms of every shape the search can meet: sparse, dense, empty, one bin, huge counts."""
    out = np.zeros((n, BINS), np.uint32)
    for i in range(n):
        kind = i % 5
        if kind == 0:
            out[i] = rng.integers(0, 1000, BINS)
        elif kind == 1:
            idx = rng.integers(0, BINS, 3)
            out[i, idx] = rng.integers(1, 1 << 20, 3)
        elif kind == 2:
            out[i, rng.integers(0, BINS)] = rng.integers(1, 1 << 32)
        elif kind == 3:
            out[i] = rng.integers(0, 1 << 32, BINS, dtype=np.uint64).astype(np.uint32)
        # kind 4: empty
    return out


def exposure_cases():
    """(hists uint32[n, 256], exposure keywords, prev) cases shared by the CPU and GPU tests."""
    rng = np.random.default_rng(0x4DA)
    hand = hand_histograms()
    cases = []
    for name, hist, permille in hand:
        cases.append((hist[None], dict(permille=permille, target=3.0, scale_min=2.0 ** -30, scale_max=2.0 ** 30,
                                       rate=1.0), None))
    allh = np.stack([h for _, h, _ in hand])
    cases.append((allh, dict(permille=990, target=1.0, scale_min=2.0 ** -16, scale_max=2.0 ** 16, rate=0.25), None))
    cases.append((allh, dict(permille=500, target=0.18, scale_min=0.01, scale_max=100.0, rate=0.25), 4.0))
    rnd = random_histograms(rng, 64)
    for permille, rate, prev in ((990, 0.5, None), (0, 1.0, 0.125), (1000, 0.0, 2.0), (731, 0.9, None)):
        cases.append((rnd, dict(permille=permille, target=1.0, scale_min=2.0 ** -12, scale_max=2.0 ** 12, rate=rate),
                      prev))
    return cases
