"""CPU: the JPEG decoder beyond the reference's seven texture files (all of them
progressive 4:2:0 1024x1024 JFIF files without restarts).  The files are the 252
Pillow-encoded ones of tests/golden/jpeg_cases.npz and the synthetic baseline files that
tests/jpeg_cases.py builds from chosen coefficients; two references that share no code with
the oracle hold it:
  - the SHA-256 of what libjpeg 9 decodes, derived from Pillow wherever no component is
    scaled (tests/golden/make_jpeg_cases.py), recorded and -- where Pillow imports --
    recomputed here;
  - the float64 inverse DCT of the chosen coefficients, which also reaches the 16x16
    scaled IDCT of 4:2:0 chroma (Adobe transform 0 makes the channels the sample planes).
The library's host parser (cg_image_jpeg_check / cg_image_jpeg_info) runs on every file;
its kernels are held to the same references in tests/test_jpeg_decode_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import cgamd
import jpeg_cases as jc
import oracle


@pytest.fixture(scope="module")
def decoded():
    """{name: the oracle's decode} of every fixture and synthetic file, computed once."""
    return {name: oracle.jpeg_decode(data) for name, data, _ in jc.all_files()}


def test_fixture_is_complete_and_synthetic_files_are_reproduced():
    fx = jc.load_fixture()
    assert sorted(fx["pillow"]) == sorted(p[0] for p in jc.pillow_case_params())
    assert len(fx["pillow"]) == 252
    assert sum(h is not None for _, h in fx["pillow"].values()) == 168         # all but the 4:2:0 files
    syn = jc.synthetic_cases()
    assert sorted(fx["synthetic"]) == sorted(c.name for c in syn)
    for c in syn:
        file_sha, h = fx["synthetic"][c.name]
        assert jc.sha(np.frombuffer(c.jpeg, np.uint8)) == file_sha, f"{c.name}: the encoder's output changed"
        assert (h is not None) == (not c.any_scaled), c.name


def test_oracle_matches_recorded_hashes(decoded):
    bad = [name for name, _, h in jc.all_files() if h is not None and jc.sha(decoded[name]) != h]
    assert not bad, f"{len(bad)} files differ from the Pillow-derived libjpeg 9 result: {bad[:8]}"


def test_recorded_hashes_match_live_pillow():
    pytest.importorskip("PIL")
    import make_jpeg_cases as mk
    bad = [name for name, data, h in jc.all_files() if h is not None and jc.sha(mk.pillow_expected(data)) != h]
    assert not bad, f"{len(bad)} recorded hashes differ from this Pillow: {bad[:8]}"


def test_colour_space_conventions(decoded):
    """libjpeg's default_decompress_parms on three-component files, as Pillow decodes them
    (the recorded hashes): (a) no JFIF, no Adobe marker, ids 1,2,3: YCbCr; (b) no markers,
    ids 'R','G','B': RGB; (c) JFIF and Adobe transform 0: YCbCr, JFIF wins; (d) Adobe
    transform 1: YCbCr.  Here: the RGB ones are the planes themselves, the YCbCr ones are
    jdcolor9() of the same planes (the 4:4:4 files of (a)-(d) share their coefficients'
    recipe but not their values, so each is checked against its own ideal planes)."""
    cases = {c.name: c for c in jc.synthetic_cases()}
    expect_planes = {"cs_a_nomarkers_ids123": False, "cs_b_nomarkers_idsRGB": True,
                     "cs_c_jfif_and_adobe0": False, "cs_d_adobe1": False}
    for stem, planes in expect_planes.items():
        for sname in ("444", "420"):
            c = cases[f"{stem}_{sname}"]
            assert c.planes == planes
            # a plane sample is within 1 of its rounded ideal (B < 1, the next test); through
            # jdcolor9 that is at most 1 + 1.772 -> 3 in a channel.  A wrong colour space is
            # off by a hundred and more.
            p =[jc.ideal_plane(cf, q, 8 * s)[:c.height, :c.width] for cf, q, s in zip(c.coef, c.quant, c.scale)]
            ycc = np.clip(np.rint(np.stack(p, -1)), 0, 255).astype(np.uint8)
            want = ycc[..., ::-1] if planes else jc.jdcolor9(ycc)
            err = np.abs(decoded[c.name].astype(int) - want.astype(int)).max()
            assert err <= 3, f"{c.name}: decoded in the wrong colour space (worst channel error {err})"


def test_oracle_within_bound_of_ideal_idct(decoded):
    """|sample - clip(ideal, 0, 255)| <= B on every plane readable through the gray or the
    Adobe-RGB output, S = 1 and S = 2, where the ideal is the float64 inverse DCT.  B is
    0.5 (rounding to an integer) plus twice the oracle's worst excess over 0.5 in this run:
    measured worst 0.5784 (S = 2; 0.5667 for S = 1; 0.5095 on the clamping set), so
    B = 0.6568.  B < 1 keeps every off-by-one sample a failure.  No sample's ideal leaves
    [-128, 383], the range in which libjpeg 9's limit table is a plain clamp."""
    B, worst = jc.bound_from(lambda data: oracle.jpeg_decode(data))
    print(f"oracle worst |sample - ideal| {worst:.4f}, B {B:.4f}")
    assert 0.5 <= worst and B < 1.0
    lo = hi = total = 0
    for c in jc.synthetic_cases():
        if not c.planes:
            continue
        err, excluded, below, above, n = jc.ideal_errors(c, decoded[c.name])
        assert excluded == 0, f"{c.name}: {excluded} ideal samples outside [-128, 383]"
        assert err <= B, f"{c.name}: worst |sample - ideal| {err:.4f} > {B:.4f}"
        if c.clamping:
            lo, hi, total = lo + below, hi + above, total + n
    assert total and lo >= 0.05 * total and hi >= 0.05 * total, (lo, hi, total)
    # both IDCT sizes and both clamps were reached
    assert any(c.any_scaled and c.planes for c in jc.synthetic_cases())


def test_baseline_equals_progressive(decoded):
    """Pillow computes the coefficients before it chooses the entropy mode, so the baseline
    and the progressive file of one image decode alike -- asserted for every pair, the
    4:2:0 ones (which no hash covers) with and without restarts included."""
    pairs = 0
    for name, _, _ in jc.all_files():
        if name.startswith("pil_") and "_base_" in name:
            a, b = decoded[name], decoded[name.replace("_base_", "_prog_")]
            assert np.array_equal(a, b), name
            pairs += "_420_" in name
    assert pairs == 42                                                            # 7 sizes x 3 restarts x 2 qualities


def test_restart_interval_does_not_change_pixels(decoded):
    """Restart markers change the entropy coding alone: the r1 and r3 files of an image
    equal its r0 file."""
    for name, _, _ in jc.all_files():
        if name.startswith("pil_") and "_r0_" in name:
            for r in ("_r1_", "_r3_"):
                assert np.array_equal(decoded[name], decoded[name.replace("_r0_", r)]), name.replace("_r0_", r)


def test_library_parser_accepts_every_file():
    """cg_image_jpeg_check and cg_image_jpeg_info (host code) on every file: accepted, with
    the file's width, height and channel count."""
    lib = cgamd.load()
    sizes = {p[0]: (p[1], 1 if p[2] == "gray" else 3) for p in jc.pillow_case_params()}
    sizes.update({c.name: ((c.width, c.height), c.channels) for c in jc.synthetic_cases()})
    for name, data, _ in jc.all_files():
        buf = np.frombuffer(data, np.uint8)
        assert lib.cg_image_jpeg_check(buf.ctypes.data, buf.size) == cgamd.CG_OK, name
        w, h, ch = C.c_int(), C.c_int(), C.c_int()
        assert lib.cg_image_jpeg_info(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), C.byref(ch)) == 0, name
        assert ((w.value, h.value), ch.value) == sizes[name], name
        assert cgamd.jpeg_info(data) == (w.value, h.value, ch.value)


def test_unsupported_formats_fail_loudly():
    """4:2:2 and 4:4:0 would need libjpeg 9's upsampler, which neither decoder has; nor
    arithmetic coding (SOF9) or 12-bit samples.  Both decoders refuse such a file
    (CG_E_INVALID / ValueError), they do not decode it wrongly."""
    lib = cgamd.load()
    files = []
    for sampling in ([(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)]):
        coef = [np.zeros(g + (8, 8), np.int64) for g in jc.grid(17, 15, sampling)]
        files.append(jc.encode(coef, [jc.Q_FLAT3] * 3, 17, 15, sampling))
    good = jc.encode([np.zeros((2, 3, 8, 8), np.int64)], [jc.Q_FLAT3], 17, 15, [(1, 1)])
    sof = good.index(b"\xff\xc0")
    assert good[sof + 4] == 8
    files.append(good[:sof + 1] + b"\xc9" + good[sof + 2:])                      # arithmetic coding
    files.append(good[:sof + 1] + b"\xc1" + good[sof + 2:sof + 4] + b"\x0c" + good[sof + 5:])   # 12-bit
    oracle.jpeg_decode(good)
    for data in files:
        buf = np.frombuffer(data, np.uint8)
        assert lib.cg_image_jpeg_check(buf.ctypes.data, buf.size) == cgamd.CG_E_INVALID
        with pytest.raises(ValueError):
            oracle.jpeg_decode(data)
