"""CPU tier of the pixel-kernel tests: what can be settled without a GPU.

The Lanczos tables against the definition, the numeric models of the scaler forms against the
exact resample, the conditions the GPU tier's inputs must meet, the path every scaler shape
selects, and the integer CSC model against float BT.709."""
import numpy as np
import pytest

from mxdesk.models.synthetic import bgrx_to_nv12 as synthetic_bgrx_to_nv12

from . import pixel_ref as R

# shape -> what scale_plan must report for it (the path the shape is in the suite for)
PLAN = {
    (322, 182, 320, 180): dict(mfma=True, nk=3, taps_x=8, taps_y=8),
    (258, 130, 86, 44): dict(mfma=True, nk=8, nrb_max=4, taps_x=19),
    (390, 100, 120, 30): dict(mfma=True, nk=8, taps_x=21, taps_y=21),
    (130, 390, 40, 120): dict(mfma=True, nrb_max=4, strip=1),
    (64, 36, 256, 144): dict(mfma=True, nk=2, strip=2, taps_x=7, taps_y=7),
    (6, 6, 64, 64): dict(mfma=True, nk=2),
    (4, 4, 32, 32): dict(mfma=True, nk=2),
    (256, 144, 64, 36): dict(mfma=False, taps_x=25, taps_y=25, valu_lds_bytes=148096),
    (200, 600, 100, 150): dict(mfma=False, taps_x=13, taps_y=25),
}
# the scaler shapes of test_gpu_pipeline.py (w, h, out_w, out_h), for the instantiation count
EXISTING = ((160, 96, 80, 48), (96, 64, 128, 96), (150, 90, 100, 60), (500, 270, 200, 108), (330, 200, 166, 100),
            (960, 540, 480, 270), (3840, 2160, 1920, 1080))
KREG_TAPS = 20  # k_scale_to_nv12 keeps up to this many horizontal weights in registers

SIZE_PAIRS = sorted({(c[0], c[2]) for c in R.SCALER_CASES} | {(c[1], c[3]) for c in R.SCALER_CASES})


def test_case_table_is_the_plan_table():
    assert [c[:4] for c in R.SCALER_CASES] == list(PLAN)


@pytest.mark.parametrize("n_in,n_out", SIZE_PAIRS)
def test_lanczos_table_matches_definition(native, n_in, n_out):
    """make_lanczos_table against the definition: same first tap, same tap count, every weight
    within float32 rounding (half an ulp, 2^-24 relative) of the float64 one, and the same dense
    operator once the taps outside the picture are folded onto the edge."""
    start, w, taps = native.lanczos_table(n_in, n_out)
    first, ref = R.lanczos_taps(n_in, n_out)
    assert taps == ref.shape[1] and w.shape == ref.shape
    assert np.array_equal(start, first)
    err = np.abs(w.astype(np.float64) - ref)
    assert np.all(err <= 2.0 ** -24 * np.abs(ref) + 1e-14), err.max()
    dense = R.lanczos_dense(n_in, n_out)
    assert np.allclose(dense.sum(axis=1), 1.0, atol=1e-12)
    assert np.abs(R.fold(first, w.astype(np.float64), n_in) - dense).max() <= taps * 2.0 ** -24


@pytest.mark.parametrize("case", R.SCALER_CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_models_stay_within_half_of_exact(case):
    """Both numeric models are within 0.5 of the exact resample before rounding, on the noise
    picture and the constants: the condition under which a rounded output is within 1 of the
    exact one.  Constants come out exact after rounding."""
    in_w, in_h, out_w, out_h, _ = case
    ref = R.scaler_reference(*case)
    for name in ("valu", "mfma"):
        err = np.abs(ref[name]["rgb"] - ref["exact"]).max()
        print(f"{case[:4]} {name}: max |model - exact| = {err:.4f}")
        assert err < 0.5, (name, err)
    for rgb in R.CONSTANTS:
        img = R.constant_picture(in_w, in_h, rgb)
        assert np.abs(R.scale_exact(img, out_w, out_h) - np.array(rgb)).max() < 1e-9
        for model in (R.valu_model, R.mfma_model):
            val, und = model(img, out_w, out_h)
            assert np.abs(val - np.array(rgb)).max() < 0.5
            assert np.array_equal(R.to_rgb8(val), R.constant_picture(out_w, out_h, rgb)) and not und.any()


@pytest.mark.parametrize("case", R.SCALER_CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_undecidable_share_within_cap(case):
    """Condition on the inputs: at most 2 % of every plane is undecidable, in both models."""
    ref = R.scaler_reference(*case)
    for name in ("valu", "mfma"):
        for plane, und in zip("Y UV".split(), ref[name]["undecided"]):
            print(f"{case[:4]} {name} {plane}: undecidable share {und.mean():.4f}")
            assert und.mean() <= 0.02, (name, plane, und.mean())


@pytest.mark.parametrize("shape", list(PLAN), ids=lambda s: "%dx%d-%dx%d" % s)
def test_shape_selects_its_path(native, shape):
    """Each shape reaches the path it is in the suite for (all nine are the shapes first
    proposed; none had to be replaced)."""
    plan = native.scale_plan(*shape)
    for key, want in PLAN[shape].items():
        assert plan[key] == want, (key, plan)
    in_w, in_h, out_w, out_h = shape
    ngy = (R.coded(out_h) + 31) // 32
    if shape == (322, 182, 320, 180):  # right-edge quad fix-up, 12 padding rows
        assert in_w % 4 == 2 and R.coded(out_h) - out_h == 12
    if shape == (258, 130, 86, 44):  # register taps, opt-in LDS size, padding on both axes
        assert plan["taps_x"] <= KREG_TAPS and plan["valu_lds_bytes"] > 64 * 1024
        assert R.coded(out_w) > out_w and R.coded(out_h) > out_h
    if shape == (390, 100, 120, 30):  # weights from LDS; a single partial tile row
        assert plan["taps_x"] > KREG_TAPS and ngy == 1 and out_h < 32
    if shape == (130, 390, 40, 120):
        assert ngy == 4
    if shape == (64, 36, 256, 144):  # strips of 2, 2 and 1 tile rows
        assert ngy == 5
    if shape in ((6, 6, 64, 64), (4, 4, 32, 32)):
        assert in_w - 4 in (0, 2)
    if shape == (256, 144, 64, 36):
        assert plan["taps_x"] > KREG_TAPS and plan["valu_lds_bytes"] <= 160 * 1024
    if not plan["mfma"]:
        assert plan["nk"] == 0 and plan["strip"] == 0


def test_every_mfma_instantiation_is_reached(native):
    """Every K-step count k_scale_mfma is instantiated for and both row-block instantiations
    (up to 3 blocks, 4 blocks) are selected by some scaler shape of the suite."""
    plans = [native.scale_plan(*s) for s in list(PLAN) + list(EXISTING)]
    plans = [p for p in plans if p["mfma"]]
    assert {p["nk"] for p in plans} == {2, 3, 4, 5, 6, 8}
    assert {p["nrb_max"] > 3 for p in plans} == {False, True}
    assert {1, 2} <= {p["strip"] for p in plans}


def test_integer_csc_within_bounds_of_float_bt709():
    """The integer CSC model against float BT.709 limited range: Y within 1.0 over all 2^24
    colours, U and V within 1.5 on a lattice of flat colours and on random 2x2 blocks; white
    gives Y 235 and black Y 16."""
    worst = 0.0
    g, b = np.meshgrid(np.arange(256.0), np.arange(256.0), indexing="ij")
    gi, bi = g.astype(np.int64), b.astype(np.int64)
    for r in range(256):
        yi = ((47 * r + 157 * gi + 16 * bi + 128) >> 8) + 16
        worst = max(worst, np.abs(yi - R.bt709_float(float(r), g, b)[0]).max())
    assert worst <= 1.0, worst
    lat = np.arange(0, 256, 3)
    flat = np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), axis=-1).reshape(-1, 1, 3).astype(np.uint8)
    flat = np.repeat(np.repeat(flat, 2, axis=0), 2, axis=1)  # one 2x2 block per colour
    rnd = np.random.default_rng(5).integers(0, 256, (400, 400, 3), dtype=np.uint8)
    for img in (flat, rnd):
        y, uv = R.nv12_from_rgb8(img, img.shape[1], img.shape[0])
        f = img.astype(np.float64)
        m = (f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]) / 4.0
        _, fu, fv = R.bt709_float(m[..., 0], m[..., 1], m[..., 2])
        assert np.abs(uv[:, 0::2] - fu).max() <= 1.5 and np.abs(uv[:, 1::2] - fv).max() <= 1.5
        assert np.abs(y - R.bt709_float(f[..., 0], f[..., 1], f[..., 2])[0]).max() <= 1.0
    for rgb, want in (((255, 255, 255), 235), ((0, 0, 0), 16)):
        y, uv = R.nv12_from_rgb8(R.constant_picture(2, 2, rgb), 2, 2)
        assert (y == want).all() and (uv == 128).all()


def test_reference_csc_is_the_projects_integer_model():
    """pixel_ref.nv12_from_rgb8 and mxdesk.models.synthetic.bgrx_to_nv12 are written apart and
    agree exactly; the padding is replication in the RGB domain."""
    img = R.csc_picture(50, 34, 2)
    y, uv = R.nv12_from_rgb8(img, 64, 48)
    sy, suv = synthetic_bgrx_to_nv12(R.bgrx(img).reshape(34, 50, 4))
    assert np.array_equal(y[:34, :50], sy) and np.array_equal(uv[:17, :50], suv.reshape(17, 50))
    padded = np.pad(img, ((0, 14), (0, 14), (0, 0)), mode="edge")
    py, puv = synthetic_bgrx_to_nv12(R.bgrx(padded).reshape(48, 64, 4))
    assert np.array_equal(y, py) and np.array_equal(uv, puv.reshape(24, 64))
    assert np.array_equal(y[:34, 50:], np.repeat(y[:34, 49:50], 14, axis=1))
    assert np.array_equal(y[34:], np.repeat(y[33:34], 14, axis=0))
