"""References for the pixel kernels that share nothing with the code under test (numpy only).

* ``lanczos_taps`` / ``lanczos_dense``: the Lanczos-3 resampling operator from its definition.
* ``scale_exact``: the separable resample in float64.
* ``nv12_from_rgb8``: the BT.709 limited-range integer CSC with the coded padding, the NV12
  reference of the CSC kernel and of every scaler form.
* ``valu_model`` / ``mfma_model``: the arithmetic of the two numeric forms of the scaler, with the
  samples whose rounding the float32 accumulation error could flip marked *undecidable*.
* content generators.

Pictures are ``[h, w, 3]`` arrays in R, G, B order; ``bgrx`` packs them for the kernels.
"""
import functools

import numpy as np

U24 = 2.0 ** -24  # float32 unit roundoff (round to nearest): one rounding is off by <= U24 * |result|


# ---------------------------------------------------------------------------- Lanczos operator
def lanczos3(x):
    x = np.abs(np.asarray(x, np.float64))
    px = np.pi * np.where(x < 1e-12, 1.0, x)
    v = 3.0 * np.sin(px) * np.sin(px / 3.0) / (px * px)
    return np.where(x < 1e-12, 1.0, np.where(x >= 3.0, 0.0, v))


def lanczos_taps(n_in, n_out):
    """(first[n_out], w[n_out, taps]) float64: output o samples the input at first[o] + k with
    weight w[o, k].  Centre (o + 0.5) * s - 0.5, kernel lanczos3(x / max(1, s)) over the open
    support |x| < 3 * max(1, s), each row normalised to sum 1; positions may lie outside
    [0, n_in).  ``first`` is the smallest integer inside the support and ``taps`` the most
    integers an interval of that length can hold, ceil(2 * support) + 1."""
    s = n_in / n_out
    f = max(1.0, s)
    support = 3.0 * f
    taps = int(np.ceil(2.0 * support)) + 1
    centre = (np.arange(n_out) + 0.5) * s - 0.5
    first = np.floor(centre - support).astype(np.int64) + 1
    pos = first[:, None] + np.arange(taps)[None, :]
    w = lanczos3((pos - centre[:, None]) / f)
    return first, w / w.sum(axis=1, keepdims=True)


def fold(first, w, n_in, dtype=np.float64):
    """Dense [n_out, n_in] operator of taps (first, w): a tap outside the picture reads the
    clamped edge sample, so its weight is accumulated onto that column (in ``dtype``, tap order)."""
    n_out, taps = w.shape
    d = np.zeros((n_out, n_in), dtype)
    rows = np.arange(n_out)
    for k in range(taps):
        d[rows, np.clip(first + k, 0, n_in - 1)] += w[:, k].astype(dtype)
    return d


def lanczos_dense(n_in, n_out):
    """float64 [n_out, n_in] resampling matrix from the definition (see lanczos_taps), rows sum
    to 1, taps outside the picture accumulated onto the clamped edge column."""
    first, w = lanczos_taps(n_in, n_out)
    return fold(first, w, n_in)


def scale_exact(img, out_w, out_h):
    """Wy @ channel @ Wx.T in float64 per channel, unrounded: [out_h, out_w, 3]."""
    h, w = img.shape[:2]
    wy, wx = lanczos_dense(h, out_h), lanczos_dense(w, out_w)
    return np.stack([wy @ img[..., c].astype(np.float64) @ wx.T for c in range(3)], axis=-1)


def to_rgb8(v):
    """Round half to even and saturate, as lrintf + clamp and v_cvt_pk_u8_f32 do."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------- CSC
def nv12_from_rgb8(rgb8, coded_w, coded_h):
    """(Y [coded_h, coded_w], UV [coded_h / 2, coded_w]) of an RGB8 picture: the picture is
    edge-replicated to the coded size in the RGB domain, then the BT.709 limited-range integer
    formulas (x256 coefficients, 2x2 chroma mean rounded half up) are applied."""
    h, w = rgb8.shape[:2]
    assert coded_w >= w and coded_h >= h and coded_w % 2 == 0 and coded_h % 2 == 0
    p = np.pad(rgb8, ((0, coded_h - h), (0, coded_w - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = ((47 * r + 157 * g + 16 * b + 128) >> 8) + 16

    def mean4(c):
        return (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2

    ra, ga, ba = mean4(r), mean4(g), mean4(b)
    uv = np.empty((coded_h // 2, coded_w), np.int64)
    uv[:, 0::2] = ((-26 * ra - 86 * ga + 112 * ba + 128) >> 8) + 128
    uv[:, 1::2] = ((112 * ra - 102 * ga - 10 * ba + 128) >> 8) + 128
    assert y.min() >= 0 and y.max() <= 255 and uv.min() >= 0 and uv.max() <= 255
    return y.astype(np.uint8), uv.astype(np.uint8)


def bt709_float(r, g, b):
    """Float BT.709 limited range (Y, U, V) of float R, G, B in 0..255."""
    ya = 0.2126 * r + 0.7152 * g + 0.0722 * b
    return (16 + ya * 219.0 / 255.0, 128 + (b - ya) / 1.8556 * 224.0 / 255.0,
            128 + (r - ya) / 1.5748 * 224.0 / 255.0)


def undecided_planes(und_rgb, coded_w, coded_h):
    """Undecidable RGB samples [h, w, 3] -> (Y, UV) planes of the coded size: a Y sample is
    undecidable if any channel of its pixel is, a U or V sample if any channel of its four."""
    h, w = und_rgb.shape[:2]
    px = np.pad(und_rgb.any(axis=-1), ((0, coded_h - h), (0, coded_w - w)), mode="edge")
    q = px[0::2, 0::2] | px[0::2, 1::2] | px[1::2, 0::2] | px[1::2, 1::2]
    return px, np.repeat(q, 2, axis=1)


# ---------------------------------------------------------------------------- numeric models
def _near_tie(v, delta):
    """|v - nearest rounding tie n + 0.5| <= delta for a tie that matters after saturation to
    0..255 (the clip points -0.5 and 255.5 are the outermost such ties)."""
    d = np.abs(v - np.floor(v) - 0.5)
    return (d <= delta) & (v >= -0.5 - delta) & (v <= 255.5 + delta)


def _seq_fma(gathered, w):
    """Sum over the last axis of gathered * w in tap order, and the float32 error bound of doing
    it with one fma per tap: fma k rounds partial sum s_k once, off by <= 2^-24 |s_k|, so the
    result is within 2^-24 * sum_k |s_k| (1 % added for the second-order terms)."""
    part = np.cumsum(gathered * w, axis=-1)
    return part[..., -1], 1.01 * U24 * np.abs(part).sum(axis=-1)


def valu_model(img, out_w, out_h):
    """The VALU kernel's arithmetic: float32 weights; the horizontal result of every input row
    rounded to 1/16 (lrintf(x * 16)); the vertical pass over those integers; / 16.
    Returns (pre-rounding RGB [out_h, out_w, 3] float64, undecidable [out_h, out_w, 3] bool).

    The model sums in float64 (exact here: products of 24-bit weights with 8- or 13-bit
    integers, a few dozen terms); the kernel accumulates in float32 with one fma per tap, in tap
    order, so its distance from the model is bounded by _seq_fma's eps (taps x 2^-24 x the
    partial sums' magnitudes); the scalings by 16 and 1/16 are exact.  A horizontal result whose
    x16 value is within 16 * eps_h of a tie may round either way, which moves every output row
    that reads it by |wy| / 16; a sample is undecidable when its own value is within
        eps_v + sum over such rows of |wy| / 16
    of a tie that matters (any n + 0.5 inside the saturation range, whose ends are the clip
    points).  This is the set of samples the error bound could flip, and no larger."""
    h, w = img.shape[:2]
    fx, wx = lanczos_taps(w, out_w)
    fy, wy = lanczos_taps(h, out_h)
    wx32, wy32 = wx.astype(np.float32).astype(np.float64), wy.astype(np.float32).astype(np.float64)
    ix = np.clip(fx[:, None] + np.arange(wx.shape[1])[None, :], 0, w - 1)  # [out_w, tx]
    iy = np.clip(fy[:, None] + np.arange(wy.shape[1])[None, :], 0, h - 1)  # [out_h, ty]
    ay = fold(fy, np.abs(wy32), h)
    val = np.empty((out_h, out_w, 3))
    und = np.empty((out_h, out_w, 3), bool)
    for c in range(3):
        p = img[..., c].astype(np.float64)
        hx, eps_h = _seq_fma(p[:, ix], wx32)                       # [h, out_w]
        h16 = hx * 16.0
        near = np.abs(h16 - np.floor(h16) - 0.5) <= 16.0 * eps_h
        hq = np.rint(h16)
        v16, eps_v = _seq_fma(np.moveaxis(hq[iy], 1, 2), wy32[:, None, :])  # [out_h, out_w]
        v = v16 / 16.0
        val[..., c] = v
        und[..., c] = _near_tie(v, eps_v / 16.0 + ay @ near.astype(np.float64) / 16.0)
    return val, und


def _to_f16(x32, scale):
    """build_scale_frags' weight conversion: float32 weight * scale, magnitudes below the f16
    normal range (2^-14) dropped, rounded to f16."""
    s = (x32.astype(np.float32) * np.float32(scale)).astype(np.float32)
    s = np.where(np.abs(s) < np.float32(2.0 ** -14), np.float32(0), s)
    return s.astype(np.float16).astype(np.float64)


def mfma_model(img, out_w, out_h):
    """The matrix-core kernels' arithmetic (tile and strip forms compute the same values):
    horizontal weights folded onto the edge columns in float32, x 2^14, to f16; vertical weights
    x 2^10 to f16 per tap (the staged rows are clamped, so a tap outside the picture keeps its own
    weight); pixels enter as p * 2^-24; the horizontal product X is rounded to f16; the vertical
    product is taken in float and is in pixel units (2^14 * 2^10 * 2^-24 = 1).
    Returns (pre-rounding RGB [out_h, out_w, 3] float64, undecidable [out_h, out_w, 3] bool).

    Every product here is exact in float32 (11-bit x 11-bit significands); the error is in the
    accumulation, whose order inside the matrix core is not documented:
        |kernel - model| <= taps * 2^-24 * sum_k |w_k| |term_k|     (eps, per sample)
    (one rounding to nearest per non-zero term -- zero terms add exactly -- of a partial sum
    that, in whatever order the matrix core adds, is no larger than the sum of magnitudes).
    An X within eps_x of the midpoint of two neighbouring f16 values may round either way, which
    moves every output that reads it by |wv| * ulp(X); a sample is undecidable when its own
    value is within eps_y + the sum of those moves of a tie that matters."""
    h, w = img.shape[:2]
    fx, wx = lanczos_taps(w, out_w)
    fy, wy = lanczos_taps(h, out_h)
    dh = _to_f16(fold(fx, wx.astype(np.float32), w, np.float32), 2.0 ** 14)  # [out_w, w]
    wv = _to_f16(wy.astype(np.float32), 2.0 ** 10)                           # [out_h, taps]
    dv, av = fold(fy, wv, h), fold(fy, np.abs(wv), h)
    tx, ty = wx.shape[1], wy.shape[1]
    val = np.empty((out_h, out_w, 3))
    und = np.empty((out_h, out_w, 3), bool)
    for c in range(3):
        p = img[..., c].astype(np.float64) * 2.0 ** -24
        x = p @ dh.T                                   # 2^-10 * filtered row, exact in float64
        eps_x = tx * U24 * (p @ np.abs(dh).T)
        x16 = x.astype(np.float16)
        xq = x16.astype(np.float64)
        ulp = np.spacing(np.abs(x16)).astype(np.float64)
        # below a power of two the spacing halves
        mant0 = (x16.view(np.uint16) & 0x03FF) == 0
        ulp = np.where(mant0 & (np.abs(x) < np.abs(xq)) & (np.abs(xq) > 2.0 ** -14), ulp / 2, ulp)
        near = (ulp / 2 - np.abs(x - xq)) <= eps_x
        v = dv @ xq
        eps_y = ty * U24 * (av @ np.abs(xq))
        val[..., c] = v
        und[..., c] = _near_tie(v, eps_y + av @ (near * ulp))
    return val, und


# ---------------------------------------------------------------------------- content
def noise_picture(w, h, seed):
    """B: 0/255 binary noise.  G: uniform noise.  R: 0 with single 255 pixels at the four
    corners and the four edge mid-points, one vertical 0 -> 255 step (rows h/4 .. h/2, at
    x = 5w/8) and one horizontal one (columns w/8 .. 3w/8, at y = 5h/8); each of those six
    coordinates is moved by 0..3 drawn from the seed, so that a seed can take the steps off the
    positions where an integer scale factor puts samples exactly on a rounding tie."""
    rng = np.random.default_rng(seed)
    sx, sy, a0, a1, b0, b1 = (int(v) for v in rng.integers(0, 4, 6))
    img = np.zeros((h, w, 3), np.uint8)
    img[..., 2] = rng.integers(0, 2, (h, w)) * 255
    img[..., 1] = rng.integers(0, 256, (h, w))
    r = img[..., 0]
    r[h // 4 + a0: h // 2 + a1, min(5 * w // 8 + sx, w - 1):] = 255
    r[min(5 * h // 8 + sy, h - 1):, w // 8 + b0: 3 * w // 8 + b1] = 255
    for y in (0, h // 2, h - 1):
        for x in (0, w // 2, w - 1):
            if (y, x) != (h // 2, w // 2):
                r[y, x] = 255
    return img


CONSTANTS = ((0, 0, 0), (255, 255, 255), (254, 128, 1))


def constant_picture(w, h, rgb):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


def csc_picture(w, h, seed):
    """Random pixels, with 2x2 blocks of the eight corners of the RGB cube from the top-left
    (as many as fit in the first two rows)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for i in range(min(8, w // 2)):
        img[0:2, 2 * i: 2 * i + 2] = [255 * (i & 1), 255 * ((i >> 1) & 1), 255 * ((i >> 2) & 1)]
    return img


def bgrx(rgb8, pitch=None, fill=None, seed=0):
    """[h, pitch] uint8 BGRx rows of an RGB8 picture; bytes beyond 4 * w (and the x byte) are
    ``fill`` or, if None, random."""
    h, w = rgb8.shape[:2]
    pitch = pitch or 4 * w
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (h, pitch), dtype=np.uint8) if fill is None else np.full((h, pitch), fill, np.uint8)
    px = out[:, : 4 * w].reshape(h, w, 4)
    px[..., 0], px[..., 1], px[..., 2] = rgb8[..., 2], rgb8[..., 1], rgb8[..., 0]
    return out


def coded(n):
    """Coded size: rounded up to 16, as the encoders'."""
    return (n + 15) // 16 * 16


# (in_w, in_h, out_w, out_h, seed of the noise picture): the scaler cases of the GPU tier.  The
# seeds are those at which every plane's undecidable share is within the 2 % cap (test_pixel_ref).
SCALER_CASES = ((322, 182, 320, 180, 1), (258, 130, 86, 44, 10), (390, 100, 120, 30, 1), (130, 390, 40, 120, 1),
                (64, 36, 256, 144, 4), (6, 6, 64, 64, 1), (4, 4, 32, 32, 2), (256, 144, 64, 36, 2),
                (200, 600, 100, 150, 2))


@functools.lru_cache(maxsize=None)
def scaler_reference(in_w, in_h, out_w, out_h, seed):
    """Everything the tests compare a scaler case with, computed once: the noise picture, the
    exact float64 result, its NV12, and per numeric model the pre-rounding RGB, its NV12 and the
    undecidable Y / UV planes."""
    cw, ch = coded(out_w), coded(out_h)
    img = noise_picture(in_w, in_h, seed)
    exact = scale_exact(img, out_w, out_h)
    ref = {"img": img, "exact": exact, "exact_nv12": nv12_from_rgb8(to_rgb8(exact), cw, ch)}
    for name, model in (("valu", valu_model), ("mfma", mfma_model)):
        val, und = model(img, out_w, out_h)
        ref[name] = {"rgb": val, "nv12": nv12_from_rgb8(to_rgb8(val), cw, ch),
                     "undecided": undecided_planes(und, cw, ch)}
    return ref
