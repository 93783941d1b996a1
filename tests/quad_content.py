"""Content for the P_8x8 tests (one vector per 8x8 quadrant) and the inputs of the golden digests
that pin the streams of EncoderConfig.partitions 0 and 1 (tools/gen_partition_digests.py)."""
import hashlib

import numpy as np

# The digests' inputs are the generators of two existing test modules, which stay where they are
# (existing test files are not edited): tools/gen_partition_digests.py therefore imports them too.
from .test_cpu_encoder import synthetic_nv12
from .test_partitions import _split_motion

# per-frame displacement (dx, dy) of quadrants TL, TR, BL, BR: frame t shows the texture moved by t times it
QUAD_STEP = ((2, 0), (0, 3), (-1, -1), (0, 0))


def _texture(w, h, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(30, 220, (h + 64, w + 64)).astype(np.uint8)
    return ((base.astype(np.int32) + np.roll(base, 1, 0) + np.roll(base, 1, 1)) // 3).astype(np.uint8)


def _with_chroma(y):
    uv = np.full((y.shape[0] // 2, y.shape[1]), 128, np.uint8)
    uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
    return y, uv


def quad_motion(w, h, t, half=False):
    """Smoothed noise in which each 8x8 quadrant of every macroblock moves by its own displacement:
    QUAD_STEP per frame, or half of it (half-sample motion on odd frames, from the mean of the two
    neighbouring whole-sample pictures) with half=True."""
    base = _texture(w, h, 5).astype(np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    quad = ((yy % 16) >= 8) * 2 + ((xx % 16) >= 8)
    y = np.empty((h, w), np.uint8)
    for q, (sx, sy) in enumerate(QUAD_STEP):
        sel = quad == q
        if half:
            lo = base[(yy + 32 - sy * (t // 2))[sel], (xx + 32 - sx * (t // 2))[sel]]
            hi = base[(yy + 32 - sy * ((t + 1) // 2))[sel], (xx + 32 - sx * ((t + 1) // 2))[sel]]
            y[sel] = ((lo + hi + 1) // 2).astype(np.uint8)
        else:
            y[sel] = base[(yy + 32 - sy * t)[sel], (xx + 32 - sx * t)[sel]].astype(np.uint8)
    return _with_chroma(y)


def window_corner(w, h, t):
    """The corner of a dragged window: one quadrant (BR) of every macroblock moves by (+2, +1) per
    frame over textured content that stays where it is."""
    base = _texture(w, h, 11)
    yy, xx = np.mgrid[0:h, 0:w]
    moving = ((yy % 16) >= 8) & ((xx % 16) >= 8)
    y = base[32:32 + h, 32:32 + w].copy()
    y[moving] = base[(yy + 32 - t)[moving], (xx + 32 - 2 * t)[moving]]
    return _with_chroma(y)


def scroll_with_quad_band(w, h, t, step, band_rows=32):
    """A page scrolled down by `step` rows per frame (the scroll hint's content) whose lowest
    `band_rows` rows carry the quad motion instead."""
    page = _texture(w, h + 64 + 8 * abs(step), 23)
    y = page[64 + 8 * abs(step) - step * t:][:h, 32:32 + w].copy()
    qy, _ = quad_motion(w, band_rows, t)
    y[h - band_rows:] = qy
    return _with_chroma(np.ascontiguousarray(y))


def encode_cpu(native, frames, w, h, **kw):
    """CPU oracle run: the access units, reconstructions, mb_info() and mb_pmv8() of every frame."""
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps = 0
    cfg.qp = 28
    cfg.search_range = 8
    for k, v in kw.items():
        setattr(cfg, k, v)
    enc = native.CpuH264Encoder(cfg)
    aus, recons, infos, pmv8 = [], [], [], []
    for y, uv in frames:
        aus.append(bytes(enc.encode(y, uv, False)))
        recons.append(enc.recon())
        infos.append(enc.mb_info().copy())
        pmv8.append(enc.mb_pmv8().copy() if hasattr(enc, "mb_pmv8") else None)
    return aus, recons, infos, pmv8


def count_p8x8(infos):
    """Inter macroblocks coded P_8x8 over the P pictures (mb_info: type at 0, part at 8)."""
    return sum(int(((i[..., 8] == 3) & (i[..., 0] == 0)).sum()) for i in infos[1:])


# ---- golden digests of the streams with partitions 0 and 1 (tests/golden/h264_partitions_parent.json)
def digest_inputs():
    out = {}
    for w, h in ((128, 64), (160, 96)):
        out[f"split_v_{w}x{h}"] = (w, h, [_split_motion(w, h, t, True) for t in range(5)])
        out[f"split_h_{w}x{h}"] = (w, h, [_split_motion(w, h, t, False) for t in range(5)])
        out[f"synthetic_{w}x{h}"] = (w, h, [synthetic_nv12(w, h, t, seed=t % 2) for t in range(5)])
    return out


def partition_digests(native):
    """{case: [SHA-256 of each access unit]} of the CPU encoder for partitions 0 / 1, both me_coarse."""
    out = {}
    for name, (w, h, frames) in digest_inputs().items():
        for partitions in (0, 1):
            for coarse in (0, 1):
                cfg = native.EncoderConfig()
                cfg.width, cfg.height = w, h
                cfg.bitrate_kbps = 0
                cfg.qp = 28
                cfg.search_range = 8
                cfg.partitions = partitions
                cfg.me_coarse = coarse
                enc = native.CpuH264Encoder(cfg)
                out[f"{name}_p{partitions}_c{coarse}"] = [
                    hashlib.sha256(bytes(enc.encode(y, uv, False))).hexdigest() for y, uv in frames]
    return out


# ---- the scroll hint's content (tests/scroll_content.py) with a band of quad motion
SCROLL_SHAPE = (208, 112)
SCROLL_MOVES = [(0, -12), (9, 0), (0, 0), (0, -16), (-13, 0)]  # within scroll_range 16, beyond search range 8
SCROLL_BAND = (80, 96)  # macroblock row 5: the lowest inside the border, and no probe row of the lattice


def scrolled_with_quad_band():
    """scroll_content's bordered document, scrolled by SCROLL_MOVES (never upwards: no scrolled row
    comes out of the band), whose rows SCROLL_BAND show the quad motion instead: P_8x8 macroblocks in
    pictures that have a hint, their quadrants searched around whichever centre the macroblock takes."""
    from . import scroll_content as sc

    w, h = SCROLL_SHAPE
    frames = []
    for t, (y, _) in enumerate(sc.make_frames(w, h, SCROLL_MOVES, sc.SPECIAL[(w, h)], oy0=400)):
        y = y.copy()
        y[slice(*SCROLL_BAND), sc.BORDER:w - sc.BORDER] = quad_motion(w, 16, t)[0][:, sc.BORDER:w - sc.BORDER]
        frames.append((y, sc._uv_of(y)))
    return frames
