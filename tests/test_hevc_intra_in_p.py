"""HEVC P pictures with intra units (EncoderConfig.hevc_intra_in_p), CPU tier: the stream decodes with
the independent Python decoder to the encoder's reconstruction, the decoder counts the intra units the
encoder chose, the option off codes the parent commit's streams, and the option reaches the session's
encoder configuration from the environment."""
import hashlib
import itertools
import json
from pathlib import Path

import numpy as np
import pytest

from mxdesk.codec.hevc_decoder import Decoder

GOLDEN = Path(__file__).parent / "golden" / "hevc_intra_in_p_parent.json"
# 96x64: 3 x 2 whole CTBs; 80x48: partial CTBs on the right and at the bottom
CASES = list(itertools.product([(96, 64), (80, 48)], [24, 34], [0, 1], [1, 2]))  # size, QP, deblock, hevc_intra_split


def intra_p_frames(w, h):
    """Three NV12 frames: noise everywhere; then a rectangle of flat panels from (20, 12) to the right
    and bottom picture edges; then the rectangle at the top left corner, noise where it was.  Most
    panels are small (sharp edges every few samples, which no 16x16 intra mode follows); a large one
    covers the units that are to win, with the two samples above and left of them:
    picture 1: unit (2, 2) -- with whole CTBs the first unit of a CTB that starts a slice -- and the
    unit in the bottom right picture corner, whose three neighbours keep the noise so that none of
    them outbids it; picture 2: unit (2, 0), the first unit of a CTB whose below-left lies in the
    left CTB of the same slice."""
    rng = np.random.default_rng(5)
    noise_y = rng.integers(16, 236, (h, w), dtype=np.uint8)
    noise_uv = rng.integers(64, 192, (h // 2, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    panel_y = (60 + 120 * ((xx // 8 + yy // 6) % 2)).astype(np.uint8)
    panel_uv = (110 + 30 * ((xx[: h // 2] // 8 + yy[: h // 2] // 6) % 2)).astype(np.uint8)
    frames = [(noise_y, noise_uv)]
    for (x0, y0), large in (((20, 12), [(2, 2), (w // 16 - 1, h // 16 - 1)]), ((0, 0), [(2, 0)])):
        y, uv = noise_y.copy(), noise_uv.copy()
        x1, y1 = x0 + w - 20, y0 + h - 12
        y[y0:y1, x0:x1] = panel_y[y0:y1, x0:x1]
        uv[y0 // 2:y1 // 2, x0:x1] = panel_uv[y0 // 2:y1 // 2, x0:x1]
        if x0:  # the corner unit's three neighbours keep the noise (static: they stay inter)
            for a, b in ((w - 32, h - 32), (w - 16, h - 32), (w - 32, h - 16)):
                y[b:b + 16, a:a + 16] = noise_y[b:b + 16, a:a + 16]
                uv[b // 2:b // 2 + 8, a:a + 16] = noise_uv[b // 2:b // 2 + 8, a:a + 16]
        for ux, uy in large:
            y[max(16 * uy - 2, 0):16 * uy + 16, 16 * ux - 2:16 * ux + 16] = 120
            uv[max(8 * uy - 1, 0):8 * uy + 8, 16 * ux - 2:16 * ux + 16] = 128
        frames.append((y, uv))
    return frames


def make_cfg(native, w, h, qp, deblock, split, intra_in_p):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps, cfg.qp, cfg.aq, cfg.search_range = 0, qp, 1, 8
    cfg.deblock, cfg.sao, cfg.hevc_intra_split = deblock, deblock, split  # no in-loop filter at all, or both
    cfg.hevc_slice_cost = 64  # at least three slices in these small P pictures
    if intra_in_p is not None:
        cfg.hevc_intra_in_p = intra_in_p
    return cfg


def encode(enc, frames, put=lambda y, uv: (y, uv)):
    """(access units, reconstructions, intra units and distortion sums per picture) of the frames
    through an encoder."""
    aus, recs, intra, sse = [], [], [], []
    for y, uv in frames:
        aus.append(bytes(enc.encode(*put(y, uv), False)))
        recs.append(tuple(np.array(p) for p in enc.recon()))
        intra.append(enc.cu_types().count(3) if hasattr(enc, "cu_types") else None)
        sse.append(tuple(enc.stats.sse))
    return aus, recs, intra, sse


def assert_decodes_to(aus, recs):
    """Decode picture by picture; returns the decoder and the slices of every picture."""
    dec, slices = Decoder(), []
    for t, (au, (ry, ruv)) in enumerate(zip(aus, recs)):
        before = dec.stats["slices"]
        dec.decode(au)
        slices.append(dec.stats["slices"] - before)
        y, u, v = dec.frames_coded[t]
        assert np.array_equal(y, ry) and np.array_equal(u, ruv[:, 0::2]) and np.array_equal(v, ruv[:, 1::2]), t
    return dec, slices


@pytest.fixture(scope="module")
def cpu_streams(native):
    """Every case coded once by the CPU encoder with the option on."""
    out = {}
    for (w, h), qp, deblock, split in CASES:
        enc = native.CpuHevcEncoder(make_cfg(native, w, h, qp, deblock, split, 1))
        out[(w, h), qp, deblock, split] = encode(enc, intra_p_frames(w, h))
    return out


@pytest.mark.parametrize("case", CASES, ids=str)
def test_cpu_intra_in_p_decodes_to_reconstruction(native, cpu_streams, case):
    (w, h), qp, deblock, split = case
    aus, recs, intra, _ = cpu_streams[case]
    units = ((w + 15) // 16) * ((h + 15) // 16)
    for n in intra[1:]:  # both P pictures hold intra and inter units
        assert 0 < n < units, intra
    dec, slices = assert_decodes_to(aus, recs)
    assert dec.stats["intra"] == sum(intra)
    assert min(slices[1:]) >= 3, slices


@pytest.mark.parametrize("case", CASES, ids=str)
def test_cpu_option_off_codes_the_parent_streams(native, case):
    (w, h), qp, deblock, split = case
    for option in (None, 0):  # the default is off
        enc = native.CpuHevcEncoder(make_cfg(native, w, h, qp, deblock, split, option))
        aus, _, intra, _ = encode(enc, intra_p_frames(w, h))
        assert intra[1:] == [0, 0]
        want = json.loads(GOLDEN.read_text())[f"{w}x{h} qp{qp} deblock{deblock} split{split}"]
        assert hashlib.sha256(b"".join(aus)).hexdigest() == want


def test_option_from_environment_to_session_config(native):
    from mxdesk.pipeline.stream import apply_encoder_args
    from mxdesk.utils import config as C

    assert C.load(env={}, argv=[]).hevc_intra_in_p == 0
    for v in (0, 1):
        assert C.load(env={"MXDESK_HEVC_INTRA_IN_P": str(v)}, argv=[]).hevc_intra_in_p == v
    for bad in ("2", "-1"):
        with pytest.raises(ValueError, match="MXDESK_HEVC_INTRA_IN_P"):
            C.load(env={"MXDESK_HEVC_INTRA_IN_P": bad}, argv=[])
    cfg = C.load(env={"MXDESK_HEVC_INTRA_IN_P": "1"}, argv=[])
    sc = native.SessionConfig()
    assert sc.enc.hevc_intra_in_p == 0 and sc.enc.intra_in_p == 0
    apply_encoder_args(sc.enc, dict(bitrate_kbps=cfg.video_bitrate, keyint=cfg.keyint_frames,
                                    search_range=cfg.search_range, scroll_range=cfg.scroll_range,
                                    partitions=cfg.h264_partitions, subpel=cfg.subpel,
                                    hevc_intra_in_p=cfg.hevc_intra_in_p))
    assert sc.enc.hevc_intra_in_p == 1 and sc.enc.intra_in_p == 0  # H.264's field is another option
