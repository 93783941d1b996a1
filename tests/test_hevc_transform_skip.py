"""HEVC P pictures with transform-skipped 4x4 luma TUs (EncoderConfig.hevc_transform_skip), CPU tier: the
stream decodes with the independent Python decoder to the encoder's reconstruction, the decoder counts
the skipped TUs the encoder chose, some but not all coded 4x4 luma TUs of every P picture are skipped,
the option does not make the P pictures larger, and it reaches the session's encoder configuration from
the environment."""
import itertools

import numpy as np
import pytest

from mxdesk.codec.hevc_decoder import Decoder

# 96x64: whole CTBs; 80x48: partial CTBs right and bottom; 72x40: units whose right / bottom 8x8 nodes
# lie outside the picture
CASES = list(itertools.product([(96, 64), (80, 48), (72, 40)], [24, 34], [0, 1]))  # size, QP, deblock + sao
BUMP = np.array([[10, 25, 25, 10], [25, 60, 60, 25], [25, 60, 60, 25], [10, 25, 25, 10]])


def stroke_frames(w, h):
    """Three NV12 frames: a flat mid-grey ground; then twice, over that ground, a different set of
    one-sample-wide horizontal and vertical strokes and isolated dots, luma +-90, about one per 8x8
    block.  The top left quadrant has no strokes: it stays smooth -- a slow ramp that changes from frame to
    frame under soft 4x4 bumps, one more per 8x8 block and frame -- so some TUs keep the transform."""
    rng = np.random.default_rng(11)
    ground = np.full((h, w), 128, np.uint8), np.full((h // 2, w), 128, np.uint8)
    yy, xx = np.mgrid[0:h // 2, 0:w // 2]
    frames = [ground]
    for t in (1, 2):
        y = ground[0].astype(np.int32)
        for by, bx in itertools.product(range(0, h, 8), range(0, w, 8)):
            if by < h // 2 and bx < w // 2:
                continue
            kind, amp = rng.integers(3), 90 * (1 - 2 * int(rng.integers(2)))
            py, px, n = by + rng.integers(8), bx + rng.integers(8), 3 + rng.integers(5)
            if kind == 0:
                y[py, px:min(px + n, w)] += amp
            elif kind == 1:
                y[py:min(py + n, h), px] += amp
            else:
                y[py, px] += amp
        # the smooth quadrant: a slow ramp that changes, and per 8x8 block one more soft 4x4 bump per frame
        q = 128 + (t * (xx + yy)) // 8
        for by, bx, tt in itertools.product(range(0, h // 2, 8), range(0, w // 2, 8), range(1, t + 1)):
            z = (by // 8 + bx // 8 + 2 * tt) % 4
            oy, ox = by + 4 * (z >> 1), bx + 4 * (z & 1)
            q[oy:oy + 4, ox:ox + 4] += BUMP[:h // 2 - oy, :w // 2 - ox]
        y[:h // 2, :w // 2] = q
        frames.append((np.clip(y, 16, 235).astype(np.uint8), ground[1]))
    return frames


def make_cfg(native, w, h, qp, filt, tskip):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps, cfg.qp, cfg.aq, cfg.search_range, cfg.tu_split = 0, qp, 1, 8, 2
    cfg.deblock, cfg.sao = filt, filt  # no in-loop filter at all, or both
    cfg.hevc_slice_cost = 64
    cfg.hevc_transform_skip = tskip
    return cfg


def encode(enc, frames, put=lambda y, uv: (y, uv)):
    """(access units, reconstructions, skipped TUs and distortion sums per picture) of the frames."""
    aus, recs, skipped, sse = [], [], [], []
    for y, uv in frames:
        aus.append(bytes(enc.encode(*put(y, uv), False)))
        recs.append(tuple(np.array(p) for p in enc.recon()))
        skipped.append(sum(bin(m).count("1") for m in enc.cu_tskip()) if hasattr(enc, "cu_tskip") else None)
        sse.append(tuple(enc.stats.sse))
    return aus, recs, skipped, sse


def assert_decodes_to(aus, recs):
    """Decode picture by picture; returns per picture the decoder's (skipped TUs, coded 4x4 luma TUs)."""
    dec, counts = Decoder(), []
    for t, (au, (ry, ruv)) in enumerate(zip(aus, recs)):
        before = dec.stats.get("transform_skip", 0), dec.stats.get("luma4_coded", 0)
        dec.decode(au)
        counts.append((dec.stats.get("transform_skip", 0) - before[0], dec.stats.get("luma4_coded", 0) - before[1]))
        y, u, v = dec.frames_coded[t]
        assert np.array_equal(y, ry) and np.array_equal(u, ruv[:, 0::2]) and np.array_equal(v, ruv[:, 1::2]), t
    return counts


@pytest.fixture(scope="module")
def cpu_streams(native):
    """Every case coded once by the CPU encoder with the option on and once with it off."""
    return {(case, on): encode(native.CpuHevcEncoder(make_cfg(native, *case[0], case[1], case[2], on)),
                               stroke_frames(*case[0]))
            for case in CASES for on in (0, 1)}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_cpu_transform_skip_decodes_to_reconstruction(cpu_streams, case):
    aus, recs, skipped, _ = cpu_streams[case, 1]
    counts = assert_decodes_to(aus, recs)
    print(case, "skipped", skipped, "decoder (skipped, coded 4x4 luma)", counts)
    assert [c[0] for c in counts] == skipped
    for t in (1, 2):  # every P picture holds skipped and transformed 4x4 luma TUs
        assert 0 < skipped[t] < counts[t][1], (skipped, counts)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_cpu_transform_skip_does_not_grow_the_p_pictures(cpu_streams, case):
    on, off = (sum(len(au) for au in cpu_streams[case, o][0][1:]) for o in (1, 0))
    print(case, "P bytes on", on, "off", off)
    assert cpu_streams[case, 0][2][1:] == [0, 0]
    assert on <= off


def test_option_from_environment_to_session_config(native):
    from mxdesk.pipeline.stream import apply_encoder_args
    from mxdesk.utils import config as C

    assert C.load(env={}, argv=[]).hevc_transform_skip == 0
    for v in (0, 1):
        assert C.load(env={"MXDESK_HEVC_TRANSFORM_SKIP": str(v)}, argv=[]).hevc_transform_skip == v
    for bad in ("2", "-1"):
        with pytest.raises(ValueError, match="MXDESK_HEVC_TRANSFORM_SKIP"):
            C.load(env={"MXDESK_HEVC_TRANSFORM_SKIP": bad}, argv=[])
    cfg = C.load(env={"MXDESK_HEVC_TRANSFORM_SKIP": "1"}, argv=[])
    sc = native.SessionConfig()
    assert sc.enc.hevc_transform_skip == 0
    apply_encoder_args(sc.enc, dict(bitrate_kbps=cfg.video_bitrate, keyint=cfg.keyint_frames,
                                    search_range=cfg.search_range, scroll_range=cfg.scroll_range,
                                    partitions=cfg.h264_partitions, subpel=cfg.subpel,
                                    hevc_transform_skip=cfg.hevc_transform_skip))
    assert sc.enc.hevc_transform_skip == 1


@pytest.mark.parametrize("intra_tu4", [False, True])
def test_token_path_codes_transform_skip_flag(native, intra_tu4):
    """Random slices with random skip masks: direct and token CABAC agree (throws on a mismatch)."""
    assert native.hevc_token_selftest(7, 40, intra_tu4, True) == 40
