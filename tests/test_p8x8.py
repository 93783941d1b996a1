"""H.264 P_8x8 macroblocks (EncoderConfig.partitions 2: one vector per 8x8 quadrant, four P_L0_8x8
sub-macroblocks) on the CPU encoder: the quadrant search, the 8x8 vector prediction and the
sub_mb_pred syntax, four-vector motion compensation and the inner-edge boundary strengths, pinned to
the independent decoder (mxdesk/codec/h264_decoder.py); and the streams of partitions 0 and 1, which
must stay what they were (tests/golden/h264_partitions_parent.json)."""
import json
from pathlib import Path

import numpy as np
import pytest

from mxdesk.codec.h264_decoder import DecodeError, Decoder

from . import quad_content as qc

CASES = [(0, 1), (1, 1), (1, 0), (0, 0)]  # (me_coarse, subpel)
CONTENT = {
    "quad": lambda w, h, t: qc.quad_motion(w, h, t),
    "quad_half": lambda w, h, t: qc.quad_motion(w, h, t, half=True),
    "corner": qc.window_corner,
}


def _check_decoder(aus, recons):
    dec = Decoder()
    dec.decode(b"".join(aus))
    assert len(dec.frames_coded) == len(recons)
    for t, ((yy, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, recons)):
        assert np.array_equal(yy, ry), f"frame {t} luma"
        assert np.array_equal(u, ruv[:, 0::2]) and np.array_equal(v, ruv[:, 1::2]), f"frame {t} chroma"


def _quad_vectors(infos, pmv8):
    """(n, 8) vectors of the inter macroblocks coded P_8x8 over all pictures."""
    out = [p[(i[..., 8] == 3) & (i[..., 0] == 0)] for i, p in zip(infos, pmv8)]
    return np.concatenate(out) if out else np.zeros((0, 8), np.int32)


@pytest.mark.parametrize("content", sorted(CONTENT))
@pytest.mark.parametrize("coarse,subpel", CASES)
def test_p8x8_decodes_to_reconstruction(native, content, coarse, subpel):
    w, h = 128, 64
    frames = [CONTENT[content](w, h, t) for t in range(5)]
    aus, recons, infos, pmv8 = qc.encode_cpu(native, frames, w, h, partitions=2, me_coarse=coarse, subpel=subpel)
    assert qc.count_p8x8(infos) > 8, [np.bincount(i[..., 8].ravel()) for i in infos]
    _check_decoder(aus, recons)
    v = _quad_vectors(infos, pmv8)
    assert (v.reshape(-1, 4, 2) != v.reshape(-1, 4, 2)[:, :1]).any(), "quadrants with different vectors"
    if content == "quad_half" and subpel:
        assert (v & 3).any(), "a fractional quadrant vector"
    if not subpel:
        assert not (v & 3).any()


def test_p8x8_with_deblocking_intra_in_p_rate_control_and_scroll_hint(native):
    # bS on the inner edges at 8 (quadrants' vectors differ), intra neighbours, per-MB QP, and a
    # search centred on the scroll hint: a scrolled page over a band of quad motion
    w, h = 160, 96
    frames = [qc.scroll_with_quad_band(w, h, t, 4) for t in range(6)]
    cfg = dict(partitions=2, deblock=1, intra_in_p=1, bitrate_kbps=500, scroll_range=16)
    aus, recons, infos, _ = qc.encode_cpu(native, frames, w, h, **cfg)
    assert qc.count_p8x8(infos) >= 1
    _check_decoder(aus, recons)
    # the same options on the plain quad motion (no hint: the centre stays zero)
    frames = [qc.quad_motion(w, h, t) for t in range(6)]
    aus, recons, infos, _ = qc.encode_cpu(native, frames, w, h, **cfg)
    assert qc.count_p8x8(infos) >= 1
    _check_decoder(aus, recons)


def test_p8x8_searched_around_the_scroll_hint(native):
    # pictures with a hint (QP 12, as the scroll tests: a scrolled macroblock has to match within the
    # static threshold) whose band of quad motion is searched around the hint or around zero
    from . import scroll_content as sc

    w, h = qc.SCROLL_SHAPE
    enc = native.CpuH264Encoder(sc.config(native, w, h, dict(scroll=16, qp=12, partitions=2, deblock=1)))
    aus, recons, hints, centred = [], [], [], 0
    for y, uv in qc.scrolled_with_quad_band():
        aus.append(bytes(enc.encode(y, uv, False)))
        recons.append(enc.recon())
        st, i = enc.stats, enc.mb_info()
        hints.append((st.scroll_dx, st.scroll_dy))
        if not st.idr:
            centred += int(((i[..., 8] == 3) & (i[..., 0] == 0) & (enc.mb_scroll_path() == 3)).sum())
    assert hints[-len(qc.SCROLL_MOVES):] == list(qc.SCROLL_MOVES)
    assert centred > 0
    _check_decoder(aus, recons)


def test_p8x8_vectors_outside_the_picture(native):
    # 136x72 is coded 144x80: the edge quadrants' vectors point outside the picture on the left
    # (quadrant TL moves right) and at the top (TR moves down)
    w, h = 136, 72
    frames = [qc.quad_motion(w, h, t) for t in range(5)]
    aus, recons, infos, pmv8 = qc.encode_cpu(native, frames, w, h, partitions=2)
    assert qc.count_p8x8(infos) > 8
    outside = 0
    for i, p in zip(infos[1:], pmv8[1:]):
        q3 = (i[..., 8] == 3) & (i[..., 0] == 0)
        outside += int((q3[:, 0] & (p[:, 0, 0] < 0)).sum())  # left column, TL: x0 + mvx / 4 < 0
        outside += int((q3[0, :] & (p[0, :, 3] < 0)).sum())  # top row, TR: y0 + mvy / 4 < 0
    assert outside > 0
    _check_decoder(aus, recons)


def test_mb_pmv8_matches_the_decoded_vectors(native):
    w, h = 128, 64
    frames = [qc.quad_motion(w, h, t, half=True) for t in range(5)]
    aus, _, infos, pmv8 = qc.encode_cpu(native, frames, w, h, partitions=2)
    dec = Decoder()
    seen = 0
    for au, info, p8 in zip(aus, infos, pmv8):
        dec.decode(au)
        mb_w = info.shape[1]
        for my, mx in zip(*np.nonzero((info[..., 8] == 3) & (info[..., 0] == 0))):
            m = dec.mbs[my * mb_w + mx]
            got = [m.mv4[0][0], m.mv4[0][2], m.mv4[2][0], m.mv4[2][2]]
            assert [tuple(int(c) for c in v) for v in got] == [tuple(int(c) for c in p8[my, mx, 2 * q: 2 * q + 2]) for q in range(4)]
            for by in range(4):
                for bx in range(4):
                    assert tuple(m.mv4[by][bx]) == tuple(got[2 * (by // 2) + bx // 2])
            seen += 1
    assert seen > 8
    # macroblocks of other shapes report zeros
    assert all(not p[(i[..., 8] != 3)].any() for i, p in zip(infos, pmv8))


def test_partitions_0_and_1_streams_are_the_parents(native):
    want = json.loads((Path(__file__).parent / "golden" / "h264_partitions_parent.json").read_text())
    got = qc.partition_digests(native)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k] == want[k], k


def test_partitions_1_never_codes_p8x8(native):
    w, h = 128, 64
    frames = [qc.quad_motion(w, h, t) for t in range(3)]
    _, _, infos, _ = qc.encode_cpu(native, frames, w, h, partitions=1)
    assert all(not (i[..., 8] == 3).any() for i in infos)


def _patch_first_sub_mb_type(au: bytes) -> bytes:
    """The access unit with the first P_8x8 macroblock's first sub_mb_type ue(0) ue(0) ue(0) ('111')
    turned into ue(1) ('010') + ue(0): mb_skip_run ue(0), mb_type ue(3) and four sub_mb_type ue(0) are
    the bit pattern 1 00100 1111, looked for behind the start code and NAL header."""
    bits = np.unpackbits(np.frombuffer(au, np.uint8))
    pat = np.array([1, 0, 0, 1, 0, 0, 1, 1, 1, 1], np.uint8)
    start = au.index(b"\x00\x00\x01") + 4  # first slice NAL: start code + NAL header byte
    for o in range(8 * start, len(bits) - len(pat)):
        if np.array_equal(bits[o:o + len(pat)], pat):
            bits[o + 6: o + 9] = (0, 1, 0)
            return np.packbits(bits).tobytes()
    raise AssertionError("no P_8x8 header found")


def test_decoder_rejects_other_sub_mb_types(native):
    w, h = 128, 64
    frames = [qc.quad_motion(w, h, t) for t in range(2)]
    aus, _, infos, _ = qc.encode_cpu(native, frames, w, h, partitions=2)
    assert infos[1][0, 0, 8] == 3 and infos[1][0, 0, 0] == 0 and infos[1][0, 0, 3] == 0  # MB 0: P_8x8, coded
    Decoder().decode(aus[0] + aus[1])
    with pytest.raises(DecodeError, match="sub_mb_type 1"):
        Decoder().decode(aus[0] + _patch_first_sub_mb_type(aus[1]))


def test_decoder_names_p8x8ref0():
    with pytest.raises(DecodeError, match="P_8x8ref0"):
        Decoder().decode_inter_mb(None, 0, 0, 4, 0, 0)  # rejected before anything is read


def test_config_reaches_the_encoder(native):
    from mxdesk.pipeline.stream import apply_encoder_args
    from mxdesk.utils import config as C

    cfg = C.load(env={"MXDESK_H264_PARTITIONS": "2"}, argv=[])
    assert cfg.h264_partitions == 2
    assert C.load(env={}, argv=[]).h264_partitions == 1
    sc = native.SessionConfig()
    apply_encoder_args(sc.enc, dict(bitrate_kbps=cfg.video_bitrate, keyint=cfg.keyint_frames, search_range=cfg.search_range,
                                    scroll_range=cfg.scroll_range, partitions=cfg.h264_partitions, subpel=cfg.subpel))
    assert sc.enc.partitions == 2
    for bad in ("3", "-1"):
        with pytest.raises(ValueError, match="MXDESK_H264_PARTITIONS"):
            C.load(env={"MXDESK_H264_PARTITIONS": bad}, argv=[])
