"""H.264 P pictures interpolate the reference where they use it: k_me_full builds its sub-sample
footprints from the search window of the reconstruction, k_inter_encode predicts fractional vectors
from a window of it staged in LDS -- no half-sample planes.  The interpolation against
h264.luma_qpel, the encoder against the CPU oracle and the independent decoder, and the two
entropy streams of depth 3 against depth 1."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from .gpu_util import pitched  # noqa: E402


# ---------------------------------------------------------------- 1. the interpolation hook
def _block_origins(w, h):
    """Integer block positions: interior, straddling each edge and each corner, wholly outside the
    picture by up to 35 samples."""
    xs_in, ys_in = (w - 16) // 2, (h - 16) // 2
    out = [(xs_in, ys_in)]
    out += [(-7, ys_in), (w - 9, ys_in), (xs_in, -6), (xs_in, h - 10)]                    # edges
    out += [(-5, -9), (w - 11, -3), (-13, h - 4), (w - 6, h - 7)]                         # corners
    out += [(-16 - 35, ys_in), (w + 35, ys_in), (xs_in, -16 - 35), (xs_in, h + 35),       # outside
            (-16 - 20, -16 - 35), (w + 35, h + 17), (-17, h + 1), (w + 2, -19)]
    return out


@pytest.mark.parametrize("w,h", [(32, 32), (48, 32)])
def test_mc_luma_gpu_matches_luma_qpel(gpu, w, h):
    rng = np.random.default_rng(1000 + w)
    ref = rng.integers(0, 256, (h, w), dtype=np.uint8)
    pitch = 256  # the encoder's pitch: the dword paths run
    refp = np.zeros((h, pitch), np.uint8)
    refp[:, :w] = ref
    refp[:, w:] = 77  # never read: the picture ends at coded_w
    bad = []
    for bx, by in _block_origins(w, h):
        for yf in range(4):
            for xf in range(4):
                x4, y4 = 4 * bx + xf, 4 * by + yf
                got = gpu.h264.mc_luma_gpu(refp, w, x4, y4)
                want = np.array([[gpu.h264.luma_qpel(ref, x4 + 4 * c, y4 + 4 * r) for c in range(16)]
                                 for r in range(16)], np.uint8)
                if not np.array_equal(got, want):
                    bad.append((bx, by, xf, yf, int((got != want).sum())))
    assert not bad, bad[:8]
    # an unaligned pitch takes the byte path
    refq = np.zeros((h, w + 3), np.uint8)
    refq[:, :w] = ref
    for bx, by in [((w - 16) // 2, (h - 16) // 2), (-5, -9)]:
        got = gpu.h264.mc_luma_gpu(refq, w, 4 * bx + 1, 4 * by + 3)
        want = np.array([[gpu.h264.luma_qpel(ref, 4 * bx + 1 + 4 * c, 4 * by + 3 + 4 * r) for c in range(16)]
                         for r in range(16)], np.uint8)
        assert np.array_equal(got, want), (bx, by)


# ---------------------------------------------------------------- 2. encoder == CPU oracle == decoder
def _texture(seed, h4, w4):
    """Smooth texture on a 4x oversampled grid (a quarter sample per texel), wrapping."""
    rng = np.random.default_rng(seed)
    n = 24  # coarse cells of 24 texels = 6 samples
    coarse = rng.integers(20, 236, (h4 // n + 3, w4 // n + 3)).astype(np.float64)
    yy = np.arange(h4) / n
    xx = np.arange(w4) / n
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
    fy, fx = fy * fy * (3 - 2 * fy), fx * fx * (3 - 2 * fx)
    a = coarse[np.ix_(y0, x0)]
    b = coarse[np.ix_(y0, x0 + 1)]
    c = coarse[np.ix_(y0 + 1, x0)]
    d = coarse[np.ix_(y0 + 1, x0 + 1)]
    return (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy


@functools.lru_cache(maxsize=None)
def _split_frames(w, h, n=4):
    """Split-motion content: two textures panning by (5, 3) and (-7, 2) quarter samples per frame,
    joined 8 rows into a macroblock row; a third pan of (6, -5) in the top-right region, which
    starts 8 columns into a macroblock."""
    m = 4 * 64  # margin in texels: the pans stay inside the textures
    tex = [_texture(s, 4 * h + 2 * m, 4 * w + 2 * m) for s in (11, 12)]
    mbh, mbw = (h + 15) // 16, (w + 15) // 16
    join_y = 16 * (mbh // 2) + 8
    reg_x, reg_y = 16 * (mbw // 2) + 8, 16 * max(1, mbh // 3)
    yy, xx = np.mgrid[0:h, 0:w]
    frames = []
    for t in range(n):
        def pan(tx, dx, dy):
            return tx[m + 4 * yy + dy * t, m + 4 * xx + dx * t]
        y = np.where(yy < join_y, pan(tex[0], 5, 3), pan(tex[1], -7, 2))
        third = (xx >= reg_x) & (yy < reg_y)
        y = np.where(third, pan(tex[1], 6, -5), y)
        y = np.clip(np.rint(y), 0, 255).astype(np.uint8)
        uv = np.full((h // 2, w), 128, np.uint8)
        uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
        uv[:, 1::2] = 200 - y[1::2, 0::2] // 2
        frames.append((y, uv))
    return frames


def _config(native, w, h, rng, coarse, deblock):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, 28, rng
    cfg.me_coarse, cfg.subpel, cfg.partitions, cfg.deblock = coarse, 1, 1, deblock
    return cfg


def _cpu_oracle(native, w, h, rng, coarse, deblock):
    """CPU access units, reconstructions and the vector statistics of the P frames."""
    cenc = native.CpuH264Encoder(_config(native, w, h, rng, coarse, deblock))
    aus, recs = [], []
    stat = dict(frac=0, outside=0, p16x8=0, p8x16=0)
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    for t, (y, uv) in enumerate(_split_frames(w, h)):
        aus.append(cenc.encode(y, uv, False))
        recs.append(tuple(a.copy() for a in cenc.recon()))
        if t == 0:
            continue
        mb = cenc.mb_info()  # (mb_h, mb_w, 9): type, qp, cbp, skip, mvx, mvy, nz, cost, part
        inter = mb[..., 0] == 0
        stat["p16x8"] += int((inter & (mb[..., 8] == 1)).sum())
        stat["p8x16"] += int((inter & (mb[..., 8] == 2)).sum())
        one = inter & (mb[..., 8] == 0)  # mvx / mvy are the coded vector of a 16x16 macroblock
        mvx, mvy = mb[..., 4], mb[..., 5]
        stat["frac"] += int((one & (((mvx | mvy) & 3) != 0)).sum())
        my, mx = np.mgrid[0:mb.shape[0], 0:mb.shape[1]]
        x4, y4 = 64 * mx + mvx, 64 * my + mvy
        out = (x4 < 0) | (y4 < 0) | (x4 > 4 * (cw - 16)) | (y4 > 4 * (ch - 16))
        stat["outside"] += int((one & out).sum())
    return aus, recs, stat


SHAPES = [(64, 48, 8, 1), (48, 48, 32, 1), (100, 60, 16, 0), (72, 40, 16, 1), (80, 48, 32, 0)]


@pytest.mark.parametrize("deblock", [0, 1])
@pytest.mark.parametrize("w,h,rng,coarse", SHAPES)
def test_gpu_otf_interpolation_vs_cpu_and_decoder(gpu, w, h, rng, coarse, deblock):
    """Split-motion content with fractional vectors, vectors pointing outside the picture and both
    partition shapes: GPU access units and reconstructions == the CPU encoder's == the decoder's
    pictures.  deblock 1: the search runs on the unfiltered copy of the reference."""
    caus, crecs, stat = _cpu_oracle(gpu, w, h, rng, coarse, deblock)
    assert stat["frac"] >= 1 and stat["outside"] >= 1 and stat["p16x8"] >= 1 and stat["p8x16"] >= 1, stat
    genc = gpu.GpuH264Encoder(_config(gpu, w, h, rng, coarse, deblock), torch.cuda.current_stream().cuda_stream)
    ch = genc.coded_height
    stream, grecs = b"", []
    for t, (y, uv) in enumerate(_split_frames(w, h)):
        dy, duv = pitched(y, genc.pitch, ch), pitched(uv, genc.pitch, ch // 2, uv=True)
        torch.cuda.synchronize()
        gau = genc.encode(dy.data_ptr(), duv.data_ptr(), False)
        assert bool(gau == caus[t]), f"frame {t}: GPU {len(gau)} B vs CPU {len(caus[t])} B"
        gy, guv = genc.recon()
        assert np.array_equal(gy, crecs[t][0]) and np.array_equal(guv, crecs[t][1]), f"frame {t}: reconstruction"
        stream += gau
        grecs.append((gy.copy(), guv.copy()))
    dec = Decoder()
    dec.decode(stream)
    assert len(dec.frames_coded) == len(grecs)
    for t, ((yy, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, grecs)):
        hh, ww = yy.shape
        assert np.array_equal(yy, ry[:hh, :ww]), f"frame {t}: decoded luma"
        assert np.array_equal(u, ruv[:hh // 2, 0:ww:2]) and np.array_equal(v, ruv[:hh // 2, 1:ww:2]), \
            f"frame {t}: decoded chroma"


# ---------------------------------------------------------------- 3. two entropy streams
def _run_session(gpu, depth, deblock, n=12, idr_at=6):
    cfg = gpu.SessionConfig()
    cfg.width, cfg.height, cfg.fps = 320, 192, 60
    cfg.codec = "h264"
    cfg.enc.bitrate_kbps = 0
    cfg.enc.pipeline_depth = depth
    if deblock is not None:
        cfg.enc.deblock = deblock
    cfg.fake_clock = 1
    s = gpu.Session(cfg)
    out, sent = [], 0
    while sent < min(depth, n):
        s.submit(sent == idr_at)
        sent += 1
    for _ in range(n):
        out.append(s.collect())
        if sent < n:
            s.submit(sent == idr_at)
            sent += 1
    assert s.in_flight == 0
    return [bytes(r.au) for r in out], [int(r.idr) for r in out], tuple(a.copy() for a in s.recon())


@pytest.mark.parametrize("deblock", [0, None])  # off; the default adaptive filter
def test_two_entropy_streams_match_depth1(gpu, deblock):
    """Depth 3, eager: the entropy chains of consecutive pictures alternate between two streams.
    Access units (in picture order, a forced IDR in the middle) and the final reconstruction equal
    depth 1 byte for byte, and the decoder's last picture is that reconstruction."""
    a_au, a_idr, a_rec = _run_session(gpu, 1, deblock)
    b_au, b_idr, b_rec = _run_session(gpu, 3, deblock)
    assert a_idr == b_idr and a_idr[6] == 1 and sum(a_idr) == 2
    for t, (x, y) in enumerate(zip(a_au, b_au)):
        assert x == y, f"frame {t}: depth 3 differs from depth 1"
    assert np.array_equal(a_rec[0], b_rec[0]) and np.array_equal(a_rec[1], b_rec[1])
    dec = Decoder()
    dec.decode(b"".join(b_au))
    assert len(dec.frames_coded) == len(b_au)
    yy = dec.frames_coded[-1][0]
    assert np.array_equal(yy, b_rec[0][:yy.shape[0], :yy.shape[1]])
