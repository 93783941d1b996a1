"""H.264 P pictures: macroblocks whose residual is known to quantise to zero (h264_mb.h
zero_sum_4x4 / zero_sum_chroma_dc) skip every transform in the coder, the SATD is formed only
for intra_in_p and the rate-distortion sums only where a residual drop is possible; and a P picture
whose reference was not deblocked is one kernel (k_p_fused: the workgroup that searched a
macroblock codes it).  deblock 0 runs the fused kernel on every P picture, deblock 1 the two
kernels (k_me_full on the unfiltered copy, k_inter_encode) on every one.  The claim: GPU access
units and reconstructions equal the CPU oracle's (which runs every transform for every
macroblock) and the independent decoder's pictures.

Content: the top macroblock rows pan (test_gpu_h264_otf's split-motion content: fractional vectors,
both partition shapes); the rows below are flat with seeded per-frame noise whose 4x4 block sums
are drawn around the bound of the case's QP and grow from picture to picture, so residual sums fall
on both sides of it.  (Flat, not textured: a textured static part leaves coding noise whose block
sums are over the bound in every picture, and no macroblock ever falls within it.)

For every case the oracle's own macroblocks are counted (CpuH264Encoder.mb_info / recon and the
bound functions, for 16x16 macroblocks with a zero vector, whose prediction is the previous
reconstruction):
  within   luma and chroma within their bounds, residual not all zero  -> must have cbp == 0
  above    some bound exceeded, yet cbp == 0
  coded    cbp != 0 (any inter macroblock)
At least 5 of each kind are asserted over a case's P pictures, with these exceptions, which the
content cannot give at these sizes:
  * "above" at QP 10: it needs a block sum over the bound of which no single coefficient reaches a
    level.  The bound there is 4 (2 at the macroblock QP 4 of the temporal classes) and nearly
    tight: a sum of 5..8 nearly always holds a coefficient that does.  The oracle shows 0..5 such
    macroblocks per case at QP 10 (0 at 48x48 with its 3 static macroblocks per picture), so
    "above" is not asserted at QP 10.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from .gpu_util import pitched  # noqa: E402
from .test_gpu_h264_otf import _split_frames  # noqa: E402

N_FRAMES = 15
# a block's sum |noise| as a multiple of the bound at the frame QP, by the picture's step
LEVELS = (0.1, 0.2, 0.3, 0.45, 0.7, 1.0, 1.5, 2.2, 3.0, 4.5, 7.0, 12.0, 24.0, 48.0)
QUIET = 3  # pictures after the IDR without noise: the P pictures finish the flat part's reconstruction


def _pan_rows(h):
    """Rows [0, this) pan: the split-motion content's partition boundaries lie inside them."""
    return 16 * (((h + 15) // 16) // 2) + 16


@functools.lru_cache(maxsize=None)
def _frames(w, h, bound):
    """The static part is flat (the encoders reconstruct it exactly, so a macroblock's residual is
    its noise alone until it is first coded) plus noise that is drawn anew for every picture and
    grows from picture to picture, macroblock columns staggered by a step."""
    pan = _split_frames(w, h, N_FRAMES)
    top = _pan_rows(h)
    rng = np.random.default_rng(7000 + 13 * w + h + 1000 * bound)
    frames = []
    for t in range(N_FRAMES):
        y = pan[t][0].copy()
        noise = np.zeros((h, w), np.int64)
        for by in range(top // 4, (h + 3) // 4):
            for bx in range((w + 3) // 4):
                k = t - QUIET - 2 + (bx // 4) % 3
                lv = LEVELS[min(k, len(LEVELS) - 1)] if k >= 0 else 0.0
                total = int(round(lv * bound * rng.uniform(0.8, 1.0)))
                mag = rng.multinomial(total, np.full(16, 1 / 16)) * rng.choice([-1, 1], 16)
                blk = np.clip(mag.reshape(4, 4), -100, 100)
                hh, ww = min(4, h - 4 * by), min(4, w - 4 * bx)
                noise[4 * by:4 * by + hh, 4 * bx:4 * bx + ww] = blk[:hh, :ww]
        if h % 16:  # the encoders replicate the last row / column into the padding: kept free of
            noise[h - 1] = 0  # noise, or a padded block would hold four copies of it
        if w % 16:
            noise[:, w - 1] = 0
        y[top:] = (128 + noise[top:]).astype(np.uint8)
        uv = np.full((h // 2, w), 128, np.uint8)
        uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
        uv[:, 1::2] = 200 - y[1::2, 0::2] // 2
        frames.append((y, uv))
    return frames


def _config(native, w, h, qp, aq, deblock, intra_in_p):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, qp, 8
    cfg.subpel, cfg.partitions, cfg.deblock, cfg.intra_in_p = 1, 1, deblock, intra_in_p
    if aq is not None:
        cfg.aq = aq
    return cfg


def _padded(y, uv, cw, ch):
    """The source as both encoders see it: last column / chroma pair and last row replicated."""
    h, w = y.shape
    yp = np.pad(y, ((0, ch - h), (0, cw - w)), mode="edge").astype(np.int64)
    c = np.pad(uv.reshape(h // 2, w // 2, 2), ((0, (ch - h) // 2), (0, (cw - w) // 2), (0, 0)), mode="edge")
    return yp, c.astype(np.int64)


def _block_sums(a):
    """Sum |a| over the 4x4 blocks of a 2-D array."""
    r, c = a.shape
    return np.abs(a).reshape(r // 4, 4, c // 4, 4).sum(axis=(1, 3))


def _cpu_oracle(native, w, h, qp, aq, deblock, intra_in_p):
    """CPU access units, reconstructions and the counts of the three kinds over the P pictures."""
    hq = native.h264
    cfg = _config(native, w, h, qp, aq, deblock, intra_in_p)
    cenc = native.CpuH264Encoder(cfg)
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    aus, recs = [], []
    n = dict(within=0, above=0, coded=0, luma_only=0, chroma_only=0, violations=0)
    for t, (y, uv) in enumerate(_frames(w, h, hq.zero_sum_4x4(qp))):
        aus.append(cenc.encode(y, uv, False))
        recs.append(tuple(a.copy() for a in cenc.recon()))
        if t == 0:
            continue
        mb = cenc.mb_info()  # (mb_h, mb_w, 9): type, qp, cbp, skip, mvx, mvy, nz, cost, part
        sy, sc = _padded(y, uv, cw, ch)
        ry = sy - recs[t - 1][0].astype(np.int64)
        rc = sc - recs[t - 1][1].reshape(ch // 2, cw // 2, 2).astype(np.int64)
        for my in range(mb.shape[0]):
            for mx in range(mb.shape[1]):
                typ, mqp, cbp, _, mvx, mvy, _, _, part = (int(v) for v in mb[my, mx])
                if typ != 0:
                    continue
                n["coded"] += cbp != 0
                if part != 0 or mvx != 0 or mvy != 0:
                    continue
                qpc = hq.chroma_qp(mqp, cfg.chroma_qp_offset)
                l = ry[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
                c = rc[8 * my:8 * my + 8, 8 * mx:8 * mx + 8]
                luma_ok = _block_sums(l).max() <= hq.zero_sum_4x4(mqp)
                chroma_ok = all(_block_sums(c[..., k]).max() <= hq.zero_sum_4x4(qpc) and
                                np.abs(c[..., k]).sum() <= hq.zero_sum_chroma_dc(qpc) for k in range(2))
                nonzero = bool(np.any(l) or np.any(c))
                if luma_ok and chroma_ok:
                    n["within"] += nonzero
                    n["violations"] += cbp != 0
                else:
                    n["above"] += cbp == 0
                    n["luma_only"] += bool(luma_ok)
                    n["chroma_only"] += bool(chroma_ok)
                    n["violations"] += bool(luma_ok and (cbp & 15)) + bool(chroma_ok and (cbp >> 4))
    return aus, recs, n


SHAPES = [(48, 48), (80, 48), (100, 60)]  # 9 and 15 macroblocks; a cropped right column and bottom row
MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (deblock, intra_in_p)


@pytest.mark.parametrize("deblock,intra_in_p", MODES)
@pytest.mark.parametrize("aq", [0, 2, 3, None])
@pytest.mark.parametrize("qp", [10, 28, 40, 51])
@pytest.mark.parametrize("w,h", SHAPES)
def test_gpu_zero_residual_shortcut_vs_cpu_and_decoder(gpu, w, h, qp, aq, deblock, intra_in_p):
    caus, crecs, n = _cpu_oracle(gpu, w, h, qp, aq, deblock, intra_in_p)
    print(f"{w}x{h} qp {qp} aq {aq} deblock {deblock} intra_in_p {intra_in_p}: {n}")
    assert n["violations"] == 0, n  # the bound against the oracle's own transforms
    assert n["within"] >= 5 and n["coded"] >= 5 and (qp == 10 or n["above"] >= 5), n
    genc = gpu.GpuH264Encoder(_config(gpu, w, h, qp, aq, deblock, intra_in_p), torch.cuda.current_stream().cuda_stream)
    ch = genc.coded_height
    stream, grecs = b"", []
    for t, (y, uv) in enumerate(_frames(w, h, gpu.h264.zero_sum_4x4(qp))):
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


def _run_session(gpu, depth, use_graph, deblock, n=12, idr_at=6):
    cfg = gpu.SessionConfig()
    cfg.width, cfg.height, cfg.fps = 320, 192, 60
    cfg.codec = "h264"
    cfg.enc.bitrate_kbps = 0
    cfg.enc.pipeline_depth = depth
    cfg.use_graph = use_graph
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


def _same_run(a, b):
    assert a[1] == b[1] and a[1][6] == 1 and sum(a[1]) == 2
    for t, (x, y) in enumerate(zip(a[0], b[0])):
        assert x == y, f"frame {t} differs"
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])


def test_depth3_matches_depth1_adaptive_filter(gpu):
    """Desktop session, the adaptive in-loop filter (the default): depth 3 through a forced IDR
    equals depth 1, access units and final reconstruction, and decodes to it."""
    a, b = _run_session(gpu, 1, 0, None), _run_session(gpu, 3, 0, None)
    _same_run(a, b)
    dec = Decoder()
    dec.decode(b"".join(b[0]))
    yy = dec.frames_coded[-1][0]
    assert np.array_equal(yy, b[2][0][:yy.shape[0], :yy.shape[1]])


def test_graph_replay_matches_eager(gpu):
    """Depth 3 with the per-frame chain replayed as hipGraphs (fixed filter: off) equals eager launches."""
    _same_run(_run_session(gpu, 3, 0, 0), _run_session(gpu, 3, 1, 0))
