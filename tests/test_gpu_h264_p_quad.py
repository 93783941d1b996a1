"""H.264 P pictures through k_p_fused (search and coding of a macroblock in one kernel, the search
scoring four horizontally adjacent candidates per v_qsad_pk_u16_u8) against the CPU oracle.  The
claim: GPU access units and reconstructions equal CpuH264Encoder's and the independent decoder's
pictures, whichever macroblocks of a picture move and whichever scoring loop the configuration
selects (partitions, the coarse even grid, the exhaustive search).

Sizes: 48x48 (9 macroblocks), 96x48 (18), 80x48 (15, rows of 5), 128x64 (32), 16x16 (a single
macroblock).

Content: a flat background, which the encoders reconstruct exactly, so a macroblock outside the
rectangle is static; a textured rectangle whose texture pans by whole and fractional samples and
whose position and size change from picture to picture (from the whole picture to less than a
macroblock), so static and moving macroblocks are neighbours in every arrangement.

Condition on the input, checked on the CPU oracle's mb_info alone: over the P pictures of every case
(except 16x16) there are groups of four consecutive macroblocks (the last group of a picture may be
shorter) with 0, 1, 2, 3 and 4 macroblocks of non-zero motion.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from .gpu_util import pitched  # noqa: E402

# per picture: the rectangle in macroblock units (x, y, w, h; clipped to the picture) and the pan of
# its texture since the previous picture in quarter samples.  A rectangle stays for two pictures: in
# the second one only its own macroblocks move, in the first one also those it has just left.
SCHEDULE = [
    ((1.2, 1.2, 0.6, 0.6), (0, 0)),     # inside one macroblock
    ((1.2, 1.2, 0.6, 0.6), (4, 0)),
    ((0.0, 0.0, 2.0, 1.0), (8, 4)),     # two macroblocks of a row
    ((0.0, 0.0, 2.0, 1.0), (1, 0)),
    ((3.0, 0.0, 2.0, 2.0), (0, 3)),     # a 2 x 2 block
    ((3.0, 0.0, 2.0, 2.0), (2, 2)),
    ((0.0, 0.0, 3.0, 9.0), (-4, 4)),    # three columns
    ((0.0, 0.0, 3.0, 9.0), (6, -1)),
    ((0.0, 0.0, 9.0, 9.0), (-3, -2)),   # everything
    ((0.0, 0.0, 9.0, 9.0), (12, 0)),
    ((0.0, 1.0, 3.0, 1.0), (5, 5)),     # three macroblocks of the second row
    ((0.0, 1.0, 3.0, 1.0), (-8, -8)),
    ((1.0, 0.0, 1.0, 9.0), (3, 0)),     # a column
    ((1.0, 0.0, 1.0, 9.0), (0, -6)),
]
N_FRAMES = len(SCHEDULE)


def _texture(u, v):
    t = 128 + 50 * np.sin(0.37 * u + 0.11 * v) + 40 * np.sin(0.13 * u - 0.41 * v + 1.0) + 20 * np.sin(0.9 * u + 0.8 * v)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ox = oy = 0
    frames = []
    for (fx, fy, fw, fh), (dx, dy) in SCHEDULE:
        ox, oy = ox + dx, oy + dy
        y = np.full((h, w), 128, np.uint8)
        x0, y0 = min(w - 8, int(16 * fx)), min(h - 8, int(16 * fy))
        x1, y1 = min(w, x0 + int(16 * fw)), min(h, y0 + int(16 * fh))
        y[y0:y1, x0:x1] = _texture(xx - ox / 4.0, yy - oy / 4.0)[y0:y1, x0:x1]
        uv = np.full((h // 2, w), 128, np.uint8)
        uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
        uv[:, 1::2] = 200 - y[1::2, 0::2] // 2
        frames.append((y, uv))
    return frames


def _config(native, w, h, o):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, o.get("qp", 28), o.get("range", 8)
    cfg.subpel, cfg.partitions, cfg.me_coarse = o.get("subpel", 1), o.get("partitions", 1), o.get("me_coarse", 0)
    cfg.deblock, cfg.intra_in_p = o.get("deblock", 0), o.get("intra_in_p", 0)
    if "aq" in o:
        cfg.aq = o["aq"]
    return cfg


def _quad_counts(mb):
    """How many groups of four consecutive macroblocks have 0..4 macroblocks of non-zero motion."""
    flat = mb.reshape(-1, mb.shape[-1])
    moving = [int(r[0]) == 0 and (int(r[4]) != 0 or int(r[5]) != 0 or int(r[8]) != 0) for r in flat]
    counts = [0] * 5
    for b in range(0, len(moving), 4):
        counts[sum(moving[b:b + 4])] += 1
    return counts


def _cpu_oracle(native, w, h, o):
    cenc = native.CpuH264Encoder(_config(native, w, h, o))
    aus, recs, counts = [], [], [0] * 5
    for t, (y, uv) in enumerate(_frames(w, h)):
        aus.append(cenc.encode(y, uv, False))
        recs.append(tuple(a.copy() for a in cenc.recon()))
        if t:
            counts = [a + b for a, b in zip(counts, _quad_counts(cenc.mb_info()))]
    return aus, recs, counts


SHAPES = [(48, 48), (96, 48), (80, 48), (128, 64), (16, 16)]
OPTIONS = [dict(partitions=p, subpel=s, me_coarse=c) for p in (0, 1) for s in (0, 1) for c in (0, 1)] + [
    dict(range=16),
    dict(intra_in_p=1),
    dict(aq=3),
    dict(qp=10),
    dict(qp=51),
]  # aq default and QP 28: every case that does not set them
CASES = [(w, h, o) for (w, h) in SHAPES for o in OPTIONS]
CASES.append((80, 48, dict(deblock=1)))  # the two kernels (k_me_full, k_inter_encode), not k_p_fused


def _id(c):
    return f"{c[0]}x{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2].items())


@pytest.mark.parametrize("w,h,o", CASES, ids=[_id(c) for c in CASES])
def test_gpu_quads_vs_cpu_and_decoder(gpu, w, h, o):
    caus, crecs, counts = _cpu_oracle(gpu, w, h, o)
    print(f"{_id((w, h, o))}: groups of four by moving macroblocks {counts}")
    if (w, h) != (16, 16):
        assert all(c > 0 for c in counts), counts
    genc = gpu.GpuH264Encoder(_config(gpu, w, h, o), torch.cuda.current_stream().cuda_stream)
    ch = genc.coded_height
    stream, grecs = b"", []
    for t, (y, uv) in enumerate(_frames(w, h)):
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


def _run_session(gpu, depth, use_graph, n=12, idr_at=6):
    """A desktop session of 13 x 7 = 91 macroblocks, in-loop filter off: every P picture is k_p_fused."""
    cfg = gpu.SessionConfig()
    cfg.width, cfg.height, cfg.fps = 208, 112, 60
    cfg.codec = "h264"
    cfg.enc.bitrate_kbps = 0
    cfg.enc.pipeline_depth = depth
    cfg.enc.deblock = 0
    cfg.use_graph = use_graph
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


@functools.lru_cache(maxsize=None)
def _eager_depth3(gpu):
    return _run_session(gpu, 3, 0)


def test_depth3_matches_depth1_through_idr(gpu):
    a, b = _run_session(gpu, 1, 0), _eager_depth3(gpu)
    _same_run(a, b)
    dec = Decoder()
    dec.decode(b"".join(b[0]))
    yy = dec.frames_coded[-1][0]
    assert np.array_equal(yy, b[2][0][:yy.shape[0], :yy.shape[1]])


def test_graph_replay_matches_eager(gpu):
    _same_run(_eager_depth3(gpu), _run_session(gpu, 3, 1))
