"""The chain of an eager H.264 picture with three frames in flight: the events between its stages
travel as stop events of the kernels that produce them (k_bgrx_to_nv12 -> analysis in a session,
k_p_fused -> entropy chain, k_pack -> host), so a lost or early event shows as an access unit or a
reconstruction that differs from the CPU oracle's.

Encoder cases (pipeline_depth 3: the launcher thread issues the entropy chain): GPU access units
== CpuH264Encoder's, the in-tree decoder's pictures == the oracle's reconstructions, the last GPU
reconstruction == the oracle's.  Sizes 16x16 (one macroblock row), 48x48 and 80x48 (three rows),
100x60 (coded 112x64: four rows, the last one padded) at QP 10 / 28 / 51; deblock=1 and
intra_in_p=1 once each (more than one kernel precedes their events, which stay recorded).

Session cases (208x112, render and conversion on the capture stream in front): depth 3 ==
depth 1 through a forced IDR, and graph replay == eager.

Content: a flat background with a textured rectangle that pans by whole and fractional samples and
changes place, so every picture has skipped, static and moving macroblocks in its rows.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from .gpu_util import pitched  # noqa: E402

# per picture: rectangle (x, y, w, h in macroblocks, clipped) and the pan of its texture in quarter samples
SCHEDULE = [
    ((0.0, 0.0, 9.0, 9.0), (0, 0)),
    ((0.0, 0.0, 2.0, 1.0), (8, 4)),
    ((0.0, 0.0, 2.0, 1.0), (1, 0)),
    ((1.0, 1.0, 3.0, 9.0), (-4, 4)),
    ((1.0, 2.0, 9.0, 1.0), (6, -1)),
    ((0.0, 3.0, 9.0, 1.0), (-3, -2)),
    ((0.0, 0.0, 9.0, 9.0), (12, 0)),
    ((1.2, 0.2, 0.6, 0.6), (5, 5)),
]


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ox = oy = 0
    frames = []
    for (fx, fy, fw, fh), (dx, dy) in SCHEDULE:
        ox, oy = ox + dx, oy + dy
        u, v = xx - ox / 4.0, yy - oy / 4.0
        tex = 128 + 50 * np.sin(0.37 * u + 0.11 * v) + 40 * np.sin(0.13 * u - 0.41 * v + 1.0) + 20 * np.sin(0.9 * u + 0.8 * v)
        y = np.full((h, w), 128, np.uint8)
        x0, y0 = min(w - 8, int(16 * fx)), min(h - 8, int(16 * fy))
        x1, y1 = min(w, x0 + int(16 * fw)), min(h, y0 + int(16 * fh))
        y[y0:y1, x0:x1] = np.clip(np.rint(tex), 0, 255).astype(np.uint8)[y0:y1, x0:x1]
        uv = np.full((h // 2, w), 128, np.uint8)
        uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
        uv[:, 1::2] = 200 - y[1::2, 0::2] // 2
        frames.append((y, uv))
    return frames


def _config(native, w, h, o, depth):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, o.get("qp", 28), 8
    cfg.deblock, cfg.intra_in_p = o.get("deblock", 0), o.get("intra_in_p", 0)
    cfg.pipeline_depth = depth
    return cfg


SHAPES = [(16, 16), (48, 48), (80, 48), (100, 60)]
CASES = [(w, h, dict(qp=qp)) for (w, h) in SHAPES for qp in (10, 28, 51)]
CASES += [(80, 48, dict(deblock=1)), (80, 48, dict(intra_in_p=1))]


def _id(c):
    return f"{c[0]}x{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2].items())


@pytest.mark.parametrize("w,h,o", CASES, ids=[_id(c) for c in CASES])
def test_depth3_encoder_vs_cpu_and_decoder(gpu, w, h, o):
    cenc = gpu.CpuH264Encoder(_config(gpu, w, h, o, 1))
    caus, crecs = [], []
    for y, uv in _frames(w, h):
        caus.append(cenc.encode(y, uv, False))
        crecs.append(tuple(a.copy() for a in cenc.recon()))
    genc = gpu.GpuH264Encoder(_config(gpu, w, h, o, 3), torch.cuda.current_stream().cuda_stream)
    ch = genc.coded_height
    src = [(pitched(y, genc.pitch, ch), pitched(uv, genc.pitch, ch // 2, uv=True)) for y, uv in _frames(w, h)]
    torch.cuda.synchronize()
    gaus, sent = [], 0
    while sent < 3:
        genc.submit(src[sent][0].data_ptr(), src[sent][1].data_ptr(), False)
        sent += 1
    for _ in src:
        gaus.append(genc.collect())
        if sent < len(src):
            genc.submit(src[sent][0].data_ptr(), src[sent][1].data_ptr(), False)
            sent += 1
    for t, (g, c) in enumerate(zip(gaus, caus)):
        assert bool(g == c), f"frame {t}: GPU {len(g)} B vs CPU {len(c)} B"
    gy, guv = genc.recon()
    assert np.array_equal(gy, crecs[-1][0]) and np.array_equal(guv, crecs[-1][1]), "last reconstruction"
    dec = Decoder()
    dec.decode(b"".join(gaus))
    assert len(dec.frames_coded) == len(crecs)
    for t, ((yy, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, crecs)):
        hh, ww = yy.shape
        assert np.array_equal(yy, ry[:hh, :ww]), f"frame {t}: decoded luma"
        assert np.array_equal(u, ruv[:hh // 2, 0:ww:2]) and np.array_equal(v, ruv[:hh // 2, 1:ww:2]), \
            f"frame {t}: decoded chroma"


def _run_session(gpu, depth, use_graph, n=12, idr_at=6):
    """A desktop session of 13 x 7 macroblocks, in-loop filter off: every P picture is k_p_fused."""
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
    src = tuple(a.copy() for a in s.nv12())
    return [bytes(r.au) for r in out], [int(r.idr) for r in out], tuple(a.copy() for a in s.recon()), src


def _same_run(a, b):
    assert a[1] == b[1] and a[1][6] == 1 and sum(a[1]) == 2
    for t, (x, y) in enumerate(zip(a[0], b[0])):
        assert x == y, f"frame {t} differs"
    assert np.array_equal(a[2][0], b[2][0]) and np.array_equal(a[2][1], b[2][1])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1]), "converted source"


@functools.lru_cache(maxsize=None)
def _eager_depth3(gpu):
    return _run_session(gpu, 3, 0)


def test_session_depth3_matches_depth1_through_idr(gpu):
    a, b = _run_session(gpu, 1, 0), _eager_depth3(gpu)
    _same_run(a, b)
    dec = Decoder()
    dec.decode(b"".join(b[0]))
    assert len(dec.frames_coded) == len(b[0])
    yy = dec.frames_coded[-1][0]
    assert np.array_equal(yy, b[2][0][:yy.shape[0], :yy.shape[1]])


def test_session_graph_replay_matches_eager(gpu):
    """The graph path keeps recorded events: same pictures and the same converted source."""
    _same_run(_eager_depth3(gpu), _run_session(gpu, 3, 1))
