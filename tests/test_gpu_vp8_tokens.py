"""VP8 token partitions boolean-coded on the GPU (EncoderConfig.vp8_tokens 1, k_vp8_tokens): every
access unit equals the CPU oracle's bytes (CpuVp8Encoder, the independent host writer that
tests/test_vp8.py pins to libwebp and the in-tree decoder), and the stream decodes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.vp8_decoder import Decoder  # noqa: E402

from .test_cpu_encoder import synthetic_nv12  # noqa: E402
from .test_gpu_production_sizes import _stream, desktop_nv12  # noqa: E402
from .test_gpu_vp8 import _dev  # noqa: E402


def _pair(gpu, w, h, tokens=1, kbps=0, qp=30, sr=8, depth=1, deblock=-1, cap=1024, aq=-1):
    cfg = gpu.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = kbps, qp, sr
    cfg.pipeline_depth, cfg.deblock, cfg.aq = depth, deblock, aq
    cfg.vp8_bpred = cfg.vp8_intra = 1
    cfg.vp8_tokens, cfg.vp8_tokens_cap = tokens, cap
    return gpu.GpuVp8Encoder(cfg, _stream()), gpu.CpuVp8Encoder(cfg)


def _moving(gpu, w, h, t):
    return synthetic_nv12(w, h, t, seed=t % 3)


def _still(gpu, w, h, t):
    return synthetic_nv12(w, h, 0, seed=1)


def _noise(gpu, w, h, t):
    r = np.random.default_rng(100 + t)
    return r.integers(0, 256, (h, w), dtype=np.uint8), r.integers(0, 256, (h // 2, w), dtype=np.uint8)


def _run(gpu, genc, cenc, w, h, content, frames, key_at=-1):
    aus = []
    for t in range(frames):
        y, uv = content(gpu, w, h, t)
        dy, duv = _dev(genc, y, uv)
        gau = genc.encode(dy.data_ptr(), duv.data_ptr(), t == key_at)
        cau = cenc.encode(y, uv, t == key_at)
        assert gau == cau, f"{w}x{h} frame {t}: GPU {len(gau)} B vs CPU {len(cau)} B"
        aus.append(gau)
    dec = Decoder()
    dec.decode(aus)
    return dec


# 1, 2, 4 and 8 partitions (3 and 9 macroblock rows: partitions of unequal row counts); ten frames
# with a forced key frame (probability updates from GPU-counted statistics, valid from frame 4);
# a still picture (repeated until the encoder has done refining it, six frames at aq 0 and QP 44:
# every macroblock of the last two is skipped, their partitions nothing but the flush); noise at
# QP 10 (the oracle's stream has levels up to 188 -- DCT_CAT3..6 extra bits -- and 0xFF bytes all
# through the token partitions: profiles/vp8_gpu_tokens/NOTES.md); B_PRED key frame and intra
# macroblocks in inter frames; the loop filter's SSE path; 1080p with rate control (120-macroblock rows, the first-frame probes).
CASES = {
    "parts1": dict(w=96, h=16, content=_moving, frames=3),
    "parts2": dict(w=96, h=48, content=_moving, frames=3),
    "parts4": dict(w=100, h=60, content=_moving, frames=3),
    "parts8": dict(w=176, h=144, content=_moving, frames=3),
    "updates": dict(w=176, h=144, content=_moving, frames=10, key_at=6),
    "still": dict(w=176, h=144, content=_still, frames=6, qp=44, aq=0),
    "noise": dict(w=320, h=192, content=_noise, frames=2, qp=10),
    "bpred_intra": dict(w=640, h=368, content=_moving, frames=3, qp=24),
    "deblock": dict(w=176, h=144, content=_moving, frames=4, qp=44, deblock=1),
    "1080p": dict(w=1920, h=1080, content=desktop_nv12, frames=3, kbps=8000, sr=16),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_vp8_tokens_bytes_equal_cpu(gpu, name):
    c = dict(CASES[name])
    w, h, content, frames, key_at = c.pop("w"), c.pop("h"), c.pop("content"), c.pop("frames"), c.pop("key_at", -1)
    genc, cenc = _pair(gpu, w, h, **c)
    dec = _run(gpu, genc, cenc, w, h, content, frames, key_at)
    assert dec.stats["key"] + dec.stats["inter"] == frames
    assert genc.gpu_tokens and genc.token_fallbacks == 0
    if name == "still":
        assert genc.stats.skipped_mbs == (w // 16) * (h // 16)
    if name == "bpred_intra":
        assert dec.stats.get("bpred", 0) > 0 and dec.stats.get("intra_p", 0) > 0
    if name == "deblock":
        assert dec.stats.get("filtered", 0) > 0


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_gpu_vp8_tokens_pipelined_matches(gpu, depth):
    """Frames in flight (statistics lag, slot reuse): the depth-1 GPU-mode stream."""
    w, h = 320, 192
    a, _ = _pair(gpu, w, h)
    b, _ = _pair(gpu, w, h, depth=depth)
    srcs = [_dev(a, *synthetic_nv12(w, h, t, seed=1)) for t in range(10)]
    ref = [a.encode(dy.data_ptr(), duv.data_ptr(), False) for dy, duv in srcs]
    out = []
    for t in range(len(srcs)):
        if t >= depth:
            out.append(b.collect())
        b.submit(srcs[t][0].data_ptr(), srcs[t][1].data_ptr(), False)
    while len(out) < len(srcs):
        out.append(b.collect())
    assert out == ref and a.token_fallbacks == 0 and b.token_fallbacks == 0


def test_gpu_vp8_tokens_overflow_falls_back(gpu):
    """A region of 256 bytes per macroblock is too small for the noise (880 per macroblock): every
    frame is coded again on the host without a differing byte -- six frames at 176x144, so that
    frames 4 and 5 fall back with valid statistics (the host writer plans again from the entry
    prepare() planned from)."""
    w, h = 176, 144
    genc, cenc = _pair(gpu, w, h, qp=10, cap=256)
    _run(gpu, genc, cenc, w, h, _noise, 6)
    assert genc.token_fallbacks == 6


def test_gpu_vp8_tokens_cap_must_be_positive(gpu):
    with pytest.raises(ValueError, match="vp8_tokens_cap"):
        _pair(gpu, 96, 48, cap=0)
