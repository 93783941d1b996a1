"""Ownership of the HIP resources (csrc/common/gpu_arena.h): every native object gives back what it
acquired -- when it is destroyed, and when its constructor throws half-way -- and an encoder built
afterwards is still the same encoder.  gpu_live_handles() counts the handles (memory, events,
streams, page-locked ranges) that all arenas of the process hold.

All sessions are 208x112 (13 x 7 macroblocks) at constant QP.
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

W, H = 208, 112


def _session_config(gpu, codec, depth=1, **enc):
    cfg = gpu.SessionConfig()
    cfg.width, cfg.height, cfg.fps = W, H, 60
    cfg.codec = codec
    cfg.enc.width, cfg.enc.height, cfg.enc.fps = W, H, 60  # what the session sets: cfg.enc also serves the CPU encoder
    cfg.enc.bitrate_kbps = 0
    cfg.enc.pipeline_depth = depth
    for k, v in enc.items():
        setattr(cfg.enc, k, v)
    cfg.fake_clock = 1
    return cfg


def _run(s, depth, n):
    out, sent = [], 0
    while sent < min(depth, n):
        s.submit(False)
        sent += 1
    for _ in range(n):
        out.append(s.collect())
        if sent < n:
            s.submit(False)
            sent += 1
    assert s.in_flight == 0
    return out


# H.264 at depth 3 creates the second entropy stream; with the filter on for every picture the side
# search stream replaces it (the arena's early release)
TEARDOWN = [(c, d, {}) for c in ("h264", "hevc", "vp8") for d in (1, 3)] + [("h264", 3, dict(deblock=1))]


@pytest.mark.parametrize("codec,depth,enc", TEARDOWN, ids=[f"{c}-d{d}" + "".join(f"-{k}{v}" for k, v in e.items())
                                                           for c, d, e in TEARDOWN])
def test_teardown_is_balanced(gpu, codec, depth, enc):
    n0 = gpu.gpu_live_handles()
    s = gpu.Session(_session_config(gpu, codec, depth, **enc))
    assert gpu.gpu_live_handles() > n0
    out = _run(s, depth, 4)
    assert all(len(r.au) > 0 for r in out)
    del s
    gc.collect()
    assert gpu.gpu_live_handles() == n0


def _pool_not_above_depth(gpu):
    cfg = _session_config(gpu, "h264", 2)
    cfg.pool_slots = 2
    gpu.Session(cfg)  # thrown after the encoder and the NV12 planes exist


def _unknown_codec(gpu):
    gpu.Session(_session_config(gpu, "nope"))  # thrown after the stream and the frame pool exist


def _vp8_region_too_large(gpu):
    # 4 macroblock rows in 4 partitions of 4 macroblocks each: a region of 2^30 * 4 = 2^32 bytes,
    # refused inside alloc_slot, eight allocations into the slot
    cfg = gpu.EncoderConfig()
    cfg.width, cfg.height = 64, 64
    cfg.bitrate_kbps = 0
    cfg.vp8_tokens, cfg.vp8_tokens_cap = 1, 1 << 30
    gpu.GpuVp8Encoder(cfg, torch.cuda.current_stream().cuda_stream)


FAILURES = [(_pool_not_above_depth, "pool_slots must exceed pipeline_depth"), (_unknown_codec, "unknown codec"),
            (_vp8_region_too_large, "vp8_tokens_cap too large")]


@pytest.mark.parametrize("build,message", FAILURES, ids=[f.__name__.strip("_") for f, _ in FAILURES])
def test_throwing_constructor_releases_everything(gpu, build, message):
    n0 = gpu.gpu_live_handles()
    with pytest.raises(ValueError, match=message):
        build(gpu)
    gc.collect()
    assert gpu.gpu_live_handles() == n0


@pytest.mark.parametrize("codec", ["h264", "hevc", "vp8"])
def test_same_encoder_after_failed_constructors(gpu, codec):
    for build, message in FAILURES:
        with pytest.raises(ValueError, match=message):
            build(gpu)
    cfg = _session_config(gpu, codec)
    cenc = {"h264": gpu.CpuH264Encoder, "hevc": gpu.CpuHevcEncoder, "vp8": gpu.CpuVp8Encoder}[codec](cfg.enc)
    s = gpu.Session(cfg)
    for t in range(3):
        gau = s.step(False).au
        y, uv = s.nv12()
        cau = cenc.encode(np.ascontiguousarray(y[:H, :W]), np.ascontiguousarray(uv[:H // 2, :W]), False)
        assert bool(gau == cau), f"{codec} frame {t}: GPU {len(gau)} B vs CPU {len(cau)} B"
