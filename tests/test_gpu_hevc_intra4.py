"""GPU tier of EncoderConfig.hevc_intra_split 2 (4x4 luma TUs with DST-VII in the intra transform tree):
the 4x4-versus-8x8 choice of k_hevc_intra_modes and the register-resident 4x4 steps of
split_intra_code give the CPU encoder's stream bit for bit, and the decoder its reconstruction."""
import numpy as np
import pytest

from mxdesk.codec.hevc_decoder import Decoder

from .hevc_intra4_content import desktop_nv12, synthetic_nv12
from .test_hevc import _cfg, _gpu_vs_cpu


def _tu4_units(native, w, h, qp, desktop, frames=3, idr_at=(2,)):
    """Units with a 4x4 luma node per picture, from the CPU encoder (== the GPU's, bit for bit) run as
    _gpu_vs_cpu runs it."""
    cfg = _cfg(native, w, h, qp=qp)
    cfg.hevc_intra_split = 2
    enc = native.CpuHevcEncoder(cfg)
    n = []
    for t in range(frames):
        y, uv = desktop_nv12(w, h, t) if desktop else synthetic_nv12(w, h, t, seed=t)
        enc.encode(y, uv, t in idr_at)
        info = np.asarray(enc.cu_info())
        n.append(int(((info[:, 0] == 3) & (info[:, 5] != 0)).sum()))
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,qp,desktop", [(320, 192, 22, True), (352, 288, 34, True), (100, 60, 30, False)])
def test_gpu_hevc_intra4_bit_exact_vs_cpu(gpu, w, h, qp, desktop):
    """IDR at frames 0 and 2 (the second into reconstruction buffers that hold a P picture): GPU == CPU
    == decoder and equal distortion sums (_gpu_vs_cpu), with intra units that carry 4x4 luma nodes."""
    n = _tu4_units(gpu, w, h, qp, desktop)
    assert n[0] > 0 and n[2] > 0, n
    _gpu_vs_cpu(gpu, w, h, 3, qp=qp, desktop=desktop, intra_split=2, idr_at=(2,))


@pytest.mark.gpu
def test_gpu_session_hevc_intra4_decodes_to_recon(gpu):
    cfg = gpu.SessionConfig()
    cfg.width, cfg.height, cfg.fps = 256, 144, 60
    cfg.codec = "hevc"
    cfg.enc.bitrate_kbps = 0
    cfg.enc.qp = 30
    cfg.enc.hevc_intra_split = 2
    s = gpu.Session(cfg)
    stream, recon = b"", []
    for i in range(3):
        r = s.step(i == 2)
        stream += r.au
        recon.append(tuple(p.copy() for p in s.recon()))
    dec = Decoder()
    dec.decode(stream)
    assert len(dec.frames_coded) == 3
    for (y, u, v), (ry, ruv) in zip(dec.frames_coded, recon):
        assert np.array_equal(y, ry) and np.array_equal(u, ruv[:, 0::2]) and np.array_equal(v, ruv[:, 1::2])
