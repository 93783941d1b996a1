"""GPU == CPU for P_8x8 macroblocks (EncoderConfig.partitions 2): the quadrant search of the _q8
instantiations of k_p_fused / k_me_full, the coder's four-window motion compensation, k_cavlc's
sub_mb_pred syntax and the deblocking strengths on the inner edges; and the decoder reproduces the
GPU reconstruction."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from . import quad_content as qc  # noqa: E402
from . import scroll_content as sc  # noqa: E402
from .gpu_util import pitched  # noqa: E402

CASES = [(0, 1), (1, 1), (1, 0), (0, 0)]  # (me_coarse, subpel)


def _run(gpu, frames, w, h, cfg):
    """Both encoders over the frames: every access unit equal, the decoder's pictures equal to the GPU
    reconstruction.  Returns the CPU oracle's mb_info and scroll paths per picture."""
    genc = gpu.GpuH264Encoder(cfg, torch.cuda.current_stream().cuda_stream)
    cenc = gpu.CpuH264Encoder(cfg)
    stream, grec, infos, paths = b"", [], [], []
    for t, (y, uv) in enumerate(frames):
        dy, duv = pitched(y, genc.pitch, genc.coded_height), pitched(uv, genc.pitch, genc.coded_height // 2, uv=True)
        torch.cuda.synchronize()
        gau = genc.encode(dy.data_ptr(), duv.data_ptr(), False)
        cau = cenc.encode(y, uv, False)
        assert bool(gau == cau), f"frame {t}: GPU {len(gau)} B vs CPU {len(cau)} B"
        stream += gau
        grec.append(tuple(a.copy() for a in genc.recon()))
        infos.append(cenc.mb_info().copy())
        paths.append(None if cenc.stats.idr else cenc.mb_scroll_path().copy())
    dec = Decoder()
    dec.decode(stream)
    assert len(dec.frames_coded) == len(grec)
    for t, ((yy, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, grec)):
        hh, ww = yy.shape
        assert np.array_equal(yy, ry[:hh, :ww]), f"picture {t}: decoded luma"
        assert np.array_equal(u, ruv[:hh // 2, 0:ww:2]) and np.array_equal(v, ruv[:hh // 2, 1:ww:2]), f"picture {t}: chroma"
    return infos, paths


def _cfg(gpu, w, h, **kw):
    cfg = gpu.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, 28, 8
    cfg.partitions = 2
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _quad_frames(w, h, half, n=5):
    return [qc.quad_motion(w, h, t, half=half) for t in range(n)]


@pytest.mark.parametrize("coarse,subpel", CASES)
def test_gpu_p8x8_fused_bit_exact(gpu, coarse, subpel):
    # k_p_fused_q8; half-sample motion where the refinement runs (fractional quadrant vectors)
    w, h = 128, 64
    infos, _ = _run(gpu, _quad_frames(w, h, bool(subpel)), w, h, _cfg(gpu, w, h, me_coarse=coarse, subpel=subpel))
    assert qc.count_p8x8(infos) > 8


@pytest.mark.parametrize("coarse,subpel", CASES)
def test_gpu_p8x8_two_kernel_path_with_deblocking(gpu, coarse, subpel):
    # deblock 1: the search reads me_ref (k_me_full_val_q8 / k_me_full_q8), k_inter_encode_q8 codes,
    # and the filtered reconstruction carries the inner edges' strengths
    w, h = 128, 64
    infos, _ = _run(gpu, _quad_frames(w, h, bool(subpel)), w, h,
                    _cfg(gpu, w, h, me_coarse=coarse, subpel=subpel, deblock=1))
    assert qc.count_p8x8(infos) > 8


@pytest.mark.parametrize("deblock", [0, 1])
def test_gpu_p8x8_with_scroll_hint(gpu, deblock):
    # the _scroll_q8 instantiations: scroll_content's document with a band of quad motion
    w, h = qc.SCROLL_SHAPE
    cfg = sc.config(gpu, w, h, dict(scroll=16, qp=12, partitions=2, deblock=deblock))
    infos, paths = _run(gpu, qc.scrolled_with_quad_band(), w, h, cfg)
    assert qc.count_p8x8(infos) > 8
    centred = sum(int(((i[..., 8] == 3) & (i[..., 0] == 0) & (p == 3)).sum()) for i, p in zip(infos[1:], paths[1:]))
    assert centred > 0, "a P_8x8 macroblock searched around the hint"


def test_gpu_p8x8_edge_clamping(gpu):
    # 136x72 (coded 144x80): quadrant vectors point outside the picture, fractional ones included
    w, h = 136, 72
    infos, _ = _run(gpu, _quad_frames(w, h, True), w, h, _cfg(gpu, w, h))
    assert qc.count_p8x8(infos) > 8
    infos, _ = _run(gpu, _quad_frames(w, h, False), w, h, _cfg(gpu, w, h, deblock=1))
    assert qc.count_p8x8(infos) > 8


@pytest.mark.parametrize("deblock", [0, 1])
def test_gpu_partitions_1_has_no_p8x8(gpu, deblock):
    w, h = 128, 64
    infos, _ = _run(gpu, _quad_frames(w, h, True), w, h, _cfg(gpu, w, h, partitions=1, deblock=deblock))
    assert all(not (i[..., 8] == 3).any() for i in infos)
    assert sum(int((i[..., 8] > 0).sum()) for i in infos[1:]) > 0  # the halves are still searched
