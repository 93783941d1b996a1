"""The HIP H.264 encoder at production sizes (VERDICT r1 "Next round" #4): GPU == CPU oracle
bit-exact on the synthetic desktop at 1920x1080 (5-slice wavefront IDR with Intra4x4, P
frames with intra macroblocks and adaptive quantisation, in-loop deblocking), 3840x2160 (the multi-row k_scan_rows / k_scan_out path,
> 8192 macroblocks) and 7680x4320, plus an independent decode of the deblocked 1080p pictures.

Reference operating point: nvh264enc on the 1080p desktop (reference Dockerfile:210)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mxdesk.codec.h264_decoder import Decoder  # noqa: E402

from .gpu_util import pitched  # noqa: E402


def _stream():
    return torch.cuda.current_stream().cuda_stream


def raw_nals(au: bytes) -> list[bytes]:
    """Annex-B access unit -> NAL units as transmitted (emulation prevention kept)."""
    out, i = [], au.find(b"\x00\x00\x01")
    while i >= 0:
        j = au.find(b"\x00\x00\x01", i + 3)
        n = au[i + 3: j if j >= 0 else len(au)]
        out.append(n.rstrip(b"\x00") if j >= 0 else n)
        i = j
    return out


def desktop_nv12(gpu, w, h, frame):
    """The HIP synthetic desktop (text, gears, scrolling terminal, moving window, noise panel)
    converted to NV12 on the GPU; host copies of the display-sized planes."""
    pitch = w * 4
    bgrx = torch.zeros((h, pitch), dtype=torch.uint8, device="cuda")
    gpu.synth(bgrx.data_ptr(), w, h, pitch, frame_id=frame, timestamp_us=frame * 16667, t=frame / 60.0,
              stream=_stream())
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    y = torch.zeros((ch, cw), dtype=torch.uint8, device="cuda")
    uv = torch.zeros((ch // 2, cw), dtype=torch.uint8, device="cuda")
    gpu.bgrx_to_nv12(bgrx.data_ptr(), pitch, w, h, y.data_ptr(), uv.data_ptr(), cw, cw, ch, _stream())
    torch.cuda.synchronize()
    return y.cpu().numpy()[:h, :w].copy(), uv.cpu().numpy()[: h // 2, :w].copy()


def _encode_both(gpu, w, h, frames, kbps, search_range=16, deblock=1):
    cfg = gpu.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps = kbps
    cfg.search_range = search_range
    cfg.deblock = deblock
    cfg.intra_in_p = 1  # exercise the intra-in-P path (off by default for throughput)
    genc = gpu.GpuH264Encoder(cfg, _stream())
    cenc = gpu.CpuH264Encoder(cfg)
    aus, recons = [], []
    ch = genc.coded_height
    for t in range(frames):
        y, uv = desktop_nv12(gpu, w, h, t)
        dy = pitched(y, genc.pitch, ch)
        duv = pitched(uv, genc.pitch, ch // 2, uv=True)
        torch.cuda.synchronize()
        gau = genc.encode(dy.data_ptr(), duv.data_ptr(), False)
        cau = cenc.encode(y, uv, False)
        assert bool(gau == cau), f"{w}x{h} frame {t}: GPU {len(gau)} B vs CPU {len(cau)} B"
        aus.append(gau)
        recons.append(genc.recon())
    return aus, recons, genc


def test_1080p_bit_exact_and_decodes(gpu):
    # in-loop deblocking on (the default): GPU == CPU bit-exact, reference pictures included, and
    # the independent decoder reproduces every deblocked 1080p picture (IDR of 17 wavefront slices
    # with Intra4x4 and Intra16x16, then P pictures with intra macroblocks and AQ classes)
    aus, recons, genc = _encode_both(gpu, 1920, 1080, 3, 8000)
    nals = raw_nals(aus[0])
    assert sum((n[0] & 0x1F) == 5 for n in nals) == 17
    dec = Decoder()
    dec.decode(b"".join(aus))
    assert len(dec.frames_coded) == 3
    for t, ((y, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, recons)):
        assert np.array_equal(y, ry[:1088, :1920]), f"frame {t} luma"
        assert np.array_equal(u, ruv[:544, 0:1920:2]) and np.array_equal(v, ruv[:544, 1:1920:2]), f"frame {t} chroma"
    assert dec.stats["i4"] > 0 and dec.stats["i16"] > 0, dec.stats  # both intra MB types on the desktop


def test_4k_bit_exact_multi_tile_scan(gpu):
    # 240 x 135 = 32400 MBs: 135 k_scan_rows / k_scan_out workgroups; IDR of 34 slices (4 MB rows)
    aus, _, _ = _encode_both(gpu, 3840, 2160, 2, 25000, search_range=8)
    assert sum((n[0] & 0x1F) == 5 for n in raw_nals(aus[0])) == 34


def test_8k_bit_exact(gpu):
    aus, recons, genc = _encode_both(gpu, 7680, 4320, 2, 60000, search_range=4)
    assert len(aus[1]) > 0 and genc.coded_height == 4320


def _hevc_encode_both(gpu, w, h, frames, kbps):
    """The HEVC encoder at its defaults (CTB 32 quadtree, 4x4 luma TUs, SAO, adaptive deblocking,
    aq 6, half-row I slices, cost-balanced P slices) on the HIP desktop: GPU == CPU oracle."""
    cfg = gpu.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps = kbps
    genc = gpu.GpuHevcEncoder(cfg, _stream())
    cenc = gpu.CpuHevcEncoder(cfg)
    ch = genc.coded_height
    aus = []
    for t in range(frames):
        y, uv = desktop_nv12(gpu, w, h, t)
        dy = pitched(y, genc.pitch, ch)
        duv = pitched(uv, genc.pitch, ch // 2, uv=True)
        torch.cuda.synchronize()
        gau = genc.encode(dy.data_ptr(), duv.data_ptr(), False)
        cau = cenc.encode(y, uv, False)
        assert bool(gau == cau), f"HEVC {w}x{h} frame {t}: GPU {len(gau)} B vs CPU {len(cau)} B"
        assert tuple(genc.stats.sse) == tuple(cenc.stats.sse), t
        aus.append(gau)
    return aus, genc


def test_hevc_4k_bit_exact(gpu):
    # BASELINE config 3 (4K60 HEVC): IDR with two I slices per CTB row, then P pictures
    aus, genc = _hevc_encode_both(gpu, 3840, 2160, 3, 18000)
    assert len(aus[0]) > len(aus[1]) > 0


def test_hevc_8k_bit_exact(gpu):
    # the wall's encode rank (BASELINE config 5: 2x2 tiled 8K60, HEVC level 6.1)
    aus, genc = _hevc_encode_both(gpu, 7680, 4320, 2, 60000)
    assert genc.coded_height == 4320 and len(aus[1]) > 0
