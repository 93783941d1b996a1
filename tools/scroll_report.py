#!/usr/bin/env python
"""What the H.264 scroll hint (EncoderConfig.scroll_range) does to a scrolled 1080p desktop.

Feeds numpy-generated frames to GpuH264Encoder, once with the hint off and once with it on, over
the same frames: a text-like "document" rectangle inside static window chrome, still at first, then
scrolled by a schedule of mouse-wheel moves, then still again, then pictures of fresh noise (every
probe of the probe pass scores all of its candidates: the pass's worst case).  Prints one JSON line
per mode with the per-picture figures -- bytes, QP, Y-PSNR, gpu_ms (device clock, first kernel to
k_pack, the probe pass included) and the hint -- and the medians per phase.

    python tools/scroll_report.py [--scroll-range 128] [--qp 0] [--bitrate 8000] [--deblock -1]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H = 1920, 1080
DOC = (240, 96, 1680, 1000)  # x0, y0, x1, y1 of the document rectangle (macroblock aligned)
STILL = 8
WHEEL = [40, 80, 120, 120, 120, 80, 40, 0, 0, -120, -120, -80, 0, 0, 64, 64, 64, 64]  # rows per picture
NOISE = 6


def _document(rows: int, cols: int, rng) -> np.ndarray:
    """A page of glyph-like marks: text lines of 2x2-sample strokes on white, in words and paragraphs."""
    page = np.full((rows, cols), 235, np.uint8)
    bits = rng.random((rows // 2, cols // 2)) < 0.42
    yy, xx = np.mgrid[0:rows // 2, 0:cols // 2]
    line = (yy % 11) < 7                       # 14-sample glyph rows every 22
    word = (rng.random((rows // 22 + 1, cols // 60 + 1)) < 0.85)[yy // 11, xx // 30] & ((xx % 30) < 26)
    para = (rng.random(rows // 220 + 1) < 0.8)[yy // 110]
    margin = (xx > 24) & (xx < cols // 2 - 24)
    ink = np.repeat(np.repeat(bits & line & word & para & margin, 2, 0), 2, 1)
    page[:ink.shape[0], :ink.shape[1]][ink] = 40
    return page


def make_frames(seed: int = 3):
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = DOC
    chrome = np.full((H, W), 200, np.uint8)
    chrome[:64] = 90                           # title bar
    chrome[64:96, :] = 170                     # tool bar
    chrome[96:, :224] = 215                    # side panel
    chrome[120:1000:40, 16:200] = 120          # its entries
    chrome[1016:] = 60                         # status bar
    span = sum(abs(d) for d in WHEEL) + 64
    doc = _document((y1 - y0) + 2 * span, x1 - x0, rng)
    moves = [0] * (STILL + 1) + WHEEL
    frames, phases, oy = [], [], span
    for t, d in enumerate(moves):
        oy += d
        y = chrome.copy()
        y[y0:y1, x0:x1] = doc[oy:oy + (y1 - y0)]
        frames.append(y)
        phases.append("idr" if t == 0 else ("still" if d == 0 else "scroll"))
    for _ in range(NOISE):
        frames.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
        phases.append("noise")
    return frames, phases, moves + [0] * NOISE


def run(N, torch, frames, scroll_range: int, qp: int, bitrate: int, deblock: int):
    cfg = N.EncoderConfig()
    cfg.width, cfg.height = W, H
    cfg.bitrate_kbps = 0 if qp else bitrate
    if qp:
        cfg.qp = qp
    cfg.scroll_range = scroll_range
    cfg.deblock = deblock
    enc = N.GpuH264Encoder(cfg, torch.cuda.current_stream().cuda_stream)
    ch, pitch = enc.coded_height, enc.pitch
    out = []
    uv_dev = torch.full((ch // 2, pitch), 128, dtype=torch.uint8, device="cuda")
    for y in frames:
        pad = np.zeros((ch, pitch), np.uint8)
        pad[:H, :W] = y
        pad[H:, :W] = y[-1]
        pad[:, W:] = pad[:, W - 1:W]
        y_dev = torch.from_numpy(pad).to("cuda")
        torch.cuda.synchronize()
        au = enc.encode(y_dev.data_ptr(), uv_dev.data_ptr(), False)
        st = enc.stats
        mse = st.sse[0] / float(W * H)
        out.append(dict(bytes=len(au), qp=st.qp, psnr_y=round(99.0 if mse == 0 else 10 * np.log10(255 * 255 / mse), 2),
                        gpu_ms=round(st.encode_ms, 4), hint=[st.scroll_dx, st.scroll_dy], skipped=st.skipped_mbs,
                        deblocked=st.deblocked))
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scroll-range", type=int, default=128)
    ap.add_argument("--qp", type=int, default=0, help="constant QP (0: rate control at --bitrate)")
    ap.add_argument("--bitrate", type=int, default=8000)
    ap.add_argument("--deblock", type=int, default=-1,
                    help="in-loop filter (EncoderConfig.deblock; the adaptive default filters pictures that move "
                         "coherently, which a hinted scroll does: 0 compares the two modes without it)")
    a = ap.parse_args()
    import torch

    from mxdesk import native

    N = native()
    N.set_device(0)
    frames, phases, moves = make_frames()
    for name, rng_ in (("hint_off", 0), ("hint_on", a.scroll_range)):
        run(N, torch, frames[:4], rng_, a.qp, a.bitrate, a.deblock)  # warm-up: kernels loaded, clocks up
        pics = run(N, torch, frames, rng_, a.qp, a.bitrate, a.deblock)
        med = {}
        for ph in ("still", "scroll", "noise"):
            sel = [p for p, q in zip(pics, phases) if q == ph]
            med[ph] = {k: round(statistics.median(p[k] for p in sel), 4) for k in ("bytes", "qp", "psnr_y", "gpu_ms", "deblocked")}
        for p, q, m in zip(pics, phases, moves):
            p["phase"], p["move"] = q, m
        print(json.dumps(dict(mode=name, scroll_range=rng_, qp=a.qp, bitrate_kbps=0 if a.qp else a.bitrate, deblock=a.deblock,
                              medians=med, pictures=pics)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
