#!/usr/bin/env python
"""What P_8x8 macroblocks (EncoderConfig.partitions 2: one vector per 8x8 quadrant) cost and buy.

Runs the GPU H.264 encoder with partitions 1 and 2 over the same pictures and prints one JSON line
per (content, mode, partitions): bytes per P picture, Y-PSNR, masked Y-PSNR, QP and GPU time per
picture (device clock, first kernel to k_pack).  Contents: the bench's synthetic desktop and its
motion content at 1920x1080 (through Session, as bench.py drives it), and the scrolled page of
tests/scroll_content.py (through GpuH264Encoder, scroll_range 64).  Modes: constant QP 28, and rate
control at 8 Mbit/s.  --save DIR keeps each run's first --save-frames access units as a file;
--count FILE decodes such a file with the in-tree decoder and prints the share of inter
macroblocks coded P_8x8 (no GPU needed).

    python tools/partition_report.py [--frames 120] [--width 1920 --height 1080] [--save DIR]
    python tools/partition_report.py --count DIR/desktop_cbr_p2.h264
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _summary(rows):
    p = [r for r in rows if not r["idr"]]
    med = lambda k: round(statistics.median(r[k] for r in p), 4)  # noqa: E731
    return dict(p_pictures=len(p), bytes_per_p=round(statistics.mean(r["bytes"] for r in p), 1), psnr_y=med("psnr_y"),
                psnr_y_masked=med("psnr_y_masked"), qp=med("qp"), gpu_ms=med("gpu_ms"),
                gpu_ms_mean=round(statistics.mean(r["gpu_ms"] for r in p), 4))


def run_session(N, content: int, partitions: int, qp: int, bitrate: int, w: int, h: int, frames: int, warmup: int):
    cfg = N.SessionConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.content = content
    cfg.noise = 0 if content else 1
    cfg.fake_clock = 1
    cfg.enc.partitions = partitions
    cfg.enc.bitrate_kbps = 0 if qp else bitrate
    if qp:
        cfg.enc.qp = qp
    if cfg.noise:  # the noise panel left out of the masked figure, as bench.py does
        cfg.mask_x0, cfg.mask_y0 = int(w * 0.04), int(h * 0.55)
        cfg.mask_x1, cfg.mask_y1 = cfg.mask_x0 + int(w * 0.16) + 1, cfg.mask_y0 + int(h * 0.22) + 1
    s = N.Session(cfg)
    rows, aus = [], []
    for f in range(warmup + frames):
        r = s.step(False)
        aus.append(bytes(r.au))
        if f >= warmup:
            rows.append(dict(idr=bool(r.idr), bytes=len(r.au), qp=r.qp, psnr_y=r.psnr_y, psnr_y_masked=r.psnr_y_masked,
                             gpu_ms=r.gpu_ms))
    return rows, aus


def run_scroll(N, torch, partitions: int, qp: int):
    from tests import scroll_content as sc

    w, h = 208, 112
    cfg = sc.config(N, w, h, dict(scroll=64, qp=qp, partitions=partitions))
    enc = N.GpuH264Encoder(cfg, torch.cuda.current_stream().cuda_stream)
    from tests.gpu_util import pitched

    rows, aus = [], []
    for y, uv in sc.frames_for(w, h):
        dy, duv = pitched(y, enc.pitch, enc.coded_height), pitched(uv, enc.pitch, enc.coded_height // 2, uv=True)
        torch.cuda.synchronize()
        au = enc.encode(dy.data_ptr(), duv.data_ptr(), False)
        st = enc.stats
        mse = st.sse[0] / float(w * h)
        psnr = round(99.0 if mse == 0 else 10 * np.log10(255 * 255 / mse), 2)
        rows.append(dict(idr=bool(st.idr), bytes=len(au), qp=st.qp, psnr_y=psnr, psnr_y_masked=psnr, gpu_ms=st.encode_ms))
        aus.append(bytes(au))
    return rows, aus


def count(path: str) -> int:
    from mxdesk.codec.h264_decoder import Decoder

    dec = Decoder()
    dec.decode(Path(path).read_bytes())
    inter = dec.stats["p"] + dec.stats["skip"]
    print(json.dumps(dict(file=path, pictures=len(dec.frames), inter_mbs=inter, coded_inter=dec.stats["p"],
                          p8x8=dec.stats["p8x8"], p8x8_share_of_inter=round(dec.stats["p8x8"] / max(1, inter), 5),
                          p8x8_share_of_coded=round(dec.stats["p8x8"] / max(1, dec.stats["p"]), 5))))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qp", type=int, default=28)
    ap.add_argument("--bitrate", type=int, default=8000)
    ap.add_argument("--only", default="", help="comma list of desktop,motion,scroll (default all)")
    ap.add_argument("--partitions", default="1,2")
    ap.add_argument("--modes", default="cqp,cbr", help="comma list of cqp (constant --qp), cbr (--bitrate)")
    ap.add_argument("--save", default="", metavar="DIR")
    ap.add_argument("--save-frames", type=int, default=4)
    ap.add_argument("--count", default="", metavar="FILE")
    a = ap.parse_args()
    if a.count:
        return count(a.count)
    import torch

    from mxdesk import native

    N = native()
    N.set_device(0)
    only = set(a.only.split(",")) if a.only else {"desktop", "motion", "scroll"}
    for content, cid in (("desktop", 0), ("motion", 1)):
        if content not in only:
            continue
        for mode, qp in (("cqp", a.qp), ("cbr", 0)):
            if mode not in a.modes.split(","):
                continue
            for parts in map(int, a.partitions.split(",")):
                rows, aus = run_session(N, cid, parts, qp, a.bitrate, a.width, a.height, a.frames, a.warmup)
                print(json.dumps(dict(content=content, mode=mode, partitions=parts, width=a.width, height=a.height,
                                      const_qp=qp, bitrate_kbps=0 if qp else a.bitrate, **_summary(rows))), flush=True)
                if a.save:
                    Path(a.save).mkdir(parents=True, exist_ok=True)
                    (Path(a.save) / f"{content}_{mode}_p{parts}.h264").write_bytes(b"".join(aus[:a.save_frames]))
    if "scroll" in only:
        for parts in map(int, a.partitions.split(",")):
            rows, aus = run_scroll(N, torch, parts, 12)
            print(json.dumps(dict(content="scroll", mode="cqp", partitions=parts, width=208, height=112, const_qp=12,
                                  scroll_range=64, **_summary(rows))), flush=True)
            if a.save:
                Path(a.save).mkdir(parents=True, exist_ok=True)
                (Path(a.save) / f"scroll_cqp_p{parts}.h264").write_bytes(b"".join(aus))
    return 0


if __name__ == "__main__":
    sys.exit(main())
