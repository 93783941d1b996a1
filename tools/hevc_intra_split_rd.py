"""HEVC IDR picture: bytes and luma PSNR per intra transform-tree depth (EncoderConfig.hevc_intra_split:
0 unsplit, 1 four 8x8 luma TUs, 2 those nodes on to 4x4 luma TUs with DST-VII), CPU encoder (the GPU's
bit-exact oracle, so no GPU is needed), fixed QPs, on the numpy synthetic desktop (CpuSyntheticDesktop)
or a frame of the GPU-rendered bench desktop (tools/dump_frames.py --npz); then the BD-rate of every
depth against the shallower ones.

    python tools/hevc_intra_split_rd.py [--width 1920 --height 1080 --qps 27,32,37,41] [--splits 0,1,2]
                                        [--noise 1] [--npz frames.npz] [--json out.json] [--csv out.csv]
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def rd_rows(N, y, uv, width, height, qps, splits, mask=None):
    """One row per (QP, depth): the IDR's bytes, luma PSNR and tree statistics."""
    if mask is None:
        mask = np.ones((height, width), bool)
    rows = []
    for qp in qps:
        for split in splits:
            cfg = N.EncoderConfig()
            cfg.width, cfg.height, cfg.fps = width, height, 60
            cfg.bitrate_kbps, cfg.qp = 0, qp
            cfg.hevc_intra_split = split
            enc = N.CpuHevcEncoder(cfg)
            au = enc.encode(y, uv, True)
            ry = enc.recon()[0][:height, :width].astype(np.float64)
            e2 = (ry - y[:height, :width]) ** 2
            mse, msem = float(np.mean(e2)), float(np.mean(e2[mask]))
            cu = np.asarray(enc.cu_info())
            rows.append({"qp": qp, "split": split, "bytes": len(au), "psnr_y": round(10 * np.log10(65025 / mse), 3),
                         "psnr_y_masked": round(10 * np.log10(65025 / msem), 3),
                         "split_units": int((cu[:, 3] == 2).sum()),
                         "tu4_nodes": int(sum(bin(int(v)).count("1") for v in cu[:, 5]))})
    return rows


def bd_table(rows, key="psnr_y"):
    """BD-rate (per cent) of every depth against every shallower one: {"2v1": .., ..}."""
    from mxdesk.utils.bdrate import bd_rate

    splits = sorted({r["split"] for r in rows})
    curve = {s: [(r["bytes"], r[key]) for r in rows if r["split"] == s] for s in splits}
    return {f"{t}v{r}": round(bd_rate(curve[r], curve[t]), 2) for t in splits for r in splits if r < t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--qps", default="27,32,37,41")
    ap.add_argument("--npz", default="")
    ap.add_argument("--splits", default="0,1,2")
    ap.add_argument("--noise", type=int, default=1, help="the synthetic desktop's noise panel (0: off)")
    ap.add_argument("--json", default="", help="write the rows and the BD-rates here")
    ap.add_argument("--csv", default="", help="write the rows here")
    a = ap.parse_args()
    import mxdesk
    from mxdesk.models.synthetic import CpuSyntheticDesktop, bgrx_to_nv12

    N = mxdesk.native()
    mask = None  # the incompressible noise panel left out (--npz)
    if a.npz:
        z = np.load(a.npz)
        a.width, a.height = int(z["width"]), int(z["height"])
        y, uv = np.ascontiguousarray(z["y"][0]), np.ascontiguousarray(z["uv"][0])
        if "mask" in z:
            mask = np.ones((a.height, a.width), bool)
            x0, y0, x1, y1 = (int(v) for v in z["mask"])
            mask[y0:y1, x0:x1] = False
    else:
        desk = CpuSyntheticDesktop(a.width, a.height, noise=bool(a.noise))
        y, uv = bgrx_to_nv12(desk.render(0, 0.0, 0))
    rows = rd_rows(N, y, uv, a.width, a.height, [int(q) for q in a.qps.split(",")],
                   [int(v) for v in a.splits.split(",")], mask)
    for row in rows:
        print(json.dumps(row), flush=True)
    bd = bd_table(rows) if len({r["split"] for r in rows}) > 1 and len({r["qp"] for r in rows}) > 1 else {}
    print(json.dumps({"bd_rate_pct": bd}))
    if a.json:
        Path(a.json).write_text(json.dumps({"width": a.width, "height": a.height, "noise": a.noise, "rows": rows,
                                            "bd_rate_pct": bd}, indent=1) + "\n")
    if a.csv:
        keys = list(rows[0])
        Path(a.csv).write_text("\n".join([",".join(keys)] + [",".join(str(r[k]) for k in keys) for r in rows]) + "\n")


if __name__ == "__main__":
    main()
