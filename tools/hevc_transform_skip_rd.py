"""HEVC sessions with EncoderConfig.hevc_transform_skip off and on: frame rate, bytes and noise-masked luma
PSNR per content (bench.py's session path and defaults: depth 3, eager launches; bench.py itself has
no switch for the option).  Each configuration is run `--runs` times in turn, so the spread of a
configuration's own repeats stands next to the difference between two of them.

    python tools/hevc_transform_skip_rd.py [--width 3840 --height 2160 --bitrate-kbps 18000]
        [--contents desktop,motion,subpel] [--options 0,1] [--steps 300 --warmup 60 --runs 2]
One JSON line per run.  A build without the option (an older commit) is measured with --options -1.

    python tools/hevc_transform_skip_rd.py --dump DIR [--dump-frames 6] ...   (GPU)
    python tools/hevc_transform_skip_rd.py --share DIR                        (no GPU)
--dump writes the first pictures of an option-1 session per content to DIR/<content>.hevc; --share
decodes them with the Python decoder and prints the share of coded 4x4 luma TUs sent with
transform_skip_flag 1.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def session(N, a, content, option):
    cfg = N.SessionConfig()
    cfg.width, cfg.height, cfg.fps = a.width, a.height, 60
    cfg.codec = "hevc"
    cfg.enc.bitrate_kbps = a.bitrate_kbps
    cfg.enc.pipeline_depth = 3
    if option >= 0:
        cfg.enc.hevc_transform_skip = option
    cfg.content = {"desktop": 0, "motion": 1, "subpel": 2}[content]
    cfg.noise = 0 if cfg.content else 1  # the motion contents have a video panel instead of the noise panel
    if cfg.noise:  # bench.py's mask: the renderer's noise panel
        cfg.mask_x0, cfg.mask_y0 = int(a.width * 0.04), int(a.height * 0.55)
        cfg.mask_x1, cfg.mask_y1 = cfg.mask_x0 + int(a.width * 0.16) + 1, cfg.mask_y0 + int(a.height * 0.22) + 1
    return N.Session(cfg), cfg


def run(N, a, content, option):
    import torch

    s, cfg = session(N, a, content, option)
    N.run_sessions([s], a.warmup, 3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = N.run_sessions([s], a.steps, 3)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"content": content, "hevc_transform_skip": option, "fps": round(a.steps / dt, 1),
            "mean_gpu_ms": round(statistics.mean(r.gpu_ms for r in res), 4),
            "kbps_at_60": round(statistics.mean(len(r.au) for r in res) * 8 * 60 / 1000, 1),
            "psnr_y_masked": round(statistics.mean(r.psnr_y_masked if cfg.noise else r.psnr_y for r in res), 3),
            "mean_qp": round(statistics.mean(r.qp for r in res), 2)}


def share(directory):
    from mxdesk.codec.hevc_decoder import Decoder

    for f in sorted(Path(directory).glob("*.hevc")):
        dec = Decoder()
        dec.decode(f.read_bytes())
        ts, coded = dec.stats.get("transform_skip", 0), dec.stats.get("luma4_coded", 0)
        print(json.dumps({"content": f.stem, "pictures": len(dec.frames_coded), "luma4_coded": coded,
                          "transform_skip": ts, "share": round(ts / max(coded, 1), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bitrate-kbps", type=int, default=18000)
    ap.add_argument("--contents", default="desktop,motion,subpel")
    ap.add_argument("--options", default="0,1")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--dump", default="")
    ap.add_argument("--dump-frames", type=int, default=6)
    ap.add_argument("--share", default="")
    a = ap.parse_args()
    if a.share:
        return share(a.share)
    import mxdesk

    N = mxdesk.native()
    N.set_device(0)
    for content in a.contents.split(","):
        if a.dump:
            s, _ = session(N, a, content, 1)
            Path(a.dump).mkdir(parents=True, exist_ok=True)
            (Path(a.dump) / f"{content}.hevc").write_bytes(b"".join(bytes(r.au) for r in N.run_sessions([s], a.dump_frames, 3)[0]))
            continue
        for k in range(a.runs):
            for option in (int(v) for v in a.options.split(",")):
                print(json.dumps(dict(run(N, a, content, option), run=k)), flush=True)


if __name__ == "__main__":
    main()
