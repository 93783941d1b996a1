"""Serial chain of one picture in a rocprofv3 kernel trace of an eager H.264 bench run.

    python tools/frame_chain.py <run_kernel_trace.csv> [--depth 3] [--pictures 200]

The n-th dispatch of every kernel of the chain belongs to the n-th picture (every stream is in
order and every P picture runs each kernel once), so the pictures are matched by counting each
kernel's dispatches back from the end of the trace (run bench.py with --quality-probe 0
--density-probe 0, so that the trace ends with the timed window).  Printed, as medians over the
last `--pictures` steady-state pictures: start and end of every kernel relative to the start of
the picture's render, the gaps between consecutive kernels of the picture, the time from the end
of k_pack to the render of the picture that reuses the frame slot (`depth` pictures later: host
turnaround plus launch latency), and the loop length over `depth` against the measured period.
"""
import argparse
import csv
import re
import statistics
from collections import defaultdict

RENDER = ("k_synth",)
CHAIN = ("k_bgrx_to_nv12", "k_p_fused", "k_cavlc", "k_scan_rows", "k_scan_out", "k_pack")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--pictures", type=int, default=200)
    a = ap.parse_args()
    by = defaultdict(list)
    for r in csv.DictReader(open(a.trace)):
        m = re.search(r"(k_[a-z0-9_]+)", r["Kernel_Name"])
        if not m:
            continue
        name = m.group(1)
        name = re.sub(r"_(scroll|q8|scroll_q8)$", "", name)
        by[name].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    for v in by.values():
        v.sort()
    render = next((n for n in RENDER if n in by), None)
    if render is None:
        raise SystemExit("no render kernel in the trace")
    names = [render] + [n for n in CHAIN if n in by]
    n_pic = min(a.pictures + a.depth, min(len(by[n]) for n in names) - 1)
    # picture j (0 = oldest kept): dispatch [-n_pic + j] of every kernel
    pics = [{n: by[n][len(by[n]) - n_pic + j] for n in names} for j in range(n_pic)]
    for p in pics:  # a mismatch (an IDR inside the window) shows as a kernel before its predecessor
        for x, y in zip(names, names[1:]):
            if p[y][0] < p[x][1] - 2000:  # back-to-back dispatches may overlap by a timestamp tick
                raise SystemExit(f"pictures do not line up ({y} starts before {x} ends): IDR in the window?")
    med = lambda v: statistics.median(v) / 1e3
    print(f"{n_pic} pictures, depth {a.depth}; medians in us, relative to the start of {render}")
    print(f"{'kernel':<16} {'start':>8} {'end':>8} {'length':>8} {'gap before':>11}")
    prev = None
    for n in names:
        s = med([p[n][0] - p[render][0] for p in pics])
        e = med([p[n][1] - p[render][0] for p in pics])
        d = med([p[n][1] - p[n][0] for p in pics])
        g = med([p[n][0] - p[prev][1] for p in pics]) if prev else 0.0
        print(f"{n:<16} {s:8.1f} {e:8.1f} {d:8.1f} {g:11.1f}")
        prev = n
    last = names[-1]
    turn = [pics[j + a.depth][render][0] - pics[j][last][1] for j in range(n_pic - a.depth)]
    loop = [pics[j + a.depth][render][0] - pics[j][render][0] for j in range(n_pic - a.depth)]
    period = [pics[j + 1][render][0] - pics[j][render][0] for j in range(n_pic - 1)]
    print(f"end of {last} -> render of the slot's next picture: median {med(turn):.1f}, "
          f"p10 {sorted(turn)[len(turn) // 10] / 1e3:.1f}, p90 {sorted(turn)[len(turn) * 9 // 10] / 1e3:.1f}")
    print(f"loop (render to render of the same slot): median {med(loop):.1f}; / {a.depth} = {med(loop) / a.depth:.1f}")
    print(f"period (render to next render): median {med(period):.1f}, mean {sum(period) / len(period) / 1e3:.1f}")
    kernels = sum(med([p[n][1] - p[n][0] for p in pics]) for n in names)
    print(f"sum of kernel lengths {kernels:.1f}; chain render start -> {last} end {med([p[last][1] - p[render][0] for p in pics]):.1f}")
    if "k_p_fused" in by:
        f = by["k_p_fused"][-n_pic:]
        print(f"k_p_fused: gap to the previous k_p_fused median {med([f[j + 1][0] - f[j][1] for j in range(len(f) - 1)]):.1f}; "
              f"start to start median {med([f[j + 1][0] - f[j][0] for j in range(len(f) - 1)]):.1f}")
        if len(names) > 2:
            conv = names[names.index('k_p_fused') - 1]
            w = [pics[j][ 'k_p_fused'][0] - max(pics[j][conv][1], pics[j - 1]['k_p_fused'][1]) for j in range(1, n_pic)]
            print(f"k_p_fused: start after the later of {conv}'s end and the previous k_p_fused's end: median {med(w):.1f}")


if __name__ == "__main__":
    main()
