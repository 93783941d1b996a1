"""Scroll hint on the GPU encoder (k_scroll_probe, and the search centred on its hint in
k_p_fused_scroll / k_me_full_scroll / k_me_full_val_scroll) against the CPU oracle: access units,
reconstructions and the reported hint equal CpuH264Encoder's for every picture, and the independent
decoder reproduces the pictures.  Content, schedules and the choice of QP 12: tests/scroll_content.py
and tests/test_scroll_hint.py, which checks on the oracle that the schedules exercise the hint's
early exit, searches centred on the hint and on zero, and partitioned macroblocks around the hint.

Cases: every combination of partitions, sub-sample refinement and the coarse grid on 208x112 (both
axes); on 96x160 the in-loop filter (the search reads the unfiltered copy of the reference: two
kernels, and with two pictures in flight the side stream), aq 3 and intra macroblocks in P pictures;
on 160x96 (centres off the dword grid) range 16 and QP 10 and 51; a picture without border whose
top macroblocks point 40 and 56 rows outside; scroll_range 192 with range 32 on 64x512 (the probe's
LDS strips at their full size); three pictures in flight through submit / collect.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from . import scroll_content as sc  # noqa: E402
from .gpu_util import pitched  # noqa: E402

ON = {(96, 160): 64, (160, 96): 64, (208, 112): 96}

CASES = [(208, 112, dict(partitions=p, subpel=s, me_coarse=c)) for p in (0, 1) for s in (0, 1) for c in (0, 1)]
CASES += [(96, 160, dict(deblock=1)), (96, 160, dict(aq=3)), (96, 160, dict(intra_in_p=1)),
          (160, 96, dict(range=16)), (160, 96, dict(qp=10)), (160, 96, dict(qp=51))]


def _id(c):
    return f"{c[0]}x{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2].items())


def _against_oracle(gpu, w, h, o, frames, key, in_flight=1):
    run = sc.cpu_run(gpu, w, h, o, frames, key=key)
    genc = gpu.GpuH264Encoder(sc.config(gpu, w, h, o), torch.cuda.current_stream().cuda_stream)
    ch = genc.coded_height
    dev = [(pitched(y, genc.pitch, ch), pitched(uv, genc.pitch, ch // 2, uv=True)) for y, uv in frames]
    torch.cuda.synchronize()
    aus, recs, hints = [], [], []

    def collect():
        t = len(aus)
        gau = genc.collect()
        assert bool(gau == run.aus[t]), f"picture {t}: GPU {len(gau)} B vs CPU {len(run.aus[t])} B"
        st = genc.stats
        assert (st.scroll_dx, st.scroll_dy) == run.hints[t], f"picture {t}: hint"
        aus.append(gau)
        hints.append(run.hints[t])

    for t, (dy, duv) in enumerate(dev):
        if in_flight == 1:
            genc.submit(dy.data_ptr(), duv.data_ptr(), False)
            collect()
            gy, guv = genc.recon()
            assert np.array_equal(gy, run.recs[t][0]) and np.array_equal(guv, run.recs[t][1]), f"picture {t}: reconstruction"
            recs.append((gy.copy(), guv.copy()))
        else:
            if t >= in_flight:
                collect()
            genc.submit(dy.data_ptr(), duv.data_ptr(), False)
    while len(aus) < len(frames):
        collect()
    if in_flight > 1:  # the last reconstruction; the decoder checks the others through the access units
        gy, guv = genc.recon()
        assert np.array_equal(gy, run.recs[-1][0]) and np.array_equal(guv, run.recs[-1][1])
        recs = run.recs
    sc.check_decoder(aus, recs)
    return hints


@pytest.mark.parametrize("w,h,o", CASES, ids=[_id(c) for c in CASES])
def test_gpu_scroll_vs_cpu_and_decoder(gpu, w, h, o):
    o = {"scroll": ON[(w, h)], "qp": 12, **o}
    hints = _against_oracle(gpu, w, h, o, sc.frames_for(w, h), None)
    print(_id((w, h, o)), hints)
    if o["qp"] == 12 and not o.get("deblock"):
        assert sum(g != (0, 0) for g in hints) >= 4  # the hint is at work in this case


def test_gpu_vectors_far_outside_the_picture(gpu):
    w, h = sc.EDGE_SHAPE
    hints = _against_oracle(gpu, w, h, dict(scroll=64, qp=12), sc.edge_frames(), "edge")
    assert hints[sc.STILL + 1:sc.STILL + 3] == sc.EDGE_MOVES[:2]


def test_gpu_full_reach(gpu):
    w, h = 64, 512
    frames = sc.make_frames(w, h, [(0, 192), (0, -192)], ((1, 5), (1, 9), (1, 21)), oy0=400)
    hints = _against_oracle(gpu, w, h, dict(scroll=192, qp=12, range=32), frames, "tall")
    assert hints[-2:] == [(0, 192), (0, -192)]


@pytest.mark.parametrize("o", [dict(depth=3), dict(depth=2, deblock=1)], ids=["depth3", "depth2-deblock"])
def test_gpu_pictures_in_flight(gpu, o):
    w, h = 208, 112
    o = {"scroll": ON[(w, h)], "qp": 12, **o}
    hints = _against_oracle(gpu, w, h, o, sc.frames_for(w, h), None, in_flight=o["depth"])
    if not o.get("deblock"):
        assert sum(g != (0, 0) for g in hints) >= 4
