"""Shared content of the hevc_intra_split tests (tests/test_hevc_intra4.py, tests/test_gpu_hevc_intra4.py)
and of tools/gen_hevc_intra_split_digests.py."""
from __future__ import annotations

import hashlib

import numpy as np

DIGEST_CASES = [(320, 192, 30), (100, 60, 26), (352, 288, 38)]  # (width, height, QP)


def synthetic_nv12(w, h, t, seed=0):
    """The moving synthetic picture of tests/test_cpu_encoder.py."""
    from tests.test_cpu_encoder import synthetic_nv12 as f

    return f(w, h, t, seed)


def desktop_nv12(w, h, t=0, noise=True):
    from mxdesk.models.synthetic import CpuSyntheticDesktop, bgrx_to_nv12

    return bgrx_to_nv12(CpuSyntheticDesktop(w, h, noise).render(t, t / 60, 0))


def encode_stream(native, w, h, qp, intra_split, frames=3, idr_at=(2,), desktop=False):
    """Access units of the CPU HEVC encoder (constant QP): the moving synthetic picture or the
    synthetic desktop, IDR at frame 0 and at idr_at."""
    cfg = native.EncoderConfig()
    cfg.width, cfg.height, cfg.fps = w, h, 60
    cfg.bitrate_kbps = 0
    cfg.qp = qp
    cfg.hevc_intra_split = intra_split
    enc = native.CpuHevcEncoder(cfg)
    aus = []
    for t in range(frames):
        y, uv = desktop_nv12(w, h, t) if desktop else synthetic_nv12(w, h, t, seed=t)
        aus.append(bytes(enc.encode(np.ascontiguousarray(y), np.ascontiguousarray(uv), t in idr_at)))
    return aus


def split_digests(native):
    """SHA-256 of the CPU encoder's streams with hevc_intra_split 0 and 1 (DIGEST_CASES)."""
    out = {}
    for w, h, qp in DIGEST_CASES:
        for m in (0, 1):
            for desktop in (False, True):
                key = f"{w}x{h}_qp{qp}_split{m}_{'desktop' if desktop else 'moving'}"
                out[key] = hashlib.sha256(b"".join(encode_stream(native, w, h, qp, m, desktop=desktop))).hexdigest()
    return out
