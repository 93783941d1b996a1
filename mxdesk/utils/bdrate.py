"""Bjontegaard delta rate between two rate-distortion curves (VCEG-M33)."""
from __future__ import annotations

import numpy as np


def bd_rate(ref, test) -> float:
    """Average bitrate difference of `test` against `ref` at equal PSNR, in per cent (negative: test
    needs fewer bits).  Each curve is a sequence of (bytes or bitrate, PSNR in dB) points, at least
    two; log-rate is fitted as a polynomial in PSNR (cubic from four points on, else of degree
    points - 1) and the two fits are integrated over the PSNR interval both curves cover."""
    def fit(points):
        r = np.log10(np.array([p[0] for p in points], np.float64))
        d = np.array([p[1] for p in points], np.float64)
        return np.polyfit(d, r, min(3, len(points) - 1)), d.min(), d.max()

    pr, lo_r, hi_r = fit(ref)
    pt, lo_t, hi_t = fit(test)
    lo, hi = max(lo_r, lo_t), min(hi_r, hi_t)
    if hi <= lo:
        raise ValueError("the curves share no PSNR interval")
    ir, it = np.polyint(pr), np.polyint(pt)
    avg = ((np.polyval(it, hi) - np.polyval(it, lo)) - (np.polyval(ir, hi) - np.polyval(ir, lo))) / (hi - lo)
    return float((10.0 ** avg - 1.0) * 100.0)
