"""The all-zero residual bounds of the H.264 P coder (h264_mb.h zero_sum_4x4 / zero_sum_chroma_dc):
a 4x4 block whose sum |residual| stays within the bound must quantise to no level at all, a chroma
plane whose sum stays within the DC bound must give no DC level.  k_inter_encode skips every
transform of such a macroblock, so a bound that is too wide would change the bitstream.

Checked against the real quantisers (quant4x4, quant_dc_chroma) and the real block pipeline
(fdct4x4, luma_block_inter), for every QP 0..51.

The smallest bound these tables give is 1 (luma / chroma AC at QP 0..2) and 4 (chroma DC at QP 0):
no QP has a bound of 0, so "only the all-zero block qualifies" does not occur; the lowest QPs and
the all-zero block are covered instead."""
import numpy as np
import pytest

QPS = list(range(52))
GAIN = np.array([[(2 if r & 1 else 1) * (2 if c & 1 else 1) for c in range(4)] for r in range(4)]).ravel()


def _levels_ac(h, res, qp, start):
    y = h.fdct4x4(np.asarray(res, np.int32))
    z, nz = h.quant4x4(y, qp, False, start)
    return np.asarray(z), nz, np.asarray(y)


def test_bounds_are_the_largest_safe_sums_per_coefficient(native):
    """The worst-case coefficient gain * T of every position quantises to 0 at every QP, in both
    signs; gain * (T + 1) does not at the binding position, so T is the largest such sum."""
    h = native.h264
    for qp in QPS:
        t = h.zero_sum_4x4(qp)
        assert t >= 1
        tight = False
        for pos in range(16):
            for sign in (1, -1):
                y = np.zeros(16, np.int32)
                y[pos] = sign * GAIN[pos] * t
                z, nz = h.quant4x4(y, qp, False, 0)
                assert nz == 0 and not np.any(z), (qp, pos, sign)
            y = np.zeros(16, np.int32)
            y[pos] = GAIN[pos] * (t + 1)
            tight |= h.quant4x4(y, qp, False, 0)[1] > 0
        assert tight, qp
        td = h.zero_sum_chroma_dc(qp)
        assert td >= 4
        for sign in (1, -1):
            z, nz = h.quant_dc_chroma(np.array([sign * td, 0, 0, 0], np.int32), qp, False)
            assert nz == 0 and not np.any(z), (qp, sign)
        assert h.quant_dc_chroma(np.array([td + 1, 0, 0, 0], np.int32), qp, False)[1] > 0, qp
    assert h.zero_sum_4x4(0) == 1  # the lowest bound: one sample off by one


def _spread(t, n=16):
    """n non-negative integers summing to t, as flat as possible."""
    v = np.full(n, t // n, np.int64)
    v[: t % n] += 1
    return v


def _blocks_at(t, rng):
    """Adversarial 4x4 blocks (raster) with sum |x| == t exactly."""
    r, c = np.divmod(np.arange(16), 4)
    out = []
    for pos in range(16):
        for sign in (1, -1):
            b = np.zeros(16, np.int64)
            b[pos] = sign * t
            out.append(b)
    flat = _spread(t)
    out += [flat, -flat]
    for sgn in ((-1) ** r, (-1) ** c, (-1) ** (r + c), (-1) ** (r // 2), (-1) ** (c // 2), (-1) ** (r // 2 + c // 2)):
        out += [flat * sgn, np.roll(flat, 5) * sgn]
    for _ in range(24):  # seeded: random split of t over the positions, random signs
        mag = rng.multinomial(t, rng.dirichlet(np.full(16, rng.choice([0.1, 1.0, 10.0]))))
        out.append(mag * rng.choice([-1, 1], 16))
    for b in out:
        assert int(np.abs(b).sum()) == t
    return out


@pytest.mark.parametrize("qp", QPS)
def test_blocks_at_the_bound_have_no_level(native, qp):
    h = native.h264
    rng = np.random.default_rng(4200 + qp)
    t = h.zero_sum_4x4(qp)
    assert h.luma_block_inter(np.zeros(16, np.int32), qp)[2] == 0
    for b in _blocks_at(t, rng):
        z, rres, nz = h.luma_block_inter(b.astype(np.int32), qp)  # the P coder's luma block pipeline
        assert nz == 0 and not np.any(z) and not np.any(rres), (qp, t, b)
        zc, nzc, _ = _levels_ac(h, b, qp, 1)  # chroma AC: the same quantiser at qpc, DC left out
        assert nzc == 0 and not np.any(zc), (qp, t, b)


@pytest.mark.parametrize("qpc", QPS)
def test_planes_at_the_dc_bound_have_no_dc_level(native, qpc):
    """8x8 chroma planes with sum |x| == zero_sum_chroma_dc(qpc): the four blocks' DC terms through
    fdct4x4 and quant_dc_chroma."""
    h = native.h264
    rng = np.random.default_rng(9100 + qpc)
    t = h.zero_sum_chroma_dc(qpc)
    r, c = np.divmod(np.arange(64), 8)
    planes = []
    for pos in (0, 7, 27, 36, 56, 63):
        for sign in (1, -1):
            p = np.zeros(64, np.int64)
            p[pos] = sign * t
            planes.append(p)
    flat = _spread(t, 64)
    planes += [flat, -flat, flat * (-1) ** (r // 4), flat * (-1) ** (c // 4), flat * (-1) ** (r // 4 + c // 4),
               flat * (-1) ** (r + c)]
    for _ in range(16):
        mag = rng.multinomial(t, rng.dirichlet(np.full(64, rng.choice([0.05, 1.0, 10.0]))))
        planes.append(mag * rng.choice([-1, 1], 64))
    for p in planes:
        assert int(np.abs(p).sum()) == t
        p8 = p.reshape(8, 8)
        dc = [int(np.asarray(h.fdct4x4(p8[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].astype(np.int32).ravel()))[0])
              for by in range(2) for bx in range(2)]
        z, nz = h.quant_dc_chroma(np.array(dc, np.int32), qpc, False)
        assert nz == 0 and not np.any(z), (qpc, t, dc)
