"""GPU tier of the pixel-kernel tests: every form of the fused Lanczos-3 + CSC scaler, the BT.709
CSC, the masked SSE and the composites against the independent references of pixel_ref.py.

Output planes are allocated larger than the coded picture (pitch = coded_w + 64, 8 extra rows)
and filled with 0xA5; no byte outside the coded area may change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from . import pixel_ref as R  # noqa: E402
from .gpu_util import to_dev  # noqa: E402

SENTINEL = 0xA5
FORMS = ("valu", "tile", "strip")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Planes:
    """NV12 output planes with a guard band of SENTINEL bytes around the coded area."""

    def __init__(self, cw, ch):
        self.cw, self.ch, self.pitch = cw, ch, cw + 64
        self.y = torch.full((ch + 8, self.pitch), SENTINEL, dtype=torch.uint8, device="cuda")
        self.uv = torch.full((ch // 2 + 8, self.pitch), SENTINEL, dtype=torch.uint8, device="cuda")

    def read(self):
        """(Y [ch, cw], UV [ch / 2, cw]) after checking that the guard band is untouched."""
        torch.cuda.synchronize()
        out = []
        for plane, rows in ((self.y.cpu().numpy(), self.ch), (self.uv.cpu().numpy(), self.ch // 2)):
            guard = plane.copy()
            guard[:rows, : self.cw] = SENTINEL
            assert (guard == SENTINEL).all(), "bytes outside the coded area were written"
            out.append(plane[:rows, : self.cw].copy())
        return out


class Scaler:
    """One scaler geometry on the device: the Lanczos tables and a launch helper."""

    def __init__(self, gpu, in_w, in_h, out_w, out_h):
        self.gpu, self.geo = gpu, (in_w, in_h, out_w, out_h)
        xs, wx, self.tx = gpu.lanczos_table(in_w, out_w)
        ys, wy, self.ty = gpu.lanczos_table(in_h, out_h)
        self.tables = [to_dev(a) for a in (xs, wx, ys, wy)]
        self.cw, self.ch = R.coded(out_w), R.coded(out_h)

    def run(self, img, form, unaligned=False):
        """Scale an RGB8 picture in the given form; returns (form reported, Y, UV).  `unaligned`:
        rows of 4 * in_w + 8 bytes from a base pointer 4 bytes into the allocation."""
        in_w, in_h, out_w, out_h = self.geo
        pitch = 4 * in_w + 8 if unaligned else 4 * in_w
        off = 4 if unaligned else 0
        buf = np.full(off + in_h * pitch + 16, 0x3C, np.uint8)
        buf[off: off + in_h * pitch] = R.bgrx(img, pitch, fill=0x3C).reshape(-1)
        src = to_dev(buf)
        out = Planes(self.cw, self.ch)
        dx, dwx, dy, dwy = self.tables
        got = self.gpu.scale_to_nv12(src.data_ptr() + off, pitch, in_w, in_h, out_w, out_h, dx.data_ptr(),
                                     dwx.data_ptr(), self.tx, dy.data_ptr(), dwy.data_ptr(), self.ty,
                                     out.y.data_ptr(), out.uv.data_ptr(), out.pitch, self.cw, self.ch, _stream(),
                                     mfma=form != "valu", strip=form == "strip")
        y, uv = out.read()
        return got, y, uv


def _check_padding(y, uv, out_w, out_h):
    """The coded padding replicates the last column and row.  Luma: as bytes.  Chroma: the
    padding is the CSC of the replicated RGB edge, so every padding pair of a row equals the
    row's first padding pair and every padding row the first one (the last real pair averages
    two columns, the padding one)."""
    ch, cw = y.shape
    assert np.array_equal(y[:out_h, out_w:], np.repeat(y[:out_h, out_w - 1: out_w], cw - out_w, axis=1))
    assert np.array_equal(y[out_h:], np.repeat(y[out_h - 1: out_h], ch - out_h, axis=0))
    if cw > out_w:
        pad = uv[:, out_w:].reshape(ch // 2, -1, 2)
        assert (pad == pad[:, :1]).all()
    if ch > out_h:
        assert (uv[out_h // 2:] == uv[out_h // 2: out_h // 2 + 1]).all()


def _check_case(gpu, case, form, unaligned=False):
    in_w, in_h, out_w, out_h, _ = case
    plan = gpu.scale_plan(in_w, in_h, out_w, out_h)
    sc = Scaler(gpu, in_w, in_h, out_w, out_h)
    if form != "valu" and not plan["mfma"]:
        # outside the matrix-core range: refused, nothing launched
        with pytest.raises(ValueError, match="MFMA kernel's range"):
            sc.run(R.constant_picture(in_w, in_h, (0, 0, 0)), form)
        return
    # 2. constants: exact in both planes, padding included (DC gain at every position)
    for rgb in R.CONSTANTS:
        got, y, uv = sc.run(R.constant_picture(in_w, in_h, rgb), form, unaligned)
        assert got == form, (got, form)  # 1. the form that was asked for ran
        ry, ruv = R.nv12_from_rgb8(R.constant_picture(out_w, out_h, rgb), sc.cw, sc.ch)
        assert np.array_equal(y, ry) and np.array_equal(uv, ruv), (rgb, form)
    ref = R.scaler_reference(*case)
    got, y, uv = sc.run(ref["img"], form, unaligned)
    assert got == form, (got, form)
    model = ref["valu" if form == "valu" else "mfma"]
    ey, euv = ref["exact_nv12"]
    my, muv = model["nv12"]
    uy, uuv = model["undecided"]
    dy, duv = np.abs(y.astype(int) - ey), np.abs(uv.astype(int) - euv)
    miss_y, miss_uv = (y != my) & ~uy, (uv != muv) & ~uuv
    print(f"scaler {case[:4]} form={got}{' unaligned' if unaligned else ''}: differs from exact Y {(dy > 0).mean():.4f} "
          f"UV {(duv > 0).mean():.4f} (max {dy.max()}, {duv.max()}); decidable samples off the model: "
          f"Y {miss_y.sum()} UV {miss_uv.sum()}; model != kernel at undecidable: Y {((y != my) & uy).sum()} "
          f"UV {((uv != muv) & uuv).sum()}")
    # 3. within 1 of the rounded exact resample, every sample of both planes
    assert dy.max() <= 1 and duv.max() <= 1, (dy.max(), duv.max())
    # 4. equal to the form's own numeric model wherever the rounding is decidable
    assert not miss_y.any() and not miss_uv.any(), (int(miss_y.sum()), int(miss_uv.sum()))
    # 5. coded padding
    _check_padding(y, uv, out_w, out_h)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", R.SCALER_CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_scaler_form_matches_references(gpu, case, form):
    """Every scaler shape in every form it admits (the matrix-core forms refuse the last two)."""
    _check_case(gpu, case, form)


@pytest.mark.parametrize("case", R.SCALER_CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_scaler_valu_unaligned_input(gpu, case):
    """The VALU kernel without 16-byte loads: input pitch 4 * in_w + 8 from a base pointer 4
    bytes off alignment."""
    _check_case(gpu, case, "valu", unaligned=True)


# ---------------------------------------------------------------------------- CSC
@pytest.mark.parametrize("w,h,cw,ch", [(122, 66, 128, 80), (258, 6, 272, 16), (4, 2, 16, 16), (120, 68, 128, 80)])
def test_csc_equals_integer_reference(gpu, w, h, cw, ch):
    """k_bgrx_to_nv12 == the integer BT.709 model of the edge-replicated picture, both planes
    with padding; bytes of the input rows beyond the picture do not reach the output."""
    img = R.csc_picture(w, h, 7)
    pitch = (4 * w + 15) // 16 * 16 + 32
    src = to_dev(R.bgrx(img, pitch, fill=None, seed=8))
    out = Planes(cw, ch)
    gpu.bgrx_to_nv12(src.data_ptr(), pitch, w, h, out.y.data_ptr(), out.uv.data_ptr(), out.pitch, cw, ch, _stream())
    y, uv = out.read()
    ry, ruv = R.nv12_from_rgb8(img, cw, ch)
    assert np.array_equal(y, ry)
    assert np.array_equal(uv, ruv)


# ---------------------------------------------------------------------------- masked SSE
def _sse_reference(a, b, w, h, mask):
    keep = np.ones((h, w), bool)
    x0, y0, x1, y1 = mask
    keep[max(y0, 0): max(y1, 0), max(x0, 0): max(x1, 0)] = False
    d = a[:h, :w].astype(np.int64) - b[:h, :w].astype(np.int64)
    return int((d * d)[keep].sum())


@pytest.mark.parametrize("w,h,pitch,mask,content", [
    (200, 120, 256, (16, 32, 96, 80), "random"),
    (33, 5, 48, (0, 0, 0, 0), "random"),        # w % 16 == 1: lanes beyond w read real bytes
    (4096, 3, 4096, (0, 0, 0, 0), "random"),    # one row per workgroup
    (200, 120, 256, (0, 0, 0, 0), "extreme"),   # a = 0, b = 255: the largest sum
    (200, 120, 256, (0, 0, 200, 120), "random"),     # everything masked
    (200, 120, 256, (150, 100, 300, 200), "random"),  # mask reaching outside the picture
])
def test_sse_masked_matches_int64_sum(gpu, w, h, pitch, mask, content):
    """k_sse_masked against an int64 numpy sum; launched twice on the same scratch buffers, the
    second total equals the first (the completion counter re-arms itself)."""
    rng = np.random.default_rng(w + h)
    a = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    b = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    if content == "extreme":
        a[:, :w], b[:, :w] = 0, 255
    want = _sse_reference(a, b, w, h, mask)
    if content == "extreme":
        assert want == w * h * 255 * 255
    if mask == (0, 0, w, h):
        assert want == 0
    da, db = to_dev(a), to_dev(b)
    got = gpu.sse_masked(da.data_ptr(), db.data_ptr(), pitch, w, h, *mask, repeat=2, stream=_stream())
    assert got == [want, want], (got, want)


@pytest.mark.parametrize("depth", [1, 3])
def test_session_hevc_masked_psnr_separate_pass(gpu, depth):
    """HEVC with SAO off: the masked PSNR comes from the separate k_sse_masked pass (one scratch
    slot per frame in flight) and equals the PSNR of the decoded picture outside the 16-aligned
    mask rectangle, with one and with three frames in flight."""
    from mxdesk.codec.hevc_decoder import Decoder as HevcDecoder

    def session(d):
        cfg = gpu.SessionConfig()
        cfg.width, cfg.height, cfg.fps = 200, 120, 60
        cfg.codec = "hevc"
        cfg.enc.bitrate_kbps = 0
        cfg.enc.qp = 30
        cfg.enc.sao = 0
        cfg.enc.pipeline_depth = d
        cfg.fake_clock = 1
        cfg.mask_x0, cfg.mask_y0, cfg.mask_x1, cfg.mask_y1 = 20, 40, 90, 75  # -> x 16..96, y 32..80
        return gpu.Session(cfg)

    n = 4
    s = session(1)  # the sources: frames are a function of the frame number alone
    res, srcs = [], []
    for _ in range(n):
        res.append(s.step(False))
        srcs.append(s.nv12()[0][:120, :200].astype(np.float64))
    if depth > 1:
        s = session(depth)
        res, sent = [], 0
        while sent < min(depth, n):
            s.submit(False)
            sent += 1
        for _ in range(n):
            res.append(s.collect())
            if sent < n:
                s.submit(False)
                sent += 1
    frames = HevcDecoder().decode(b"".join(r.au for r in res))
    assert len(frames) == n
    keep = np.ones((120, 200), bool)
    keep[32:80, 16:96] = False
    for (dy, _, _), sy, r in zip(frames, srcs, res):
        mse = np.mean(((dy[:120, :200].astype(np.float64) - sy) ** 2)[keep])
        want = 99.0 if mse == 0 else min(99.0, 10 * np.log10(255.0 ** 2 / mse))
        assert abs(want - r.psnr_y_masked) < 1e-6, (want, r.psnr_y_masked)


# ---------------------------------------------------------------------------- composites
@pytest.mark.parametrize("dy", [0, 9])
@pytest.mark.parametrize("dx", [0, 4, 6, 333])
def test_composite_unaligned_tile(gpu, dx, dy):
    """ops.composite with a tile width that is no multiple of 4 and destinations on and off the
    16-byte grid: the rectangle equals the tile, nothing else changed."""
    from mxdesk import ops

    rng = np.random.default_rng(dx + dy)
    wide = to_dev(rng.integers(0, 256, (6, 324, 4), dtype=np.uint8))
    tile = wide[:, :322]
    dst = torch.full((16, 656, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    ops.composite(tile, dst, dx, dy)
    torch.cuda.synchronize()
    want = np.full((16, 656, 4), SENTINEL, np.uint8)
    want[dy: dy + 6, dx: dx + 322] = tile.cpu().numpy()
    assert np.array_equal(dst.cpu().numpy(), want)


def test_composite_nv12_byte_path(gpu):
    """k_composite_nv12 with a tile width that is no multiple of 16 (byte copies): 2 x 2 tiles
    of 72 x 6 into planes of pitch 160; nothing outside the tiles changed."""
    tw, th, pitch = 72, 6, 160
    rng = np.random.default_rng(9)
    tiles = rng.integers(0, 256, (4, th * 3 // 2, tw), dtype=np.uint8)
    d = to_dev(tiles)
    y = torch.full((2 * th + 4, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
    uv = torch.full((th + 4, pitch), SENTINEL, dtype=torch.uint8, device="cuda")
    gpu.composite_nv12(d.data_ptr(), tw, th, 2, 2, y.data_ptr(), uv.data_ptr(), pitch, _stream())
    torch.cuda.synchronize()
    wy = np.full((2 * th + 4, pitch), SENTINEL, np.uint8)
    wuv = np.full((th + 4, pitch), SENTINEL, np.uint8)
    for r in range(4):
        ox, oy = (r % 2) * tw, (r // 2) * th
        wy[oy: oy + th, ox: ox + tw] = tiles[r, :th]
        wuv[oy // 2: oy // 2 + th // 2, ox: ox + tw] = tiles[r, th:]
    assert np.array_equal(y.cpu().numpy(), wy) and np.array_equal(uv.cpu().numpy(), wuv)
