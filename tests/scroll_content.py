"""Scrolling test content and the CPU-oracle runs shared by test_scroll_hint.py and
test_gpu_scroll_hint.py.

A picture is a flat border one macroblock wide, which the encoders reconstruct exactly and which
stays static, around a "document" rectangle: a window onto a non-periodic texture that moves by
whole samples per picture (a move (mx, my) means picture(x, y) = previous picture(x + mx, y + my)
inside the rectangle, so a scrolled macroblock's vector is (4 mx, 4 my) and the expected hint is
the move).  Three macroblocks of the rectangle, none of them a probe of the lattice, do not scroll:
  * CURSOR: the lower half of a macroblock is fresh noise in every picture (the upper half scrolls
    with the document: a 16x8 partitioning around the hint);
  * STICKY: a fixed texture with a little fresh noise, closer to its own place in the reference
    than to the scrolled one (a search centred on zero while the picture has a hint);
  * NOISE: fresh noise all over (a full search around whichever centre).
Every schedule starts with still pictures: the encoders refine static content over a few pictures
(EncoderConfig::aq), as a page does before somebody scrolls it, and a scrolled macroblock votes
only when it matches its reference within the static threshold.
"""
import functools

import numpy as np

BORDER = 16
STILL = 3  # pictures without a move after the IDR

# shape -> moves (mx, my) after the still pictures.  Range 8: every move but (0, -8), (0, 0) and
# (3, 2) lies beyond the search.  A move leaves rectangle height (width) - |move| samples of the
# previous rectangle on screen; the moves are as large as still leaves the vote floor of three probe
# macroblocks (every second one in x and in y) wholly inside that overlap.
SCHEDULES = {
    (96, 160): [(0, -40), (0, 56), (0, -8), (0, 0), (0, 24), (3, 2), (0, -64)],
    (160, 96): [(57, 0), (-42, 0), (0, 0), (-64, 0), (3, 2), (24, 0)],  # also centres off the dword grid
    (208, 112): [(0, -40), (56, 0), (-88, 0), (0, 24), (3, 2), (0, 0), (72, 0), (0, -8)],
}
# macroblocks (mbx, mby) that do not scroll, per shape: cursor, sticky, noise
SPECIAL = {
    (96, 160): ((3, 3), (1, 5), (3, 7)),
    (160, 96): ((3, 3), (5, 1), (7, 3)),
    (208, 112): ((3, 3), (5, 1), (9, 5)),
}


def texture(u, v):
    t = (128 + 50 * np.sin(0.37 * u + 0.11 * v) + 40 * np.sin(0.13 * u - 0.41 * v + 1.0)
         + 20 * np.sin(0.9 * u + 0.8 * v) + 12 * np.sin(0.051 * u * np.sqrt(2.0) + 0.043 * v + 0.01 * u * v / 64.0))
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def _uv_of(y):
    h, w = y.shape
    uv = np.full((h // 2, w), 128, np.uint8)
    uv[:, 0::2] = y[0::2, 0::2] // 2 + 64
    uv[:, 1::2] = 200 - y[1::2, 0::2] // 2
    return uv


def stripes(u):
    return np.clip(np.rint(128 + 60 * np.sin(0.23 * u) + 30 * np.sin(0.071 * u + 2.0)), 0, 255).astype(np.uint8)


def make_frames(w, h, moves, special=None, seed=7, border=BORDER, bands=None, oy0=0):
    """[(y, uv)], one picture per move after STILL + 1 still ones; (0, 0) moves repeat the picture
    but for the special macroblocks.  The document above its row 0 is vertical stripes (the same in
    every row): with border 0 and oy0 < 0 a scroll towards them brings in rows equal to the picture's
    replicated top edge.  bands: [(x_from, x_to)] column ranges; move k is then a list of one
    move per band."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    inner = (slice(border, h - border), slice(border, w - border))
    sticky_tex = texture(xx * 1.3 + 500.0, yy * 0.7 + 300.0)
    nb = len(bands) if bands else 1
    ox, oy = [0] * nb, [oy0] * nb
    frames = []
    for mv in [(0, 0)] * (STILL + 1) + list(moves):
        doc = np.zeros((h, w), np.uint8)
        for b in range(nb):
            mx, my = mv[b] if (bands and mv != (0, 0)) else mv
            ox[b], oy[b] = ox[b] + mx, oy[b] + my
            d = np.where(yy + oy[b] < 0, stripes(xx + ox[b]), texture(xx + ox[b], yy + oy[b]))
            cols = slice(*bands[b]) if bands else slice(0, w)
            doc[:, cols] = d[:, cols]
        y = np.full((h, w), 128, np.uint8)
        y[inner] = doc[inner]
        if special:
            (cx, cy), (sx, sy), (nx, ny) = special
            y[16 * cy + 8:16 * cy + 16, 16 * cx:16 * cx + 16] = rng.integers(0, 256, (8, 16), dtype=np.uint8)
            blk = (slice(16 * sy, 16 * sy + 16), slice(16 * sx, 16 * sx + 16))
            y[blk] = np.clip(sticky_tex[blk].astype(np.int32) + rng.integers(-12, 13, (16, 16)), 0, 255).astype(np.uint8)
            y[16 * ny:16 * ny + 16, 16 * nx:16 * nx + 16] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
        frames.append((y, _uv_of(y)))
    return frames


@functools.lru_cache(maxsize=None)
def frames_for(w, h):
    return make_frames(w, h, SCHEDULES[(w, h)], SPECIAL[(w, h)], oy0=400)  # never reaches the stripes


# A picture without a border that scrolls towards the stripes: the rows that come in at the top equal
# the replicated top edge of the reference, so the top macroblocks match at the hint, 40 and 56 rows
# outside the picture (further than the decoder's fixed padding of 24 and than any +-R reach).
EDGE_SHAPE = (96, 160)
EDGE_MOVES = [(0, -40), (0, -56), (0, 0)]  # further moves would leave little but stripes, which match at any shift


@functools.lru_cache(maxsize=None)
def edge_frames():
    return make_frames(*EDGE_SHAPE, EDGE_MOVES, None, border=0, oy0=-8)


def moves_for(w, h):
    """The move of every picture of frames_for(w, h)."""
    return [(0, 0)] * (STILL + 1) + list(SCHEDULES[(w, h)])


def config(native, w, h, o):
    cfg = native.EncoderConfig()
    cfg.width, cfg.height = w, h
    cfg.bitrate_kbps, cfg.qp, cfg.search_range = 0, o.get("qp", 24), o.get("range", 8)
    cfg.subpel, cfg.partitions, cfg.me_coarse = o.get("subpel", 1), o.get("partitions", 1), o.get("me_coarse", 0)
    cfg.deblock, cfg.intra_in_p = o.get("deblock", 0), o.get("intra_in_p", 0)
    cfg.pipeline_depth = o.get("depth", 1)
    if "aq" in o:
        cfg.aq = o["aq"]
    if "scroll" in o:  # absent: the field is not touched at all
        cfg.scroll_range = o["scroll"]
    return cfg


class Run:
    """What the CPU oracle made of a sequence: per picture the access unit, the reconstruction, the
    reported hint, mb_info, the partition vectors and the path every macroblock's search took."""

    def __init__(self, native, w, h, o, frames):
        enc = native.CpuH264Encoder(config(native, w, h, o))
        self.aus, self.recs, self.hints, self.mbs, self.pmvs, self.paths, self.sse = [], [], [], [], [], [], []
        for y, uv in frames:
            self.aus.append(enc.encode(y, uv, False))
            self.recs.append(tuple(a.copy() for a in enc.recon()))
            st = enc.stats
            self.hints.append((st.scroll_dx, st.scroll_dy) if "scroll" in o else (0, 0))
            self.mbs.append(enc.mb_info().copy())
            self.pmvs.append(enc.mb_pmv().copy())
            self.paths.append(enc.mb_scroll_path().copy() if not st.idr else None)
            ry = self.recs[-1][0][:h, :w].astype(np.int64)
            self.sse.append(int(((ry - y.astype(np.int64)) ** 2).sum()))


_runs = {}


def cpu_run(native, w, h, o, frames=None, key=None):
    """The oracle's run of a shape's schedule under options o, computed once."""
    k = (w, h, tuple(sorted(o.items())), key)
    if k not in _runs:
        _runs[k] = Run(native, w, h, o, frames if frames is not None else frames_for(w, h))
    return _runs[k]


def check_decoder(stream_aus, recs):
    """The independent decoder's pictures equal the reconstructions."""
    from mxdesk.codec.h264_decoder import Decoder

    dec = Decoder()
    dec.decode(b"".join(stream_aus))
    assert len(dec.frames_coded) == len(recs)
    for t, ((yy, u, v), (ry, ruv)) in enumerate(zip(dec.frames_coded, recs)):
        hh, ww = yy.shape
        assert np.array_equal(yy, ry[:hh, :ww]), f"picture {t}: decoded luma"
        assert np.array_equal(u, ruv[:hh // 2, 0:ww:2]) and np.array_equal(v, ruv[:hh // 2, 1:ww:2]), \
            f"picture {t}: decoded chroma"
