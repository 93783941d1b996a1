"""Scroll hint of the H.264 P-picture search (EncoderConfig.scroll_range) on the CPU encoder, which
is the GPU encoder's bit-exact oracle: the probe pass finds the move of a scrolled rectangle, the
search takes it where it helps and nowhere else, the pictures get smaller, nothing changes without
a hint, and the independent decoder reproduces every picture.

Shapes, content and schedules: tests/scroll_content.py.  96x160 scrolls vertically, 160x96
horizontally, 208x112 both ways; search range 8.

QP: constant 12.  A probe votes, and a macroblock takes the hint outright, only when the scrolled
block matches the reference within the search's static threshold (static_sad: 0.5 per sample up to
QP 17).  The reference is the lossy reconstruction: the texture used here is reconstructed within
that at QP 12, only in part at QP 16 and not at QP 20 to 36, where the hint stays (0, 0) and the
pictures are coded as without it (profiles/scroll_hint/NOTES.md).
"""
import numpy as np
import pytest

from . import scroll_content as sc

N = None  # the compiled extension (the suite's `native` fixture)


@pytest.fixture(autouse=True)
def _extension(native):
    global N
    N = native

SHAPES = list(sc.SCHEDULES)
ON = {(96, 160): 64, (160, 96): 64, (208, 112): 96}  # scroll_range per shape: the largest move fits
STATIC, NO_HINT, HINT_EXIT, HINT_CENTRE, HINT_ZERO = range(5)  # MeScrollPath


def _on(w, h, **o):
    return sc.cpu_run(N, w, h, dict(scroll=ON[(w, h)], qp=12, **o))


def _off(w, h, **o):
    return sc.cpu_run(N, w, h, dict(scroll=0, qp=12, **o))


def _beyond(m):
    return max(abs(m[0]), abs(m[1])) > 8


def _scrolled_mbs(w, h, move):
    """Interior macroblocks whose whole block comes from the previous picture's rectangle and from
    none of its special macroblocks, and that are not special themselves."""
    mx, my = move
    out = []
    for mby in range(1, h // 16 - 1):
        for mbx in range(1, w // 16 - 1):
            xs, ys = 16 * mbx + mx, 16 * mby + my
            if xs < sc.BORDER or ys < sc.BORDER or xs + 16 > w - sc.BORDER or ys + 16 > h - sc.BORDER:
                continue
            if (mbx, mby) in sc.SPECIAL[(w, h)]:
                continue
            if any(xs < 16 * sx + 16 and xs + 16 > 16 * sx and ys < 16 * sy + 16 and ys + 16 > 16 * sy
                   for sx, sy in sc.SPECIAL[(w, h)]):
                continue
            out.append((mbx, mby))
    return out


@pytest.mark.parametrize("w,h", SHAPES)
def test_hint_is_the_move_and_scrolled_macroblocks_take_it(w, h):
    run, moves = _on(w, h), sc.moves_for(w, h)
    checked = 0
    for t, move in enumerate(moves):
        print(f"{w}x{h} picture {t}: move {move}, hint {run.hints[t]}")
        if not _beyond(move):
            continue
        assert run.hints[t] == move, f"picture {t}"
        mb = run.mbs[t]
        inner = _scrolled_mbs(w, h, move)
        assert len(inner) >= 3
        for mbx, mby in inner:
            assert tuple(mb[mby, mbx, [0, 4, 5, 8]]) == (0, 4 * move[0], 4 * move[1], 0), (t, mbx, mby, mb[mby, mbx])
        border = np.ones(mb.shape[:2], bool)
        border[1:-1, 1:-1] = False
        assert not mb[border][:, [4, 5, 8]].any(), f"picture {t}: a border macroblock moves"
        assert (run.paths[t][border] == STATIC).all()
        checked += 1
    assert checked >= 3


def test_every_path_of_the_search_occurs():
    """Conditions on the input, on the oracle alone: over the runs a search is centred on the hint and
    on zero under a hint, the hint's early exit is taken, and a partitioned macroblock is found
    around the hint."""
    seen, part_at_g = set(), 0
    for w, h in SHAPES:
        run = _on(w, h)
        for t, p in enumerate(run.paths):
            if p is None:
                continue
            seen |= set(int(v) for v in np.unique(p))
            part_at_g += int(((p == HINT_CENTRE) & (run.mbs[t][:, :, 8] != 0)).sum())
    print("paths seen", sorted(seen), "partitioned macroblocks around the hint", part_at_g)
    assert {STATIC, NO_HINT, HINT_EXIT, HINT_CENTRE, HINT_ZERO} <= seen
    assert part_at_g >= 1


@pytest.mark.parametrize("w,h", SHAPES)
def test_scrolled_pictures_are_smaller_with_the_hint(w, h):
    on, off = _on(w, h), _off(w, h)
    n = 0
    for t, move in enumerate(sc.moves_for(w, h)):
        if not _beyond(move):
            continue
        print(f"{w}x{h} picture {t} move {move}: {len(off.aus[t])} B / luma SSE {off.sse[t]} without, "
              f"{len(on.aus[t])} B / luma SSE {on.sse[t]} with the hint")
        assert len(on.aus[t]) < len(off.aus[t]), f"picture {t}"
        n += 1
    assert n >= 3


@pytest.mark.parametrize("w,h", SHAPES)
def test_range_zero_is_the_untouched_config(w, h):
    a, b = _off(w, h), sc.cpu_run(N, w, h, dict(qp=12))
    assert a.aus == b.aus
    assert all(hh == (0, 0) for hh in a.hints)


SMALL_MOVES = [(3, 2), (0, 0), (-2, 1), (1, -3), (3, 2), (-5, -7), (0, 0)]  # all inside the range of 8


@pytest.mark.parametrize("w,h", SHAPES)
def test_no_hint_no_change(w, h):
    """Content that never moves beyond the range: the access units equal the hint-off run's, picture
    by picture up to the first one that reports a hint (after it the references may differ)."""
    frames = sc.make_frames(w, h, SMALL_MOVES, sc.SPECIAL[(w, h)], oy0=400)
    on = sc.cpu_run(N, w, h, dict(scroll=ON[(w, h)], qp=12), frames, key="small")
    off = sc.cpu_run(N, w, h, dict(scroll=0, qp=12), frames, key="small")
    compared = 0
    for t in range(len(frames)):
        if on.hints[t] != (0, 0):
            break
        assert on.aus[t] == off.aus[t], f"picture {t}"
        compared += 1
    print(f"{w}x{h}: {compared} of {len(frames)} pictures compared, hints {on.hints}")
    assert compared >= sc.STILL + 2  # the still pictures and the first (3, 2) pan at least
    sc.check_decoder(on.aus, on.recs)


def _hints(w, h, frames, key, rng_=None):
    run = sc.cpu_run(N, w, h, dict(scroll=rng_ or ON[(w, h)], qp=12), frames, key=key)
    sc.check_decoder(run.aus, run.recs)
    return run.hints


def test_no_hint_on_a_static_sequence():
    w, h = 96, 160
    assert all(g == (0, 0) for g in _hints(w, h, sc.make_frames(w, h, [(0, 0)] * 4, None, oy0=400), "static"))


def test_no_hint_when_only_noise_changes():
    w, h = 96, 160  # the special macroblocks change in every picture, nothing moves
    assert all(g == (0, 0) for g in _hints(w, h, sc.make_frames(w, h, [(0, 0)] * 4, sc.SPECIAL[(w, h)], oy0=400), "noise"))


def test_no_hint_when_no_move_has_half_the_votes():
    """Three column bands of the 208x112 rectangle scroll by different amounts; the probe columns
    (macroblocks 2, 4 | 6, 8 | 10, rows 2 and 4) give 4, 4 and 2 votes: no bin has half of them.
    Each amount alone, over the whole rectangle, is found."""
    w, h = 208, 112
    amounts = [(0, -16), (0, 16), (0, -12)]
    for k, m in enumerate(amounts):
        assert _hints(w, h, sc.make_frames(w, h, [m], None, oy0=400), f"alone{k}")[-1] == m
    bands = [(16, 80), (80, 144), (144, 192)]
    mixed = sc.make_frames(w, h, [amounts], None, oy0=400, bands=bands)
    assert _hints(w, h, mixed, "bands")[-1] == (0, 0)


def test_vectors_stay_inside_the_level_limit():
    """scroll_range 192 and search range 32 on a picture tall enough for a 192-sample scroll: every
    vector stays within the vertical range [-256, +255.75] of level 3.0."""
    w, h = 64, 512
    special = ((1, 5), (1, 9), (1, 21))
    frames = sc.make_frames(w, h, [(0, 192), (0, -192)], special, oy0=400)
    run = sc.cpu_run(N, w, h, dict(scroll=192, qp=12, range=32), frames, key="tall")
    assert run.hints[-2:] == [(0, 192), (0, -192)], run.hints
    centred = 0
    for t in (-2, -1):
        mvy = np.concatenate([run.mbs[t][:, :, 5].ravel(), run.pmvs[t][:, :, 1].ravel(), run.pmvs[t][:, :, 3].ravel()])
        print("vertical vectors (quarter samples):", int(mvy.min()), "..", int(mvy.max()))
        assert mvy.min() >= -1024 and mvy.max() <= 1023
        assert np.abs(mvy).max() >= 4 * 192
        centred += int((run.paths[t] == HINT_CENTRE).sum())
    assert centred >= 1
    sc.check_decoder(run.aus, run.recs)


def test_reach_is_clamped_and_rounded():
    """scroll_range 500 is 192; 61 is 64 (a move of 64 is found, one of 65 is outside the reach)."""
    w, h = 96, 160
    assert sc.cpu_run(N, w, h, dict(scroll=61, qp=12)).hints[-1] == (0, -64)
    f65 = sc.make_frames(w, h, [(0, -65)], None, oy0=400)
    assert _hints(w, h, f65, "m65", 61)[-1] == (0, 0)
    assert _hints(w, h, f65, "m65", 500)[-1] == (0, -65)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("hint", [0, 1])
def test_decoder_reproduces_the_schedules(w, h, hint):
    run = _on(w, h) if hint else _off(w, h)
    sc.check_decoder(run.aus, run.recs)


def test_decoder_follows_vectors_far_outside_the_picture():
    """Macroblocks at the picture's top edge whose vector points 40 and 56 rows outside."""
    w, h = sc.EDGE_SHAPE
    run = sc.cpu_run(N, w, h, dict(scroll=64, qp=12), sc.edge_frames(), key="edge")
    moves = [(0, 0)] * (sc.STILL + 1) + sc.EDGE_MOVES
    far = 0
    for t, move in enumerate(moves):
        if move != (0, 0):
            assert run.hints[t] == move, (t, run.hints)
            far += int((run.mbs[t][0, :, 5] <= -4 * 40).sum())  # top row: y0 + mvy / 4 <= -40
    assert far >= 3
    sc.check_decoder(run.aus, run.recs)
