"""Spatial registration read off the grid of Engine.shift / video_processing.frame_shift: pure host code over exact integers.

sse is [n, 2R + 1, 2R + 1] (uint64 array or nested lists); entry [j][a][b] is the squared error between encoded frame j and its
reference frame read at the shift (dy, dx) = (a - R, b - R), every entry over the same core (include/vqa.h).  A minimum at
(dy, dx) says that the encoded picture shows at (y, x) what the reference shows at (y + dy, x + dx).  Everything here works in
Python integers and fractions: no rounding until psnr_gain and subpixel, one formula each in double."""
import math
from fractions import Fraction

SHIFT_KEYS = ("SHIFT_RADIUS", "SHIFT_DY", "SHIFT_DX", "SHIFT_FRAMES_OFF", "SHIFT_PSNR_GAIN")
PSNR_GAIN_CAP = 100.0


def _grid(grid):
    g = [[int(v) for v in row] for row in grid]
    if not g or len(g) % 2 != 1 or len(g) < 3 or any(len(r) != len(g) for r in g):
        raise ValueError("a grid must be [2 radius + 1, 2 radius + 1] with radius >= 1")
    return g, len(g) // 2


def _grids(sse):
    grids = [_grid(g)[0] for g in sse]
    if not grids or any(len(g) != len(grids[0]) for g in grids):
        raise ValueError("sse must be [n, 2 radius + 1, 2 radius + 1] with n >= 1")
    return grids, len(grids[0]) // 2


def best_of(grid):
    """The shift (dy, dx) with the smallest value.  Shifts are examined in the order (dy^2 + dx^2, dy, dx) and replaced only on
    a strict improvement: a tie goes to the nearest to (0, 0), then to the smaller dy, then to the smaller dx."""
    g, R = _grid(grid)
    best, at = None, (0, 0)
    for dy, dx in sorted(((dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)),
                         key=lambda s: (s[0] * s[0] + s[1] * s[1], s[0], s[1])):
        v = g[dy + R][dx + R]
        if best is None or v < best:
            best, at = v, (dy, dx)
    return at


def psnr_gain(sse_given, sse_shifted, shift):
    """10 log10(sse_given / sse_shifted): what comparing in place costs in PSNR.  0.0 when the shift is (0, 0) or nothing is
    gained, capped at 100.0 (a shifted error of 0)"""
    if tuple(shift) == (0, 0) or sse_given <= sse_shifted:
        return 0.0
    if sse_shifted == 0:
        return PSNR_GAIN_CAP
    return min(PSNR_GAIN_CAP, 10.0 * math.log10(Fraction(sse_given, sse_shifted)))


def _vertex(lo, mid, hi):
    """the vertex of the parabola through (-1, lo), (0, mid), (1, hi); 0.0 where the second difference is not positive"""
    second = lo - 2 * mid + hi
    if second <= 0:
        return 0.0
    return float(Fraction(lo - hi, 2 * second))


def analyse(sse):
    """-> dict: shift (dy, dx) - best_of the exact per-entry sums over all frames -, per_frame (best_of each frame's own grid),
    frames_off (the frames whose own best differs from the clip's), edge (the clip's best lies on the band's border: the true
    shift may lie beyond the radius), sse_given (the summed entry at (0, 0)), sse_shifted (the summed entry at the shift),
    psnr_gain, and subpixel (dy, dx) as floats: what the vertex of the parabola through the three summed entries about the
    minimum adds to the integer shift on each axis, 0.0 at the border or where the second difference is not positive."""
    grids, R = _grids(sse)
    side = 2 * R + 1
    total = [[sum(g[a][b] for g in grids) for b in range(side)] for a in range(side)]
    dy, dx = best_of(total)
    per_frame = [best_of(g) for g in grids]
    a, b = dy + R, dx + R
    sub_y = _vertex(total[a - 1][b], total[a][b], total[a + 1][b]) if 0 < a < side - 1 else 0.0
    sub_x = _vertex(total[a][b - 1], total[a][b], total[a][b + 1]) if 0 < b < side - 1 else 0.0
    given, shifted = total[R][R], total[a][b]
    return {"shift": (dy, dx), "per_frame": per_frame, "frames_off": sum(1 for s in per_frame if s != (dy, dx)),
            "edge": abs(dy) == R or abs(dx) == R, "sse_given": given, "sse_shifted": shifted,
            "psnr_gain": psnr_gain(given, shifted, (dy, dx)), "subpixel": (sub_y, sub_x)}


def log_keys(result, radius):
    """analyse's dict -> the five top-level keys of the log and the row (SHIFT_KEYS, in that order)"""
    return {"SHIFT_RADIUS": int(radius), "SHIFT_DY": int(result["shift"][0]), "SHIFT_DX": int(result["shift"][1]),
            "SHIFT_FRAMES_OFF": int(result["frames_off"]), "SHIFT_PSNR_GAIN": float(result["psnr_gain"])}
