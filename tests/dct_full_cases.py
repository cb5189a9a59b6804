"""Full-frame DCT (dct_mode = full): the planes of every size class of its three implementations, their contents and the probe
frames.  Shared by tests/test_dct_full_host.py (does every class have a case, is the reference alone stable, do the probes have
teeth?) and tests/test_gpu_dct_full.py (the parity matrix), so that both see the same bytes.  Every frame is integer-only and
seeded, like probe_cases.py; the float64 side (scipy.fft.dctn) is at the end.

The plane's size alone picks the implementation, per side, so every class is reached by a small plane: 128 x 4000 is half a
megapixel.  path_of() restates that choice from the launchers; CASES names the class each size was placed for."""
import functools
from collections import namedtuple

import numpy as np

# ---- the dispatch ----------------------------------------------------------------------------------------------------------------
FFT_MIN, FFT_MAX = 128, 4000          # csrc/k_dct_fft.hip:486
LDS_CAP = 64 * 1024                   # csrc/k_dct_fft.hip:521


def fft_radices(n):
    """csrc/k_dct_fft.hip:484-496, dct_fft_factor: the radix of every pass of an n-point transform - 8 first, then 4, 2, 3, 5 - or
    None where the planner refuses n (odd, another prime factor, below 128 or above 4000)"""
    if n < FFT_MIN or n > FFT_MAX or n & 1:
        return None
    out, m = [], n
    for r in (8, 4, 2, 3, 5):
        while m % r == 0:
            out.append(r)
            m //= r
    return out if m == 1 else None


def fft_lengths():
    """every length the planner admits, ascending"""
    return [n for n in range(FFT_MIN, FFT_MAX + 1) if fft_radices(n) is not None]


def rows_class(w):
    """csrc/k_dct_fft.hip:531-536, launch_dct_full_fft: the row kernel's register class and workgroup size"""
    return "rows<2048,256>" if w <= 2048 else "rows<4096,512>"


def cols_class(h):
    """csrc/k_dct_fft.hip:540-558: eight columns per workgroup up to 2040 rows (two register classes), above that a column pair
    per workgroup - both planes at once where 4 h float2 fit the LDS, else one after the other"""
    if h <= 1152:
        return "cols8<1152>"
    if h <= 2040:
        return "cols8<2048>"
    return "cols<true>" if 4 * h * 8 <= LDS_CAP - 64 else "cols<false>"


def path_of(h, w):
    """the implementation an h x w plane takes in full mode: "valu", "mfma" or ("fft", rows class, cols class).
    csrc/vqa_capi.hip:1306 asks dct_fft_supported (csrc/k_dct_fft.hip:505-509: both sides factor) first; every other plane goes to
    launch_dct_full, whose products run on the matrix cores when both sides reach 128 (csrc/k_dct_full.hip:231)"""
    if fft_radices(h) is not None and fft_radices(w) is not None:
        return ("fft", rows_class(w), cols_class(h))
    return "mfma" if h >= 128 and w >= 128 else "valu"


def lds_bytes(h, w):
    """dynamic + static shared memory of the row and of the column kernel of an FFT plane (csrc/k_dct_fft.hip:532-557; the static
    part is the block reduction's: a double per wave) -> (rows, columns)"""
    _fft, _rows, cols = path_of(h, w)
    dyn = {"cols8<1152>": 32 * h, "cols8<2048>": 32 * h, "cols<true>": 4 * h * 8, "cols<false>": 2 * h * 8}[cols]
    return w * 8, dyn + 4 * 8


def auto_is_full(h, w):
    """csrc/vqa_capi.hip:1278: what VQA_DCT_AUTO resolves to"""
    return h * w <= 128 * 128


# ---- the cases -------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "h w path why native radices")


def _case(h, w, path, why, native=False, radices=None):
    return Case(h, w, path, why, native, radices)


_R2, _R4 = "rows<2048,256>", "rows<4096,512>"
_C1, _C2, _CP = "cols8<1152>", "cols8<2048>", "cols<false>"
SRC = (96, 160)     # the source every case without `native` is the resize of
CASES = [
    # FFT, the row classes (128 rows: one cols8<1152> slab of four pairs each, sixteen row groups)
    _case(128, 2048, ("fft", _R2, _C1), "the last 256-thread width", radices=(8, 8, 8, 4)),
    _case(128, 2160, ("fft", _R4, _C1), "the first 512-thread width", radices=(8, 2, 3, 3, 3, 5)),
    _case(128, 4000, ("fft", _R4, _C1), "the longest transform: 32000 bytes of LDS, radix 5 three times", radices=(8, 4, 5, 5, 5)),
    _case(128, 1458, ("fft", _R2, _C1), "seven passes, none of radix 8 or 4", radices=(2, 3, 3, 3, 3, 3, 3)),
    _case(128, 1250, ("fft", _R2, _C1), "2 * 5^4", radices=(2, 5, 5, 5, 5)),
    # FFT, the column classes
    _case(1152, 128, ("fft", _R2, _C1), "the last height of cols8<1152>"),
    _case(1200, 128, ("fft", _R2, _C2), "the first height of cols8<2048>"),
    _case(2000, 128, ("fft", _R2, _C2), "the last slab: 64000 + 32 bytes of LDS"),
    _case(2048, 128, ("fft", _R2, _CP), "the pair kernel's first height"),
    _case(4000, 128, ("fft", _R2, _CP), "the pair kernel's last: 64000 + 32 bytes of LDS"),
    _case(1458, 128, ("fft", _R2, _C2), "seven passes in the slab"),
    # FFT, a ragged work split
    _case(150, 162, ("fft", _R2, _C1), "150 rows: the last group of 8 holds 6; 162 columns: the last slab holds one pair"),
    _case(162, 150, ("fft", _R2, _C1), "162 rows: the last group holds 2; 150 columns: the last slab holds three pairs"),
    _case(2048, 150, ("fft", _R2, _CP), "the pair kernel with 75 pairs: 80 workgroups, five return at once"),
    # MFMA, odd sides
    _case(129, 131, "mfma", "both sides odd, one past the tile"),
    _case(135, 241, "mfma", "the thumbnail the other kinds test"),
    _case(128, 129, "mfma", "the predicate's edge, an odd K and ldb"),
    _case(257, 385, "mfma", "3 x 4 tiles, each last tile one sample wide, K % 16 = 1 in both products"),
    _case(255, 129, "mfma", "K % 16 = 15 and 1"),
    _case(255, 129, "mfma", "the same, the frame's own size: no resize pass", native=True),
    _case(143, 137, "mfma", "K % 16 = 9 and 15"),
    # vector ALU, and the planes with one side on either side of 128
    _case(127, 128, "valu", "the predicate's edge: h = 127"),
    _case(128, 127, "valu", "the predicate's edge: w = 127"),
    _case(64, 1920, "valu", "K = 1920 in the first product"),
    _case(1080, 64, "valu", "K = 1080 in the second product"),
    _case(100, 500, "valu", "7 x 32 tiles, both ragged"),
    _case(64, 256, "valu", "exactly 128 * 128 samples: AUTO is FULL"),
    _case(64, 258, "valu", "129 * 128 samples: AUTO is the 8 x 8 metric"),
]
PROBED = [(128, 4000), (2048, 150), (1200, 128), (257, 385), (135, 241), (64, 1920)]     # one case of each path and class
FRAMES = 3          # per case, plus prev0


def case_id(c):
    return "%dx%d%s" % (c.h, c.w, "-native" if c.native else "")


@functools.lru_cache(maxsize=None)
def clip(h, w, native=False):
    """-> uint8 [1 + FRAMES, sh, sw, 3]: prev0 and the batch of a case (its source frames: the case's plane is their resize)"""
    from rtvqa_amd import synth
    sh, sw = (h, w) if native else SRC
    fr = synth.s_natural(1 + FRAMES, sh, sw, seed=1000 + 7 * h + w)
    fr.setflags(write=False)
    return fr


# ---- the probe frames ------------------------------------------------------------------------------------------------------------
IMPULSE, AMPLITUDE = 40, 30
BASE_LO, BASE_HI = 70, 176      # the base: noise in 70 .. 175, so base + 40 <= 215 and base - 30 >= 40: nothing clips


@functools.lru_cache(maxsize=None)
def base_plane(h, w):
    a = np.random.default_rng(9000 + 7 * h + w).integers(BASE_LO, BASE_HI, (h, w))
    a.setflags(write=False)
    return a


def _unique(seq):
    out = []
    for p in seq:
        if p not in out:
            out.append(p)
    return out


def impulses(h, w):
    """(row, column) of the one pixel each impulse frame adds 40 to.  Rows 1, 7, 8: the second row of a pair and both sides of the
    row kernel's group of 8; columns 7, 8: both sides of an eight-column slab; 127, 128 and the last one: the MFMA tile"""
    my, mx = h // 2, w // 2
    rows, cols = [1, 7, 8, h - 2, h - 1], [1, 7, 8, w - 2, w - 1]
    if path_of(h, w) == "mfma":
        rows += [r for r in (127, 128) if r < h]
        cols += [c for c in (127, 128) if c < w]
    return _unique([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (my, mx)] + [(r, mx) for r in rows] + [(my, c) for c in cols])


def cosines(h, w):
    """(u, v) of the one basis function each cosine frame adds: the last frequency of each axis alone and both together, the
    first, the middle, and a pair that is neither"""
    return [(0, w - 1), (h - 1, 0), (h - 1, w - 1), (1, 1), (h // 2, w // 2), (3, w // 2 - 1)]


def cosine_plane(h, w, u, v):
    """rint(30 cos(pi (2 y + 1) u / 2 h) cos(pi (2 x + 1) v / 2 w)) as int64"""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    return np.rint(AMPLITUDE * np.cos(np.pi * (2 * y + 1) * u / (2.0 * h)) * np.cos(np.pi * (2 * x + 1) * v / (2.0 * w))).astype(np.int64)


def probes(h, w):
    """every probe of a plane in batch order: ("impulse", (row, column)) and ("cosine", (u, v))"""
    return [("impulse", p) for p in impulses(h, w)] + [("cosine", p) for p in cosines(h, w)]


def probe_plane(h, w, probe):
    """the gray plane of a probe frame, int64"""
    kind, p = probe
    a = base_plane(h, w)
    if kind == "impulse":
        a = a.copy()
        a[p] += IMPULSE
        return a
    return a + cosine_plane(h, w, *p)


def probe_batch(h, w):
    """-> uint8 [2 k + 1, h, w, 3]: base, p_1, base, p_2, .., base with B = G = R (bgr2gray returns the sample).  Frame 2 k - 1
    against its predecessor is the pair (p_k, base), frame 2 k the same pair reversed"""
    pr = probes(h, w)
    g = np.repeat(base_plane(h, w)[None], 2 * len(pr) + 1, axis=0)
    for k, probe in enumerate(pr):
        g[2 * k + 1] = probe_plane(h, w, probe)
    assert g.min() >= 40 and g.max() <= 215
    return np.repeat(g.astype(np.uint8)[..., None], 3, axis=3)


# ---- the float64 side ------------------------------------------------------------------------------------------------------------
RTOL = 1e-4     # the project's bar: BASELINE.json's north star, RTOL of tests/test_gpu_parity.py


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


ROWS_FIRST = (1, 0)     # scipy.fft.dctn takes its passes in the order of `axes`: every row (along x), then every column


def dct2(a, dtype=np.float64, axes=ROWS_FIRST):
    """the orthonormal 2-D DCT-II, as cv2.dct computes it.  The row pass comes first, as in both kernel families (k_dct_fft_rows
    before the column kernels; Tt = C_w X^T before Tt C_h^T in k_dct_full.hip).  In float64 the order moves no judged value by more
    than 1e-13; in float32 it decides which plane's magnitude the rounding noise of the second pass is relative to
    (tests/test_dct_full_host.py, test_the_order_of_the_passes)"""
    import scipy.fft
    return scipy.fft.dctn(np.asarray(a).astype(dtype), norm="ortho", axes=axes)


def energy(a, dtype=np.float64):
    return float((dct2(a, dtype).astype(np.float64) ** 2).sum())


def l1(prev, curr, dtype=np.float64):
    """sum |dct(prev) - dct(curr)|, each transform rounded to `dtype` as the reference's float32 pipeline does"""
    return float(np.abs(dct2(prev, dtype).astype(np.float64) - dct2(curr, dtype).astype(np.float64)).sum())


@functools.lru_cache(maxsize=None)
def basis_l1(n):
    """S_n(i) = sum_k |c_k(i)|, c_k(i) = s_k cos(pi (2 i + 1) k / 2 n) the orthonormal DCT-II basis: an impulse of height a at
    (y, x) has the separable spectrum a c_u(y) c_v(x), so its L1 is a S_h(y) S_w(x).  float64 [n]"""
    i, k = np.arange(n)[None, :], np.arange(n)[:, None]
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * i + 1) * k / (2.0 * n))
    c[0] = np.sqrt(1.0 / n)
    return np.abs(c).sum(axis=0)


def planes_of(c):
    """the gray planes of a case, uint8 [1 + FRAMES, h, w]: what the engine's plane A holds (gray, then resize: the reference's
    order, complexity_metrics.py:358-359)"""
    from oracle import c_oracle as co
    fr = clip(c.h, c.w, c.native)
    g = [co.bgr2gray(f) for f in fr]
    return np.stack(g if c.native else [co.resize_linear(a, c.w, c.h) for a in g])
