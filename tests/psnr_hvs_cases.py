"""The contents of the PSNR-HVS parity matrix, shared by tests/test_psnr_hvs_host.py (is the reference's own float32 run stable on
a content?) and tests/test_gpu_psnr_hvs.py (the GPU against the float64 reference), so that both see the same bytes: natural
texture and uniform noise, and hostile_cases' plane pairs - flat fields at either end of the range, the checkerboard against its
inverse, noisy checkerboards, the shifted step, faint texture around mid-grey, 0 against the maximum.  Integer-only and seeded."""
import numpy as np

import hostile_cases as HC

DEPTHS = (8, 10, 16)
ORDINARY = ("natural", "noise", "noise_small")
HOSTILE = HC.PAIRS + (HC.ENDS,)
CONTENTS = ORDINARY + HOSTILE
SHAPE = (40, 136)              # 5 x 17 blocks: two workgroups, the second ragged
ADMIT = 5e-5                   # the reference's float32 run against its float64 run, on both S: half the GPU bar
GPU_BAR = 1e-4                 # the family's bar (VIF, ADM)
# what tests/test_psnr_hvs_host.py finds unstable in the reference's own float32 run: (content, depth) left out by name
EXCLUDED = ()
MAX_EXCLUDED_SHARE = 0.1       # at most one case in ten


def pair(name, h, w, depth, seed=0):
    """-> (ref, dist) int64 [h, w] planes of `depth` bits"""
    L = (1 << depth) - 1
    if name == "natural":
        return HC.natural_pair(h, w, depth, seed)
    if name in ("noise", "noise_small"):
        rng = np.random.default_rng(77 * depth + seed)
        r = rng.integers(0, L + 1, (h, w))
        amp = L // 8 if name == "noise" else max(L // 128, 1)
        return r, np.clip(r + rng.integers(-amp, amp + 1, (h, w)), 0, L)
    return HC.pair(name, h, w, depth, seed)


def matrix():
    """every (name, depth) of the GPU matrix: the contents less the exclusions"""
    return [(n, d) for d in DEPTHS for n in CONTENTS if (n, d) not in EXCLUDED]
