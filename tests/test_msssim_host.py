"""Multi-scale SSIM on the host side (no GPU): the float64 reference of tests/msssim_reference.py against closed forms and
against hbd_reference's single-scale SSIM, the additive ABI (VQA_SSIM_MS, vqa_ms_scales, vqa_quality_wait_ms) and the
config key's new value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hbd_reference as R
import msssim_reference as M
from rtvqa_amd import _native as N
from rtvqa_amd import video_processing as vp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = {"crf": 23, "vmaf_model_path": None, "resize_width": 64, "resize_height": 64, "frame_interval": 10}

# A uniform-random 177x263 8-bit pair whose level-1 cs mean is negative in the reference (-0.0028): two consecutive draws
# of np.random.default_rng(NEGATIVE_CS_SEED).integers(0, 256, (177, 263)).  Found by searching seeds 0.. for cs_1 < -1e-3.
NEGATIVE_CS_SEED = 156


def negative_cs_pair():
    rng = np.random.default_rng(NEGATIVE_CS_SEED)
    return rng.integers(0, 256, (177, 263)), rng.integers(0, 256, (177, 263))


def _texture(h, w, seed, depth=8):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    v = 0.5 + 0.25 * np.sin(x / 7.0) * np.cos(y / 11.0) + 0.2 * np.sin((x + 2 * y) / 23.0) + 0.03 * rng.standard_normal((h, w))
    return np.clip(np.rint(v * ((1 << depth) - 1)), 0, (1 << depth) - 1).astype(np.int64)


def test_identical_planes_give_one_everywhere():
    a = _texture(161, 200, 1)
    cs, ssim, ms = M.msssim(a, a, 255)
    assert np.allclose(cs, 1.0, rtol=0, atol=1e-12) and np.allclose(ssim, 1.0, rtol=0, atol=1e-12)
    assert abs(ms - 1.0) <= 1e-12


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_level_0_is_the_single_scale_reference(depth):
    mx = (1 << depth) - 1
    a = _texture(177, 263, 2, depth)
    b = np.clip(a + np.random.default_rng(3).integers(-3, 4, a.shape) * (1 << (depth - 8)), 0, mx)
    cs, ssim, _ms = M.msssim(a, b, mx)
    assert abs(ssim[0] - R.ssim_gauss(a, b, mx)) <= 1e-15
    assert (cs >= ssim - 1e-12).all()   # the luminance factor is at most 1


def test_pyramid_of_an_odd_ramp_by_hand():
    """5 x 3 ramp x[i][j] = 10 i + j.  Level 1 (3 x 2): the last row and the last column are duplicated before the 2x2 means;
    level 2 (2 x 1) duplicates level 1's last row and column again - the padding is per level, not once at level 0."""
    x = np.array([[10 * i + j for j in range(3)] for i in range(5)])
    l1 = M.downsample(x.astype(np.float64))
    assert l1.tolist() == [[5.5, 7.0], [25.5, 27.0], [40.5, 42.0]]
    l2 = M.downsample(l1)
    assert l2.tolist() == [[16.25], [41.25]]
    lv = M.pyramid(np.zeros((161, 177)))
    assert [v.shape for v in lv] == [(161, 177), (81, 89), (41, 45), (21, 23), (11, 12)]
    # the clamped-index form of the definition
    rng = np.random.default_rng(5)
    y = rng.integers(0, 1024, (13, 9)).astype(np.float64)
    h, w = y.shape
    want = np.array([[0.25 * sum(y[min(2 * i + di, h - 1), min(2 * j + dj, w - 1)] for di in (0, 1) for dj in (0, 1))
                      for j in range((w + 1) // 2)] for i in range((h + 1) // 2)])
    assert (M.downsample(y) == want).all()


def test_a_negative_cs_mean_gives_exactly_zero():
    a, b = negative_cs_pair()
    cs, ssim, ms = M.msssim(a, b, 255)
    assert cs[1] < -1e-3, cs
    assert ms == 0.0
    assert M.combine(cs, ssim) == 0.0 and M.value_bound(cs, ssim) is None


def test_planes_below_161_are_refused_by_the_reference():
    with pytest.raises(ValueError):
        M.msssim(np.zeros((160, 400)), np.zeros((160, 400)), 255)
    M.msssim(np.zeros((161, 161)), np.zeros((161, 161)), 255)


def test_constant_planes_in_closed_form():
    a, b = np.full((161, 170), 100), np.full((161, 170), 140)
    cs, ssim, ms = M.msssim(a, b, 255)
    lum = (2 * 100 * 140 + 6.5025) / (100 ** 2 + 140 ** 2 + 6.5025)
    assert np.allclose(cs, 1.0, rtol=0, atol=1e-9) and np.allclose(ssim, lum, rtol=0, atol=1e-9)
    assert abs(ms - lum ** M.WEIGHTS[4]) <= 1e-9


def test_the_additive_abi():
    assert N.SSIM_MS == 2 and (N.SSIM_GAUSS, N.SSIM_FFMPEG) == (0, 1)
    assert N.VQA_ABI_VERSION == 8
    assert C.sizeof(N.VqaMsScales) == 80
    assert (N.VqaMsScales.cs.offset, N.VqaMsScales.ssim.offset) == (0, 40)
    assert N.K_MS_PYRAMID == 11 and N.K_COUNT == 12
    assert N.MS_WEIGHTS == M.WEIGHTS and N.MS_MIN_DIM == M.MIN_DIM and N.MS_LEVELS == M.LEVELS
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    defs = dict(re.findall(r"^#define\s+VQA_(SSIM_\w+)\s+(\d+)", txt, flags=re.M))
    assert defs == {"SSIM_GAUSS": "0", "SSIM_FFMPEG": "1", "SSIM_MS": "2"}
    assert re.search(r"VQA_K_MS_PYRAMID\s*=\s*11", txt) and re.search(r"VQA_K_COUNT\s*=\s*12", txt)
    assert re.search(r"typedef struct vqa_ms_scales \{\s*double cs\[5\];[^}]*double ssim\[5\];[^}]*\} vqa_ms_scales;", txt)
    lib = N.load()
    assert lib.vqa_quality_wait_ms is not None and "vqa_quality_wait_ms" in N.SIGNATURES
    lib.vqa_kernel_name.restype = C.c_char_p
    assert lib.vqa_kernel_name(N.K_MS_PYRAMID) == b"k_ms_pyramid"
    # argument checks that need no device
    assert lib.vqa_quality_wait_ms(None, None, None, 0) == N.VQA_ERR_INVALID


def test_the_header_struct_is_80_bytes_to_the_c_compiler(tmp_path):
    import subprocess
    src = '#include <stdio.h>\n#include "vqa.h"\nint main(void){printf("%zu %d\\n", sizeof(vqa_ms_scales), VQA_SSIM_MS);return 0;}\n'
    (tmp_path / "m.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(tmp_path / "m"), str(tmp_path / "m.c")])
    assert subprocess.check_output([str(tmp_path / "m")]).decode().split() == ["80", "2"]


def test_config_accepts_msssim_and_still_refuses_the_pinned_values():
    vp.validate_config(dict(GOOD, ssim_mode="msssim"))
    for v in ("gauss", "ffmpeg"):
        vp.validate_config(dict(GOOD, ssim_mode=v))
    for bad in ("ms-ssim", None, 1, "MSSSIM", "ms_ssim"):
        with pytest.raises(ValueError) as e:
            vp.validate_config(dict(GOOD, ssim_mode=bad))
        assert str(e.value) == "ssim_mode must be 'gauss' or 'ffmpeg'."
    assert vp._SSIM_MODES["msssim"] == N.SSIM_MS


def test_scales_are_a_multi_scale_matter():
    from rtvqa_amd import stream
    with pytest.raises(ValueError):
        stream.Quality([(161, 161, 0, 161, 1)], N.SSIM_GAUSS, scales=True)
    assert stream.Quality([(161, 161, 0, 161, 1)], N.SSIM_MS, scales=True).scales
    assert not stream.Quality([(161, 161, 0, 161, 1)]).scales


def test_stats_lines_carry_whatever_the_mode_computed():
    """the ssim stats file keeps FFmpeg's format; All: is area-weighted (4:2:0: (4 Y + U + V) / 6)"""
    line = vp.ssim_stats_line(1, [0.9, 0.6, 0.3], [(322, 386), (161, 193), (161, 193)], "yuv")
    m = re.match(r"n:1 Y:0\.900000 U:0\.600000 V:0\.300000 All:(\d\.\d+) \((\d+\.\d+)\)\n", line)
    assert m and abs(float(m.group(1)) - (4 * 0.9 + 0.6 + 0.3) / 6) <= 1e-6
