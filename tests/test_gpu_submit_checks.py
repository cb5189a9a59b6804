"""The plane-batch submits whose arguments are those of VIF or of motion (quality, VIF, ADM, motion, SI/TI, PSNR-HVS, GMSD,
HaarPSI) answer the shared bad inputs with the same status, in the same order of precedence, and a refused submit leaves the ctx
idle and usable.  One table, driven through the C ABI.  (The other kinds take further arguments - a colour model, a prev0 beside
the pair, one stream, a block map at the wait - and have their refusals in their own files; tests/test_gpu_all_kinds.py has all
sixteen kinds pending at once.)

Order of the checks (include/vqa.h states the rules; the order is behaviour): arguments, mem_kind, [quality: ssim_mode],
a pending batch of the same kind, then per plane in plane order - depth, 16-bit alignment, geometry (INVALID), the metric's
own limits (UNSUPPORTED) - and the frame strides after all planes."""
import ctypes as C

import numpy as np
import pytest

from rtvqa_amd import _native as N
from rtvqa_amd.engine import plane_descs

pytestmark = pytest.mark.gpu

W = H = 32
N_FRAMES = 2
INVALID, UNSUPPORTED, STATE, OK = N.VQA_ERR_INVALID, N.VQA_ERR_UNSUPPORTED, N.VQA_ERR_STATE, N.VQA_OK


def _planes(depth=8):
    """two W x H planes behind each other; (width, height, offset, row_stride, pixel_step, bit_depth)"""
    bps = 2 if depth > 8 else 1
    return [(W, H, 0, W * bps, bps, depth if depth > 8 else 0), (W, H, W * H * bps, W * bps, bps, depth if depth > 8 else 0)]


# metric -> (submit symbol, wait symbol, record type, smallest plane side, takes a dist stream)
METRICS = {
    "quality": ("vqa_quality_submit", "vqa_quality_wait", N.VqaPlaneMetrics, 11, True),
    "vif": ("vqa_vif_submit", "vqa_vif_wait", N.VqaVifMetrics, N.VIF_MIN_DIM, True),
    "adm": ("vqa_adm_submit", "vqa_adm_wait", N.VqaAdmMetrics, N.ADM_MIN_DIM, True),
    "motion": ("vqa_motion_submit", "vqa_motion_wait", N.VqaMotionMetrics, N.MOTION_MIN_DIM, False),
    "siti": ("vqa_siti_submit", "vqa_siti_wait", N.VqaSitiMetrics, N.SITI_MIN_DIM, False),
    "psnr_hvs": ("vqa_psnr_hvs_submit", "vqa_psnr_hvs_wait", N.VqaPsnrHvsMetrics, N.PSNR_HVS_MIN_DIM, True),
    "gmsd": ("vqa_gmsd_submit", "vqa_gmsd_wait", N.VqaGmsdMetrics, N.GMSD_MIN_DIM, True),
    "haarpsi": ("vqa_haarpsi_submit", "vqa_haarpsi_wait", N.VqaHaarpsiMetrics, N.HAARPSI_MIN_DIM, True),
}


class Call:
    """one submit's arguments; `with_(...)` gives an edited copy"""

    def __init__(self, depth=8):
        rng = np.random.default_rng(5)
        dt = np.uint16 if depth > 8 else np.uint8
        self.ref = rng.integers(0, 1 << depth, (N_FRAMES, 2 * W * H)).astype(dt)
        self.dist = rng.integers(0, 1 << depth, (N_FRAMES, 2 * W * H)).astype(dt)
        self.args = dict(ctx=True, ref=True, dist=True, planes=_planes(depth), descs=True, mem_kind=N.VQA_MEM_HOST, n=N_FRAMES,
                         n_planes=2, frame_stride=self.ref.nbytes // N_FRAMES, ssim_mode=N.SSIM_GAUSS)

    def with_(self, **edits):
        c = Call.__new__(Call)
        c.ref, c.dist, c.args = self.ref, self.dist, dict(self.args, **edits)
        return c

    def plane(self, p, **fields):
        """an edited copy whose plane p has the given vqa_plane_desc fields replaced"""
        names = ("width", "height", "offset", "row_stride", "pixel_step", "bit_depth")
        planes = [list(q) for q in self.args["planes"]]
        for k, v in fields.items():
            planes[p][names.index(k)] = v
        return self.with_(planes=[tuple(q) for q in planes])

    def submit(self, eng, metric):
        a = self.args
        sub, _wait, _rec, _min, pair = METRICS[metric]
        ctx = eng.ctx if a["ctx"] else None
        ref = self.ref.ctypes.data if a["ref"] else None
        dist = self.dist.ctypes.data if a["dist"] else None
        descs = plane_descs(a["planes"]) if a["descs"] else None
        fs = a["frame_stride"]
        fn = getattr(eng.lib, sub)
        if metric == "quality":
            return fn(ctx, ref, dist, a["mem_kind"], a["n"], fs, fs, descs, a["n_planes"], a["ssim_mode"])
        if pair:
            return fn(ctx, ref, dist, a["mem_kind"], a["n"], fs, fs, descs, a["n_planes"])
        return fn(ctx, ref, None, a["mem_kind"], a["n"], fs, descs, a["n_planes"])


def _wait(eng, metric, entries=N_FRAMES * 2):
    _sub, wait, rec, _min, _pair = METRICS[metric]
    out = (rec * entries)()
    return getattr(eng.lib, wait)(eng.ctx, out, entries), bytes(out)


def _idle_and_usable(eng, metric, good, want):
    """nothing is pending, and the valid submit goes through with the records it had before"""
    assert _wait(eng, metric)[0] == STATE
    assert good.submit(eng, metric) == OK
    st, got = _wait(eng, metric)
    assert st == OK and got == want


BASE8, BASE16 = Call(8), Call(10)
BIG = 1 << 14

# name -> (the call as a function of the metric's smallest plane side, the status every one of the submits gives)
CASES = {
    # arguments
    "null ctx": (lambda m: BASE8.with_(ctx=False), INVALID),
    "null ref": (lambda m: BASE8.with_(ref=False), INVALID),
    "null planes": (lambda m: BASE8.with_(descs=False), INVALID),
    "n zero": (lambda m: BASE8.with_(n=0), INVALID),
    "n negative": (lambda m: BASE8.with_(n=-1), INVALID),
    "no planes": (lambda m: BASE8.with_(n_planes=0), INVALID),
    "five planes": (lambda m: BASE8.with_(n_planes=5), INVALID),
    "bad mem_kind": (lambda m: BASE8.with_(mem_kind=7), INVALID),
    # depth
    "depth 7": (lambda m: BASE8.plane(0, bit_depth=7).plane(1, bit_depth=7), INVALID),
    "depth 17": (lambda m: BASE16.plane(0, bit_depth=17).plane(1, bit_depth=17), INVALID),
    "mixed depths": (lambda m: BASE16.plane(1, bit_depth=0), INVALID),
    "mixed depths, 8 first": (lambda m: BASE8.plane(1, bit_depth=10), INVALID),
    # 16-bit alignment
    "odd offset at 16 bits": (lambda m: BASE16.plane(1, offset=2 * W * H + 1), INVALID),
    "odd row stride at 16 bits": (lambda m: BASE16.plane(0, row_stride=2 * W + 1), INVALID),
    "odd step at 16 bits": (lambda m: BASE16.plane(0, pixel_step=3, row_stride=3 * W), INVALID),
    # geometry
    "zero width": (lambda m: BASE8.plane(1, width=0), INVALID),
    "negative height": (lambda m: BASE8.plane(0, height=-H), INVALID),
    "negative offset": (lambda m: BASE8.plane(0, offset=-1), INVALID),
    "zero step": (lambda m: BASE8.plane(0, pixel_step=0), INVALID),
    "row stride too small": (lambda m: BASE8.plane(0, row_stride=W - 1), INVALID),
    "row stride too small at 16 bits": (lambda m: BASE16.plane(1, row_stride=2 * W - 2), INVALID),
    "frame stride below the span": (lambda m: BASE8.with_(frame_stride=2 * W * H - 1), INVALID),
    # a plane whose last byte does not fit int64_t: a wrapped end is negative, leaves the span to plane 0 and would pass the
    # frame-stride rule (refused before a byte is read: the frames are the small ones)
    "plane end beyond int64, by the offset": (lambda m: BASE8.plane(1, offset=(1 << 63) - W * H), INVALID),
    "plane end beyond int64, by the offset at 16 bits": (lambda m: BASE16.plane(1, offset=(1 << 63) - 2 * W * H), INVALID),
    "plane end beyond int64, by the row stride": (lambda m: BASE8.plane(1, row_stride=1 << 59), INVALID),
    # the metric's own limits
    "plane too narrow": (lambda m: BASE8.plane(0, width=m - 1), UNSUPPORTED),
    "plane too low": (lambda m: BASE8.plane(1, height=m - 1), UNSUPPORTED),
    # precedence: per plane in plane order, all of one plane's rules before the next plane's
    "small plane ahead of a malformed one": (lambda m: BASE8.plane(0, width=m - 1).plane(1, width=0), UNSUPPORTED),
    "small plane ahead of a depth mismatch": (lambda m: BASE8.plane(0, height=m - 1).plane(1, bit_depth=10), UNSUPPORTED),
    "malformed plane ahead of a small one": (lambda m: BASE8.plane(0, pixel_step=0).plane(1, width=m - 1), INVALID),
    "malformed plane behind a good one": (lambda m: BASE8.plane(1, row_stride=W - 1), INVALID),
    "within a plane: alignment ahead of the size": (lambda m: BASE16.plane(0, width=m - 1, offset=1), INVALID),
    "within a plane: geometry ahead of the size": (lambda m: BASE8.plane(0, width=m - 1, offset=-1), INVALID),
    # the frame strides are looked at after every plane
    "small plane ahead of a short frame stride": (lambda m: BASE8.plane(1, width=m - 1).with_(frame_stride=1), UNSUPPORTED),
}


@pytest.fixture(scope="module")
def want(engine):
    """the records of the valid 8-bit call, per metric"""
    out = {}
    for metric in METRICS:
        assert BASE8.submit(engine, metric) == OK, metric
        st, out[metric] = _wait(engine, metric)
        assert st == OK, metric
    return out


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("metric", list(METRICS))
def test_refused_submit(engine, want, metric, case):
    make, status = CASES[case]
    call = make(METRICS[metric][3])
    assert call.submit(engine, metric) == status
    _idle_and_usable(engine, metric, BASE8, want[metric])


@pytest.mark.parametrize("metric", ["quality", "vif", "adm"])
def test_null_dist(engine, want, metric):
    assert BASE8.with_(dist=False).submit(engine, metric) == INVALID
    _idle_and_usable(engine, metric, BASE8, want[metric])


@pytest.mark.parametrize("metric", list(METRICS))
def test_valid_16_bit_call_and_one_frame_with_any_frame_stride(engine, want, metric):
    """the table's 16-bit base call is itself valid, and the frame-stride rule holds for n > 1 only"""
    assert BASE16.submit(engine, metric) == OK
    assert _wait(engine, metric)[0] == OK
    assert BASE8.with_(n=1, frame_stride=1).submit(engine, metric) == OK
    st, got = _wait(engine, metric, 2)
    assert st == OK and got == want[metric][:len(got)]


@pytest.mark.parametrize("metric", ["vif", "adm", "motion"])
def test_plane_above_two_to_the_28_samples(engine, want, metric):
    """(refused before a byte of it is read: the frames are the small ones)"""
    big = BASE8.with_(n=1, n_planes=1).plane(0, width=BIG + 1, height=BIG, row_stride=BIG + 1)
    assert big.submit(engine, metric) == UNSUPPORTED
    _idle_and_usable(engine, metric, BASE8, want[metric])


def test_quality_rows_spanning_two_gib(engine, want):
    """the Gaussian modes address a plane's rows with 32 bits; the 8x8 mode has no such limit to trip over here"""
    far = BASE8.with_(n=1, n_planes=1).plane(0, height=1 << 16, row_stride=1 << 15)
    assert far.submit(engine, "quality") == UNSUPPORTED
    assert far.with_(ssim_mode=N.SSIM_MS).plane(0, width=N.MS_MIN_DIM).submit(engine, "quality") == UNSUPPORTED
    _idle_and_usable(engine, "quality", BASE8, want["quality"])


def test_quality_mode_limits(engine, want):
    small = BASE8.plane(0, width=10)
    assert small.submit(engine, "quality") == UNSUPPORTED
    assert small.with_(ssim_mode=N.SSIM_FFMPEG).submit(engine, "quality") == OK      # the 8x8 mode takes planes from 8 x 8
    assert _wait(engine, "quality")[0] == OK
    assert BASE8.plane(0, width=7).with_(ssim_mode=N.SSIM_FFMPEG).submit(engine, "quality") == UNSUPPORTED
    assert BASE8.with_(ssim_mode=N.SSIM_MS).submit(engine, "quality") == UNSUPPORTED   # 32 x 32 is below 161 x 161
    for mode in (-1, 3):
        assert BASE8.with_(ssim_mode=mode).submit(engine, "quality") == INVALID
    _idle_and_usable(engine, "quality", BASE8, want["quality"])


@pytest.mark.parametrize("metric", list(METRICS))
def test_second_submit_while_one_is_pending(engine, want, metric):
    """STATE comes after the argument and mem_kind checks and before the planes are looked at; the pending batch survives
    every refusal"""
    assert BASE8.submit(engine, metric) == OK
    try:
        assert BASE8.submit(engine, metric) == STATE
        assert BASE8.plane(0, width=0).submit(engine, metric) == STATE
        assert BASE8.plane(0, width=METRICS[metric][3] - 1).submit(engine, metric) == STATE
        assert BASE8.with_(mem_kind=7).submit(engine, metric) == INVALID
        assert BASE8.with_(ref=False).submit(engine, metric) == INVALID
        assert BASE8.with_(n_planes=5).submit(engine, metric) == INVALID
        if metric == "quality":   # the mode is tested before the pending batch
            assert BASE8.with_(ssim_mode=3).submit(engine, metric) == INVALID
            assert BASE8.with_(ssim_mode=N.SSIM_FFMPEG).submit(engine, metric) == STATE
    finally:
        st, got = _wait(engine, metric)
    assert st == OK and got == want[metric]
    _idle_and_usable(engine, metric, BASE8, want[metric])


def test_a_pending_batch_of_one_kind_refuses_no_other_kind(engine, want):
    for metric in METRICS:
        assert BASE8.submit(engine, metric) == OK, metric
    for metric in reversed(list(METRICS)):
        st, got = _wait(engine, metric)
        assert st == OK and got == want[metric], metric
