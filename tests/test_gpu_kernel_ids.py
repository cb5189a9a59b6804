"""vqa_profile_read's acceptance set as a whole on a live context: every id from -2 to VQA_K_EAVE + 2, nothing launched."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu


def test_profile_read_accepts_exactly_the_table_on_a_fresh_context():
    import rtvqa_amd
    from rtvqa_amd import _native as N
    with rtvqa_amd.Engine(0) as eng:
        for k in range(-2, N.K_EAVE + 3):
            ms, cnt = C.c_double(-1.0), C.c_int64(-1)
            st = eng.lib.vqa_profile_read(eng.ctx, k, C.byref(ms), C.byref(cnt), 0)
            if k in N.K_IDS_EXTANT:
                assert (st, ms.value, cnt.value) == (N.VQA_OK, 0.0, 0), k
            else:
                assert (st, ms.value, cnt.value) == (N.VQA_ERR_INVALID, -1.0, -1), k   # refused before anything is written
        assert eng.profile_read() == {}
