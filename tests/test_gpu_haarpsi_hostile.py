"""GPU: HaarPSI on hostile content - flat fields at 0 and at the peak, 0 against the peak, anti-correlated pairs, a one-level
step - at every depth.  tests/test_haarpsi_host.py shows the float64 restatement stable on exactly these pairs first (its
quantised form stays within the bar of it, and the flat fields have exact answers); the GPU is held to the same bar,
haarpsi_cases.BAR = 4e-8 on haarpsi and on similarity, and to the restatement's den exactly."""
import pytest

import haarpsi_cases as HC
import haarpsi_reference as R
from test_gpu_haarpsi import check_one, mono

pytestmark = pytest.mark.gpu

MATRIX = HC.hostile_matrix()
WORST = {"gap": 0.0, "tag": ""}


@pytest.mark.parametrize("name,shape,depth", MATRIX, ids=["%s-%dx%d-%d" % (c, s[0], s[1], dp) for c, s, dp in MATRIX])
def test_parity_on_hostile_content(engine, name, shape, depth):
    rp, dp = HC.pair(name, shape[0], shape[1], depth)
    g = mono(engine, rp, dp, depth)
    check_one(g, rp, dp, depth, "%s %dx%d %d bits" % (name, shape[0], shape[1], depth), WORST)
    if name in ("flat_zero", "flat_peak"):
        assert g["haarpsi"] == 1.0 and g["similarity"] == R.U1 / R.FIX
    if name == "flat_zero":
        assert int(g["den"]) == 0 and int(g["num_lo"]) == 0 and int(g["num_hi"]) == 0
    if name == "ends":     # H of the zero plane is 0 everywhere: sim_s = c / (H^2 + c) and the score is far below 1
        assert 0.0 < g["haarpsi"] < 0.1
    if name == "step":     # one level moves the score off 1, by little
        assert 0.999 < g["haarpsi"] < 1.0


def test_the_worst_gap_on_hostile_content():
    print("hostile content: largest gap %.3e (%s), bar %.3e" % (WORST["gap"], WORST["tag"], HC.BAR))
    assert WORST["gap"] <= HC.BAR
