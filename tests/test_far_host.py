"""CPU: the geometry of tests/far_cases.py, from its integers alone - what tests/test_gpu_far_addresses.py relies on when it lets a
kernel form addresses beyond 2^32 on a shared device: every byte a case describes is inside the arena and outside its guards, no
two pieces of any two cases share a byte, and every case crosses the powers of two it is named for."""
import pytest

import far_cases as FC

ALL = [FC.place(*s) for s in FC.slots()]
IDS = ["%s-%s-%s" % s for s in FC.slots()]


def test_the_slots_are_distinct_and_few():
    assert len(set(FC.slots())) == len(FC.slots()) <= FC.MAX_SLOTS
    assert FC.MAX_SLOTS * FC.SLOT < FC.R
    for name in list(FC.CLIPS) + list(FC.ROW_CLIPS):
        assert "natural" in FC.contents_of(name)


@pytest.mark.parametrize("pl", ALL, ids=IDS)
def test_every_described_byte_is_inside_the_arena_and_outside_the_guards(pl):
    for shift in (0, pl.isz if pl.case == "F1a" else 0):      # (F1a is the case the control moves one sample on)
        for first, last in FC.described(pl, shift):
            assert FC.GUARD <= first <= last < FC.ARENA - FC.GUARD, (pl.clip, pl.case, first, last)


@pytest.mark.parametrize("pl", ALL, ids=IDS)
def test_the_written_pieces_are_the_described_bytes(pl):
    """every byte the descriptors address is in exactly one written piece (and the zero sample behind an F1 frame is what the
    moved descriptors add)"""
    written = sorted((a, a + n) for a, n, *_r in FC.runs(pl))
    assert all(a1 <= b0 for (_a0, a1), (b0, _b1) in zip(written, written[1:]))
    for shift in (0, pl.isz if pl.case == "F1a" else 0):
        for key, (spot, fs) in pl.streams.items():
            for f in range(1 if key == "prev0" else pl.n):
                for (w, h, off, rs, step, *_r) in pl.planes:
                    for y in range(h):
                        a = spot + f * fs + off + shift + y * rs
                        b = a + w * step                      # (a row's samples follow each other: step is one sample)
                        inside = [(p, q) for p, q in written if p < b and q > a]
                        covered = sum(min(q, b) - max(p, a) for p, q in inside)
                        assert covered == b - a, (pl.clip, pl.case, key, f, y, shift)
    if pl.case not in ("F1a", "F1b"):                         # nothing but samples is written
        assert sum(n for _a, n, *_r in FC.runs(pl)) == 3 * FC.frame_bytes(pl.clip)


def test_no_two_pieces_of_any_two_cases_share_a_byte():
    spans = sorted((a, a + n, at) for at, pl in enumerate(ALL) for a, n, *_r in FC.runs(pl))
    assert len(spans) > 1000
    for (a0, a1, s0), (b0, _b1, s1) in zip(spans, spans[1:]):
        assert a1 <= b0, (IDS[s0], IDS[s1], a0, b0)
    assert spans[0][0] >= FC.GUARD and max(s[1] for s in spans) <= FC.ARENA - FC.GUARD


@pytest.mark.parametrize("pl", ALL, ids=IDS)
def test_every_case_crosses_what_it_claims(pl):
    assert FC.crossings(pl) == FC.CLAIMS[pl.case], (pl.clip, pl.case)
    if pl.case in ("F1a", "F1b"):
        assert pl.streams["ref"][1] == (1 << 31) + 5 * 4096 and pl.streams["dist"][0] - pl.streams["ref"][0] == 1 << 20
        assert (pl.streams["dist"][1] == pl.streams["ref"][1]) == (pl.case == "F1a")
        assert pl.streams["prev0"][0] > pl.streams["ref"][0] + 2 * pl.streams["ref"][1]
        assert pl.streams["ref"][1] >= 1 << 31 and 2 * pl.streams["ref"][1] >= 1 << 32
    if pl.case == "F2" and len(pl.planes) == 3:
        y, u, v = pl.planes
        assert (y[2], u[2], v[2]) == (0, (1 << 31) + 2 * 4099, (1 << 32) + 2 * 8209) and u[3:5] == v[3:5]
        assert pl.streams["prev0"][0] - pl.streams["ref"][0] == 1 << 18
    if pl.case == "F3":
        rows = [y for y in range(pl.planes[0][1]) if y * FC.R >= 1 << 31], [y for y in range(pl.planes[0][1]) if y * FC.R >= 1 << 32]
        assert all(p[3] == FC.R for p in pl.planes)
        if len(pl.planes) == 3:
            assert (pl.planes[0][1], pl.planes[1][1]) == (34, 17) and rows == (list(range(16, 34)), [32, 33])
            assert [p[2] for p in pl.planes] == [0, 1 << 16, 1 << 17]
        else:
            assert rows[1] == [32] or pl.planes[0][1] == 34


def test_the_plane_that_pins_the_row_rule_for_ms_ssim():
    """MS_ROWS rows at MS_FAR span 2^31 bytes as vqa_quality_submit counts them (height * row_stride + width * step + sample
    size), at MS_NEAR they do not; both planes, and a row address wrapped to 32 bits, are bytes of the arena outside the guards"""
    n = FC.MS_ROWS
    assert n * FC.MS_FAR + n + 1 >= 1 << 31 and n * FC.MS_NEAR + n + 1 < 1 << 31
    assert FC.MS_SPOT >= FC.GUARD + FC.SLOT * len(FC.slots())
    for rs in (FC.MS_FAR, FC.MS_NEAR):
        assert FC.MS_DIST + n <= rs and FC.MS_SPOT + FC.MS_DIST + (n - 1) * rs + n <= FC.ARENA - FC.GUARD      # (dist's rows between ref's)
        for y in range(n):
            for wrong in _wrapped(y * rs):
                assert 0 <= FC.MS_SPOT + wrong and FC.MS_SPOT + FC.MS_DIST + wrong + n < FC.ARENA


def _wrapped(t):
    """a term formed in 32 bits: read back unsigned, and signed"""
    u = t % (1 << 32)
    return u, u - (1 << 32) if u >= 1 << 31 else u


def test_a_dropped_upper_half_or_a_wrong_sign_stays_inside_the_arena():
    """what the guards are for: the address of any sample of any case, with any one of its terms (frame * frame stride, the plane's
    offset, row * row stride) or their sum formed in 32 bits, is still a byte of the arena"""
    seen = 0
    for pl in ALL:
        for key, (spot, fs) in pl.streams.items():
            for f in range(1 if key == "prev0" else pl.n):
                for (w, h, off, rs, step, *_r) in pl.planes:
                    for y in range(h):
                        terms = (f * fs, off, y * rs)
                        inner = (w - 1) * step + pl.isz - 1
                        for at in range(4):
                            whole = sum(terms) if at == 3 else terms[at]
                            for wrong in _wrapped(whole):
                                a = spot + sum(terms) - whole + wrong
                                assert 0 <= a and a + inner < FC.ARENA, (pl.clip, pl.case, key, f, y, at)
                                seen += wrong != whole
    assert seen > 100
