"""The kernel ids as one set (no GPU): include/vqa.h's enum, _native's K_TABLE / K_MARKERS and vqa_kernel_name of the built library
against each other and against tests/golden/kernel_ids.json, the answers of the commit before the table existed (recorded once from
that commit's library; nothing here writes it).  The per-kind *_host.py files pin their own two or three ids; this is the whole."""
import ctypes as C
import json
import os
import re

from rtvqa_amd import _native as N

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "kernel_ids.json")))
GAPS = (14, 15, 18, 20, 22, 24, 26, 28, 33, 36, 38, 41, 43, 47, 50, 52, 55, 62, 65, 67, 69, 71, 74)   # below 78, unknown for good
# the cumulative id lists in the order the features shipped: (name, the ids it added to the list before it)
CHAIN = (("K_IDS_ALL", (19,)), ("K_IDS_KNOWN", (21,)), ("K_IDS_EVERY", (23,)), ("K_IDS_NAMED", (25,)), ("K_IDS_LISTED", (27,)),
         ("K_IDS_TOLD", (29, 30, 31, 32)), ("K_IDS_GIVEN", (34, 35)), ("K_IDS_SHOWN", (37,)), ("K_IDS_OPEN", (39, 40)),
         ("K_IDS_FULL", (42,)), ("K_IDS_WHOLE", (44, 45, 46)), ("K_IDS_TOTAL", (48, 49)), ("K_IDS_SUM", (51,)),
         ("K_IDS_GRAND", (53, 54)), ("K_IDS_ENTIRE", (56, 57, 58, 59, 60, 61)), ("K_IDS_COMPLETE", (63, 64)), ("K_IDS_PRESENT", (66,)),
         ("K_IDS_CURRENT", (68,)), ("K_IDS_LATEST", (70,)), ("K_IDS_NEWEST", (72, 73)), ("K_IDS_EXTANT", (75, 76, 77)))


def _kernel_name():
    lib = N.load()
    lib.vqa_kernel_name.restype = C.c_char_p
    return lambda k: lib.vqa_kernel_name(k).decode()


def test_the_header_and_the_binding_name_the_same_ids():
    txt = open(os.path.join(REPO, "include", "vqa.h")).read()
    enum = re.search(r"enum vqa_kernel_id \{(.*?)\}", txt, flags=re.S).group(1)
    pairs = re.findall(r"^\s*VQA_(K_\w+)\s*=\s*(\d+)", enum, flags=re.M)
    header = {name: int(v) for name, v in pairs}
    assert len(pairs) == len(header) == 55 + 24                     # no name twice in the header
    table = {name: k for name, k, _ in N.K_TABLE}
    assert len(N.K_TABLE) == len(table) == 55 and len(N.K_MARKERS) == 24 and not set(table) & set(N.K_MARKERS)
    assert set(header) == set(table) | set(N.K_MARKERS), set(header) ^ (set(table) | set(N.K_MARKERS))
    for name, v in header.items():
        assert {**table, **N.K_MARKERS}[name] == v and getattr(N, name) == v, name
    ids = [k for _, k, _ in N.K_TABLE]
    assert len(set(ids)) == 55 and ids == sorted(ids)               # no id in two rows; ascending, like the C table
    assert ids[0] == 0 and ids[-1] == N.K_EAVE - 1 == 77
    assert sorted(set(range(N.K_EAVE)) - set(ids)) == list(GAPS)


def test_kernel_names_are_the_parents_and_the_bindings():
    name = _kernel_name()
    assert re.fullmatch(r"[0-9a-f]{40}", GOLDEN["parent_commit"])
    assert (GOLDEN["first_id"], GOLDEN["last_id"]) == (-2, N.K_EAVE + 2)
    assert sorted(int(k) for k in GOLDEN["names"]) == list(range(-2, N.K_EAVE + 3))
    for k in range(-2, N.K_EAVE + 3):
        assert name(k) == GOLDEN["names"][str(k)] == N.K_NAMES.get(k, "?"), k
    assert tuple(GOLDEN["accepted"]) == N.K_IDS_EXTANT
    assert {k: kernel for _, k, kernel in N.K_TABLE} == N.K_NAMES
    names = [name(k) for k in N.K_IDS_EXTANT]
    assert len(set(names)) == 55 and "?" not in names
    assert (name(N.K_GRAY_HIST), name(N.K_FARNEBACK), name(N.K_SIG_BEST)) == ("k_bgr2gray_hist", "farneback(pyramid)", "k_sig_best")


def test_the_markers_and_the_gaps_stay_unknown():
    """Every marker's value names "?" - but for K_COUNT's: 12 has been K_VIF's id since VIF shipped (the parent answers
    "k_vif_stats" there, and so does the golden), the one marker whose value a kernel took."""
    name = _kernel_name()
    assert N.K_MARKERS["K_COUNT"] == N.K_VIF == 12 and name(12) == "k_vif_stats"
    for marker, v in N.K_MARKERS.items():
        if marker != "K_COUNT":
            assert name(v) == "?" and v not in N.K_NAMES, marker
    assert set(N.K_MARKERS.values()) - {12, N.K_EAVE} | {15} == set(GAPS)   # the gaps: the markers' values, and 15
    for k in GAPS + (-2, -1, N.K_EAVE, N.K_EAVE + 1, N.K_EAVE + 2):
        assert name(k) == "?", k
    lib = N.load()
    for k in range(-2, N.K_EAVE + 3):                               # without a context every id is refused
        assert lib.vqa_profile_read(None, k, None, None, 0) == N.VQA_ERR_INVALID


def test_the_id_lists_are_the_ones_each_feature_shipped():
    assert N.K_IDS == tuple(range(14)) + (16, 17)
    assert N.K_IDS_EVERY == tuple(range(14)) + (16, 17, 19, 21, 23)
    prev = N.K_IDS
    for ids, added in CHAIN:
        assert getattr(N, ids) == prev + added, ids
        prev = getattr(N, ids)
    assert N.K_IDS_EXTANT == tuple(sorted(N.K_NAMES)) and len(N.K_IDS_EXTANT) == 55
    assert N.K_IDS_CAMBI == (N.K_CAMBI_MASK, N.K_CAMBI_DECIMATE, N.K_CAMBI_CONTRAST, N.K_CAMBI_TOPK) == (29, 30, 31, 32)
    assert (N.K_COUNT, N.K_COUNT_ALL, N.K_COUNT_EXT, N.K_EAVE) == (12, 14, 18, 78)
