"""A NumPy restatement of vqa_conform_submit's definition (include/vqa.h): slicing for the window, fancy indexing for the frame
gather, a take for the table, the matrix in int64.  One frame is a list of [h_p, w_p] sample arrays, a stream is a list of
frames; nothing here knows about strides or pads (tests/conform_cases.py lays the results into byte canvases)."""
import numpy as np


def apply_lut(planes, lut, depth):
    """s_p = lut[p][min(sample, peak)]; lut None: the samples as they are -> int64 arrays"""
    peak = (1 << depth) - 1
    if lut is None:
        return [np.asarray(a).astype(np.int64) for a in planes]
    return [np.asarray(lut[p]).astype(np.int64)[np.minimum(np.asarray(a).astype(np.int64), peak)] for p, a in enumerate(planes)]


def apply_matrix(s, matrix, depth):
    """the three planes of one frame, at every SOURCE position, after the 2^-16 fixed-point matrix [3][4]"""
    peak = (1 << depth) - 1
    M = [[int(v) for v in row] for row in matrix]
    s0, s1, s2 = s
    h, w = s0.shape
    hc, wc = s1.shape
    assert s2.shape == (hc, wc) and hc in (h, (h + 1) // 2) and wc in (w, (w + 1) // 2)
    sy, sx = int(hc != h), int(wc != w)

    def out(k, a, b, c):
        return np.clip((M[k][0] * a + M[k][1] * b + M[k][2] * c + M[k][3] + (1 << 15)) >> 16, 0, peak)

    cy, cx = np.minimum(np.arange(h) >> sy, hc - 1), np.minimum(np.arange(w) >> sx, wc - 1)
    t0 = out(0, s0, s1[cy][:, cx], s2[cy][:, cx])
    # Ybar: the rounded mean of the luma samples of the cell that exist
    ph, pw = hc << sy, wc << sx
    tot, cnt = np.zeros((ph, pw), np.int64), np.zeros((ph, pw), np.int64)
    tot[:h, :w], cnt[:h, :w] = s0, 1
    tot = tot.reshape(hc, 1 << sy, wc, 1 << sx).sum((1, 3))
    cnt = cnt.reshape(hc, 1 << sy, wc, 1 << sx).sum((1, 3))
    assert cnt.min() >= 1
    ybar = (tot + cnt // 2) // cnt
    return [t0, out(1, ybar, s1, s2), out(2, ybar, s1, s2)]


def conform_frame(planes, sizes, origin=None, lut=None, matrix=None, depth=8):
    """one frame: planes [h_p, w_p] arrays, sizes [(oh_p, ow_p)], origin None or [(y0_p, x0_p)] -> the output planes"""
    t = apply_lut(planes, lut, depth)
    if matrix is not None:
        assert len(t) == 3
        t = apply_matrix(t, matrix, depth)
    out = []
    for p, a in enumerate(t):
        y0, x0 = (0, 0) if origin is None else (int(origin[p][0]), int(origin[p][1]))
        oh, ow = sizes[p]
        assert 0 <= y0 and 0 <= x0 and y0 + oh <= a.shape[0] and x0 + ow <= a.shape[1]
        out.append(a[y0:y0 + oh, x0:x0 + ow].astype(np.uint16 if depth > 8 else np.uint8))
    return out


def conform(frames, sizes, origin=None, index=None, lut=None, matrix=None, depth=8):
    """a stream: frames [n_in] of plane lists -> [n_out] of plane lists; index None: identity"""
    index = range(len(frames)) if index is None else [int(i) for i in index]
    assert all(0 <= i < len(frames) for i in index)
    return [conform_frame(frames[i], sizes, origin, lut, matrix, depth) for i in index]
