"""The score curve restated on the host in integers and float64 (numpy): the binning of a float32 score, the histogram split by label, the
suffix sums, precision / recall / F1 per threshold, the average precision, the summary and its tie rule -- the definition that
include/bidate_hip.h gives for bdn_score_hist / bdn_score_curve, written without reference to how the kernels compute it.
tests/test_curve_cpu.py pins it against brute force and sklearn; the GPU tests compare the kernels with it."""
import numpy as np


def softmax_scores(logits, pos):
    """float64 softmax(logits [n,ncls,...], axis 1)[:, pos]."""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(1, keepdims=True))
    return e[:, pos] / e.sum(1)


def bins(scores, n_bins):
    """Bin index of float32 scores: n_bins - 1 if s >= 1, (int)(s * n_bins) if s > 0 (exact: n_bins is a power of two), 0 otherwise (NaN too)."""
    s = np.asarray(scores, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        prod = np.where((s > 0) & (s < 1), s, np.float32(0)) * np.float32(n_bins)         # float32 product
        b = np.where(s >= 1, n_bins - 1, np.where(s > 0, prod.astype(np.int64), 0))
    return b.astype(np.int64)


def histogram(scores, labels, n_bins, pos=1, ignore=None):
    """int64 [2, n_bins], negatives first, of the valid pixels (label != ignore); positive iff label == pos."""
    s, l = np.asarray(scores, dtype=np.float32).reshape(-1), np.asarray(labels).reshape(-1).astype(np.int64)
    valid = np.ones(l.shape, bool) if ignore is None else l != ignore
    b = bins(s, n_bins)
    h = np.zeros((2, n_bins), dtype=np.int64)
    h[0] = np.bincount(b[valid & (l != pos)], minlength=n_bins)
    h[1] = np.bincount(b[valid & (l == pos)], minlength=n_bins)
    return h


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)       # integers below 2^53: exact
    return np.divide(num, den, out=np.zeros_like(num), where=den != 0)


def curve(hist):
    """hist int [2, n_bins] -> dict of TP, FP (int64 suffix sums), P, R, F (float64, one division each, 0 on a zero denominator)."""
    h = np.asarray(hist).astype(np.int64)
    fp, tp = h[0, ::-1].cumsum()[::-1], h[1, ::-1].cumsum()[::-1]
    n_pos = tp[0]
    return {'TP': tp, 'FP': fp, 'P': _ratio(tp, tp + fp), 'R': _ratio(tp, np.full_like(tp, n_pos)), 'F': _ratio(2 * tp, 2 * tp + fp + (n_pos - tp))}


def summary(hist):
    """{F_best, t_best, i_best, P_best, R_best, AP, n_pos, n_neg} as bdn_score_curve's summary[8]: the first maximum of F in ascending
    threshold; AP = sum_i (R_i - R_{i+1}) P_i with R_{n_bins} = 0."""
    c = curve(hist)
    n = len(c['F'])
    i = int(np.argmax(c['F']))                              # numpy: the first maximum
    r_next = np.append(c['R'][1:], 0.0)
    return {'F_best': float(c['F'][i]), 't_best': i / n, 'i_best': i, 'P_best': float(c['P'][i]), 'R_best': float(c['R'][i]),
            'AP': float(((c['R'] - r_next) * c['P']).sum()), 'n_pos': int(c['TP'][0]), 'n_neg': int(c['FP'][0])}


def summary_vector(hist):
    s = summary(hist)
    return np.array([s['F_best'], s['t_best'], s['i_best'], s['P_best'], s['R_best'], s['AP'], s['n_pos'], s['n_neg']], dtype=np.float64)
