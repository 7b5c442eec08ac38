"""float64 numpy restatement of the feature post-processing rules (include/sidekit_amd/features.h, sidekit_amd/features_server.py): RASTA,
the delta convolution, segment moments, the five normalisations of a stream of speech frames and the post-processing order with its
label semantics.  Written from the rules, not from the reference; tests/test_features_reference_cpu.py pins it to what the reference
computes (tests/golden/features.npz), tests/test_gpu_features.py holds the kernels to it."""
import numpy
from scipy.special import ndtri

DEFAULT_FILTER = numpy.array([.25, .5, .25, 0, -.25, -.5, -.25])


def rasta(x):
    x = numpy.asarray(x, dtype=numpy.float64)
    y = numpy.zeros_like(x)
    for t in range(4, x.shape[0]):
        y[t] = 0.2 * x[t] + 0.1 * x[t - 1] - 0.1 * x[t - 3] - 0.2 * x[t - 4] + 0.94 * y[t - 1]
    return y


def delta(x, filt=DEFAULT_FILTER):
    """'same' convolution with zeros outside the stream: y[t] = sum_k filt[k] x[t + half - k]"""
    x = numpy.asarray(x, dtype=numpy.float64)
    filt = numpy.asarray(filt, dtype=numpy.float64)
    n, half = x.shape[0], (filt.shape[0] - 1) // 2
    padded = numpy.zeros((n + 2 * half, x.shape[1]))
    padded[half:half + n] = x
    y = numpy.zeros_like(x)
    for k in range(filt.shape[0]):
        y += filt[k] * padded[2 * half - k:2 * half - k + n]
    return y


def moments(x):
    x = numpy.asarray(x, dtype=numpy.float64)
    if x.shape[0] == 0:
        return numpy.zeros(x.shape[1]), numpy.ones(x.shape[1])
    return x.mean(0), x.std(0)


def window_geometry(n, win, warp):
    """(w, m): the window length and the possibly extended stream length"""
    w = win
    if warp and n < win:
        w = n if n % 2 == 1 else n + 1
    return w, max(n, w)


def window_starts(n, w, m):
    t = numpy.arange(n)
    return numpy.minimum(numpy.maximum(t - (w - 1) // 2, 0), m - w)


def _windows(x, win, warp):
    n = x.shape[0]
    w, m = window_geometry(n, win, warp)
    ext = numpy.concatenate((x, x[-1:])) if m > n else x
    lo = window_starts(n, w, m)
    return ext[lo[:, None] + numpy.arange(w)[None, :]], w      # (n, w, D)


def warp_counts(x, win):
    """(c, w): per row and column the number of window values strictly below the row's own, and the window length"""
    x = numpy.asarray(x, dtype=numpy.float64)
    if x.shape[0] == 0:
        return numpy.zeros(x.shape, dtype=numpy.int64), win
    wins, w = _windows(x, win, True)
    return (wins < x[:, None, :]).sum(1), w


def warp_ties(x, win):
    """per row and column the number of window values EQUAL to the row's own, itself included (1 everywhere on a tie-free stream of odd
    or sufficient length; 2 for the last row of an even stream below the window, whose duplicate sits behind it)"""
    x = numpy.asarray(x, dtype=numpy.float64)
    if x.shape[0] == 0:
        return numpy.ones(x.shape, dtype=numpy.int64)
    wins, _ = _windows(x, win, True)
    return (wins == x[:, None, :]).sum(1)


def normalise(x, mode, win=301, mean=None, std=None):
    """One stream of speech frames under ``mode`` in ('cms', 'cmvn', 'cms_sliding', 'cmvn_sliding', 'stg')"""
    x = numpy.asarray(x, dtype=numpy.float64)
    n = x.shape[0]
    if n == 0:
        return x.copy()
    if mode == 'stg':
        c, w = warp_counts(x, win)
        return ndtri((c + 0.5) / w)
    if mean is None:
        mean, std = moments(x)
    with numpy.errstate(divide='ignore', invalid='ignore'):
        if mode in ('cms', 'cmvn') or n <= win:
            y = x - mean
            return y / std if mode in ('cmvn', 'cmvn_sliding') else y
        wins, w = _windows(x, win, False)
        mu = wins.sum(1) / w
        y = x - mu
        if mode == 'cmvn_sliding':
            y = y / numpy.sqrt(((wins - mu[:, None, :]) ** 2).sum(1) / (w - 1))
        return y


def sliding_std(x, win):
    """per row and column the standard deviation ``cmvn_sliding`` divides by: the stream's own (ddof = 0) for at most ``win`` rows, the
    window's (ddof = 1) beyond"""
    x = numpy.asarray(x, dtype=numpy.float64)
    if x.shape[0] <= win:
        return numpy.broadcast_to(moments(x)[1], x.shape)
    wins, w = _windows(x, win, False)
    return wins.std(1, ddof=1)


def post_process(x, label=None, rasta_on=False, delta_on=False, double_delta=False, filt=DEFAULT_FILTER, mask=None, feat_norm=None, win=301,
                 global_mean=None, global_std=None, keep_all=True, round32=True):
    """One utterance through the post-processing order -> (features, labels).  ``round32``: True, every kernel's output is rounded to
    float32 as the device stores it, so that the next stage sees the operands the device sees; 'delta', the deltas only, as the
    reference stores them; False, nothing."""
    r32 = lambda a: a.astype(numpy.float32).astype(numpy.float64)   # noqa: E731
    r = r32 if round32 is True else (lambda a: a)
    rd = r32 if round32 else (lambda a: a)
    x = numpy.array(x, dtype=numpy.float64)
    n = x.shape[0]
    label = numpy.ones(n, dtype=bool) if label is None else numpy.array(label, dtype=bool)
    if rasta_on:
        x = r(rasta(x))
        if n >= 3:
            x[:2] = x[2]
            label[:2] = label[2]
    if delta_on:
        d = rd(delta(x, filt))
        x = numpy.column_stack((x, d, rd(delta(d, filt)))) if double_delta else numpy.column_stack((x, d))
    if mask is not None:
        x = x[:, mask]
    count = int(label.sum())
    if feat_norm in ('cms', 'cmvn'):
        if global_mean is not None and (feat_norm == 'cms' or global_std is not None):
            x = r(normalise(x, feat_norm, win, numpy.asarray(global_mean, dtype=numpy.float64), None if global_std is None else numpy.asarray(global_std, dtype=numpy.float64)))
        elif count:
            mean, std = moments(x[label])
            x = r(normalise(x, feat_norm, win, mean, std))
    elif feat_norm is not None and count:
        if feat_norm != 'stg' and count <= win:
            mean, std = moments(x[label])
            x = r(normalise(x, 'cmvn' if feat_norm == 'cmvn_sliding' else 'cms', win, mean, std))
        else:
            x[label] = r(normalise(x[label], feat_norm, win))
    if not keep_all:
        x, label = x[label], label[label]
    return x, label
