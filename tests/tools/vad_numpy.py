"""Float64 numpy restatement of the speech-activity path: the tests' yardstick, pinned against the reference's own output
(tests/golden/vad.npz, tests/test_vad_cpu.py).

``frame_log_energy``  the log-energy ``power_spectrum`` returns (sidekit/frontend/features.py:363-389): framing, pre-emphasis inside each
                      frame, ``log(sum(frame ** 2))``;
``vad_energy``        sidekit/mixture.py:67-113 with the degenerate rule of ``sk_vad_energy`` on top (threshold NaN, every frame kept);
``label_fusion``      sidekit/frontend/vad.py:409-428 for one channel: closing then opening, scipy's 'reflect' boundary;
``collect_labels`` / ``collect_segments``  the gathers, by numpy concatenation.
"""
import numpy

NWIN, SHIFT, PREFAC = 400, 160, 0.97      # 25 ms / 10 ms at 16 kHz


def n_frames(n, nwin=NWIN, shift=SHIFT):
    return (n - nwin) // shift + 1 if n >= nwin else 0


def frame_log_energy(x, nwin=NWIN, shift=SHIFT, prefac=PREFAC):
    """x: 1-D samples (int16 is widened as x / 32768) -> float64 log-energy per frame."""
    x = numpy.asarray(x)
    x = x.astype(numpy.float64) / 32768.0 if x.dtype == numpy.int16 else x.astype(numpy.float64)
    t = n_frames(x.shape[0], nwin, shift)
    if t == 0:
        return numpy.zeros(0)
    idx = numpy.arange(t)[:, None] * shift + numpy.arange(nwin)[None, :]
    frames = x[idx]
    prev = numpy.concatenate([frames[:, :1], frames[:, :-1]], axis=1)
    y = frames - prev * prefac
    return numpy.log((y * y).sum(axis=1))


def em_threshold(z, n_iter=8, flooring=0.0001, ceiling=1.0, alpha=2.0):
    """The mixture of ``vad_energy`` on standardised log-energies z -> threshold.  The first E-step has A = 0: the reference scores its
    hand-initialised Mixture before ``_compute_all`` has ever run."""
    w, mu, ic, A = numpy.ones(3) / 3, numpy.array([-2.0, 0.0, 2.0]), numpy.ones(3), numpy.zeros(3)
    z2 = z * z
    with numpy.errstate(all="ignore"):
        for _ in range(n_iter):
            lp = -0.5 * ((z2[:, None] * ic[None, :] - 2.0 * (z[:, None] * (mu * ic)[None, :])) + A[None, :])
            m = lp.max(axis=1)
            ll = m + numpy.log(numpy.exp(lp - m[:, None]).sum(axis=1))
            ll = numpy.where(numpy.isfinite(m), ll, m)
            pp = numpy.exp(lp - ll[:, None])
            s0, s1, s2 = pp.sum(axis=0), (z[:, None] * pp).sum(axis=0), (z2[:, None] * pp).sum(axis=0)
            w = s0 / s0.sum()
            mu = s1 / s0
            cov = s2 / s0 - mu * mu
            cov = numpy.where(cov <= flooring, flooring, cov)
            cov = numpy.where(cov >= ceiling, ceiling, cov)
            ic = 1.0 / cov
            cst = 1.0 / (numpy.sqrt(1.0 / ic) * (2.0 * numpy.pi) ** 0.5)
            A = mu * mu * ic - 2.0 * (numpy.log(w) + numpy.log(cst))
        if numpy.isnan(mu).any():
            return numpy.nan
        k = int(numpy.argmax(mu))
        return mu[k] - alpha * numpy.sqrt(1.0 / ic[k])


def reflect(i, n):
    i = numpy.mod(i, 2 * n)
    return numpy.where(i < n, i, 2 * n - 1 - i)


def _window(label, win, op):
    n, r = label.shape[0], win // 2
    idx = reflect(numpy.arange(n)[:, None] + numpy.arange(-r, r + 1)[None, :], n)
    return op(label[idx], axis=1)


def label_fusion(label, win=3):
    label = numpy.asarray(label, dtype=bool)
    if win == 0 or label.shape[0] == 0:
        return label.copy()
    closed = _window(_window(label, win, numpy.max), win, numpy.min)
    return _window(_window(closed, win, numpy.min), win, numpy.max)


def vad_energy(le, n_iter=8, flooring=0.0001, ceiling=1.0, alpha=2.0, fusion_win=0):
    """-> (labels, threshold, z) under the rule of ``sk_vad_energy``: a degenerate utterance keeps every frame, threshold NaN."""
    le = numpy.asarray(le, dtype=numpy.float64)
    n = le.shape[0]
    keep_all = (numpy.ones(n, dtype=bool), numpy.nan, numpy.zeros(n))
    if n < 1:
        return keep_all
    with numpy.errstate(all="ignore"):
        sd = numpy.std(le)
        if not numpy.isfinite(sd) or sd <= 0.0:
            return keep_all
        z = (le - numpy.mean(le)) / sd
    thr = em_threshold(z, n_iter, flooring, ceiling, alpha)
    if numpy.isnan(thr):
        return keep_all
    label = label_fusion(z > thr, fusion_win)
    if not label.any():
        return keep_all
    return label, thr, z


def sample_mask(label, n, shift=SHIFT):
    """The label-to-sample rule: sample s is kept iff label[min(s // shift, nframes - 1)]; no frame at all keeps everything."""
    label = numpy.asarray(label, dtype=bool)
    if label.shape[0] < 1:
        return numpy.ones(n, dtype=bool)
    return label[numpy.minimum(numpy.arange(n) // shift, label.shape[0] - 1)]


def collect_labels(x, label, shift=SHIFT):
    return x[sample_mask(label, x.shape[0], shift)]


def collect_segments(x, segments):
    return numpy.concatenate([x[:0]] + [x[s:e] for s, e in segments])


def labels_to_segments(label, n, shift=SHIFT):
    """Maximal runs of kept samples as [start, end) pairs."""
    m = numpy.concatenate([[False], sample_mask(label, n, shift), [False]])
    edges = numpy.flatnonzero(m[1:] != m[:-1])
    return [(int(s), int(e)) for s, e in zip(edges[::2], edges[1::2])]
