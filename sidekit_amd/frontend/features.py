"""``sidekit.frontend.features``: the part of the reference's module the feature post-processing needs, ``compute_delta``
(``sidekit/frontend/features.py:133-166``), computed on the GPU (``sc_feat_delta``).  The reference's numpy MFCC / PLP extraction is not
built.  There is no CPU fallback; importing the module needs neither a GPU nor torch."""
import numpy

from .. import PARAM_TYPE


def compute_delta(features, win=3, method='filter', filt=numpy.array([.25, .5, .25, 0, -.25, -.5, -.25])):
    """The delta coefficients of ``features`` (frames x coefficients) -> float32, as the reference executes them:
    ``numpy.convolve(column, filt)[win:-win]``, a 'same' convolution with zeros (not the replicated edge frames the reference builds and
    leaves unused) outside the stream.  ``method='diff'``: ``filt`` is -1 at its first tap and 1 at its last.  ``filt`` must have
    ``2 win + 1`` taps (the reference fails with a broadcast error otherwise)."""
    from ..features_server import delta_device
    features = numpy.asarray(features)
    if method == 'diff':
        filt = numpy.zeros(2 * win + 1, dtype=PARAM_TYPE)
        filt[0] = -1
        filt[-1] = 1
    filt = numpy.asarray(filt, dtype=numpy.float64).reshape(-1)
    if filt.shape[0] != 2 * win + 1:
        raise ValueError('the delta filter has {} taps, the window 2 * {} + 1'.format(filt.shape[0], win))
    return delta_device(numpy.asarray(features, dtype=numpy.float32), None, filt).cpu().numpy().astype(PARAM_TYPE)
