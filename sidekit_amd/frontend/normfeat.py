"""``sidekit.frontend.normfeat``: RASTA filtering and the feature normalisations with the reference's parameter lists
(``sidekit/frontend/normfeat.py``), numpy in and numpy out, computed on the GPU by the kernels of ``sidekit_amd.features_server``
(``include/sidekit_amd/features.h``).  The four normalisers work in place as the reference's do; the values are the float32 device
results.  A stream without a labelled frame is left as it is (the reference's ``cms`` gives NaN there and its ``stg`` raises); the tie
rule of ``stg`` for an even number of frames below the window is in ``sidekit_amd.features_server``'s module text.  There is no CPU
fallback; importing the module needs neither a GPU nor torch."""
import numpy


def rasta_filt(x):
    """RASTA filtering of every column of ``x`` (frames x bands) -> a new float64 array: zeros for the first four frames, then the FIR
    ``[.2, .1, 0, -.1, -.2]`` (whose history are those four frames) followed by a single pole at 0.94 that starts at zero."""
    from ..features_server import rasta_device
    x = numpy.asarray(x)
    return rasta_device(numpy.asarray(x, dtype=numpy.float32)).cpu().numpy().astype(numpy.float64).reshape(x.shape)


def cms(features, label=None, global_mean=None):
    """Cepstral mean subtraction in place: the mean of the labelled frames (or ``global_mean``) is taken off every frame"""
    from ..features_server import normalise_host
    normalise_host(features, label, "cms", global_mean=global_mean)


def cmvn(features, label=None, global_mean=None, global_std=None):
    """Mean and variance normalisation in place: by the mean and the standard deviation (ddof = 0) of the labelled frames, or by
    ``global_mean`` and ``global_std`` when both are given"""
    from ..features_server import normalise_host
    normalise_host(features, label, "cmvn", global_mean=global_mean, global_std=global_std)


def stg(features, label=None, win=301):
    """Feature warping (short-term Gaussianisation) of the labelled frames in place, on a sliding window of ``win`` frames (odd)"""
    if win % 2 != 1:
        raise Exception('Sliding window should have an odd length')
    from ..features_server import normalise_host
    normalise_host(features, label, "stg", win=win)


def cep_sliding_norm(features, win=301, label=None, center=True, reduce=False):
    """Mean (and, with ``reduce``, sample standard deviation) normalisation of the labelled frames on a sliding window of ``win`` frames
    (odd), in place; at most ``win`` labelled frames: ``cms`` / ``cmvn`` of the whole stream.  As in the reference nothing happens
    without ``center`` when the window applies."""
    if win % 2 != 1:
        raise ValueError('Sliding window should have an odd length')
    count = features.shape[0] if label is None else int(numpy.sum(label))
    if count > win and not center:
        return
    from ..features_server import normalise_host
    normalise_host(features, label, "cmvn_sliding" if reduce else "cms_sliding", win=win)
