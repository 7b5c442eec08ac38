"""GMM-supervector SVM scoring -- mirror of ``sidekit/svm_scoring.py``: ``svm_scoring`` and ``svm_scoring_singleThread`` (:49-128), the
score of a test supervector ``x`` under the linear SVM ``(w, b)`` of a model, ``w . x + b``.

The reference loops over the test segments in Python; here the scores of all models against all segments are one float64 GEMM on the
device (``svm_score_device``) and the trial mask picks from it.  A test segment is looked up in ``test_sv`` by its name (the reference
takes row ``ts`` of ``test_sv`` for segment ``ts`` of the ``Ndx``, which is the same row whenever the two are aligned, as ``svm_scoring``
leaves them).  There is no CPU fallback; importing the module needs neither a GPU nor torch.
"""
import logging

import numpy

from . import sv_utils
from .bosaris import Ndx, Scores
from .bosaris._sets import first_index
from .statserver import StatServer


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.svm_scoring computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def svm_score_device(W, b, test):
    """``scores[m, s] = W[m] . test[s] + b[m]``: ``W`` (M, D), ``b`` (M,), ``test`` (S, D), CUDA tensors or host arrays, float64 on the
    device.  Returns the (M, S) float64 scores, on the device when ``test`` was there."""
    torch = _torch()
    host = not torch.is_tensor(test)
    dev = test.device if not host and test.is_cuda else torch.device("cuda", torch.cuda.current_device())

    def f64(a):
        if not torch.is_tensor(a):
            a = torch.as_tensor(numpy.array(a, dtype=numpy.float64, order='C'))
        return a.to(device=dev, dtype=torch.float64).contiguous()

    W, b, test = f64(W), f64(b), f64(test)
    assert W.dim() == 2 and test.dim() == 2 and W.shape[1] == test.shape[1] and b.shape == (W.shape[0],), "W: (M, D), b: (M,), test: (S, D)"
    scores = torch.matmul(W, test.t()) + b[:, None]
    return scores.cpu().numpy() if host else scores


def svm_scoring_singleThread(svm_filename_structure, test_sv, ndx, score, seg_idx=None):
    """The trials of the test segments ``seg_idx`` of ``ndx`` (all when ``None``) into ``score.scoremat`` (models of ``ndx`` x segments of
    ``ndx``), :49-87.  The SVM of model ``m`` is read from ``svm_filename_structure.format(m)``; ``test_sv.stat1`` holds the test
    supervectors.  Entries outside the trial mask keep what ``score.scoremat`` holds."""
    assert isinstance(test_sv, StatServer), 'Second parameter should be a StatServer'
    assert isinstance(ndx, Ndx), 'Third parameter should be an Ndx'
    if seg_idx is None:
        seg_idx = range(ndx.segset.shape[0])
    cols = numpy.array([int(t) for t in seg_idx], dtype=numpy.int64)
    if cols.shape[0] == 0 or ndx.modelset.shape[0] == 0:
        return
    W = numpy.zeros((ndx.modelset.shape[0], test_sv.stat1.shape[1]))
    b = numpy.zeros(ndx.modelset.shape[0])
    for m, name in enumerate(ndx.modelset):
        W[m, :], b[m] = sv_utils.read_svm(svm_filename_structure.format(name))
    logging.info('Compute trials involving %d test segments of %d', cols.shape[0], ndx.segset.shape[0])
    rows = first_index(test_sv.segset, ndx.segset[cols])
    scores = svm_score_device(W, b, test_sv.stat1[rows, :])
    mask = ndx.trialmask[:, cols]
    block = score.scoremat[:, cols]
    block[mask] = scores[mask]
    score.scoremat[:, cols] = block


def svm_scoring(svm_filename_structure, test_sv, ndx, num_thread=1):
    """Scores of the trials of ``ndx`` (:90-128) -> ``Scores`` with the models of ``ndx`` whose SVM file exists and the segments that
    ``test_sv`` holds, ``scoremask`` = the trial mask and 0 where there is no trial.  ``num_thread`` is accepted and unused."""
    existing_models, _ = sv_utils.check_file_list(ndx.modelset, svm_filename_structure)
    clean_ndx = ndx.filter(existing_models, test_sv.segset, True)
    score = Scores()
    score.scoremat = numpy.zeros(clean_ndx.trialmask.shape)
    score.modelset = clean_ndx.modelset
    score.segset = clean_ndx.segset
    score.scoremask = clean_ndx.trialmask
    svm_scoring_singleThread(svm_filename_structure, test_sv, clean_ndx, score)
    return score
