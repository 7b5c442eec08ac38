"""GMM-supervector SVM training -- mirror of ``sidekit/svm_training.py``: ``svm_training`` and ``svm_training_singleThread`` (:49-131),
one two-class linear SVM per speaker, the speaker's supervectors against a set of background supervectors.

The reference trains one libsvm problem per speaker, one after the other, each built as a Python list of ``(B + msn) x (B + msn + 1)``
floats.  All those problems share the ``B x B`` background block of the Gram matrix and differ in a few rows.  Here the Gram blocks are
float64 GEMMs on the device, every model's dual is solved by one workgroup of one launch (``sc_svm_train``,
``include/sidekit_amd/svm.h``: libsvm's C-SVC solver without shrinking, float64), and the weights of all models are one more GEMM.
``svm_train_device`` works on resident supervectors.  There is no CPU fallback; importing the module needs neither a GPU nor torch.

One departure from the reference, on purpose.  It pads every problem to ``msn`` target rows (the largest session count), which leaves
all-zero kernel rows labelled as targets and stale columns of the previous model in the problems of speakers with fewer sessions, and then
indexes the support vectors into a matrix without those rows: its result is defined only when every speaker has ``msn`` sessions.  Here
each model is solved on its own ``B + csn`` points.  The two are identical when all session counts are equal (DESIGN.md section 4,
"SVM back end").
"""
import logging
import os

import numpy

from . import _lib, sv_utils
from .statserver import StatServer

MAX_N = _lib.SC_SVM_MAX_N   # SC_SVM_MAX_N (include/sidekit_amd/svm.h): background rows plus a model's own, of one problem
EPS = 1e-3          # libsvm's default stopping tolerance (the reference passes none): what svm_training trains with
MAX_ITER = 100000   # the updates a model may make in svm_training


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.svm_training computes on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _rows(torch, a, dev=None):
    """A host array or a tensor -> ((N, D) contiguous float64 tensor on the device, whether it came from the host)"""
    host = not torch.is_tensor(a)
    if host:
        a = torch.as_tensor(numpy.array(a, dtype=numpy.float64, order='C'))
    if dev is None:
        dev = a.device if a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a = a.to(device=dev, dtype=torch.float64).contiguous()
    assert a.dim() == 2 and a.shape[0] > 0 and a.shape[1] > 0, "supervectors: (N, D), N > 0"
    return a, host


def _groups(model_of, M):
    """``model_of`` (one model number per enrolment row) -> the rows sorted by model (a model's rows keep their order), the M + 1 row
    offsets and the session counts"""
    model_of = numpy.asarray(model_of)
    assert model_of.ndim == 1 and model_of.shape[0] > 0 and numpy.issubdtype(model_of.dtype, numpy.integer), "model_of: one model number per enrolment row"
    assert model_of.min() >= 0 and model_of.max() < M, "model_of: model numbers in [0, M)"
    counts = numpy.bincount(model_of, minlength=M)
    assert counts.min() >= 1, "every model needs at least one enrolment row"
    return numpy.argsort(model_of, kind="stable"), numpy.concatenate(([0], numpy.cumsum(counts))), counts


def svm_solve_device(k_bb, k_eb, k_ee, en_off, ee_off, c, eps=1e-3, max_iter=100000):
    """``sc_svm_train`` on resident Gram blocks: ``k_bb`` (B, B), ``k_eb`` (Ne, B), ``k_ee`` the packed per-model target blocks (1-D),
    float64 CUDA tensors; ``en_off`` (M + 1 row offsets) and ``ee_off`` (M block offsets), host integers; ``c`` (M,) float64 CUDA tensor.
    Returns ``(coef (M, B + max csn), rho (M,), iterations (M,) int32, gap (M,), status (M,) int32)`` on the device; row ``m`` of
    ``coef`` holds ``B + csn_m`` values, zeros behind them.  A problem of more than ``MAX_N`` points raises ``ValueError`` before
    anything is launched."""
    torch = _torch()
    dev = k_bb.device
    en_off = numpy.asarray(en_off, dtype=numpy.int64)
    ee_off = numpy.asarray(ee_off, dtype=numpy.int64)
    B, Ne, M = k_bb.shape[0], k_eb.shape[0], en_off.shape[0] - 1
    counts = numpy.diff(en_off)
    assert k_bb.shape == (B, B) and k_eb.shape == (Ne, B) and k_ee.dim() == 1, "Gram blocks: (B, B), (Ne, B) and the packed target blocks"
    assert all(t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() for t in (k_bb, k_eb, k_ee, c)), "contiguous float64 CUDA tensors"
    assert M >= 1 and ee_off.shape == (M,) and c.shape == (M,), "one block offset and one cost per model"
    assert en_off[0] >= 0 and en_off[-1] <= Ne and counts.min() >= 1, "en_off: ascending row offsets within the rows of k_eb, a row at least per model"
    assert ee_off.min() >= 0 and (ee_off + counts * counts).max() <= k_ee.shape[0], "ee_off: blocks inside k_ee"
    max_csn = int(counts.max())
    if B + max_csn > MAX_N:
        raise ValueError(f"a problem of {B} background rows and {max_csn} of its own has more than {MAX_N} points: it does not fit the LDS "
                         f"of one workgroup and is never split (SC_SVM_MAX_N, include/sidekit_amd/svm.h)")
    assert Ne < 2 ** 31 and M < 2 ** 31
    coef = torch.zeros((M, B + max_csn), dtype=torch.float64, device=dev)
    rho, gap = torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.float64, device=dev)
    iters, status = torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev)
    d_en = torch.as_tensor(en_off.astype(numpy.int32)).to(dev)
    d_ee = torch.as_tensor(ee_off).to(dev)
    _lib.launch("sc_svm_train", dev, k_bb, B, k_eb, Ne, k_ee, k_ee.shape[0], d_en, d_ee, M, max_csn, c, float(eps), int(max_iter),
                coef, rho, iters, gap, status)
    return coef, rho, iters, gap, status


def svm_train_device(background, enroll, model_of, c=None, eps=1e-3, max_iter=100000):
    """One linear SVM per model: ``background`` (B, D) and ``enroll`` (Ne, D) supervectors, CUDA tensors or host arrays (float64 on the
    device); ``model_of`` (Ne,) the model number in ``[0, M)`` of every enrolment row, every model with a row at least.  Model ``m``'s
    problem is the background rows (libsvm's positive class) against its own rows, in the order they have in ``enroll``.  ``c``: the cost,
    a number or one per model; ``None``: the reference's ``1 / mean(diag(gram))`` of that model's own Gram matrix.  ``eps``: libsvm's
    stopping tolerance; a model that makes ``max_iter`` updates without reaching it logs a warning and returns what it has, as libsvm
    does.

    Returns ``(W (M, D), b (M,), info)``: the score of a test vector ``x`` is ``W[m] . x + b[m]``.  ``info``: ``iterations``, ``gap``,
    ``status`` (``SC_SVM_CONVERGED`` / ``SC_SVM_MAX_ITER``), ``c`` and ``n`` (points) per model, and ``coef`` (M, B + max csn), row ``m``:
    ``a y`` of model ``m``'s ``n[m]`` points.  Tensors on the device when the supervectors were there, host arrays otherwise.
    The Gram blocks are float64 GEMMs; ``W = -(coef[:, :B] . background + the models' own rows weighted by their coefficients)``."""
    return _train(background, enroll, model_of, c, eps, max_iter, None)


def _train(background, enroll, model_of, c, eps, max_iter, k_bb):
    """``svm_train_device``; ``k_bb``: the background's Gram matrix when the caller holds it already, or ``None``"""
    torch = _torch()
    bg, host = _rows(torch, background)
    dev = bg.device
    en, _ = _rows(torch, enroll, dev)
    B, D = bg.shape
    assert en.shape[1] == D, "background and enrolment supervectors differ in dimension: {:d} / {:d}".format(D, en.shape[1])
    model_of = numpy.asarray(model_of)
    assert model_of.shape == (en.shape[0],), "model_of: one model number per enrolment row"
    M = int(model_of.max()) + 1
    order, en_off, counts = _groups(model_of, M)
    max_csn = int(counts.max())
    if B + max_csn > MAX_N:   # before the Gram GEMMs
        raise ValueError(f"a problem of {B} background rows and {max_csn} of its own has more than {MAX_N} points: it does not fit the LDS "
                         f"of one workgroup and is never split (SC_SVM_MAX_N, include/sidekit_amd/svm.h)")
    en = en[torch.as_tensor(order).to(dev)].contiguous()
    if k_bb is None:
        k_bb = torch.matmul(bg, bg.t())
    else:
        k_bb, _ = _rows(torch, k_bb, dev)
        assert k_bb.shape == (B, B), "k_bb: the background's (B, B) Gram matrix"
    k_eb = torch.matmul(en, bg.t()).contiguous()
    # the models' own blocks, the models of one session count together: one batched GEMM per count (a row's squared length at count 1,
    # where a batch of 1 x 1 products is 10 ms for 1 024 models)
    ee_off = numpy.zeros(M, dtype=numpy.int64)
    blocks, diag_ee, at = [], torch.empty(en.shape[0], dtype=torch.float64, device=dev), 0
    by_count = []
    for csn in (int(v) for v in numpy.unique(counts)):
        ms = numpy.flatnonzero(counts == csn)
        rows = torch.as_tensor((en_off[ms][:, None] + numpy.arange(csn)[None, :]).reshape(-1)).to(dev)
        e = en[rows].reshape(len(ms), csn, D)
        blk = (e * e).sum(dim=2, keepdim=True) if csn == 1 else torch.bmm(e, e.transpose(1, 2))
        diag_ee[rows] = torch.diagonal(blk, dim1=1, dim2=2).reshape(-1)
        ee_off[ms] = at + numpy.arange(len(ms)) * csn * csn
        at += len(ms) * csn * csn
        blocks.append(blk.reshape(-1))
        by_count.append((torch.as_tensor(ms).to(dev), e, csn))
    k_ee = torch.cat(blocks).contiguous()
    if c is None:   # 1 / mean(diag) of the model's own Gram matrix: the background's trace once, the model's own added to it
        trace_bb, d_ee = float(torch.diagonal(k_bb).sum()), diag_ee.cpu().numpy()
        cost = (B + counts) / (trace_bb + numpy.add.reduceat(d_ee, en_off[:-1]))
    else:
        cost = numpy.broadcast_to(numpy.asarray(c, dtype=numpy.float64), (M,)).copy()
    d_c = torch.as_tensor(cost).to(dev)
    coef, rho, iters, gap, status = svm_solve_device(k_bb, k_eb, k_ee, en_off, ee_off, d_c, eps, max_iter)
    h_status = status.cpu().numpy()
    if numpy.any(h_status == _lib.SC_SVM_BAD_OFFSETS):
        raise RuntimeError("sc_svm_train refused the offsets of a model")
    for m in numpy.flatnonzero(h_status == _lib.SC_SVM_MAX_ITER):
        logging.warning('SVM model %d: reaching max number of iterations (%d), gap %g', m, max_iter, float(gap[m]))
    W = torch.matmul(coef[:, :B], bg)
    for d_ms, e, csn in by_count:   # a model's own rows: a sum over its sessions in row order
        own = coef[d_ms, B:B + csn]
        W[d_ms] += own[:, 0:1] * e[:, 0, :] if csn == 1 else (own[:, :, None] * e).sum(dim=1)
    W = -W
    info = {"iterations": iters, "gap": gap, "status": status, "c": d_c, "n": torch.as_tensor(B + counts).to(dev), "coef": coef}
    if host:
        return W.cpu().numpy(), rho.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
    return W, rho, info


def svm_training_singleThread(K, msn, bsn, svm_dir, background_sv, models, enroll_sv):
    """Train the SVMs of ``models`` (ids of ``enroll_sv.modelset``) against the supervectors of ``background_sv`` and write
    ``<svm_dir>/<model>.svm`` for each (:49-94).  ``K``: the background's Gram matrix (``background_sv.precompute_svm_kernel_stat1()``),
    ``bsn`` its size, ``msn`` the largest session count: accepted as the reference passes them; a problem is not padded to ``msn``
    (see the module's note).  The reference's cost, ``1 / mean(diag(gram))``, and libsvm's default tolerance (``EPS``)."""
    assert isinstance(background_sv, StatServer) and isinstance(enroll_sv, StatServer), 'background_sv and enroll_sv have to be StatServers'
    K = numpy.asarray(K)
    assert K.shape == (bsn, bsn) and bsn == background_sv.stat1.shape[0], "K: the Gram matrix of the background supervectors"
    models = numpy.asarray(models)
    if models.shape[0] == 0:
        return
    number = {name: i for i, name in enumerate(models)}
    assert len(number) == models.shape[0], "a model is listed twice"
    keep = numpy.array([name in number for name in enroll_sv.modelset], dtype=bool)
    model_of = numpy.array([number[name] for name in enroll_sv.modelset[keep]], dtype=numpy.int64)
    missing = sorted(set(number) - set(enroll_sv.modelset[keep]))
    assert not missing, "models without a session in enroll_sv: {}".format(missing)
    assert numpy.bincount(model_of).max() <= msn, "a model has more than msn sessions"
    for name in models:
        logging.info('Train SVM model for %s', name)
    W, b, _ = _train(background_sv.stat1, enroll_sv.stat1[keep], model_of, None, EPS, MAX_ITER, K)
    for i, name in enumerate(models):
        sv_utils.save_svm(os.path.join(svm_dir, name + '.svm'), W[i], b[i])


def svm_training(svmDir, background_sv, enroll_sv, num_thread=1):
    """One SVM per unique model of ``enroll_sv`` against all the supervectors of ``background_sv``, written to
    ``<svmDir>/<model>.svm`` (:97-131).  All models are one launch; ``num_thread`` is accepted and unused."""
    assert isinstance(background_sv, StatServer), 'Second parameter has to be a StatServer'
    assert isinstance(enroll_sv, StatServer), 'Third parameter has to be a StatServer'
    K = background_sv.precompute_svm_kernel_stat1()
    names = enroll_sv.modelset.tolist()
    msn = max(numpy.unique(names, return_counts=True)[1])
    svm_training_singleThread(K, msn, K.shape[0], svmDir, background_sv, numpy.unique(enroll_sv.modelset), enroll_sv)
