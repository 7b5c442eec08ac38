"""PLDA training -- mirror of ``sidekit/factor_analyser.py``: ``FactorAnalyser`` with ``plda`` (:830-932), ``write`` / ``read``
(:265-324), and ``plda_device`` for x-vectors that are already on the GPU.

The producer of the ``(mean, F, Sigma)`` that ``iv_scoring.fast_PLDA_scoring`` consumes.  The split is the scoring side's: everything
with an utterance (N) or class (C) dimension runs on the device in float64 through the C ABI -- ``sc_class_sums`` (the sums
``StatServer.sum_stat_per_model`` forms with one Python pass over all model ids per class), ``sc_gemm_tn`` (total scatter and the
EM accumulators, f64 MFMA with fixed-order split-K), ``sc_dgemm_nn`` (whitening and the E-step) -- and the ``D x D`` / ``rank x rank``
algebra (``eigh``, ``solve``, ``cholesky``, one ``inv``) stays on the host.  x-vectors are read as float32 or float64 and widened in the
load: there is no float64 copy of the corpus and, in ``plda_device``, no host copy either.

The E-step is restated.  The reference inverts ``I + n F'F`` once per distinct session count (``fa_model_loop``, :188-205); with
``F_w'F_w = U diag(a) U'`` from one host ``eigh`` the posterior mean of class ``i`` is ``E_h[i] = ((F_w' s_i) U / (1 + n_i a)) U'``,
so the device forms ``Q = (S_w F_w U) / (1 + n a')`` in one GEMM with a per-element scale, the accumulators ``Q'Q``, ``Q' diag(n) Q``,
``Q' S_w`` are rotated back by ``U`` on the host, and the two sums of inverses become ``U diag(sum_i 1 / (1 + n_i a)) U'`` and
``U diag(sum_i n_i / (1 + n_i a)) U'``.  ``F`` is defined up to the sign of each column (the eigenvectors that initialise it have none).
There is no CPU fallback for training; importing the module, ``write`` and ``read`` work on any host.
"""
import ctypes
import logging
import os

import numpy
import scipy.linalg

from . import _lib, hdf5_lite
from .statserver import STAT_TYPE, StatServer

SLICE_ROWS = 256   # rows one workgroup of the class-sum kernel adds; longer classes are cut into slices joined in order


class ClassIndex:
    """The class index of N rows as the CSR ``sc_class_sums`` takes (host arrays): ``ids`` = sorted unique labels, ``inverse`` = class
    number per row, ``counts`` = rows per class, ``rows`` = row numbers grouped by class (ascending inside a class), ``slice_off`` /
    ``class_slice_off`` = the cut of ``rows`` into slices of at most ``SLICE_ROWS`` that never straddle a class."""

    def __init__(self, class_index):
        labels = numpy.asarray(class_index)
        assert labels.ndim == 1 and labels.shape[0] > 0, "one class label per row"
        self.ids, self.inverse = numpy.unique(labels, return_inverse=True)
        n_classes = self.ids.shape[0]
        self.counts = numpy.bincount(self.inverse, minlength=n_classes)
        self.rows = numpy.argsort(self.inverse, kind="stable").astype(numpy.int32)
        class_off = numpy.concatenate(([0], numpy.cumsum(self.counts)))
        slices = (self.counts + SLICE_ROWS - 1) // SLICE_ROWS
        self.class_slice_off = numpy.concatenate(([0], numpy.cumsum(slices))).astype(numpy.int32)
        owner = numpy.repeat(numpy.arange(n_classes), slices)
        within = numpy.arange(owner.shape[0]) - self.class_slice_off[owner]
        self.slice_off = numpy.concatenate((class_off[owner] + within * SLICE_ROWS, [labels.shape[0]])).astype(numpy.int32)


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sidekit_amd.factor_analyser trains on the GPU only (no CPU fallback) and no GPU is visible")
    return torch


def _stream(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _f64(torch, x, device):
    """host array or tensor -> contiguous float64 tensor on `device`"""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(numpy.ascontiguousarray(x, dtype=numpy.float64)).to(device)


def _rows(torch, x):
    """(N, D) CUDA tensor, float32 or float64, used where it is"""
    assert torch.is_tensor(x) and x.is_cuda and x.dim() == 2, "expected an (N, D) CUDA tensor"
    assert x.dtype in (torch.float32, torch.float64), "x-vectors must be float32 or float64"
    return x.contiguous(), (_lib.XT_F32 if x.dtype == torch.float32 else _lib.XT_F64)


def _ptr(t):
    return None if t is None else t.data_ptr()


def class_sums_device(xv, index):
    """Per-class sums of the rows of ``xv`` ((N, D) CUDA tensor, float32 or float64): ``index`` is a ``ClassIndex`` (or the labels).
    Returns ``(S, colsum)``, float64 device tensors (C, D) and (D,); ``colsum / N`` is the mean."""
    torch = _torch()
    index = index if isinstance(index, ClassIndex) else ClassIndex(index)
    x, dt = _rows(torch, xv)
    N, D = x.shape
    assert index.rows.shape[0] == N, "one class label per row"
    dev = x.device
    rows, soff, coff = (torch.as_tensor(a).to(dev) for a in (index.rows, index.slice_off, index.class_slice_off))
    C = index.ids.shape[0]
    S = torch.empty((C, D), dtype=torch.float64, device=dev)
    colsum = torch.empty(D, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_class_sums(x.data_ptr(), dt, N, D, rows.data_ptr(), soff.data_ptr(), soff.shape[0] - 1, coff.data_ptr(), C,
                                            S.data_ptr(), colsum.data_ptr(), _stream(torch, dev)))
    return S, colsum


def gemm_tn_device(A, B=None, w=None, a=None, b=None):
    """``G = sum_k w[k] (A[k] - a)' (B[k] - b)``: A (K, M) and B (K, Nn) CUDA tensors of one dtype (float32 or float64; ``B=None``: A),
    ``w`` (K,), ``a`` (M,), ``b`` (Nn,) optional float64.  Returns the (M, Nn) float64 device tensor."""
    torch = _torch()
    A, dt = _rows(torch, A)
    B = A if B is None else _rows(torch, B)[0]
    assert B.dtype == A.dtype and B.shape[0] == A.shape[0] and B.device == A.device, "A and B: same dtype, rows and device"
    dev = A.device
    w, a, b = (None if v is None else _f64(torch, v, dev) for v in (w, a, b))
    assert w is None or w.shape == (A.shape[0],)
    assert a is None or a.shape == (A.shape[1],)
    assert b is None or b.shape == (B.shape[1],)
    G = torch.empty((A.shape[1], B.shape[1]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_gemm_tn(A.data_ptr(), B.data_ptr(), dt, A.shape[0], A.shape[1], B.shape[1], _ptr(w), _ptr(a), _ptr(b),
                                         G.data_ptr(), _stream(torch, dev)))
    return G


def dgemm_nn_device(A, B, alpha=1., rowv=None, colv=None, epilogue=_lib.SC_EPI_RANK1):
    """``alpha * A . B`` (float64, A on the device) with ``- rowv colv'`` (``SC_EPI_RANK1``) or ``/ (1 + rowv colv')`` (``SC_EPI_POSTERIOR``)."""
    torch = _torch()
    dev = A.device
    A, B = _f64(torch, A, dev), _f64(torch, B, dev)
    assert A.shape[1] == B.shape[0]
    rowv, colv = (None if v is None else _f64(torch, v, dev) for v in (rowv, colv))
    assert rowv is None or (rowv.shape == (A.shape[0],) and colv.shape == (B.shape[1],))
    C = torch.empty((A.shape[0], B.shape[1]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_dgemm_nn(A.data_ptr(), B.data_ptr(), A.shape[0], B.shape[1], A.shape[1], float(alpha), _ptr(rowv), _ptr(colv),
                                          int(epilogue), C.data_ptr(), _stream(torch, dev)))
    return C


def _em(xv, index, rank_f, nb_iter, scaling_factor, stat0_sums=None, after_iteration=None):
    """The EM of ``FactorAnalyser.plda`` on device-resident rows.  ``stat0_sums``: per-class sums of the zero-order statistics (the
    session counts when None, as for x-vectors).  ``after_iteration(it, mean, F, Sigma)`` is called after every iteration."""
    torch = _torch()
    N, D = xv.shape
    assert 0 < rank_f <= D, "rank_f must be in [1, D]"
    dev = xv.device
    C = index.ids.shape[0]
    S, colsum = class_sums_device(xv, index)
    mean = colsum.cpu().numpy() / N
    mean_d = _f64(torch, mean, dev)
    sigma_obs = gemm_tn_device(xv, None, None, mean_d, mean_d).cpu().numpy() / N          # get_total_covariance_stat1
    sessions = index.counts.astype(STAT_TYPE) * scaling_factor                            # session_per_model (:863)
    n = sessions if stat0_sums is None else numpy.asarray(stat0_sums, dtype=STAT_TYPE) * scaling_factor   # model stat0 (:861)
    n_d = _f64(torch, n, dev)
    evals, evecs = scipy.linalg.eigh(sigma_obs)
    F = evecs.real[:, numpy.argsort(evals)[::-1][:rank_f]]
    Sigma = sigma_obs.copy()
    for it in range(nb_iter):
        logging.info('Estimate between class covariance, it %d / %d', it + 1, nb_iter)
        lam, vec = scipy.linalg.eigh(Sigma)
        order = lam.real.argsort()[::-1]
        W = vec.real[:, order] * (1 / numpy.sqrt(lam.real[order]))                        # sqr_inv_sigma (:886-891)
        # whitened, centred class sums (S - n mu') W = scaling * S_raw W - n (mu' W)
        Sw = dgemm_nn_device(S, W, scaling_factor, n_d, mean.dot(W), _lib.SC_EPI_RANK1)
        Fw = W.T.dot(F)
        a, U = numpy.linalg.eigh(Fw.T.dot(Fw))
        Q = dgemm_nn_device(Sw, Fw.dot(U), 1., n_d, a, _lib.SC_EPI_POSTERIOR)             # E_h U: posterior means in the eigenbasis
        QQ, QnQ, QS = gemm_tn_device(Q), gemm_tn_device(Q, None, n_d), gemm_tn_device(Q, Sw)
        QQ, QnQ, QS = QQ.cpu().numpy(), QnQ.cpu().numpy(), QS.cpu().numpy()
        g = 1.0 / (1.0 + n[:, None] * a[None, :])                                         # posterior covariances, diagonal in U
        R = (U * g.sum(axis=0)).dot(U.T) + U.dot(QQ).dot(U.T)                             # sum_i E[h h']
        A = (U * (n[:, None] * g).sum(axis=0)).dot(U.T) + U.dot(QnQ).dot(U.T)             # sum_i n_i E[h h']
        Cm = U.dot(QS).dot(scipy.linalg.inv(W))
        F = scipy.linalg.solve(A, Cm).T                                                   # M-step
        Sigma = sigma_obs - F.dot(Cm) / sessions.sum()
        F = F.dot(scipy.linalg.cholesky(R / C))                                           # minimum divergence
        if after_iteration is not None:
            after_iteration(it, mean, F, Sigma)
    return mean, F, Sigma


def plda_device(xv, class_index, rank_f, nb_iter=10, scaling_factor=1.):
    """Train PLDA on x-vectors that are on the GPU: ``xv`` (N, D) CUDA tensor, float32 or float64, ``class_index`` one integer label
    per row (tensor or array).  Returns ``(mean, F, Sigma)`` as float64 numpy arrays; ``xv`` is never copied to the host."""
    torch = _torch()
    if torch.is_tensor(class_index):
        class_index = class_index.cpu().numpy()
    return _em(xv, ClassIndex(class_index), rank_f, nb_iter, scaling_factor)


class FactorAnalyser:
    """``sidekit.FactorAnalyser`` (factor_analyser.py:208-262) for PLDA: attributes ``mean, F, G, H, Sigma``."""

    def __init__(self, input_file_name=None, mean=None, F=None, G=None, H=None, Sigma=None):
        self.mean = self.F = self.G = self.H = self.Sigma = None
        if input_file_name is not None:
            fa = FactorAnalyser.read(input_file_name)
            self.mean, self.F, self.G, self.H, self.Sigma = fa.mean, fa.F, fa.G, fa.H, fa.Sigma
        for name, value in (("mean", mean), ("F", F), ("G", G), ("H", H), ("Sigma", Sigma)):
            if value is not None:
                setattr(self, name, value)

    _DATASETS = (("mean", "fa/mean"), ("F", "fa/f"), ("G", "fa/g"), ("H", "fa/h"), ("Sigma", "fa/sigma"))

    def write(self, output_file_name):
        """The reference's layout (:265-300): ``fa/mean, fa/f, fa/g, fa/h, fa/sigma`` for the fields that are set, ``fa/kind`` = int16[5]
        flags of which ones are."""
        folder = os.path.dirname(output_file_name)
        if folder:
            os.makedirs(folder, exist_ok=True)
        w = hdf5_lite.Writer()
        kind = numpy.zeros(5, dtype="int16")
        for i, (name, path) in enumerate(self._DATASETS):
            value = getattr(self, name)
            if value is not None:
                kind[i] = 1
                w[path] = numpy.asarray(value)
        w["fa/kind"] = kind
        w.save(output_file_name)

    @staticmethod
    def read(input_filename):
        fa = FactorAnalyser()
        with hdf5_lite.File(input_filename) as fh:
            kind = fh["fa/kind"][()]
            for i, (name, path) in enumerate(FactorAnalyser._DATASETS):
                if kind[i] != 0:
                    setattr(fa, name, fh[path][()])
        return fa

    def plda(self, stat_server, rank_f, nb_iter=10, scaling_factor=1., output_file_name=None, save_partial=False, save_final=True,
             num_thread=1):
        """Simplified PLDA (no within-class sub-space, full residual covariance), factor_analyser.py:830-932: classes are
        ``numpy.unique(stat_server.modelset)``, the statistics are scaled by ``scaling_factor``, ``F`` starts from the top ``rank_f``
        eigenvectors of the total covariance.  ``stat1`` is uploaded once; the rest is ``plda_device``'s code.  ``num_thread`` is
        accepted and ignored.  Saves ``<output_file_name>_it-<k>.h5`` / ``<output_file_name>.h5`` when the reference does."""
        torch = _torch()
        assert stat_server.stat0.shape[1] == 1, "PLDA training takes one zero-order statistic per session (x-vectors / i-vectors)"
        index = ClassIndex(stat_server.modelset)
        stat0_sums = numpy.bincount(index.inverse, weights=stat_server.stat0[:, 0], minlength=index.ids.shape[0])
        xv = torch.as_tensor(numpy.ascontiguousarray(stat_server.stat1, dtype=STAT_TYPE)).to(torch.device("cuda", torch.cuda.current_device()))
        if output_file_name is None:
            output_file_name = "plda"

        def save(it, mean, F, Sigma):
            self.mean, self.F, self.Sigma = mean, F, Sigma
            if save_partial and it < nb_iter - 1:
                self.write(output_file_name + "_it-{}.h5".format(it))
            elif it == nb_iter - 1 and save_final:
                self.write(output_file_name + ".h5")

        self.mean, self.F, self.Sigma = _em(xv, index, rank_f, nb_iter, scaling_factor, stat0_sums, save)
