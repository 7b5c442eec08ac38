"""Back-end normalisation of x-vectors that are on the GPU -- the device-resident form of ``StatServer``'s covariance, LDA, WCCN,
Mahalanobis and spectral-normalisation methods (``sidekit/statserver.py:797-1054, 1279-1333``).

The producers of what ``iv_scoring.cosine_scoring(wccn=)``, ``mahalanobis_scoring`` and ``two_covariance_scoring`` consume, and the two
steps the reference's PLDA recipe puts in front of ``FactorAnalyser.plda``: LDA, then spectral normalisation.  The split is
``factor_analyser``'s: everything with an utterance (N) or class (C) dimension runs on the device in float64 through the C ABI --
``sc_class_sums`` (class sums and the mean), ``sc_scatter_within`` (the class-centred, class-weighted scatter: within covariance, ``Sw``
of LDA, the WCCN matrix, the covariance of ``sphNorm``), ``sc_gemm_tn`` (total and between-class scatter), ``sc_whiten_rows`` (centre,
right-multiply, length-normalise in one pass) -- and the ``D x D`` algebra (``eigh``, ``inv``, ``cholesky``) stays on the host.  The
reference runs one Python pass over all model ids per class for each of these; here the labels are grouped once (``ClassIndex``).
x-vectors are read as float32 or float64 and widened in the load; nothing with an N dimension is copied to the host.  Results are small
float64 numpy arrays, or device tensors for anything with an N dimension.  There is no CPU fallback.
"""
import functools

import numpy
import scipy.linalg

from . import _lib, statserver
from .factor_analyser import ClassIndex, _f64, _ptr, _rows, _stream, _torch, class_sums_device, gemm_tn_device


def _index(torch, class_index):
    if isinstance(class_index, ClassIndex):
        return class_index
    if torch.is_tensor(class_index):
        class_index = class_index.cpu().numpy()
    return ClassIndex(class_index)


def scatter_within_device(xv, cls, class_means, weights=None):
    """``G = sum_k w[cls[k]] (x_k - Mc[cls[k]])' (x_k - Mc[cls[k]])`` (``sc_scatter_within``): ``xv`` (N, D) CUDA tensor, float32 or
    float64; ``cls`` (N,) class number per row; ``class_means`` (C, D); ``weights`` (C,) or None.  Returns the (D, D) float64 device
    tensor.  Rows whose class number is outside ``[0, C)`` are skipped."""
    torch = _torch()
    x, dt = _rows(torch, xv)
    dev = x.device
    cls = torch.as_tensor(cls).to(device=dev, dtype=torch.int32).contiguous()
    Mc = _f64(torch, class_means, dev)
    w = None if weights is None else _f64(torch, weights, dev)
    assert cls.shape == (x.shape[0],), "one class number per row"
    assert Mc.dim() == 2 and Mc.shape[1] == x.shape[1], "class means: (C, D)"
    assert w is None or w.shape == (Mc.shape[0],), "one weight per class"
    G = torch.empty((x.shape[1], x.shape[1]), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_scatter_within(x.data_ptr(), dt, x.shape[0], x.shape[1], cls.data_ptr(), Mc.data_ptr(), _ptr(w), Mc.shape[0],
                                                G.data_ptr(), _stream(torch, dev)))
    return G


def whiten_rows_device(xv, mu, R, normalize=False, out_dtype=None):
    """``Y[i] = f((xv[i] - mu) . R)`` with ``f`` the identity or ``v / max(|v|, 1e-8)`` (``sc_whiten_rows``): ``xv`` (N, D) CUDA tensor,
    float32 or float64; ``mu`` (D,) or None; ``R`` (D, P).  Returns a new (N, P) device tensor of ``out_dtype`` (``torch.float64``, the
    default, or ``torch.float32``: the float64 result rounded once)."""
    torch = _torch()
    x, dt = _rows(torch, xv)
    dev = x.device
    out_dtype = torch.float64 if out_dtype is None else out_dtype
    assert out_dtype in (torch.float32, torch.float64), "out_dtype: torch.float32 or torch.float64"
    R = _f64(torch, R, dev)
    mu = None if mu is None else _f64(torch, mu, dev)
    assert R.dim() == 2 and R.shape[0] == x.shape[1], "R: (D, P)"
    assert mu is None or mu.shape == (x.shape[1],), "mu: (D,)"
    Y = torch.empty((x.shape[0], R.shape[1]), dtype=out_dtype, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().sc_whiten_rows(x.data_ptr(), dt, x.shape[0], x.shape[1], _ptr(mu), R.data_ptr(), R.shape[1], int(bool(normalize)),
                                             Y.data_ptr(), _lib.XT_F32 if out_dtype == torch.float32 else _lib.XT_F64, _stream(torch, dev)))
    return Y


class _Moments:
    """Mean (host) and, when asked for, class means and ``cls`` (device) of resident rows: what every function below starts from."""

    def __init__(self, torch, xv, index):
        assert index.rows.shape[0] == xv.shape[0], "one class label per row"
        self._torch, self._index, self._device = torch, index, xv.device
        self.N = xv.shape[0]
        self.C = index.ids.shape[0]
        self._S, colsum = class_sums_device(xv, index)
        self.counts = index.counts.astype(numpy.float64)
        self.mean = colsum.cpu().numpy() / self.N

    @functools.cached_property
    def class_means(self):
        return self._S / _f64(self._torch, self.counts, self._device)[:, None]

    @functools.cached_property
    def cls(self):
        return self._torch.as_tensor(self._index.inverse.astype(numpy.int32)).to(self._device)

    def within(self, xv, weights=None):
        return scatter_within_device(xv, self.cls, self.class_means, weights).cpu().numpy()

    def between(self, weights=None):
        """``sum_c w_c (m_c - mu)' (m_c - mu)`` over the class means"""
        return gemm_tn_device(self.class_means, None, weights, self.mean, self.mean).cpu().numpy()


def within_covariance_device(xv, class_index):
    """``get_within_covariance_stat1`` (:940-956): the class-centred scatter over N."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    return m.within(xv) / m.N


def between_covariance_device(xv, class_index):
    """``get_between_covariance_stat1`` (:958-978): the class means about the global mean, weighted by the session counts, over N."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    return m.between(m.counts) / m.N


def covariances_device(xv, class_index):
    """``(mean, within, between, total)`` of ``get_mean_stat1`` and the three ``get_*_covariance_stat1`` (:920-978), each over N."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    total = gemm_tn_device(xv, None, None, m.mean, m.mean).cpu().numpy() / m.N
    return m.mean, m.within(xv) / m.N, m.between(m.counts) / m.N, total


def lda_device(xv, class_index, rank):
    """``get_lda_matrix_stat1`` (:980-1019) -> ``L`` (D, rank), columns by descending eigenvalue.  As in the reference ``Sb`` is the
    unweighted outer product of the centred class means, ``Sw`` weights each class by ``1 / n_c``, and the eigenvectors are what
    ``scipy.linalg.eigh`` returns for ``(Sb . inv(Sw))'`` -- a matrix that is not symmetric, of which LAPACK reads the lower triangle."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    assert 0 < rank <= xv.shape[1], "rank must be in [1, D]"
    Sw = m.within(xv, 1.0 / m.counts)
    Sb = m.between()
    discrimination = numpy.dot(Sb, scipy.linalg.inv(Sw)).transpose()
    eigen_values, eigen_vectors = scipy.linalg.eigh(discrimination)
    idx = eigen_values.real.argsort()[-rank:][::-1]
    return eigen_vectors.real[:, idx]


def wccn_device(xv, class_index):
    """``get_wccn_choleski_stat1`` (:1031-1054): the lower Cholesky factor of the inverse of ``(1 / C) sum_c cov_c``."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    wccn = m.within(xv, 1.0 / m.counts) / m.C
    return scipy.linalg.cholesky(scipy.linalg.inv(wccn)).T


def mahalanobis_device(xv, class_index):
    """``get_mahalanobis_matrix_stat1`` (:1021-1029): the inverse of the within-class covariance."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    return scipy.linalg.inv(m.within(xv) / m.N)


def whitening_transform(sigma):
    """The matrix ``whiten_stat1`` multiplies by (:863-878): ``1 / sqrt`` of a diagonal covariance (1-D), ``StatServer``'s own
    ``V diag(lambda^-1/2)`` of a full one."""
    sigma = numpy.asarray(sigma, dtype=numpy.float64)
    if sigma.ndim == 1:
        return numpy.diag(1 / numpy.sqrt(sigma))
    if sigma.ndim != 2:
        raise Exception('Wrong dimension of Sigma, must be 1 or 2')
    return statserver.whitening_transform(sigma)


def spectral_norm_estimate_device(xv, class_index=None, it=1, mode='efr'):
    """``estimate_spectral_norm_stat1`` (:1279-1315) -> ``(means, covs, transformed)``: the reference's two lists and the rows after the
    ``it`` iterations of centre, whiten, length-normalise, as an (N, D) float64 device tensor (the reference discards its copy).
    ``mode='efr'`` whitens by the total covariance (``class_index`` may be None), ``'sphNorm'`` by the within-class one.  ``xv`` is not
    modified."""
    torch = _torch()
    assert mode in ('efr', 'sphNorm'), "mode: 'efr' or 'sphNorm'"
    assert mode == 'efr' or class_index is not None, "sphNorm needs the class labels"
    index = _index(torch, numpy.zeros(xv.shape[0], dtype=numpy.int32) if class_index is None else class_index)
    means, covs, cur = [], [], xv
    for _ in range(it):
        m = _Moments(torch, cur, index)
        means.append(m.mean)
        if mode == 'efr':
            covs.append(gemm_tn_device(cur, None, None, m.mean, m.mean).cpu().numpy() / m.N)
        else:
            covs.append(m.within(cur) / m.N)
        cur = whiten_rows_device(cur, means[-1], whitening_transform(covs[-1]), True)
    if cur is xv:
        cur = xv.to(torch.float64, copy=True)
    return means, covs, cur


def spectral_norm_apply_device(xv, spectral_norm_mean, spectral_norm_cov, is_sqr_inv_sigma=False, out_dtype=None):
    """``spectral_norm_stat1`` (:1317-1333): for each ``(mu, cov)`` centre, whiten (by ``cov`` itself when ``is_sqr_inv_sigma``),
    length-normalise.  Returns a new device tensor of ``out_dtype`` (float64 by default); intermediate iterations are float64."""
    torch = _torch()
    assert len(spectral_norm_mean) == len(spectral_norm_cov), 'Number of mean vectors and covariance matrices is different'
    out_dtype = torch.float64 if out_dtype is None else out_dtype
    cur, last = xv, len(spectral_norm_mean) - 1
    for i, (mu, cov) in enumerate(zip(spectral_norm_mean, spectral_norm_cov)):
        R = numpy.asarray(cov, dtype=numpy.float64) if is_sqr_inv_sigma and numpy.ndim(cov) == 2 else whitening_transform(cov)
        cur = whiten_rows_device(cur, mu, R, True, out_dtype if i == last else torch.float64)
    if cur is xv:
        cur = xv.to(out_dtype, copy=True)
    return cur
