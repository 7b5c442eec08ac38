"""Gaussian back-end -- mirror of ``sidekit/lid_utils.py``: closed-set identification of x-vectors.  Which of C known classes (a
language, a speaker of a closed set, a channel, a corpus) produced a vector: ``gaussian_backend_train`` (:75-91, one tied covariance),
``gaussian_backend_train_hetero`` (:94-130, one covariance per class, smoothed towards the pooled one), ``gaussian_backend_test`` /
``gaussian_backend_test_hetero`` (:149-263, the ``modelset x segset`` log-likelihoods) and ``compute_log_likelihood_ratio`` (:57-72, the
calibrated closed-set LLRs).

The split is ``backend``'s: everything with an utterance (N) or class (C) dimension runs on the device in float64 through the C ABI --
``sc_class_sums`` and ``sc_scatter_within`` (class means, the tied covariance), ``sc_class_scatter`` (the C per-class scatters in one
call), ``sc_plda_fast`` (the tied log-likelihoods: ``cst - 0.5 (x - m)' P (x - m)`` is its form with ``Phi = -P``, ``Psi = P``, as in
``mahalanobis_scoring``), ``sc_gauss_loglik`` (the heteroscedastic ones, without an (N x D) intermediate), ``sc_closed_set_llr`` -- and
the ``D x D`` algebra (``cholesky``, ``inv``, ``slogdet``) stays on the host.  The ``*_device`` functions work on resident tensors and
copy nothing with an N dimension to the host; the reference-named ones take and return ``StatServer`` / ``Scores``.  The ``diag=True``
branches need ``Mixture`` (GMM era, out of scope) and raise.  There is no CPU fallback; importing the module needs no GPU.
"""
import numpy
import scipy.linalg

from . import _lib
from .backend import _Moments, _index
from .bosaris import Scores
from .factor_analyser import _f64, _rows, _torch, class_sums_device
from .statserver import STAT_TYPE, StatServer


def log_sum_exp(x):
    """``log(sum(exp(x), axis=0))`` about the column maxima (:47-54)"""
    top = x.max(axis=0)
    return top + numpy.log(numpy.exp(x - top).sum(axis=0))


def _check_llr_args(shape, p_tar):
    assert len(shape) == 2 and shape[0] >= 2 and shape[1] > 0, "closed-set LLRs need a (C, N) matrix with C >= 2 classes"
    assert 0.0 < p_tar < 1.0, "p_tar must be in (0, 1)"


# ---- on resident tensors --------------------------------------------------------------------------------------------------------------

def class_scatter_device(xv, class_index):
    """The per-class scatters ``S_c = sum_{k in c} (x_k - m_c)' (x_k - m_c)`` (``sc_class_scatter``): ``xv`` (N, D) CUDA tensor, float32
    or float64; ``class_index`` one label per row (or a ``ClassIndex``).  Returns ``(S, class_means)``, float64 device tensors (C, D, D)
    and (C, D), classes in sorted order.  ``S`` takes ``C D^2 8`` bytes; the rows are grouped by class through one ``index_select``."""
    torch = _torch()
    x, dt = _rows(torch, xv)
    index = _index(torch, class_index)
    N, D = x.shape
    assert index.rows.shape[0] == N, "one class label per row"
    dev = x.device
    C = index.ids.shape[0]
    sums, _ = class_sums_device(x, index)
    means = sums / _f64(torch, index.counts.astype(numpy.float64), dev)[:, None]
    grouped = x.index_select(0, torch.as_tensor(index.rows.astype(numpy.int64)).to(dev))
    offsets = torch.as_tensor(numpy.concatenate(([0], numpy.cumsum(index.counts))).astype(numpy.int32)).to(dev)
    S = torch.empty((C, D, D), dtype=torch.float64, device=dev)
    _lib.launch("sc_class_scatter", dev, grouped, dt, N, D, offsets, means, C, int(index.counts.max()), S)
    return S, means


def _constant(sigma):
    """``-0.5 (logdet Sigma + D log 2 pi)`` (:89,127)"""
    return - 0.5 * (numpy.linalg.slogdet(sigma)[1] + sigma.shape[0] * numpy.log(2 * numpy.pi))


def gaussian_backend_device(xv, class_index):
    """``gaussian_backend_train`` on resident rows -> ``(means, sigma, cst)``: the (C, D) float64 device tensor of class means (sorted
    classes), the tied within-class covariance as a (D, D) numpy array and its constant."""
    torch = _torch()
    m = _Moments(torch, xv, _index(torch, class_index))
    sigma = m.within(xv) / m.N
    return m.class_means, sigma, _constant(sigma)


def gaussian_backend_hetero_device(xv, class_index, alpha=0.1):
    """``gaussian_backend_train_hetero`` on resident rows -> ``(means, sigmas, csts)``: class means ((C, D) device tensor), the covariances
    ``alpha S_c / n_c + (1 - alpha) sum_c S_c / N`` as a (C, D, D) numpy array and their C constants.  The scatters come from one
    ``sc_class_scatter`` call; they go to the host, where the per-class Cholesky factors are taken anyway."""
    torch = _torch()
    index = _index(torch, class_index)
    S, means = class_scatter_device(xv, index)
    S = S.cpu().numpy()
    W = numpy.zeros(S.shape[1:])
    for c in range(S.shape[0]):
        W += S[c]
    W /= xv.shape[0]
    sigmas = alpha * (S / index.counts[:, None, None]) + (1 - alpha) * W
    return means, sigmas, numpy.array([_constant(s) for s in sigmas])


def _precision_factors(sigmas):
    """``W_c`` with ``inv(Sigma_c) = W_c W_c'``: ``inv(L_c)'`` of the Cholesky factor ``Sigma_c = L_c L_c'``, one factorisation per class"""
    eye = numpy.eye(sigmas.shape[1])
    return numpy.stack([scipy.linalg.solve_triangular(scipy.linalg.cholesky(s, lower=True), eye, lower=True).T for s in sigmas])


def gaussian_loglik_device(xv, means, sigma, cst):
    """The (C, N) float64 device tensor ``ll[c][n] = cst_c - 0.5 (x_n - m_c)' inv(Sigma_c) (x_n - m_c)``.  ``xv`` (N, D) CUDA tensor;
    ``means`` (C, D); ``sigma`` one (D, D) covariance with a scalar ``cst`` (the tied model: ``sc_plda_fast``) or C of them, (C, D, D) or
    a list, with C constants (``sc_gauss_loglik``)."""
    sigma = numpy.asarray(sigma, dtype=numpy.float64)
    D, C = sigma.shape[-1], numpy.shape(means)[0]
    assert sigma.ndim in (2, 3) and sigma.shape[-2] == D, "sigma: one (D, D) covariance or C of them"
    assert tuple(numpy.shape(means)) == (C, D), 'Gaussian back-end means and covariance dimension mismatch'
    assert tuple(xv.shape[1:]) == (D,) and xv.shape[0] > 0, 'I-vectors and Gaussian back-end dimension mismatch'
    if sigma.ndim == 2:
        assert numpy.ndim(cst) == 0, "one covariance comes with one constant"
        from . import iv_scoring
        P = numpy.linalg.inv(sigma)
        return iv_scoring.plda_matrix_device(means, xv, -P, P, float(cst), device=xv.device)
    cst = numpy.asarray(cst, dtype=numpy.float64)
    assert sigma.shape[0] == C and cst.shape == (C,), "one covariance and one constant per class"
    torch = _torch()
    assert torch.is_tensor(xv) and xv.is_cuda, "expected an (N, D) CUDA tensor"
    x = _f64(torch, xv, xv.device)
    dev = x.device
    out = torch.empty((C, x.shape[0]), dtype=torch.float64, device=dev)
    _lib.launch("sc_gauss_loglik", dev, x, x.shape[0], D, _f64(torch, means, dev), _f64(torch, _precision_factors(sigma), dev),
                _f64(torch, cst, dev), C, out)
    return out


def closed_set_llr_device(M, p_tar=0.5, out=None):
    """``compute_log_likelihood_ratio`` of a (C, N) float64 CUDA tensor (``sc_closed_set_llr``); ``out`` may be ``M`` itself (in place)."""
    _check_llr_args(tuple(M.shape), p_tar)
    torch = _torch()
    assert torch.is_tensor(M) and M.is_cuda and M.dtype == torch.float64 and M.is_contiguous(), "expected a contiguous (C, N) float64 CUDA tensor"
    if out is None:
        out = torch.empty_like(M)
    assert out.shape == M.shape and out.dtype == M.dtype and out.device == M.device and out.is_contiguous(), "out: a tensor like M"
    _lib.launch("sc_closed_set_llr", M.device, M, M.shape[0], M.shape[1], float(p_tar), out)
    return out


# ---- the reference's names ------------------------------------------------------------------------------------------------------------

def compute_log_likelihood_ratio(M, p_tar=0.5):
    """Closed-set log-likelihood ratios (:57-72) of a ``nb_models x nb_test_segments`` matrix of log-likelihoods, on the GPU."""
    M = numpy.ascontiguousarray(M, dtype=numpy.float64)
    _check_llr_args(M.shape, p_tar)
    torch = _torch()
    dev = torch.device("cuda", torch.cuda.current_device())
    scores = torch.as_tensor(M).to(dev)
    return closed_set_llr_device(scores, p_tar, out=scores).cpu().numpy()


def _resident(stat_server):
    assert isinstance(stat_server, StatServer), 'First parameter should be a StatServer'
    return stat_server._device_rows()


def gaussian_backend_train(train_ss):
    """One mean per class and a full tied covariance (:75-91) -> ``(gb_mean, gb_sigma, gb_cst)``: a ``StatServer``, (D, D), a float."""
    gb_sigma = train_ss.get_within_covariance_stat1()
    gb_mean = train_ss.mean_stat_per_model()
    return gb_mean, gb_sigma, _constant(gb_sigma)


def gaussian_backend_train_hetero(train_ss, alpha=0.1):
    """One mean and one covariance per class (:94-130) -> ``(gb_mean, gb_sigma, gb_cst)``: a ``StatServer``, a list of C (D, D) arrays
    and a list of C floats; ``alpha`` weighs the class's own covariance against the pooled one."""
    xv, index = _resident(train_ss)
    _, sigmas, csts = gaussian_backend_hetero_device(xv, index, alpha)
    return train_ss.mean_stat_per_model(), list(sigmas), [float(c) for c in csts]


def _gaussian_backend_train(data, label):
    """``gaussian_backend_train`` of rows and their labels (:133-146)"""
    label = numpy.asarray(label)
    return gaussian_backend_train(StatServer.from_arrays(label, label, numpy.asarray(data, dtype=STAT_TYPE)))


def _test(test_ss, params, diag, compute_llr, hetero):
    gb_mean, gb_sigma, gb_cst = params
    if diag:
        raise NotImplementedError("diag=True scores through sidekit.Mixture (GMM era), which sidekit_amd does not mirror")
    sigma = numpy.asarray(gb_sigma, dtype=numpy.float64)
    assert (sigma[0] if hetero else sigma).ndim == 2
    assert gb_mean.stat1.shape[1] == test_ss.stat1.shape[1], 'I-vectors dimension mismatch'
    assert not compute_llr or gb_mean.modelset.shape[0] >= 2, "closed-set LLRs need a (C, N) matrix with C >= 2 classes"
    xv, _ = _resident(test_ss)
    ll = gaussian_loglik_device(xv, gb_mean.stat1, sigma, numpy.asarray(gb_cst, dtype=numpy.float64) if hetero else gb_cst)
    if compute_llr:
        ll = closed_set_llr_device(ll, out=ll)
    scores = Scores()
    scores.modelset = gb_mean.modelset
    scores.segset = test_ss.segset
    scores.scoremat = ll.cpu().numpy()
    scores.scoremask = numpy.ones(scores.scoremat.shape, dtype='bool')
    assert scores.validate()
    return scores


def gaussian_backend_test(test_ss, params, diag=False, compute_llr=True):
    """Score ``test_ss`` against the tied Gaussian back-end ``params = (gb_mean, gb_sigma, gb_cst)`` (:149-202) -> ``Scores``
    (``modelset x segset``, all trials): log-likelihood ratios, or the log-likelihoods when ``compute_llr`` is false."""
    return _test(test_ss, params, diag, compute_llr, False)


def gaussian_backend_test_hetero(test_ss, params, diag=False, compute_llr=True):
    """Score ``test_ss`` against the heteroscedastic back-end of ``gaussian_backend_train_hetero`` (:205-263) -> ``Scores``."""
    return _test(test_ss, params, diag, compute_llr, True)
