"""float64 numpy restatement of the joint factor analysis of ``sidekit/statserver.py`` (``factor_analysis`` :1798-1949 with its three
estimations and ``estimate_hidden``) and of ``sidekit/jfa_scoring.py``, written from the mathematics of ``M = m + V y + U x + D z`` in the
steps the device code is cut into: the shift / centring / whitening pass (``sc_jfa_shift``), the total-variability posterior
(tests/tools/ivector_numpy.py), the accumulators, the host M-step, the MAP accumulators (``sc_jfa_map_acc``), the scores.  The tests'
reference: held to 1e-12 against what the reference's own module computed (tests/golden/jfa.npz, make_jfa_golden.py)."""
import numpy

import ivector_numpy as ivn

rel = ivn.rel


def spread(stat0, D):
    """stat0[:, index_map]: every count repeated over the D coefficients of its component"""
    return numpy.repeat(stat0, D, axis=1)


def shift(stat0, stat1, W=None, H=None, rows=None, mean=None, scale=None):
    """(stat1 - stat0 (mean + H[rows] W')) scale: rows None = the session's own row, a row outside [0, Nh) is a zero factor"""
    N, CD = stat1.shape
    offset = numpy.zeros((N, CD))
    if W is not None and W.shape[1] > 0:
        rows = numpy.arange(N) if rows is None else numpy.asarray(rows)
        ok = (rows >= 0) & (rows < H.shape[0])
        factors = numpy.zeros((N, W.shape[1]))
        factors[ok] = H[rows[ok]]
        offset = factors.dot(W.T)
    if mean is not None:
        offset = mean[None, :] + offset
    out = stat1 - spread(stat0, CD // stat0.shape[1]) * offset
    return out if scale is None else out * scale[None, :]


def map_acc(stat0, stat1, D, sigma):
    """the accumulators of one MAP E-step from per-model statistics, centred and shifted, not whitened -> (_A, _C)"""
    n = spread(stat0, stat1.shape[1] // stat0.shape[1])
    lam = 1.0 + n * D ** 2 / sigma
    e = stat1 * D / (lam * sigma)
    return ((1.0 / lam + e ** 2) * n).sum(axis=0), (e * stat1).sum(axis=0)


def model_sums(stat0, stat1, labels):
    """-> (sorted unique labels, class number per row, summed stat0, summed stat1)"""
    ids, inverse = numpy.unique(labels, return_inverse=True)
    onehot = (inverse[None, :] == numpy.arange(ids.shape[0])[:, None]).astype(numpy.float64)
    return ids, inverse, onehot.dot(stat0), onehot.dot(stat1)


def hidden(stat0, stat1, mean, sigma, V=None, U=None, D=None):
    """(y, x) jointly under W = [V U] from the centred, whitened statistics; z = f D / (1 + n D^2) on the whitened statistics less
    n (W [y x]) with W NOT whitened -> (y, x, z or None)"""
    N, CD = stat1.shape
    C = stat0.shape[1]
    V = numpy.zeros((CD, 0)) if V is None else V
    U = numpy.zeros((CD, 0)) if U is None else U
    W = numpy.hstack((V, U))
    scale = 1.0 / numpy.sqrt(sigma)
    sw = shift(stat0, stat1, mean=mean, scale=scale)
    e_h = ivn.e_step(stat0, sw, W * scale[:, None])[0] if W.shape[1] else numpy.zeros((N, 0))
    z = None
    if D is not None:
        z = shift(stat0, sw, W, e_h) * D / (1.0 + spread(stat0, CD // C) * D ** 2)
    return e_h[:, :V.shape[1]], e_h[:, V.shape[1]:], z


def batches(n, size):
    """consecutive batches of `size` sessions, as _expectation cuts them"""
    return [numpy.arange(a, min(a + size, n)) for a in range(0, n, size)]


def e_step(stat0, stat1, phi, mean, sigma, batch_size, W=None, H=None, rows=None):
    """the accumulators of one E-step over the sessions, shifted by stat0 (H[rows] W'), centred and whitened, added in batch order
    -> (_A (C, P) packed, _C (R, C D) not whitened, _R (P,) packed, not divided)"""
    scale = 1.0 / numpy.sqrt(sigma)
    phi_w = phi * scale[:, None]
    G = ivn.gram(phi_w, stat0.shape[1], stat1.shape[1] // stat0.shape[1])
    if W is not None and rows is None:
        rows = numpy.arange(stat0.shape[0])
    acc = None
    for idx in batches(stat0.shape[0], batch_size):
        sw = shift(stat0[idx], stat1[idx], W, H, None if rows is None else rows[idx], mean, scale)
        e_h, e_hh = ivn.e_step(stat0[idx], sw, phi_w, G)
        part = ivn.accumulate(stat0[idx], sw, e_h, e_hh)
        acc = part if acc is None else tuple(a + p for a, p in zip(acc, part))
    return acc[0], acc[1] / scale[None, :], acc[2]


def subspace(stat0, stat1, phi, mean, sigma, nb_iter, batch_size, min_div=True, W=None, H=None, rows=None):
    """nb_iter EM iterations of a loading matrix -> (phi, the first iteration's accumulators)"""
    first = None
    for it in range(nb_iter):
        acc = e_step(stat0, stat1, phi, mean, sigma, batch_size, W, H, rows)
        first = acc if first is None else first
        phi = ivn.m_step(*acc, stat0.shape[0], min_div)
    return phi, first


def train(stat0, stat1, labels, mean, sigma, F, G, H, it_nb, batch_size, min_div=True):
    """factor_analysis with every stage run (ranks above 0, H given) -> dict of F, G, H and the first-iteration accumulators"""
    ids, inverse, m0, m1 = model_sums(stat0, stat1, labels)
    out = {}
    F, (out["A_F"], out["C_F"], out["R_F"]) = subspace(m0, m1, F, mean, sigma, it_nb[0], batch_size, min_div)
    y = hidden(m0, m1, mean, sigma, F)[0]
    G, (out["A_G"], out["C_G"], out["R_G"]) = subspace(stat0, stat1, G, mean, sigma, it_nb[1], batch_size, min_div, F, y, inverse)
    less_speaker = shift(stat0, stat1, F, y, inverse)
    x = hidden(stat0, less_speaker, mean, sigma, None, G)[1]
    centred = shift(stat0, shift(stat0, stat1, F, y, inverse, mean), G, x)
    s1 = model_sums(stat0, centred, labels)[3]
    for it in range(it_nb[2]):
        a, c = map_acc(m0, s1, H, sigma)
        if it == 0:
            out["A_H"], out["C_H"] = a, c
        H = c / a
    out.update(F=F, G=G, H=H)
    return out


def score(ubm_mean, ubm_invcov, enroll0, enroll1, test0, test1, mean, sigma, V, U, D):
    """the channel-point-estimate linear scores (models x segments); enrolment statistics summed per model already.  Both sides are
    centred on the UBM's means and divided by the square roots of its INVERSE covariances first, as the reference does."""
    scale = 1.0 / numpy.sqrt(ubm_invcov)
    e1, t1 = shift(enroll0, enroll1, mean=ubm_mean, scale=scale), shift(test0, test1, mean=ubm_mean, scale=scale)
    y, _, z = hidden(enroll0, e1, mean, sigma, V, U, D)
    models = y.dot(V.T) + z * D
    x = hidden(test0, t1, mean, sigma, None, U)[1]
    return models.dot((shift(test0, t1, U, x) / test0.sum(axis=1)[:, None]).T)


def restated(fx):
    """every recorded output from the fixture's inputs by the numpy restatement -> dict under the fixture's names"""
    mean, sigma = fx["mu"].reshape(-1), 1.0 / fx["invcov"].reshape(-1)
    out = train(fx["stat0"], fx["stat1"], fx["speaker_of"], mean, sigma, fx["F_init"], fx["G_init"], fx["H_init"],
                tuple(int(i) for i in fx["it_nb"]), int(fx["batch_size"]))
    n_models, n = numpy.unique(fx["speaker_of"]).shape[0], fx["stat0"].shape[0]
    for tag, count in (("F", n_models), ("G", n)):   # as _expectation returns them: full matrices, _R over the number of rows
        rank = out["C_" + tag].shape[0]
        out["A_" + tag], out["R_" + tag] = ivn.unpack(out["A_" + tag], rank), ivn.unpack(out["R_" + tag], rank) / count
    V, U, Dm = out["F"], out["G"], out["H"]
    for tag, args in (("v", (V, None, None)), ("u", (None, U, None)), ("vu", (V, U, None)), ("vud", (V, U, Dm))):
        y, x, z = hidden(fx["stat0"], fx["stat1"], mean, sigma, *args)
        out.update({f"hid_{tag}_y": y, f"hid_{tag}_x": x})
        if z is not None:
            out[f"hid_{tag}_z"] = z
    ubm_mean, ubm_invcov = fx["mu"].reshape(-1), fx["invcov"].reshape(-1)
    first = numpy.array([list(fx["enroll_of"]).index(m) for m in range(4)])
    out["scores_checked"] = score(ubm_mean, ubm_invcov, fx["enroll_stat0"][first], fx["enroll_stat1"][first], fx["test_stat0"],
                                      fx["test_stat1"], mean, sigma, V, U, Dm)
    _, _, e0, e1 = model_sums(fx["enroll_stat0"], fx["enroll_stat1"], fx["enroll_of"])
    out["scores_unchecked"] = score(ubm_mean, ubm_invcov, e0, e1, fx["test_stat0"], fx["test_stat1"], mean, sigma, V, U, Dm)
    return out


RECORDED = ("F", "G", "H", "A_F", "C_F", "R_F", "A_G", "C_G", "R_G", "A_H", "C_H", "hid_v_y", "hid_v_x", "hid_u_y", "hid_u_x", "hid_vu_y",
            "hid_vu_x", "hid_vud_y", "hid_vud_x", "hid_vud_z", "scores_checked", "scores_unchecked")
