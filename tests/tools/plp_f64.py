"""The PLP front end restated for the tests (csrc/plp.hip, sidekit_amd/plp.py): the four configurations and the rows of
tests/golden/plp.npz (the signals of tests/tools/mfcc_f64.py, regenerated from stored seeds), the float64 evaluation of the formulas of
include/sidekit_amd/plp.h on given operands in the kernel's order, the float64 evaluation of the whole chain from a float32 signal,
and a CPU route with a single-precision head (``scipy.fft.rfft`` on float32 frames, float32 bank sums and logs) and the float64 tail,
whose deviation from the float64 evaluation is one of the two yardsticks the chain is held to.  numpy / scipy only; nothing here
reads the package under test."""
import numpy

import mfcc_f64 as mf
import normfeat_numpy as nn

CONFIGS = (
    dict(fs=16000, nwin=0.025, shift=0.01, nceps=13, rasta=False),     # window 400, n_fft 512, 21 bands
    dict(fs=16000, nwin=0.025, shift=0.01, nceps=13, rasta=True),
    dict(fs=8000, nwin=0.025, shift=0.01, nceps=16, rasta=False),      # 200, 256, 17 bands: the largest number of cepstra
    dict(fs=8000, nwin=0.025, shift=0.01, nceps=16, rasta=True),
)
ROWS = mf.ROWS
PREFAC = mf.PREFAC
OUTPUTS = ("energy", "cep", "post")


def bands(cfg):
    return int(numpy.ceil(6. * numpy.arcsinh(cfg["fs"] / 2 / 600.)) + 1)


def head_cfg(cfg):
    """The configuration as mfcc_f64's functions read it: the bank is handed in, one cepstrum is computed and dropped"""
    return dict(fs=cfg["fs"], nwin=cfg["nwin"], shift=cfg["shift"], nceps=1)


def signals(cfg, seed):
    return mf.signals(head_cfg(cfg), seed)


def acw_f64(nb, order):
    """acw[k][j] of include/sidekit_amd/plp.h"""
    M = 2 * (nb - 1)
    w = numpy.empty((order + 1, nb))
    for k in range(order + 1):
        for j in range(nb):
            w[k, j] = 2.0 * numpy.cos(numpy.pi * j * k / (nb - 1)) / M
        w[k, 0] = 1.0 / M
        w[k, nb - 1] = (-1.0) ** k / M
    return w


def lift_f64(nceps):
    return numpy.hstack((1.0, numpy.arange(1, nceps) ** 0.6))


def postaud_f64(logband, eql):
    """Steps 1-3: ``y`` (N, nb) from the log band energies (N, nb)"""
    with numpy.errstate(all="ignore"):
        z = (eql[None, :] * numpy.exp(numpy.asarray(logband, dtype=numpy.float64))) ** 0.33
    y = z.copy()
    y[:, 0], y[:, -1] = z[:, 1], z[:, -2]
    return y


def cepstra_f64(y, acw, lift):
    """Steps 4-7 on ``y`` (N, nb), every frame at once, every sum in the kernel's order -> liftered cepstra (N, order + 1)"""
    order, nb = acw.shape[0] - 1, acw.shape[1]
    N = y.shape[0]
    with numpy.errstate(all="ignore"):
        r = numpy.zeros((N, order + 1))
        for k in range(order + 1):
            for j in range(nb):
                r[:, k] = r[:, k] + acw[k, j] * y[:, j]
        A = numpy.zeros((N, order))
        P = r[:, 0].copy()
        for k in range(order):
            s = r[:, k + 1].copy()
            for j in range(k):
                s = s + A[:, j] * r[:, k - j]
            t = -s / P
            P = P * (1.0 - t * t)
            A[:, k] = t
            for j in range((k + 1) // 2):
                i = k - j - 1
                aj, ai = A[:, j].copy(), A[:, i].copy()
                A[:, j] = aj + t * ai
                if i != j:
                    A[:, i] = ai + t * aj
        c = numpy.zeros((N, order + 1))
        c[:, 0] = numpy.log(P)
        for n in range(1, order + 1):
            total = numpy.zeros(N)
            for m in range(1, n):
                total = total + (float(n - m) * A[:, m - 1]) * c[:, n - m]
            c[:, n] = -(A[:, n - 1] + total / float(n))
        return c * lift[None, :]


def plp_cepstra_f64(logband, eql, acw, lift):
    """The kernel's formulas on its operands -> ``(cep (N, order + 1), y (N, nb))``"""
    y = postaud_f64(logband, eql)
    return cepstra_f64(y, acw, lift), y


def _tail(energy, logband, cfg, eql):
    nb = eql.shape[0]
    logband = numpy.asarray(logband, dtype=numpy.float64)
    if cfg["rasta"]:
        logband = nn.rasta(logband)
    cep, y = plp_cepstra_f64(logband, eql, acw_f64(nb, cfg["nceps"] - 1), lift_f64(cfg["nceps"]))
    return numpy.asarray(energy, dtype=numpy.float64), cep, y, logband


def plp_f64(sig, cfg, bank, eql):
    """The whole chain in float64 on the float32 operands (``sig`` float32 samples, ``bank`` the float32 bark bank)
    -> ``(energy (T,), cep (T, nceps), post (T, nb), logband (T, nb) as it enters the exponential)``"""
    energy, fb, _, _ = mf.mfcc_f64(sig, head_cfg(cfg), bank)
    return _tail(energy, fb, cfg, eql)


def plp_single(sig, cfg, bank, eql):
    """Single-precision FFT, float32 bank sums and float32 logs (mfcc_f64.mfcc_single), then the float64 tail"""
    energy, fb, _, _ = mf.mfcc_single(sig, head_cfg(cfg), bank)
    return _tail(energy, fb, cfg, eql)


def deviations(got, want):
    """Maximum absolute deviation of energy and cep, and of post relative to each frame's largest band (its values span five decades
    between a faint frame and a loud one) -> ``[energy, cep, post]``"""
    out = [float(numpy.abs(numpy.asarray(g, dtype=numpy.float64) - w).max()) if w.size else 0.0 for g, w in zip(got[:2], want[:2])]
    if want[2].size:
        out.append(float((numpy.abs(numpy.asarray(got[2], dtype=numpy.float64) - want[2]).max(axis=1) / numpy.abs(want[2]).max(axis=1)).max()))
    else:
        out.append(0.0)
    return out
