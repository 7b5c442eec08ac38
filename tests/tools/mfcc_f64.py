"""The cepstral front end restated for the tests (csrc/cepstrum.hip, sidekit_amd/features_extractor.py): the four configurations and
the rows of tests/golden/extractor.npz, the signals regenerated from stored ``RandomState`` seeds, the float64 evaluation of the
formulas of include/sidekit_amd/cepstrum.h on the float32 operands, and a CPU single-precision route (``scipy.fft.rfft`` on the float32
windowed frames, then the float32 bank, log and DCT) whose own deviation from the float64 evaluation is one of the two yardsticks the
kernel is held to.  numpy / scipy only; nothing here reads the package under test."""
import numpy
import scipy.fft

CONFIGS = (
    dict(fs=16000, nwin=0.025, shift=0.01, lowfreq=100, maxfreq=8000, nlinfilt=0, nlogfilt=24, nceps=13),    # window 400, n_fft 512
    dict(fs=8000, nwin=0.025, shift=0.01, lowfreq=300, maxfreq=3400, nlinfilt=0, nlogfilt=24, nceps=19),     # 200, 256
    dict(fs=16000, nwin=0.032, shift=0.01, lowfreq=0, maxfreq=8000, nlinfilt=40, nlogfilt=0, nceps=20),      # 512 = n_fft: no zero padding
    dict(fs=16000, nwin=0.020, shift=0.01, lowfreq=100, maxfreq=8000, nlinfilt=0, nlogfilt=24, nceps=13),    # 320
)
ROWS = ("no frame", "one frame", "one frame and a tail", "two frames", "five frames", "white noise", "low-passed noise")
PREFAC = 0.97


def frame_shape(cfg):
    """-> (window length, shift, n_fft) in samples"""
    window = int(round(cfg["nwin"] * cfg["fs"]))
    return window, int(cfg["shift"] * cfg["fs"]), 2 ** int(numpy.ceil(numpy.log2(window)))


def n_frames(n, cfg):
    window, shift, _ = frame_shape(cfg)
    return (n - window) // shift + 1 if n >= window else 0


def row_lengths(cfg):
    window, shift, _ = frame_shape(cfg)
    long = int(2.6 * cfg["fs"])
    return (window - 1, window, window + shift - 1, window + shift, window + 4 * shift, long, long)


def signals(cfg, seed):
    """The rows of one configuration, int16: short rows of white noise; two long rows of loud bursts between stretches of faint noise
    (what the energy VAD separates), the second passed through an 8-tap moving average."""
    rs = numpy.random.RandomState(seed)
    fs, rows = cfg["fs"], []
    for r, n in enumerate(row_lengths(cfg)):
        if r < 5:
            x = rs.randn(n) * 3000.0
        else:
            x, pos, loud = numpy.zeros(n), 0, bool(rs.randint(2))
            while pos < n:
                d = min(int(rs.uniform(0.08, 0.5) * fs), n - pos)
                amp = rs.uniform(1500, 9000) if loud else rs.uniform(15, 60)
                x[pos:pos + d] = rs.randn(d) * amp * (0.6 + 0.4 * numpy.sin(numpy.arange(d) / rs.uniform(300, 900)))
                pos, loud = pos + d, not loud
            if r == 6:
                x = numpy.convolve(x, numpy.full(8, 0.25))[:n]
        rows.append(numpy.clip(numpy.round(x), -32768, 32767).astype(numpy.int16))
    return rows


def frames_of(sig, cfg):
    """(frames, window) view of the frames of a 1-D signal"""
    window, shift, _ = frame_shape(cfg)
    T = n_frames(sig.shape[0], cfg)
    idx = numpy.arange(T)[:, None] * shift + numpy.arange(window)[None, :]
    return sig[idx] if T else numpy.zeros((0, window), dtype=sig.dtype)


def dct_f64(nceps, nfilt):
    """Rows 1 .. nceps of the orthonormal DCT-II basis, float64, from scipy"""
    return scipy.fft.dct(numpy.eye(nfilt), type=2, norm='ortho', axis=-1).T[1:nceps + 1]


def mfcc_f64(sig, cfg, bank, prefac=PREFAC):
    """The formulas in float64 on the float32 operands: ``sig`` holds float32 samples, ``bank`` the float32 ``trfbank`` matrix, the
    pre-emphasis factor is the float32 the kernel multiplies by; window and DCT are exact.
    -> ``(energy (T,), fb (T, nfilt), cep (T, nceps), spec (T, n_fft / 2 + 1))``"""
    window, _, n_fft = frame_shape(cfg)
    x = frames_of(numpy.asarray(sig, dtype=numpy.float32), cfg).astype(numpy.float64)
    p = float(numpy.float32(prefac))
    y = x - p * numpy.concatenate((x[:, :1], x[:, :-1]), axis=1)
    with numpy.errstate(divide="ignore"):
        energy = numpy.log((y * y).sum(axis=1))
        X = numpy.fft.rfft(y * numpy.hanning(window), n_fft, axis=-1)
        spec = X.real ** 2 + X.imag ** 2
        fb = numpy.log(spec @ numpy.asarray(bank, dtype=numpy.float64).T)
    cep = fb @ dct_f64(cfg["nceps"], bank.shape[0]).T
    return energy, fb, cep, spec


def mfcc_single(sig, cfg, bank, prefac=PREFAC):
    """The same in single precision on the CPU: float32 pre-emphasis as the reference's, ``scipy.fft.rfft`` of the float32 windowed
    frames (complex64), float32 bank product, log and ``scipy.fft.dct``"""
    window, _, n_fft = frame_shape(cfg)
    x = frames_of(numpy.asarray(sig, dtype=numpy.float32), cfg)
    y = x - numpy.concatenate((x[:, :1], x[:, :-1]), axis=1) * numpy.float32(prefac)
    assert y.dtype == numpy.float32
    with numpy.errstate(divide="ignore"):
        energy = numpy.log((y ** 2).sum(axis=1))
        X = scipy.fft.rfft((y * numpy.hanning(window)).astype(numpy.float32), n_fft, axis=-1)
        assert X.dtype == numpy.complex64
        spec = X.real ** 2 + X.imag ** 2
        fb = numpy.log(numpy.dot(spec, numpy.asarray(bank, dtype=numpy.float32).T))
    cep = scipy.fft.dct(fb, type=2, norm='ortho', axis=-1)[:, 1:cfg["nceps"] + 1]
    assert energy.dtype == fb.dtype == cep.dtype == numpy.float32
    return energy, fb, cep, spec


def deviations(got, want):
    """Maximum absolute deviation of energy, fb and cep, and of the spectrum relative to each frame's largest bin ->
    ``[energy, fb, cep, spec]``; ``got`` may leave the spectrum out (None)"""
    out = [float(numpy.abs(numpy.asarray(g, dtype=numpy.float64) - w).max()) if w.size else 0.0 for g, w in zip(got[:3], want[:3])]
    if got[3] is not None and want[3].size:
        out.append(float((numpy.abs(numpy.asarray(got[3], dtype=numpy.float64) - want[3]).max(axis=1) / want[3].max(axis=1)).max()))
    else:
        out.append(0.0)
    return out
