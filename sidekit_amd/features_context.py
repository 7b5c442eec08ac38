"""Context features -- what fills the "temporal context" slot of ``FeaturesServer.post_processing`` beside the deltas
(``sidekit/features_server.py:217-223``) and the two methods of the same family (:325-394): stacked context (``get_context``), shifted
delta cepstra (``shifted_delta_cepstral``, ``sidekit/frontend/features.py:197-223``), DCT-PCA (``pca_dct``, :169-194; McLaren and Lei,
2015) and TRAPs (``get_traps``).

All four are one operation: a linear map over a window of frames around ``t``, the segment's first and last row repeated past its ends
(``cl(i) = min(max(i, 0), n - 1)``), on a stacked ragged batch -- float32 ``(N, D)`` rows and ``S + 1`` row offsets, as
``features_server.post_process_device`` takes and returns them.  They run on the device through the C ABI
(``include/sidekit_amd/context.h``) and never build the ``(N, W D)`` window matrix:

  * ``context_device``   ``out[t, w D + c] = x[cl(t + w - L), c]``, ``W = L + R + 1``: a copy (``sc_ctx_gather``), bit-exact;
  * ``sdc_device``       ``out = [x | sdc]``, ``sdc[t, b D + c] = x[cl(t + b p - d), c] - x[cl(t + b p + d), c]``, one float32
                         subtraction (``sc_ctx_gather``), bit-exact;
  * ``pca_dct_device``   ``z[t, c W + j] = sum_w x[cl(t + w - L), c] B[w, j]`` with ``B = dct_basis(W, W).T`` (``sc_ctx_basis``), and
                         with a PCA matrix ``P`` (``D W x Q``) ``out = z P`` as ONE product with ``M[w D + c, q] = sum_j B[w, j]
                         P[c W + j, q]`` on the f64 matrix cores (``sc_ctx_project``);
  * ``traps_device``     ``out[t, c nb + j] = sum_w x[cl(t + w - L), c] H[w, j]``, ``H[w, j] = dct_basis(nb, W)[j, w] hamming(W)[w]``
                         (``sc_ctx_basis``).

Sums are float64 in a fixed order, rounded once to float32; a segment's bits depend on its own rows alone.  ``post_process_context_device``
is ``post_process_device`` with the slot filled; ``ContextFeaturesServer`` is ``FeaturesServer`` with ``dct_pca``, ``sdc``, ``get_context``
and ``get_traps`` built (``FeaturesServer`` itself keeps refusing them).  There is no CPU fallback; importing the module needs neither a
GPU nor torch.

Where this differs from the reference, on purpose:
  * SDC subtracts the later frame from the earlier one.  That is what the reference computes: its ``compute_delta(method='diff')`` runs
    the filter ``[-1, 0 .., 1]`` through ``numpy.convolve``, which flips it;
  * the reference pads ``3 k + d`` rows after the stream whatever ``p`` is, so the formula above holds only while ``(k - 1) p <= 3 k``;
    past that the reference reads zeros and then wraps its index vector.  Such configurations are refused with ``ValueError``;
  * ``get_traps`` pads by ``get_context``'s rule.  The reference's passes a negative pad width to ``numpy.pad`` when
    ``start > context[0]`` and raises; here both methods return rows ``start:stop`` of windows that read the whole stream, clamped at the
    stream's ends (not at ``start`` / ``stop``);
  * a one-row stream follows the formulas (the reference's ``framing`` squeezes a single window away and ``pca_dct`` then fails);
  * the reference's ``framing`` calls ``numpy.lib.pad``, an alias numpy 2 removed; nothing here depends on it;
  * the values are float32 device results, whatever the dtype they are returned in.

Limits (``include/sidekit_amd/context.h``): windows of at most ``MAX_W`` = 64 frames for ``pca_dct_device`` and ``traps_device``, and with
``P`` at most ``PROJ_MAX_D`` = 128 coefficients and ``PROJ_MAX_Q`` = 512 columns; at most ``MAX_BLOCKS`` = 256 blocks whose offsets span
at most ``MAX_SPAN`` = 256 rows for ``context_device`` and ``sdc_device``.
"""
import numpy

from . import _lib
from . import features_server as fs
from .features_server import FeaturesServer, post_process_device

MAX_BLOCKS, MAX_SPAN, MAX_W, PROJ_MAX_D, PROJ_MAX_Q = (_lib.SC_CTX_MAX_BLOCKS, _lib.SC_CTX_MAX_SPAN, _lib.SC_CTX_MAX_W, _lib.SC_CTX_PROJ_MAX_D,
                                                       _lib.SC_CTX_PROJ_MAX_Q)

# ---- the tables, on the host ------------------------------------------------------------------------------------------------------------

def _count(name, value, low):
    if int(value) != value or value < low:
        raise ValueError(f"{name} must be an integer >= {low} (got {value!r})")
    return int(value)


def context_offsets(left, right):
    """``plus`` of a stacked context ``(left, right)``: block ``w`` is row ``t + w - left``"""
    left, right = _count("left", left, 0), _count("right", right, 0)
    if left + right + 1 > MAX_BLOCKS or left + right > MAX_SPAN:
        raise ValueError(f"a context of {left} + 1 + {right} frames is beyond the {MAX_BLOCKS} blocks / {MAX_SPAN} rows sc_ctx_gather spans")
    return numpy.arange(-left, right + 1, dtype=numpy.int32)


def sdc_offsets(d=1, p=3, k=7):
    """``(plus, minus)`` of the shifted deltas: block ``b`` is row ``t + b p - d`` less row ``t + b p + d``"""
    d, p, k = _count("d", d, 1), _count("p", p, 1), _count("k", k, 1)
    if (k - 1) * p > 3 * k:
        raise ValueError(f"sdc ({d}, {p}, {k}): (k - 1) p = {(k - 1) * p} > 3 k = {3 * k}; the reference pads 3 k + d rows after the stream "
                         f"whatever p is, and past that bound it reads zeros and then wraps its index vector: such a configuration is not built")
    if k > MAX_BLOCKS or (k - 1) * p + 2 * d > MAX_SPAN or (k - 1) * p + d > MAX_SPAN:
        raise ValueError(f"sdc ({d}, {p}, {k}) is beyond the {MAX_BLOCKS} blocks / {MAX_SPAN} rows sc_ctx_gather spans")
    shift = numpy.arange(k, dtype=numpy.int32) * p
    return shift - d, shift + d


def _window(left, right):
    left, right = _count("left", left, 0), _count("right", right, 0)
    if left + right + 1 > MAX_W:
        raise ValueError(f"a window of {left} + 1 + {right} frames is beyond the {MAX_W} frames the kernels hold")
    return left, right, left + right + 1


def dct_pca_basis(left_ctx=12, right_ctx=12):
    """``B = dct_basis(W, W).T``, ``W x W`` float64: ``B[w, j]`` weighs frame ``w`` of the window in DCT coefficient ``j``"""
    from .frontend.features import dct_basis
    _, _, W = _window(left_ctx, right_ctx)
    return numpy.ascontiguousarray(dct_basis(W, W).T)


def traps_basis(left, right, dct_nb):
    """``H[w, j] = dct_basis(nb, W)[j, w] hamming(W)[w]``, ``W x nb`` float64"""
    from .frontend.features import dct_basis
    _, _, W = _window(left, right)
    nb = _count("dct_nb", dct_nb, 1)
    if nb > W:
        raise ValueError(f"traps: {nb} DCT coefficients of a window of {W} frames")
    return numpy.ascontiguousarray((dct_basis(nb, W) * numpy.hamming(W)).T)


def projection_matrix(basis, p, D):
    """The composite of the temporal basis and the PCA: ``M[w D + c, q] = sum_j B[w, j] P[c W + j, q]``, ``(W D, Q)`` float64, time-major
    in its rows.  ``basis``: ``W x J``; ``p``: ``(D J, Q)``."""
    basis = numpy.asarray(basis, dtype=numpy.float64)
    p = numpy.asarray(p, dtype=numpy.float64)
    W, J = basis.shape
    if p.ndim != 2 or p.shape[0] != D * J:
        raise ValueError(f"the PCA matrix must have D W = {D} x {J} = {D * J} rows (got shape {p.shape})")
    Q = p.shape[1]
    if D > PROJ_MAX_D or not 1 <= Q <= PROJ_MAX_Q:
        raise ValueError(f"a projection of {D} coefficients onto {Q} columns is beyond the {PROJ_MAX_D} coefficients / {PROJ_MAX_Q} columns "
                         f"sc_ctx_project holds")
    return numpy.ascontiguousarray(numpy.einsum("wj,cjq->wcq", basis, p.reshape(D, J, Q)).reshape(W * D, Q))


# ---- the device functions ---------------------------------------------------------------------------------------------------------------

def _batch(frames, seg_off):
    torch = fs._torch()
    x = fs._rows(torch, frames)
    off = fs._offsets(torch, seg_off, x.shape[0], x.device)
    return torch, x, off


def _wide(torch, x, width, out):
    if out is None:
        return torch.empty((x.shape[0], width), dtype=torch.float32, device=x.device)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == (x.shape[0], width)
            and (out.shape[0] <= 1 or out.stride(1) == 1)):
        raise ValueError(f"out: a float32 CUDA matrix of {x.shape[0]} x {width} with contiguous rows")
    return out


def _grid_rows(x, max_rows):
    """``max_rows`` of the entry points: a bound of the longest segment that sizes the grid and nothing else; the matrix's rows by default"""
    return x.shape[0] if max_rows is None else _count("max_rows", max_rows, 1)


class _Composite:
    """A resident ``(W D, Q)`` float64 composite of the DCT basis and a PCA matrix (``projection_matrix``), time-major in its rows: what
    ``ContextFeaturesServer`` puts in the place of ``dct_pca_config``'s ``P`` once it has formed it.  A type of its own, because ``P``
    itself has the same shape."""

    def __init__(self, matrix):
        self.matrix = matrix


def gather_device(frames, seg_off, plus, minus=None, out=None, max_rows=None):
    """``sc_ctx_gather``: ``out[t, b D + c] = x[cl(t + plus[b]), c]``, less ``x[cl(t + minus[b]), c]`` with ``minus`` (one float32
    subtraction).  ``out`` may be a column block of a wider matrix, and of the one ``frames`` is a column block of.  ``max_rows`` (here and
    in ``basis_device`` / ``project_device``): a bound of the longest segment, the matrix's rows by default; it sizes the grid and changes
    no bit of the result."""
    plus = numpy.ascontiguousarray(plus, dtype=numpy.int32).reshape(-1)
    both = plus if minus is None else numpy.concatenate((plus, numpy.ascontiguousarray(minus, dtype=numpy.int32).reshape(-1)))
    J, lo, span = plus.shape[0], int(both.min()), int(both.max() - both.min())
    if not 1 <= J <= MAX_BLOCKS or both.shape[0] not in (J, 2 * J) or span > MAX_SPAN or max(abs(lo), abs(lo + span)) > MAX_SPAN:
        raise ValueError(f"{J} blocks whose offsets span {span} rows from {lo}: beyond the {MAX_BLOCKS} blocks / {MAX_SPAN} rows sc_ctx_gather spans")
    torch, x, off = _batch(frames, seg_off)
    y = _wide(torch, x, J * x.shape[1], out)
    if x.shape[0]:
        table = torch.as_tensor(both).to(x.device)
        _lib.launch("sc_ctx_gather", x.device, x, fs._ld(x), off, off.shape[0] - 1, x.shape[1], _grid_rows(x, max_rows), table[:J],
                    None if minus is None else table[J:], J, lo, span, y, fs._ld(y))
    return y


def context_device(frames, seg_off, left, right, out=None):
    """Every frame with its ``left`` and ``right`` neighbours, ``(N, (left + 1 + right) D)``: ``out[t, w D + c] = x[cl(t + w - left), c]``"""
    return gather_device(frames, seg_off, context_offsets(left, right), None, out)


def sdc_device(frames, seg_off, d=1, p=3, k=7):
    """``shifted_delta_cepstral`` of every segment, ``(N, D (k + 1))``: the frames, then ``k`` blocks
    ``x[cl(t + b p - d)] - x[cl(t + b p + d)]`` (float32).  ``ValueError`` while ``(k - 1) p > 3 k`` (see the module's head)."""
    plus, minus = sdc_offsets(d, p, k)
    torch, x, off = _batch(frames, seg_off)
    D = x.shape[1]
    out = torch.empty((x.shape[0], D * (plus.shape[0] + 1)), dtype=torch.float32, device=x.device)
    out[:, :D] = x
    gather_device(x, off, plus, minus, out=out[:, D:])
    return out


def basis_device(frames, seg_off, basis, left, out=None, max_rows=None):
    """``sc_ctx_basis``: ``out[t, c J + j] = sum_w basis[w, j] x[cl(t + w - left), c]`` for a ``W x J`` float64 ``basis`` (a host array,
    or a resident tensor)"""
    resident = hasattr(basis, "is_cuda")
    if not resident:
        basis = numpy.ascontiguousarray(basis, dtype=numpy.float64)
    W, J = basis.shape
    if not (1 <= W <= MAX_W and 1 <= J <= W and 0 <= left < W):
        raise ValueError(f"a basis of {W} x {J} at left = {left}: the window holds at most {MAX_W} frames, the basis at most W columns")
    torch, x, off = _batch(frames, seg_off)
    table = (basis if resident else torch.as_tensor(basis)).to(device=x.device, dtype=torch.float64).contiguous()
    y = _wide(torch, x, J * x.shape[1], out)
    if x.shape[0]:
        _lib.launch("sc_ctx_basis", x.device, x, fs._ld(x), off, off.shape[0] - 1, x.shape[1], _grid_rows(x, max_rows), table, W, J, int(left), y,
                    fs._ld(y))
    return y


def project_device(frames, seg_off, matrix, W, left, out=None, max_rows=None):
    """``sc_ctx_project``: ``out[t, q] = sum_k x[cl(t + w - left), c] matrix[k, q]``, ``k = w D + c``, for a ``(W D, Q)`` float64
    ``matrix`` (a host array, or a resident tensor) on the f64 matrix cores"""
    torch = fs._torch()
    if not torch.is_tensor(matrix):
        matrix = torch.as_tensor(numpy.ascontiguousarray(matrix, dtype=numpy.float64))
    torch, x, off = _batch(frames, seg_off)
    D, Q = x.shape[1], matrix.shape[1]
    if not (1 <= W <= MAX_W and 0 <= left < W and D <= PROJ_MAX_D and 1 <= Q <= PROJ_MAX_Q) or matrix.shape[0] != W * D:
        raise ValueError(f"a ({matrix.shape[0]}, {Q}) projection of windows of {W} frames of {D} coefficients: beyond W <= {MAX_W}, "
                         f"D <= {PROJ_MAX_D}, Q <= {PROJ_MAX_Q} or not W D rows")
    m = matrix.to(device=x.device, dtype=torch.float64).contiguous()
    y = _wide(torch, x, Q, out)
    if x.shape[0]:
        _lib.launch("sc_ctx_project", x.device, x, fs._ld(x), off, off.shape[0] - 1, D, _grid_rows(x, max_rows), m, W, int(left), Q, y, fs._ld(y))
    return y


def pca_dct_device(frames, seg_off, left_ctx=12, right_ctx=12, p=None):
    """``pca_dct`` of every segment: the DCT over time of each coefficient's window, ``(N, D W)`` with ``p=None``, else its projection
    ``(N, Q)`` by the ``(D W, Q)`` PCA matrix ``p`` (a host array or a tensor, the reference's ``P`` either way) -- as one product with
    ``projection_matrix``, formed here on the host at every call; ``ContextFeaturesServer`` forms it once per configuration."""
    left_ctx, right_ctx, W = _window(left_ctx, right_ctx)
    basis = dct_pca_basis(left_ctx, right_ctx)
    if p is None:
        return basis_device(frames, seg_off, basis, left_ctx)
    torch, x, off = _batch(frames, seg_off)
    if isinstance(p, _Composite):
        return project_device(x, off, p.matrix, W, left_ctx)
    if torch.is_tensor(p):
        p = p.detach().cpu().numpy()
    return project_device(x, off, projection_matrix(basis, p, x.shape[1]), W, left_ctx)


def traps_device(frames, seg_off, left, right, dct_nb):
    """TRAPs of every segment, ``(N, D dct_nb)``: the first ``dct_nb`` DCT coefficients of each coefficient's Hamming-weighted window"""
    basis = traps_basis(left, right, dct_nb)
    return basis_device(frames, seg_off, basis, int(left))


_OPTIONS = ("rasta", "delta", "double_delta", "delta_filter", "mask", "feat_norm", "win", "global_mean", "global_std", "keep_all_features")


def post_process_context_device(frames, seg_off, labels=None, *, dct_pca=False, dct_pca_config=None, sdc=False, sdc_config=None, **options):
    """``post_process_device`` with the temporal-context slot filled, in the reference's order (:213-245): RASTA, then ONE of deltas /
    ``dct_pca`` (``dct_pca_config = (left, right, P)``, ``(12, 12, None)`` by default) / ``sdc`` (``sdc_config = (d, p, k)``,
    ``(1, 3, 7)``), then the mask, the normalisation and the selection.  The precedence is the reference's ``if / elif``: with ``delta``
    or ``double_delta`` set the other two are ignored, and ``dct_pca`` goes before ``sdc``.  ``options`` are ``post_process_device``'s.
    With neither option in effect the result is ``post_process_device``'s, bit for bit."""
    unknown = sorted(set(options) - set(_OPTIONS))
    if unknown:
        raise TypeError(f"post_process_context_device got unexpected options {unknown}")
    if options.get("delta") or options.get("double_delta") or not (dct_pca or sdc):
        return post_process_device(frames, seg_off, labels, **options)
    if dct_pca:
        left, right, p = (12, 12, None) if dct_pca_config is None else dct_pca_config
        _window(left, right)
    else:
        d, p_shift, k = (1, 3, 7) if sdc_config is None else sdc_config
        sdc_offsets(d, p_shift, k)
    x, labels, off = post_process_device(frames, seg_off, labels, rasta=bool(options.get("rasta")))
    x = pca_dct_device(x, off, left, right, p) if dct_pca else sdc_device(x, off, d, p_shift, k)
    rest = {key: options[key] for key in _OPTIONS[3:] if key in options and key != "delta_filter"}
    return post_process_device(x, off, labels, **rest)


# ---- the numpy surface ------------------------------------------------------------------------------------------------------------------

class ContextFeaturesServer(FeaturesServer):
    """``FeaturesServer`` with the reference's constructor and ``dct_pca``, ``sdc``, ``get_context`` and ``get_traps`` built:
    ``post_processing``, ``load``, ``get_features``, ``stack_features`` and ``stack_features_device`` honour ``dct_pca`` /
    ``dct_pca_config = (left, right, P)`` and ``sdc`` / ``sdc_config = (d, p, k)``; ``context`` and ``traps_dct_nb`` are read by
    ``get_context`` / ``get_traps`` alone, as in the reference."""

    _BUILDS_CONTEXT = True

    def __init__(self,
                 features_extractor=None,
                 feature_filename_structure=None,
                 sources=None,
                 dataset_list=None,
                 mask=None,
                 feat_norm=None,
                 global_cmvn=None,
                 dct_pca=False,
                 dct_pca_config=None,
                 sdc=False,
                 sdc_config=None,
                 delta=None,
                 double_delta=None,
                 delta_filter=None,
                 context=None,
                 traps_dct_nb=None,
                 rasta=None,
                 keep_all_features=True):
        super().__init__(features_extractor, feature_filename_structure, sources, dataset_list, mask, feat_norm, global_cmvn, dct_pca,
                         dct_pca_config, sdc, sdc_config, delta, double_delta, delta_filter, context, traps_dct_nb, rasta, keep_all_features)
        self._composite = None      # (key, M): the resident composite of the DCT basis and the PCA matrix of dct_pca_config

    def _context_options(self):
        """``dct_pca_config`` with its PCA matrix replaced by the resident composite, formed once per configuration"""
        config = tuple(self.dct_pca_config)
        if self.dct_pca and not (self.delta or self.double_delta) and config[2] is not None:
            key = (config[0], config[1], id(config[2]))
            if self._composite is None or self._composite[0] != key:
                p = numpy.asarray(config[2].detach().cpu().numpy() if hasattr(config[2], "detach") else config[2], dtype=numpy.float64)
                left, right, W = _window(config[0], config[1])
                if p.ndim != 2 or p.shape[0] % W:
                    raise ValueError(f"the PCA matrix must have D W rows, W = {W} (got shape {p.shape})")
                torch = fs._torch()
                m = projection_matrix(dct_pca_basis(left, right), p, p.shape[0] // W)
                self._composite = (key, _Composite(torch.as_tensor(m).to(torch.device("cuda", torch.cuda.current_device()))))
            config = (config[0], config[1], self._composite[1])
        return dict(dct_pca=bool(self.dct_pca), dct_pca_config=config, sdc=bool(self.sdc), sdc_config=tuple(self.sdc_config))

    def _process(self, frames, seg_off, labels, **options):
        return post_process_context_device(frames, seg_off, labels, **self._context_options(), **options)

    def _windows(self, feat, start, stop, label, device_fn):
        """Rows ``start:stop`` of ``device_fn`` over the whole stream: the stream is extended by its first / last row to cover
        ``[min(start, 0), max(stop, n))``, which leaves every window as the clamp at the stream's ends makes it"""
        feat = numpy.asarray(feat)
        n = feat.shape[0]
        start = 0 if start is None else int(start)
        stop = n if stop is None else int(stop)
        if n == 0 or stop <= start:
            raise ValueError(f"rows {start}:{stop} of a stream of {n} frames")
        before, after = max(-start, 0), max(stop - n, 0)
        padded = numpy.pad(numpy.asarray(feat, dtype=numpy.float32), ((before, after), (0, 0)), mode='edge')
        out = device_fn(padded).cpu().numpy()[start + before:stop + before]
        dtype = feat.dtype if numpy.issubdtype(feat.dtype, numpy.floating) else numpy.float64
        return out.astype(dtype), (None if label is None else label[start:stop])

    def get_context(self, feat, start=None, stop=None, label=None):
        """Rows ``start:stop`` of ``feat`` (one frame per row), each with its ``context = (left, right)`` neighbours, and
        ``label[start:stop]``: ``out[i, w D + c] = feat[cl(start + i + w - left), c]``.  The windows read the whole stream, its first
        and last frame repeated past its ends; ``start`` and ``stop`` may lie beyond them."""
        left, right = self.context
        return self._windows(feat, start, stop, label, lambda x: context_device(x, None, left, right))

    def get_traps(self, feat, start=None, stop=None, label=None):
        """TRAPs of rows ``start:stop``: the first ``traps_dct_nb`` DCT coefficients of each coefficient's Hamming-weighted window of
        ``context = (left, right)`` frames, and ``label[start:stop]``.  The rows and the padding follow ``get_context``'s rule (the
        reference's own padding here takes a negative width when ``start > context[0]`` and raises)."""
        left, right = self.context
        return self._windows(feat, start, stop, label, lambda x: traps_device(x, None, left, right, self.traps_dct_nb))
