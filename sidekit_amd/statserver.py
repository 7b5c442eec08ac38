"""``StatServer`` -- the container the scoring functions exchange (subset of ``sidekit/statserver.py``).

Mirrors the attributes (``modelset, segset, start, stop, stat0, stat1``; ``statserver.py:202-231``) and
the ~10 methods the x-vector scoring path calls: ``validate`` (:318-336), ``align_models`` /
``align_segments`` (:656-684), ``norm_stat1`` / ``rotate_stat1`` / ``center_stat1`` / ``whiten_stat1``
(:797-817,852-896), ``get_mean_stat1`` (:789-795), ``sum_stat_per_model`` (:1335-1355), ``mean_stat_per_model`` (:1357-1374), and the
back-end normalisations of x-vectors, which run on the GPU through ``sidekit_amd.backend`` (``get_within_covariance_stat1`` ...
``get_wccn_choleski_stat1`` :940-1054, ``whiten_cholesky_stat1`` :898-918, spectral normalisation :1279-1333).  ``accumulate_stat`` (:687-739) computes the Baum-Welch
statistics of a diagonal ``Mixture`` on the GPU (``sidekit_amd.mixture``), which ``FactorAnalyser.total_variability`` /
``extract_ivectors`` consume (``sidekit_amd.factor_analyser``); ``adapt_mean_map`` / ``adapt_mean_map_multisession`` (:1075-1157) adapt the UBM's
means to each session or model on the host (element-wise work on ``sessions x C D`` numbers; ``sidekit_amd.gmm_scoring.map_adapt_device`` does the
same on resident statistics) for ``sidekit_amd.gmm_scoring``; ``factor_analysis`` with ``estimate_between_class`` / ``estimate_within_class`` /
``estimate_map`` / ``estimate_hidden`` / ``subtract_weighted_stat1`` (:819-850, :1494-1949) train the joint factor analysis model on the GPU
(``sidekit_amd.jfa_scoring``); ``precompute_svm_kernel_stat1`` (:1159-1168), ``get_nap_matrix_stat1`` (:1056-1073) and ``get_model_segments``
(:635-643) serve the SVM back end (``sidekit_amd.svm_training``); ``read`` / ``write`` (:392-489) exchange HDF5 files with the reference through ``sidekit_amd.hdf5_lite``.  Values are float64
(``STAT_TYPE``, ``sidekit/__init__.py:59``); the alignments use hashed lookups instead of per-id scans.
"""
import copy
import logging
import os

import numpy
import scipy.linalg

from . import hdf5_lite
from .bosaris import IdMap, _h5
from .bosaris._sets import first_index

STAT_TYPE = numpy.float64


def whitening_transform(sigma):
    """The matrix ``whiten_stat1`` multiplies by for a full covariance (``statserver.py:871-878``): ``V diag(lambda^-1/2)``, eigenvalues in
    descending order -- not the symmetric inverse square root.  Shared with ``sidekit_amd.backend``."""
    lam, vec = scipy.linalg.eigh(sigma)                     # ascending
    lam, vec = lam.real[::-1], vec.real[:, ::-1]            # largest first
    return vec * (1 / numpy.sqrt(lam))[numpy.newaxis, :]


class StatServer:
    def __init__(self, statserver_file_name=None, distrib_nb=0, feature_size=0, index=None, ubm=None):
        self.modelset = numpy.empty(0, dtype="|O")
        self.segset = numpy.empty(0, dtype="|O")
        self.start = numpy.empty(0, dtype="|O")
        self.stop = numpy.empty(0, dtype="|O")
        self.stat0 = numpy.array([], dtype=STAT_TYPE)
        self.stat1 = numpy.array([], dtype=STAT_TYPE)
        if statserver_file_name is None:
            return
        if isinstance(statserver_file_name, IdMap):
            im = statserver_file_name
            self.modelset, self.segset, self.start, self.stop = im.leftids, im.rightids, im.start, im.stop
            self.stat0 = numpy.zeros((self.segset.shape[0], distrib_nb), dtype=STAT_TYPE)
            self.stat1 = numpy.zeros((self.segset.shape[0], distrib_nb * feature_size), dtype=STAT_TYPE)
            return
        if isinstance(statserver_file_name, str):   # statserver.py:237-245: an HDF5 file written by StatServer.write
            tmp = StatServer.read(statserver_file_name)
            self.modelset, self.segset, self.start, self.stop = tmp.modelset, tmp.segset, tmp.start, tmp.stop
            self.stat0, self.stat1 = tmp.stat0, tmp.stat1
            return
        raise TypeError("StatServer(): expected a file name or an IdMap")

    @staticmethod
    def read(statserver_file_name, prefix=''):
        """``statserver.py:392-424``: the six datasets ``<prefix>modelset, segset, start, stop, stat0, stat1``; identifiers come
        back as unicode, ``start`` / ``stop`` as object arrays with ``None`` where the file holds -1, statistics as float64."""
        with hdf5_lite.File(statserver_file_name) as f:
            statserver = StatServer()
            statserver.modelset = _h5.ids_from_file(f[prefix + "modelset"][()])
            statserver.segset = _h5.ids_from_file(f[prefix + "segset"][()])
            statserver.start = _h5.bounds_from_file(f[prefix + "start"][()])
            statserver.stop = _h5.bounds_from_file(f[prefix + "stop"][()])
            statserver.stat0 = f[prefix + "stat0"][()].astype(dtype=STAT_TYPE)
            statserver.stat1 = f[prefix + "stat1"][()].astype(dtype=STAT_TYPE)
        assert statserver.validate(), "Error: wrong StatServer format"
        return statserver

    def write(self, output_file_name, prefix='', mode='w'):
        """``statserver.py:427-489``: float32 statistics, byte-string identifiers, int32 ``start`` / ``stop`` (-1 = unset), every
        dataset gzip + Fletcher-32 with unlimited rows.  ``mode='a'`` on a file that already holds ``<prefix>`` datasets appends
        the rows to them (the reference resizes in place; here the file is rewritten -- other groups of the file are kept, and
        the new file replaces the old one atomically, ``os.replace``, so an interrupted save leaves the stored statistics
        intact); ``mode='a'`` with a new prefix adds the six datasets beside what the file holds.  One divergence on purpose:
        with ``prefix=''`` the reference's test ``prefix in f`` (``statserver.py:440``) is never true, so its ``mode='a'`` then
        tries to CREATE datasets that exist and raises; here ``prefix=''`` appends like any other prefix."""
        assert self.validate(), "Error: wrong StatServer format"
        new = {"modelset": self.modelset.astype('S'), "segset": self.segset.astype('S'), "stat0": self.stat0.astype(numpy.float32),
               "stat1": self.stat1.astype(numpy.float32), "start": _h5.bounds_to_file(self.start), "stop": _h5.bounds_to_file(self.stop)}
        existing = {}
        if mode != 'w' and os.path.exists(output_file_name):
            existing = hdf5_lite.read_all(output_file_name)
        w = hdf5_lite.Writer()
        for path, arr in existing.items():
            if not (path.startswith(prefix) and path[len(prefix):] in new):
                w[path] = arr
        for name, arr in new.items():
            old = existing.get(prefix + name)
            if old is not None:
                if name in ("modelset", "segset"):   # widen the byte strings to the longer of the two
                    width = max(old.dtype.itemsize, arr.dtype.itemsize)
                    old, arr = old.astype(f"S{width}"), arr.astype(f"S{width}")
                arr = numpy.concatenate((old, arr.astype(old.dtype, copy=False)), axis=0)
            w[prefix + name] = arr
        w.save(output_file_name)

    def __repr__(self):
        line = '-' * 30 + '\n'
        return (line + 'modelset: ' + repr(self.modelset) + '\nsegset: ' + repr(self.segset) + '\nseg start:' + repr(self.start)
                + '\nseg stop:' + repr(self.stop) + '\nstat0:' + repr(self.stat0) + '\nstat1:' + repr(self.stat1) + '\n' + line)

    def validate(self, warn=False):
        ok = self.modelset.ndim == 1 \
            and (self.modelset.shape == self.segset.shape == self.start.shape == self.stop.shape) \
            and (self.stat0.shape[0] == self.stat1.shape[0] == self.modelset.shape[0]) \
            and (not bool(self.stat1.shape[1] % self.stat0.shape[1]))
        if warn and (self.segset.shape != numpy.unique(self.segset).shape):
            logging.warning('Duplicated segments in StatServer')
        return ok

    def _take(self, indx):
        self.segset = self.segset[indx]
        self.modelset = self.modelset[indx]
        self.start = self.start[indx]
        self.stop = self.stop[indx]
        self.stat0 = self.stat0[indx, :]
        self.stat1 = self.stat1[indx, :]

    def align_segments(self, segment_list):
        """Reorder / reduce the sessions to match ``segment_list`` (first occurrence of each id)."""
        self._take(first_index(self.segset, segment_list))

    def align_models(self, model_list):
        """Reorder / reduce the sessions to match ``model_list`` (first occurrence of each id)."""
        self._take(first_index(self.modelset, model_list))

    def get_model_stat0(self, mod_id):
        return self.stat0[self.modelset == mod_id, :]

    def get_model_stat1(self, mod_id):
        return self.stat1[self.modelset == mod_id, :]

    def get_segment_stat1(self, seg_id):
        return self.stat1[self.segset == seg_id, :]

    def get_model_segments(self, mod_id):
        """The segments of model ``mod_id`` (``statserver.py:635-643``)."""
        return self.segset[self.modelset == mod_id]

    def get_mean_stat1(self):
        return numpy.mean(self.stat1, axis=0)

    def get_total_covariance_stat1(self):
        c = self.stat1 - self.stat1.mean(axis=0)
        return numpy.dot(c.transpose(), c) / self.stat1.shape[0]

    def norm_stat1(self):
        """Every session's first-order statistic scaled to unit Euclidean length; a (near-)zero vector is divided by 1e-8 instead
        (``statserver.py:797-800``)."""
        x = self.stat1
        length = numpy.sqrt((x * x).sum(axis=1))
        self.stat1 = x / numpy.maximum(length, 1e-08)[:, numpy.newaxis]

    def rotate_stat1(self, R):
        self.stat1 = self.stat1 @ R

    def _blocks(self):
        """``stat1`` seen as (sessions, distributions, features per distribution): x-vectors are the one-distribution case."""
        n, n_distrib = self.stat0.shape
        return self.stat1.reshape(n, n_distrib, self.stat1.shape[1] // n_distrib)

    def center_stat1(self, mu):
        """Subtract the occupation-weighted mean: block c of a session loses ``stat0[session, c] * mu[block c]`` (``statserver.py:810-817``)."""
        blocks = self._blocks()
        mean = numpy.asarray(mu, dtype=STAT_TYPE).reshape(blocks.shape[1], blocks.shape[2])
        self.stat1 = (blocks - self.stat0[:, :, numpy.newaxis] * mean).reshape(self.stat1.shape)

    def whiten_stat1(self, mu, sigma, isSqrInvSigma=False):
        """Centre on ``mu``, then whiten: by the square roots of a diagonal covariance (1-D ``sigma``), or by ``V diag(lambda^-1/2)`` of a
        full one (2-D; eigenvalues in descending order, ``statserver.py:852-896``) -- or by ``sigma`` itself when the caller already
        holds that matrix (``isSqrInvSigma``)."""
        if sigma.ndim not in (1, 2):
            raise Exception('Wrong dimension of Sigma, must be 1 or 2')
        self.center_stat1(mu)
        if sigma.ndim == 1:
            self.stat1 = self.stat1 / numpy.sqrt(sigma.astype(STAT_TYPE))
            return
        self.rotate_stat1(sigma if isSqrInvSigma else whitening_transform(sigma))

    # ---- Baum-Welch statistics on the GPU (sidekit_amd/mixture.py): no CPU fallback ------------------------------------------------------

    ACCUMULATE_BYTES = 1 << 30   # frames of the segments that go to the device in one accumulate_stat group, and the bound of its workspace

    def accumulate_stat_device(self, ubm, frames, seg_off):
        """Zeroth and first order statistics of every session from resident frames: session i is frames ``[seg_off[i], seg_off[i + 1])``
        of ``frames`` ((N, D) CUDA tensor, float32 or float64).  Fills ``stat0`` (sessions x C) and ``stat1`` (sessions x C D)."""
        from .mixture import gmm_stats_device
        self._accumulate_device(ubm, frames, seg_off, gmm_stats_device)

    def accumulate_stat_topc_device(self, ubm, frames, seg_off, top_c=10):
        """``accumulate_stat_device`` on the ``top_c`` components per frame that score best under ``ubm`` (between 1 and 32, at most the
        mixture's own): posteriors renormalised over each frame's list (``mixture.gmm_stats_topc_device``)."""
        self._accumulate_device(ubm, frames, seg_off, self._stats_topc(ubm, top_c))

    def accumulate_stat_full_device(self, ubm, frames, seg_off):
        """``accumulate_stat_device`` under a full-covariance ``mixture_full.FullMixture`` (``gmm_stats_full_device``); nothing else is
        accepted."""
        from .mixture_full import FullMixture, gmm_stats_full_device
        self._accumulate_device(ubm, frames, seg_off, gmm_stats_full_device, accepted=FullMixture)

    def _accumulate_device(self, ubm, frames, seg_off, gmm_stats_device, accepted=None):
        """``accumulate_stat_device`` with the statistics from ``gmm_stats_device(ubm, frames, seg_off, order=, max_workspace_bytes=)``;
        ``accepted``: the class ``ubm`` has to be (``None``: ``Mixture``)"""
        self._check_ubm(ubm, accepted)
        assert len(seg_off) == self.segset.shape[0] + 1, "seg_off: one offset per session and the end of the last"
        if not ubm.dim() == frames.shape[1]:
            raise Exception('dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), frames.shape[1]))
        stat0, stat1, _, _ = gmm_stats_device(ubm, frames, seg_off, order=1, max_workspace_bytes=self.ACCUMULATE_BYTES)
        to_host = (lambda t: t) if isinstance(stat0, numpy.ndarray) else (lambda t: t.cpu().numpy())
        self.stat0 = to_host(stat0).astype(STAT_TYPE, copy=False)
        self.stat1 = to_host(stat1).reshape(stat0.shape[0], ubm.sv_size()).astype(STAT_TYPE, copy=False)

    @staticmethod
    def _stats_topc(ubm, top_c):
        """``mixture.gmm_stats_topc_device`` at ``top_c`` under ``gmm_stats_device``'s arguments; the mixture and ``top_c`` are checked here"""
        from . import gmm_scoring
        from .mixture import Mixture, gmm_stats_topc_device
        assert isinstance(ubm, Mixture), 'First parameter has to be a Mixture'
        gmm_scoring._top_c(ubm, top_c)

        def stats(ubm, frames, seg_off, order, max_workspace_bytes):
            return gmm_stats_topc_device(ubm, frames, seg_off, order=order, top_c=top_c, max_workspace_bytes=max_workspace_bytes)
        return stats

    def accumulate_stat(self, ubm, feature_server, seg_indices=None, channel_extension=("", "_b"), num_thread=1):
        """Statistics of the sessions ``seg_indices`` (all when ``None``) under ``ubm`` (``statserver.py:687-739``).  ``feature_server``: any
        object whose ``load(show, channel=)`` returns ``(cep, vad_label)``; each session is cut to its ``start`` / ``stop`` and to its
        speech frames as in the reference, the sessions are stacked in groups of at most ``ACCUMULATE_BYTES`` of frames and a group is
        one ``gmm_stats_device`` call.  ``num_thread`` is accepted and unused."""
        from .mixture import gmm_stats_device
        self._accumulate(ubm, feature_server, seg_indices, channel_extension, gmm_stats_device)

    def accumulate_stat_topc(self, ubm, feature_server, top_c=10, seg_indices=None, channel_extension=("", "_b"), num_thread=1):
        """``accumulate_stat`` on the ``top_c`` components per frame that score best under ``ubm`` (between 1 and 32, at most the
        mixture's own), posteriors renormalised over each frame's list (``mixture.gmm_stats_topc_device``): the same sessions, frames,
        groups and placement.  ``num_thread`` is accepted and unused."""
        self._accumulate(ubm, feature_server, seg_indices, channel_extension, self._stats_topc(ubm, top_c))

    def accumulate_stat_full(self, ubm, feature_server, seg_indices=None, channel_extension=("", "_b"), num_thread=1):
        """``accumulate_stat`` under a full-covariance ``mixture_full.FullMixture`` (``statserver.py:731-739`` with ``invcov.ndim == 3``;
        ``gmm_stats_full_device``): the same sessions, frames, groups and placement; nothing else is accepted.  ``num_thread`` is accepted
        and unused."""
        from .mixture_full import FullMixture, gmm_stats_full_device
        self._accumulate(ubm, feature_server, seg_indices, channel_extension, gmm_stats_full_device, accepted=FullMixture)

    @staticmethod
    def _check_ubm(ubm, accepted=None):
        if accepted is None:
            from .mixture import Mixture as accepted
        assert isinstance(ubm, accepted), 'First parameter has to be a {}'.format(accepted.__name__)

    def _accumulate(self, ubm, feature_server, seg_indices, channel_extension, gmm_stats_device, accepted=None):
        """``accumulate_stat`` with a group's statistics from ``gmm_stats_device`` (``_accumulate_group``); ``accepted``: the class ``ubm``
        has to be (``None``: ``Mixture``)"""
        self._check_ubm(ubm, accepted)
        sessions = self.segset.shape[0]
        if seg_indices is None or self.stat0.shape[0] != sessions or self.stat1.shape[0] != sessions:   # nothing usable is held: every session
            self.stat0 = numpy.zeros((sessions, ubm.distrib_nb()), dtype=STAT_TYPE)
            self.stat1 = numpy.zeros((sessions, ubm.sv_size()), dtype=STAT_TYPE)
            seg_indices = range(sessions)
        feature_server.keep_all_features = True
        group, held = [], 0
        for idx in seg_indices:
            frames = self._speech_frames(idx, feature_server, channel_extension)
            if frames.shape[1] != ubm.dim():
                raise Exception('dimension of ubm and features differ: {:d} / {:d}'.format(ubm.dim(), frames.shape[1]))
            group.append((idx, frames))
            held += frames.nbytes
            if held >= self.ACCUMULATE_BYTES:
                self._accumulate_group(ubm, group, gmm_stats_device)
                group, held = [], 0
        self._accumulate_group(ubm, group, gmm_stats_device)

    def _speech_frames(self, idx, feature_server, channel_extension):
        """The frames of session ``idx`` that count: rows ``start`` to ``stop`` (to the end of the labels when ``stop`` is unset or beyond
        it) of what the server loads for the show, those the VAD labels keep.  A show name that ends in the second channel's extension
        is channel 1 when a features extractor stands behind the server; the channel's extension is cut off the name that is loaded."""
        name = self.segset[idx]
        second = getattr(feature_server, "features_extractor", None) is not None and name.endswith(channel_extension[1])
        extension = channel_extension[1 if second else 0]
        cep, labels = feature_server.load(name[:name.rfind(extension)], channel=int(second))
        first, last = self.start[idx], labels.shape[0]
        if self.stop[idx] is not None:
            last = min(self.stop[idx], last)
        logging.info('%s: frames %s to %s', name, first, last)
        return cep[first:last][labels[first:last]]

    def _accumulate_group(self, ubm, group, gmm_stats_device):
        """One ``gmm_stats_device`` call for the stacked frames of ``group`` = [(session, frames)]; sessions without frames keep zeros"""
        if not group:
            return
        rows = [idx for idx, _ in group]
        offsets = numpy.concatenate(([0], numpy.cumsum([f.shape[0] for _, f in group])))
        self.stat0[rows, :] = 0.0
        self.stat1[rows, :] = 0.0
        if offsets[-1] > 0:
            stat0, stat1, _, _ = gmm_stats_device(ubm, numpy.concatenate([f for _, f in group]), offsets, order=1,
                                                  max_workspace_bytes=self.ACCUMULATE_BYTES)
            self.stat0[rows, :] = stat0
            self.stat1[rows, :] = stat1.reshape(len(rows), ubm.sv_size())

    # ---- MAP adaptation of the UBM's means (host: element-wise on sessions x C D numbers) ------------------------------------------------

    @staticmethod
    def _map_means(stat0, stat1, alpha, ubm, norm):
        """``alpha m + (1 - alpha) mu_ubm`` per distribution with ``m = stat1 / stat0`` (0 where the occupation is 0); ``norm`` scales
        by ``sqrt(w invcov)`` of a diagonal UBM (the KL-divergence normalisation of the super-vector kernel)"""
        per_coefficient = numpy.repeat(numpy.arange(ubm.distrib_nb()), ubm.dim())
        with numpy.errstate(divide='ignore', invalid='ignore'):
            mean = stat1 / stat0[:, per_coefficient]
        mean[numpy.isnan(mean)] = 0
        weight = alpha[:, per_coefficient]
        mean = weight * mean + (1 - weight) * ubm.get_mean_super_vector()[numpy.newaxis, :]
        if norm:
            if ubm.invcov.ndim != 2:
                from .mixture import _full_covariance
                raise _full_covariance()
            mean = mean * numpy.sqrt(numpy.repeat(ubm.w, ubm.dim()) * ubm.get_invcov_super_vector())
        return mean.astype(STAT_TYPE)

    def adapt_mean_map(self, ubm, r=16, norm=False):
        """MAP adaptation of the UBM's mean super-vector with relevance factor ``r``, one model per session (``statserver.py:1075-1113``)
        -> a ``StatServer`` with the sessions of this one, ``stat0 = 1`` and the adapted super-vectors as ``stat1``.  As in the
        reference, float32 ``eps`` is added to the occupations inside ``alpha`` (not in the means), so a distribution without
        occupation gets ``1 - eps / (eps + r)`` of the UBM's mean."""
        out = StatServer()
        out.modelset, out.segset, out.start, out.stop = self.modelset, self.segset, self.start, self.stop
        out.stat0 = numpy.ones((self.segset.shape[0], 1), dtype=STAT_TYPE)
        eps = numpy.finfo(numpy.float32).eps
        alpha = (self.stat0 + eps) / (self.stat0 + eps + r)
        out.stat1 = self._map_means(self.stat0, self.stat1, alpha, ubm, norm)
        out.validate()
        return out

    def adapt_mean_map_multisession(self, ubm, r=16, norm=False):
        """MAP adaptation, one model per model id from the summed statistics of its sessions (``statserver.py:1115-1157``) -> a
        ``StatServer`` with ``modelset = segset =`` the sorted unique model ids, ``stat0 = 1`` and the adapted super-vectors as ``stat1``
        (no ``eps`` in this form, as in the reference)."""
        summed = self.sum_stat_per_model()[0]
        out = StatServer()
        out.modelset = numpy.unique(self.modelset)
        out.segset = numpy.unique(self.modelset)
        out.start = numpy.empty(out.modelset.shape, dtype="|O")
        out.stop = numpy.empty(out.modelset.shape, dtype="|O")
        out.stat0 = numpy.ones((out.modelset.shape[0], 1), dtype=STAT_TYPE)
        out.stat1 = self._map_means(summed.stat0, summed.stat1, summed.stat0 / (summed.stat0 + r), ubm, norm)
        out.validate()
        return out

    # ---- the SVM back end (sidekit_amd/svm_training.py): float64 on the GPU, host arrays in and out, no CPU fallback ------------------

    def _device_stat1(self):
        from .svm_training import _rows, _torch
        torch = _torch()
        return torch, _rows(torch, self.stat1)[0]

    def precompute_svm_kernel_stat1(self):
        """The background's part of the SVM Gram matrix, ``stat1 . stat1'`` (``statserver.py:1159-1168``): one float64 GEMM."""
        torch, s = self._device_stat1()
        return torch.matmul(s, s.t()).cpu().numpy()

    def get_nap_matrix_stat1(self, co_rank):
        """The Nuisance Attribute Projection matrix of co-rank ``co_rank`` (``statserver.py:1056-1073``) -> (D, co_rank): the leading
        eigenvectors of ``stat1 . stat1' / D`` mapped back through ``stat1'`` and scaled to unit length, columns by descending
        eigenvalue.  The eigen-decomposition is ``torch.linalg.eigh`` on the device in float64; a column is defined up to its sign."""
        torch, s = self._device_stat1()
        vect_size = s.shape[1]
        assert 0 < co_rank <= s.shape[0], "co_rank must be in [1, number of sessions]"
        lam, vec = torch.linalg.eigh(torch.matmul(s, s.t()) / vect_size)     # ascending
        lam, vec = torch.flip(lam[-co_rank:], (0,)), torch.flip(vec[:, -co_rank:], (1,))
        return (torch.matmul(s.t(), vec) / torch.sqrt(vect_size * lam)[None, :]).cpu().numpy()

    # ---- back-end normalisation on the GPU (sidekit_amd/backend.py): stat1 is uploaded once per call, no CPU fallback ----------------

    def _device_rows(self):
        """``stat1`` as a float64 tensor on the current GPU and the class index of ``modelset``; x-vectors only (one distribution
        per session, occupation 1, so that centring subtracts ``mu`` itself)."""
        from .factor_analyser import ClassIndex, _torch
        torch = _torch()
        assert self.stat0.shape[1] == 1 and numpy.all(self.stat0 == 1), \
            "the back-end normalisations take x-vectors: one distribution per session with stat0 == 1"
        xv = torch.as_tensor(numpy.ascontiguousarray(self.stat1, dtype=STAT_TYPE)).to(torch.device("cuda", torch.cuda.current_device()))
        return xv, ClassIndex(self.modelset)

    def get_within_covariance_stat1(self):
        """Within-class covariance, over the number of sessions (``statserver.py:940-956``)."""
        from . import backend
        return backend.within_covariance_device(*self._device_rows())

    def get_between_covariance_stat1(self):
        """Between-class covariance: class means about the global mean, weighted by the session counts (``statserver.py:958-978``)."""
        from . import backend
        return backend.between_covariance_device(*self._device_rows())

    def get_lda_matrix_stat1(self, rank):
        """LDA matrix (D, rank), columns by descending eigenvalue (``statserver.py:980-1019``; ``backend.lda_device`` on what defines it)."""
        from . import backend
        return backend.lda_device(*self._device_rows(), rank)

    def get_mahalanobis_matrix_stat1(self):
        """Inverse of the within-class covariance (``statserver.py:1021-1029``)."""
        from . import backend
        return backend.mahalanobis_device(*self._device_rows())

    def get_wccn_choleski_stat1(self):
        """Lower Cholesky factor of the inverse WCCN matrix (``statserver.py:1031-1054``)."""
        from . import backend
        return backend.wccn_device(*self._device_rows())

    def whiten_cholesky_stat1(self, mu, sigma):
        """Centre on ``mu`` and whiten by the Cholesky factor of ``inv(sigma)`` (2-D) or by the square roots of a diagonal covariance
        (1-D), ``statserver.py:898-918``."""
        from . import backend
        if sigma.ndim == 2:
            transform = scipy.linalg.cholesky(scipy.linalg.inv(sigma)).T
        elif sigma.ndim == 1:
            transform = numpy.diag(1 / numpy.sqrt(sigma.astype(STAT_TYPE)))
        else:
            raise Exception('Wrong dimension of Sigma, must be 1 or 2')
        self.stat1 = backend.whiten_rows_device(self._device_rows()[0], numpy.asarray(mu, dtype=STAT_TYPE), transform).cpu().numpy()

    def estimate_spectral_norm_stat1(self, it=1, mode='efr'):
        """Means and covariances of ``it`` iterations of spectral normalisation (``statserver.py:1279-1315``): ``mode='efr'`` (total
        covariance) or ``'sphNorm'`` (within-class covariance).  ``self.stat1`` is left as it is."""
        from . import backend
        xv, index = self._device_rows()
        spectral_norm_mean, spectral_norm_cov, _ = backend.spectral_norm_estimate_device(xv, index, it, mode)
        return spectral_norm_mean, spectral_norm_cov

    def spectral_norm_stat1(self, spectral_norm_mean, spectral_norm_cov, is_sqr_inv_sigma=False):
        """For each ``(mean, covariance)``: centre, whiten, scale to unit length (``statserver.py:1317-1333``), in place."""
        from . import backend
        assert len(spectral_norm_mean) == len(spectral_norm_cov), 'Number of mean vectors and covariance matrices is different'
        self.stat1 = backend.spectral_norm_apply_device(self._device_rows()[0], spectral_norm_mean, spectral_norm_cov, is_sqr_inv_sigma).cpu().numpy()

    def sum_stat_per_model(self):
        """Sum the statistics of the sessions sharing a model id (``statserver.py:1335-1355``) -> ``(StatServer, session_per_model)``: one
        session per (sorted) model and the float64 session counts.  The reference scans all model ids once per class; here one grouping
        of the ids, then the class-sum kernel (``sc_class_sums``, rows of a class added in row order) when a GPU is visible and the same
        grouping on the host otherwise."""
        from .factor_analyser import ClassIndex, class_sums_device
        index = ClassIndex(self.modelset)
        out = StatServer()
        out.modelset = index.ids
        out.segset = copy.deepcopy(out.modelset)
        out.start = numpy.empty(out.segset.shape, '|O')
        out.stop = numpy.empty(out.segset.shape, '|O')
        import torch
        if torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
            out.stat0, out.stat1 = (class_sums_device(torch.as_tensor(numpy.ascontiguousarray(x, dtype=STAT_TYPE)).to(dev), index)[0].cpu().numpy()
                                    for x in (self.stat0, self.stat1))
        else:
            first = numpy.concatenate(([0], numpy.cumsum(index.counts)[:-1]))
            out.stat0, out.stat1 = (numpy.add.reduceat(numpy.asarray(x, dtype=STAT_TYPE)[index.rows], first, axis=0) for x in (self.stat0, self.stat1))
        return out, index.counts.astype(STAT_TYPE)

    def mean_stat_per_model(self):
        """Average the statistics of the sessions sharing a model id -> one session per (sorted) model."""
        out = StatServer()
        out.modelset, inverse = numpy.unique(self.modelset, return_inverse=True)
        out.segset = copy.deepcopy(out.modelset)
        out.start = numpy.empty(out.segset.shape, '|O')
        out.stop = numpy.empty(out.segset.shape, '|O')
        out.stat0 = numpy.zeros((out.modelset.shape[0], self.stat0.shape[1]), dtype=STAT_TYPE)
        out.stat1 = numpy.zeros((out.modelset.shape[0], self.stat1.shape[1]), dtype=STAT_TYPE)
        for idx in range(out.modelset.shape[0]):
            sel = inverse == idx
            out.stat0[idx, :] = self.stat0[sel, :].mean(axis=0)
            out.stat1[idx, :] = self.stat1[sel, :].mean(axis=0)
        return out

    # ---- joint factor analysis on the GPU (sidekit_amd/jfa_scoring.py): no CPU fallback; the caller's statistics are left as they are ---------

    def subtract_weighted_stat1(self, sts):
        """A copy of this server whose ``stat1`` is ``stat1 - stat0[:, index_map] * sts.stat1``, the sessions of ``sts`` matched to these by
        sorted ``segset`` (``statserver.py:819-850``).  Any mismatch of the model sets, the segment sets or the shapes raises."""
        if not (self.modelset.shape == sts.modelset.shape and self.segset.shape == sts.segset.shape
                and all(numpy.sort(sts.modelset) == numpy.sort(self.modelset)) and all(numpy.sort(sts.segset) == numpy.sort(self.segset))
                and sts.stat0.shape == self.stat0.shape and sts.stat1.shape == self.stat1.shape):
            raise Exception('Statserver are not compatible')
        new_sts = copy.deepcopy(self)
        aligned = numpy.empty(self.stat1.shape, dtype=STAT_TYPE)
        aligned[self.segset.argsort(), :] = sts.stat1[sts.segset.argsort(), :]
        n, n_distrib = self.stat0.shape
        new_sts.stat1 = (self._blocks() - self.stat0[:, :, numpy.newaxis] * aligned.reshape(n, n_distrib, -1)).reshape(self.stat1.shape)
        return new_sts

    def estimate_between_class(self, itNb, V, mean, sigma_obs, batch_size=100, Ux=None, Dz=None, minDiv=True, num_thread=1,
                               re_estimate_residual=False, save_partial=False):
        """``itNb`` EM iterations of the eigenvoice matrix ``V`` from the statistics (less ``stat0 * Ux`` when given) summed per model
        (``statserver.py:1494-1567``) -> ``(V, sigma_obs)``.  ``Dz`` is refused: the reference calls a ``subtract`` it does not have.
        ``batch_size`` and ``num_thread`` are accepted and unused."""
        from . import jfa_scoring
        jfa_scoring._refuse(save_partial, re_estimate_residual)
        if Dz is not None:
            raise NotImplementedError("estimate_between_class with Dz is not built (the reference's own call fails: StatServer has no subtract)")
        shifted = self if Ux is None else self.subtract_weighted_stat1(Ux)
        return jfa_scoring.server_estimate_subspace(shifted, itNb, V, mean, sigma_obs, minDiv, per_model=True), sigma_obs

    def estimate_within_class(self, it_nb, U, mean, sigma_obs, batch_size=100, Vy=None, Dz=None, min_div=True, num_thread=1, save_partial=False):
        """``it_nb`` EM iterations of the eigenchannel matrix ``U`` from the sessions less ``stat0 * Vy`` and ``stat0 * Dz`` when given
        (``statserver.py:1569-1628``) -> ``U``.  ``batch_size`` and ``num_thread`` are accepted and unused."""
        from . import jfa_scoring
        jfa_scoring._refuse(save_partial)
        shifted = self
        for shift in (Vy, Dz):
            if shift is not None:
                shifted = shifted.subtract_weighted_stat1(shift)
        return jfa_scoring.server_estimate_subspace(shifted, it_nb, U, mean, sigma_obs, min_div, per_model=False)

    def estimate_map(self, itNb, D, mean, Sigma, Vy=None, Ux=None, num_thread=1, save_partial=False):
        """``itNb`` EM iterations of the diagonal MAP term ``D`` from the statistics centred on ``mean``, less ``stat0 * Vy`` and
        ``stat0 * Ux`` when given, summed per model (``statserver.py:1630-1685``) -> ``D``.  ``num_thread`` is accepted and unused."""
        from . import jfa_scoring
        jfa_scoring._refuse(save_partial)
        shifted = self
        for shift in (Vy, Ux):
            if shift is not None:
                shifted = shifted.subtract_weighted_stat1(shift)
        return jfa_scoring.server_estimate_map(shifted, itNb, D, mean, Sigma)

    def estimate_hidden(self, mean, sigma, V=None, U=None, D=None, batch_size=100, num_thread=1):
        """Point estimates ``(y, x, z)`` of the hidden variables of every session under ``M = mean + V y + U x + D z``, ``(y, x)`` jointly
        (``statserver.py:1687-1796``) -> three ``StatServer`` objects (``z`` is an empty one without ``D``).  The statistics are not
        whitened by the caller and, unlike in the reference, not whitened here either.  ``batch_size`` and ``num_thread`` are accepted
        and unused."""
        from . import jfa_scoring
        return jfa_scoring.server_estimate_hidden(self, mean, sigma, V, U, D)

    def factor_analysis(self, rank_f, rank_g=0, rank_h=None, re_estimate_residual=False, it_nb=(10, 10, 10), min_div=True, ubm=None,
                        batch_size=100, num_thread=1, save_partial=False, init_matrices=(None, None, None)):
        """Train the JFA model ``(mean, F, G, H, sigma)`` on these statistics with ``ubm`` as the origin (``statserver.py:1798-1949``;
        ``sidekit_amd.jfa_scoring.factor_analysis_device``).  ``ubm=None``, ``re_estimate_residual`` and ``save_partial`` are refused;
        ``batch_size`` and ``num_thread`` are accepted and unused."""
        from . import jfa_scoring
        if ubm is not None:
            jfa_scoring._refuse(save_partial, re_estimate_residual)
        return jfa_scoring.server_factor_analysis(self, rank_f, rank_g, rank_h, it_nb, min_div, ubm, init_matrices)

    @staticmethod
    def from_arrays(modelset, segset, stat1, start=None, stop=None):
        """Convenience used by ``extract_embeddings``: x-vectors as ``stat1``, ones as ``stat0`` (xvector.py:1905-1914)."""
        s = StatServer()
        s.modelset = numpy.asarray(modelset)
        s.segset = numpy.asarray(segset)
        n = s.segset.shape[0]
        s.start = numpy.empty(n, dtype="|O") if start is None else numpy.asarray(start)
        s.stop = numpy.empty(n, dtype="|O") if stop is None else numpy.asarray(stop)
        s.stat0 = numpy.ones((n, 1), dtype=STAT_TYPE)
        s.stat1 = numpy.asarray(stat1, dtype=STAT_TYPE)
        return s
