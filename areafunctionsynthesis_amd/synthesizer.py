"""Host-side mirror of the reference's synthesis API on top of libafs.so.

* :class:`Context` -- one ``afs_ctx`` (device, sampling rate, solver, TdsModel options).
* :class:`Synthesizer` -- the stateful ``Synthesizer::synthesizeSignalTds`` equivalent
  (``src/Backend/Synthesizer.cpp:515-639``) for a batch of independent voices, backed by
  an ``afs_session`` whose state stays on the GPU.
* :meth:`Context.synthesize` -- whole trajectories (latch frame 0, then ``F-1`` calls of
  ``hop`` samples) for ``B`` utterances in one go.
* :meth:`Context.synthesize_ragged` -- the same for utterances of different lengths; with
  ``packed=True`` the rows come back without padding, as one flat int16 or float32 array plus offsets
  (:func:`ragged_offsets`).
* :meth:`Context.synthesize_stream` -- continuous batching: a corpus streamed through a pool of
  voices (:meth:`Synthesizer.synthesize_frames`, :meth:`Synthesizer.restart`), a few frames per
  voice and call.
* :meth:`Context.synthesize_corpus` -- the same over one flat corpus array that the voices read in
  place by index (:func:`stream_corpus`): no frame and no audio array is built per step.
* :meth:`Context.synthesize_candidates` -- branching: a prefix played once, forked into K voices
  (:meth:`Synthesizer.fork`, :meth:`Synthesizer.save_voices`, :meth:`Synthesizer.load_voices`,
  :meth:`Synthesizer.copy_voices`), each playing its own continuation.
* :meth:`Context.play_target_sequences` -- ``Synthesizer::playTargetSequence``
  (``src/Backend/Synthesizer.cpp:1299-1422``) for ``B`` utterances: four target shapes each,
  per-sample area-function tubes built on the GPU.

Arrays may be numpy arrays (host) or torch tensors on the GPU (device pointers are
passed straight to the library).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _native
from .frames import FRAME_DTYPE

_vp = ctypes.c_void_p

SOLVERS = {"cholesky": _native.AFS_SOLVER_CHOLESKY, "tree": _native.AFS_SOLVER_TREE, "sor": _native.AFS_SOLVER_SOR}


def _addr(x) -> int:
    if x is None:
        return 0
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    if isinstance(x, np.ndarray):
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError("array must be C-contiguous")
        return int(x.ctypes.data)
    raise TypeError(f"unsupported buffer type {type(x)}")


def _nbytes(x) -> int:
    if hasattr(x, "element_size"):
        return int(x.numel() * x.element_size())
    return int(x.nbytes)


def _pcm_rows(out, B: int):
    """(address, row stride in samples) of the int16 destination ``out[B, width]`` of a PCM call: a
    numpy array or torch tensor whose samples are adjacent within a row; the rows may be strided
    (a slice of a wider buffer)."""
    if len(out.shape) != 2 or int(out.shape[0]) != B:
        raise ValueError("a PCM out must be int16 [B, samples]")
    if isinstance(out, np.ndarray):
        if out.dtype != np.int16:
            raise ValueError("a PCM out must be int16")
        inner, row = out.strides[1] // 2, out.strides[0] // 2
        exact = out.strides[1] % 2 == 0 and out.strides[0] % 2 == 0
        addr = int(out.ctypes.data)
    else:
        if "int16" not in str(out.dtype):
            raise ValueError("a PCM out must be int16")
        inner, row, exact = int(out.stride(1)), int(out.stride(0)), True
        addr = int(out.data_ptr())
    width = int(out.shape[1])
    if not exact or (width > 1 and inner != 1) or (B > 1 and row < width):
        raise ValueError("a PCM out needs adjacent samples in rows that do not overlap")
    return addr, (row if B > 1 else max(row, width))


def _sample_rows(out, B: int, dtype):
    """:func:`_pcm_rows` for a destination of ``dtype`` samples (int16 or float32): (address, row stride)."""
    if dtype == np.int16:
        return _pcm_rows(out, B)
    if len(out.shape) != 2 or int(out.shape[0]) != B:
        raise ValueError("a float32 out must be float32 [B, samples]")
    if isinstance(out, np.ndarray):
        if out.dtype != np.float32:
            raise ValueError("a float32 out must be float32")
        inner, row = out.strides[1] // 4, out.strides[0] // 4
        exact = out.strides[1] % 4 == 0 and out.strides[0] % 4 == 0
        addr = int(out.ctypes.data)
    else:
        if "float32" not in str(out.dtype):
            raise ValueError("a float32 out must be float32")
        inner, row, exact = int(out.stride(1)), int(out.stride(0)), True
        addr = int(out.data_ptr())
    width = int(out.shape[1])
    if not exact or (width > 1 and inner != 1) or (B > 1 and row < width):
        raise ValueError("a float32 out needs adjacent samples in rows that do not overlap")
    return addr, (row if B > 1 else max(row, width))


def _sample_format(pcm: bool, f32: bool, packed: bool = False):
    """(afs_sample_format, numpy dtype) of a call's ``pcm`` / ``f32`` switches, None for the float64 call."""
    if pcm and f32:
        raise ValueError("pcm and f32 are two sample formats: choose one")
    if packed and not (pcm or f32):
        raise ValueError("packed needs pcm=True or f32=True: there is no packed float64 form (the float64 rows "
                         "are written by the synthesis kernel itself, not by the output stage)")
    if f32:
        return _native.AFS_SAMPLE_F32, np.float32
    if pcm:
        return _native.AFS_SAMPLE_I16, np.int16
    return None, np.float64


def ragged_offsets(num_frames, hop: int) -> np.ndarray:
    """afs_ragged_offsets: int64[B + 1], the exclusive prefix sum of ``(num_frames[u]-1)*hop`` with the total
    last -- the tight layout of a packed call; row u is ``flat[offsets[u]:offsets[u + 1]]``."""
    counts = np.ascontiguousarray(num_frames, dtype=np.int32).reshape(-1)
    off = np.zeros(counts.size + 1, dtype=np.int64)
    _native.check(_native.load().afs_ragged_offsets(_vp(_addr(counts)), int(counts.size), int(hop), _vp(_addr(off))),
                  None, "afs_ragged_offsets")
    return off


def _packed_out(out, offsets, lengths, dtype):
    """The destination and row starts of a packed call: (out, its address, offsets int64[B + 1] or [B], the
    host array of row starts to pass or None for tight packing).  ``lengths[u]``: row u's samples (None: the
    row is absent).  ``out=None``: a numpy array of the span; ``offsets=None``: tight in order."""
    B = len(lengths)
    own = None
    if offsets is None:
        off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum([0 if n is None else int(n) for n in lengths], out=off[1:])
        span = int(off[B])
    else:
        own = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if own.size not in (B, B + 1):
            raise ValueError("offsets must hold one row start per utterance")
        off = own
        own = np.ascontiguousarray(own[:B])
        span = max([0] + [int(own[u]) + int(n) for u, n in enumerate(lengths) if n])
    if out is None:
        out = np.zeros(span, dtype=dtype)
    if len(out.shape) != 1:
        raise ValueError("a packed out is 1-D")
    if isinstance(out, np.ndarray):
        if out.dtype != dtype or not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"a packed out must be contiguous {np.dtype(dtype).name}")
    elif np.dtype(dtype).name not in str(out.dtype) or (out.shape[0] > 1 and int(out.stride(0)) != 1):
        raise ValueError(f"a packed out must be contiguous {np.dtype(dtype).name}")
    if int(out.shape[0]) < span:
        raise ValueError(f"a packed out must hold {span} samples")
    return out, (_addr(out) if int(out.shape[0]) else 0), off, own


class Context:
    """An afs_ctx: device + sampling rate + solver + options (TdsModel::Options)."""

    def __init__(self, sampling_rate_hz: float = 22050.0, solver: str = "tree", device: int = 0,
                 async_calls: bool = False, profile: bool = False, lanes: Optional[int] = None, **options):
        """``lanes``: tree solver, lanes per utterance (16: the throughput kernel, 64: the voice
        kernel); None lets the library pick per batch (AFS_LANES_16 / AFS_LANES_64, afs.h)."""
        lib = _native.load()
        cfg = _native.AfsConfig()
        lib.afs_config_default(ctypes.byref(cfg))
        cfg.sampling_rate_hz = float(sampling_rate_hz)
        cfg.solver = SOLVERS[solver]
        cfg.device = int(device)
        cfg.flags = (_native.AFS_ASYNC if async_calls else 0) | (_native.AFS_PROFILE if profile else 0)
        if lanes is not None:
            cfg.flags |= {16: _native.AFS_LANES_16, 64: _native.AFS_LANES_64}[int(lanes)]
        for k, v in options.items():
            if not hasattr(cfg.options, k):
                raise TypeError(f"unknown option {k}")
            if k == "flow_separation_area_ratio":
                setattr(cfg.options, k, float(v))
            elif k in ("glottis_loss", "glottis_model"):
                setattr(cfg.options, k, int(v))
            else:
                setattr(cfg.options, k, int(bool(v)))
        h = _vp()
        _native.check(lib.afs_create(ctypes.byref(h), ctypes.byref(cfg)), None, "afs_create")
        self._lib = lib
        self._h = h
        self.sampling_rate_hz = float(sampling_rate_hz)
        self.solver = solver
        self.device = int(device)

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h:
            self._lib.afs_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lanes_per_utterance(self, batch: int) -> int:
        """Lanes per utterance the tree solver uses for a batch of this size."""
        return int(self._lib.afs_lanes_per_utterance(self._h, int(batch)))

    def synthesis_kernel(self, batch: int) -> str:
        """Name of the synthesis kernel a batch of this size runs (for matching profiler output)."""
        return self._lib.afs_synthesis_kernel(self._h, int(batch)).decode()

    def set_stream(self, stream_handle: int) -> None:
        """Issue all work on this hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""
        _native.check(self._lib.afs_set_stream(self._h, _vp(stream_handle)), self._h, "afs_set_stream")

    def synchronize(self) -> None:
        _native.check(self._lib.afs_synchronize(self._h), self._h, "afs_synchronize")

    def set_taps(self, taps) -> None:
        """The signal taps ``synthesize(..., taps=True)`` and ``synthesize_signal_tds(..., taps=True)``
        return beside the audio (tree solver): up to AFS_MAX_TAPS entries, each a name of
        :data:`TAPS`, ``("pressure", section)`` or ``("current", index)`` in the reference's
        numbering.  An empty list clears them."""
        taps = [tap(t) for t in taps]
        arr = (_native.AfsTap * max(len(taps), 1))(*[_native.AfsTap(k, i) for k, i in taps])
        _native.check(self._lib.afs_set_taps(self._h, arr, len(taps)), self._h, "afs_set_taps")
        self.n_taps = len(taps)

    def memory_info(self) -> dict:
        """afs_memory_info_get: the device memory the context holds now -- ``total_bytes``, and
        ``sample_buffer_bytes``, the part holding one fp64 value per utterance-sample (the launch
        windows, staged fp64 audio or taps)."""
        m = _native.AfsMemoryInfo()
        _native.check(self._lib.afs_memory_info_get(self._h, ctypes.byref(m)), self._h, "afs_memory_info_get")
        return {"total_bytes": int(m.total_bytes), "sample_buffer_bytes": int(m.sample_buffer_bytes)}

    def synthesize(self, frames, hop: int, seeds=None, out=None, report: bool = False, nonfinite=None,
                   taps=False, taps_out=None, pcm: bool = False, f32: bool = False):
        """frames[B, F] (FRAME_DTYPE array, or a uint8 torch tensor [B, F, 1072] on the GPU)
        -> audio[B, (F-1)*hop] float64.  ``seeds=None``: 1 .. B.  ``nonfinite``: optional uint8
        array / tensor of B flags (1 = the utterance's audio holds NaN/Inf); with ``report``
        the returned dict carries them under ``nonfinite`` too.  ``taps=True``: returns
        ``(audio, taps[B, n_taps, T])`` -- the taps of :meth:`set_taps` after every sample
        (``taps_out``: a numpy array or GPU tensor to receive them) -- and with ``report``
        ``(audio, taps, report)``.  ``pcm=True``: the audio as int16[B, T] (afs_synthesize_pcm: bit
        for bit :meth:`to_int16` of the float64 audio, which is then never stored); ``out`` may be an
        int16 numpy array or GPU tensor [B, T] with strided rows.  No taps with ``pcm``.  ``f32=True``:
        the audio as float32[B, T] likewise (afs_synthesize_f32: bit for bit ``np.float32`` of the float64
        audio, non-finite values included); ``pcm`` and ``f32`` together is an error."""
        fmt, dtype = _sample_format(pcm, f32)
        pcm = fmt is not None  # (below: a call of the sample-format family)
        if pcm and taps:
            raise ValueError("the PCM calls have no taps")
        if isinstance(frames, np.ndarray):
            if frames.dtype != FRAME_DTYPE or frames.ndim != 2:
                raise ValueError("frames must be a 2-D FRAME_DTYPE array [B, F]")
            B, F = frames.shape
            frames = np.ascontiguousarray(frames)
        else:
            B, F = int(frames.shape[0]), int(frames.shape[1])
            if _nbytes(frames) != B * F * FRAME_DTYPE.itemsize:
                raise ValueError("device frames must hold B*F*1072 bytes")
        T = (F - 1) * hop
        if seeds is None:
            seeds = np.arange(1, B + 1, dtype=np.uint32)
        if isinstance(seeds, np.ndarray):
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if out is None:
            out = np.zeros((B, T), dtype=dtype)
        if pcm:
            if tuple(out.shape) != (B, T):
                raise ValueError("a PCM or float32 out must be [B, (F-1)*hop]")
            pcm_addr, pcm_stride = _sample_rows(out, B, dtype)
        elif _nbytes(out) != B * T * 8:
            raise ValueError("out must hold B*(F-1)*hop doubles")
        if nonfinite is None and report:
            nonfinite = np.zeros(B, dtype=np.uint8)
        if nonfinite is not None and _nbytes(nonfinite) != B:
            raise ValueError("nonfinite must hold B bytes")
        # (a report makes the call wait for the device: only when asked, so that an AFS_ASYNC context's
        # calls with device buffers return once queued)
        rep = _native.AfsReport()
        if taps:
            nt = getattr(self, "n_taps", 0)
            if taps_out is None:
                taps_out = np.zeros((B, nt, T), dtype=np.float64)
            if nt and _nbytes(taps_out) != B * nt * T * 8:  # (no taps set: the library refuses the call)
                raise ValueError("taps_out must hold B*n_taps*(F-1)*hop doubles")
            st = self._lib.afs_synthesize_taps(self._h, _vp(_addr(frames)), _vp(_addr(seeds)), B, F, hop,
                                               _vp(_addr(out)), _vp(_addr(taps_out)), _vp(_addr(nonfinite)),
                                               ctypes.byref(rep) if report else None)
            _native.check(st, self._h, "afs_synthesize_taps")
        elif pcm:
            name = "afs_synthesize_f32" if f32 else "afs_synthesize_pcm"
            st = getattr(self._lib, name)(self._h, _vp(_addr(frames)), _vp(_addr(seeds)), B, F, hop, _vp(pcm_addr),
                                          pcm_stride, _vp(_addr(nonfinite)), ctypes.byref(rep) if report else None)
            _native.check(st, self._h, name)
        else:
            st = self._lib.afs_synthesize(self._h, _vp(_addr(frames)), _vp(_addr(seeds)), B, F, hop,
                                          _vp(_addr(out)), _vp(_addr(nonfinite)), ctypes.byref(rep) if report else None)
            _native.check(st, self._h, "afs_synthesize")
        res = (out, taps_out) if taps else (out,)
        if report:
            res += ({"device_ms": rep.device_ms, "samples": rep.samples,
                     "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                     "nonfinite": nonfinite},)
        return res if len(res) > 1 else res[0]

    def synthesize_ragged(self, frames, num_frames, hop: int, seeds=None, out=None, report: bool = False,
                          nonfinite=None, taps=False, taps_out=None, pcm: bool = False, f32: bool = False,
                          packed: bool = False, offsets=None):
        """:meth:`synthesize` for utterances of different lengths in one call (tree solver).
        ``frames``: a ``[B, Fmax]`` FRAME_DTYPE array or uint8 GPU tensor ``[B, Fmax, 1072]`` of which
        utterance u plays the first ``num_frames[u]`` frames (the rest is never read), or a list of
        per-utterance FRAME_DTYPE arrays (``num_frames=None``: their lengths), which is padded.
        Returns ``(audio[B, out_stride], lengths[B])`` with ``lengths[u] = (num_frames[u]-1)*hop``
        valid samples in row u -- ``out_stride`` is the longest utterance's, or the row length of a
        given ``out`` -- then the taps ``[B, n_taps, out_stride]`` and the report as :meth:`synthesize`
        appends them.  Row u is bit for bit ``synthesize(frames[u:u+1, :num_frames[u]], hop)`` with
        its seed.  Nothing is written past a row's end: an ``out`` allocated here is zero there.
        ``pcm=True``: the audio as int16 (afs_synthesize_ragged_pcm; ``out``: int16 ``[B, out_stride]``,
        numpy or GPU tensor, rows may be strided); no taps.
        ``packed=True`` with ``pcm=True`` or ``f32=True`` (afs_synthesize_ragged_packed): returns ``(flat,
        offsets)`` (then the report) instead -- the rows without padding in one 1-D int16 or float32 array,
        row u at ``flat[offsets[u]:offsets[u + 1]]``, ``offsets`` int64 ``[B + 1]`` (:func:`ragged_offsets`).
        ``out``: a 1-D numpy array or GPU tensor of that dtype to receive them; ``offsets``: the caller's
        own row starts ``[B]`` in samples, in any order and with gaps (returned as given; row u is
        ``flat[offsets[u]:offsets[u] + (num_frames[u]-1)*hop]``, nothing else is written).  ``f32`` needs
        ``packed``; there is no packed float64 form."""
        fmt, dtype = _sample_format(pcm, f32, packed)
        if f32 and not packed:
            raise ValueError("a ragged float32 call is packed: pass packed=True")
        if offsets is not None and not packed:
            raise ValueError("offsets belong to a packed call")
        pcm = fmt is not None
        if pcm and taps:
            raise ValueError("the PCM calls have no taps")
        if isinstance(frames, (list, tuple)):
            rows = [np.ascontiguousarray(f, dtype=FRAME_DTYPE).reshape(-1) for f in frames]
            if num_frames is None:
                num_frames = [len(r) for r in rows]
            padded = np.zeros((len(rows), max(len(r) for r in rows)), dtype=FRAME_DTYPE)
            for u, r in enumerate(rows):
                padded[u, : len(r)] = r
            frames = padded
        if isinstance(frames, np.ndarray):
            if frames.dtype != FRAME_DTYPE or frames.ndim != 2:
                raise ValueError("frames must be a 2-D FRAME_DTYPE array [B, Fmax]")
            B, fstride = frames.shape
            frames = np.ascontiguousarray(frames)
        else:
            B, fstride = int(frames.shape[0]), int(frames.shape[1])
            if _nbytes(frames) != B * fstride * FRAME_DTYPE.itemsize:
                raise ValueError("device frames must hold B*Fmax*1072 bytes")
        counts = None
        if num_frames is not None:  # (a host array: the library builds the launch layout from it)
            counts = np.ascontiguousarray(num_frames, dtype=np.int32)
            if counts.shape != (B,):
                raise ValueError("num_frames must hold B counts")
        lengths = None if counts is None else (counts.astype(np.int64) - 1) * hop
        if seeds is None:
            seeds = np.arange(1, B + 1, dtype=np.uint32)
        if isinstance(seeds, np.ndarray):
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if nonfinite is None and report:
            nonfinite = np.zeros(B, dtype=np.uint8)
        if nonfinite is not None and _nbytes(nonfinite) != B:
            raise ValueError("nonfinite must hold B bytes")
        if packed:
            if lengths is None:
                raise ValueError("num_frames must hold B counts")
            out, addr, off, own = _packed_out(out, offsets, [max(int(n), 0) for n in lengths], dtype)
            rep = _native.AfsReport()
            st = self._lib.afs_synthesize_ragged_packed(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                        _vp(_addr(seeds)), B, hop, fmt, _vp(addr), _vp(_addr(own)),
                                                        _vp(_addr(nonfinite)), ctypes.byref(rep) if report else None)
            _native.check(st, self._h, "afs_synthesize_ragged_packed")
            if report:
                return out, off, {"device_ms": rep.device_ms, "samples": rep.samples,
                                  "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                                  "nonfinite": nonfinite}
            return out, off
        if out is None:
            out = np.zeros((B, max(int(lengths.max()), 0) if lengths is not None else 0),
                           dtype=np.int16 if pcm else np.float64)
        if tuple(out.shape)[:1] != (B,) or len(out.shape) != 2:
            raise ValueError("out must be [B, out_stride] doubles")
        ostride = int(out.shape[1])
        if pcm:
            pcm_addr, pcm_stride = _pcm_rows(out, B)
        elif _nbytes(out) != B * ostride * 8:
            raise ValueError("out must be [B, out_stride] doubles")
        if nonfinite is None and report:
            nonfinite = np.zeros(B, dtype=np.uint8)
        if nonfinite is not None and _nbytes(nonfinite) != B:
            raise ValueError("nonfinite must hold B bytes")
        if taps:
            nt = getattr(self, "n_taps", 0)
            if taps_out is None:
                taps_out = np.zeros((B, nt, ostride), dtype=np.float64)
            if nt and _nbytes(taps_out) != B * nt * ostride * 8:  # (no taps set: the library refuses the call)
                raise ValueError("taps_out must hold B*n_taps*out_stride doubles")
        rep = _native.AfsReport()
        if pcm:
            st = self._lib.afs_synthesize_ragged_pcm(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                     _vp(_addr(seeds)), B, hop, _vp(pcm_addr), pcm_stride,
                                                     _vp(_addr(nonfinite)), ctypes.byref(rep) if report else None)
            _native.check(st, self._h, "afs_synthesize_ragged_pcm")
        else:
            st = self._lib.afs_synthesize_ragged(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                 _vp(_addr(seeds)), B, hop, _vp(_addr(out)), ostride,
                                                 _vp(_addr(taps_out) if taps else 0), _vp(_addr(nonfinite)),
                                                 ctypes.byref(rep) if report else None)
            _native.check(st, self._h, "afs_synthesize_ragged")
        res = (out, lengths) + ((taps_out,) if taps else ())
        if report:
            res += ({"device_ms": rep.device_ms, "samples": rep.samples,
                     "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                     "nonfinite": nonfinite},)
        return res

    def synthesize_stream(self, utterances, hop: int, slots: int, chunk_frames: int, seeds=None, pcm: bool = True,
                          finished=None):
        """Continuous batching (tree solver): a generator over ``utterances``, an iterable of
        per-utterance FRAME_DTYPE arrays of at least 2 frames, yielding ``(index, audio)`` as each one
        ends -- int16 with ``pcm``, else float64; ``(F-1)*hop`` samples.  A session of ``slots`` voices
        plays up to ``chunk_frames`` frames of every live utterance per step (:func:`stream_utterances`),
        so the frames and audio held at a time are slots x chunk_frames, whatever the corpus holds.
        ``seeds``: indexable by utterance (None: index + 1).  Utterance i's audio is bit for bit
        ``synthesize(utterances[i][None], hop, seeds=[seed_i])`` on a context of the session's lane
        width.  ``finished(index, slot, session, nonfinite)``: called when an utterance ends, before its
        voice is restarted."""
        session = Synthesizer(self, int(slots))
        try:
            yield from stream_utterances(session, utterances, hop, chunk_frames, seeds=seeds, pcm=pcm,
                                         finished=finished)
        finally:
            session.close()

    def synthesize_corpus(self, frames, frame_offsets, hop: int, slots: int, chunk_frames: int, seeds=None,
                          pcm: bool = True, f32: bool = False, out=None):
        """Continuous batching over a flat corpus (tree solver): ``frames`` is one 1-D FRAME_DTYPE array or
        GPU tensor holding every utterance, utterance i at ``frames[frame_offsets[i]:frame_offsets[i + 1]]``
        (at least 2 frames).  A session of ``slots`` voices plays up to ``chunk_frames`` frames of every
        live utterance per step, reading them in place by index (afs_session_synthesize_indexed_packed) and
        writing each sample at its final offset; a voice that finishes takes the next utterance
        (:func:`stream_corpus`).  Returns ``(flat, offsets, nonfinite)``: utterance i's audio is
        ``flat[offsets[i]:offsets[i + 1]]``, int16 (``pcm``) or float32 (``f32``), bit for bit
        ``synthesize_ragged(..., packed=True)`` of the corpus and ``synthesize(utterance_i[None], hop,
        seeds=[seed_i])`` on a context of the session's lane width.  ``seeds``: one per utterance (None:
        index + 1).  ``out``: a 1-D buffer of ``offsets[n]`` samples of the caller's, numpy or GPU tensor."""
        _, dtype = _sample_format(pcm, f32, True)
        buf = out
        if buf is None:  # (the audio stays on this context's device for the whole run and comes back once)
            import torch
            counts = np.diff(np.ascontiguousarray(frame_offsets, dtype=np.int64).reshape(-1))
            total = int((np.maximum(counts, 1) - 1).sum()) * int(hop)
            buf = torch.zeros(total, dtype=torch.int16 if dtype == np.int16 else torch.float32,
                              device=torch.device("cuda", self.device))
        session = Synthesizer(self, int(slots))
        try:
            flat, offsets, nonfinite = stream_corpus(session, frames, frame_offsets, hop, chunk_frames, seeds=seeds,
                                                     pcm=pcm, f32=f32, out=buf)
        finally:
            session.close()
        return (flat.cpu().numpy() if out is None else flat), offsets, nonfinite

    def synthesize_candidates(self, prefix, candidates, hop: int, seed: int = 1, pcm: bool = False):
        """Branching (tree solver): ``prefix[Fp]`` is played once, on voice 0 of a session of K voices
        seeded ``seed``; that voice is forked into all K, and voice k plays ``candidates[k][Fc]``
        (a ``[K, Fc]`` FRAME_DTYPE array).  Returns the candidates' audio ``[K, Fc*hop]`` -- float64, or
        int16 with ``pcm`` -- row k bit for bit the last ``Fc*hop`` samples of
        ``synthesize(concat(prefix, candidates[k])[None], hop, seeds=[seed])`` on a context of the
        session's lane width: prefix + K x candidate samples are computed instead of K x (prefix +
        candidate)."""
        candidates = np.ascontiguousarray(candidates, dtype=FRAME_DTYPE)
        if candidates.ndim != 2 or candidates.shape[0] < 1:
            raise ValueError("candidates must be a FRAME_DTYPE array [K, Fc]")
        K = candidates.shape[0]
        session = Synthesizer(self, K, np.full(K, int(seed), dtype=np.uint32))
        try:
            return branch_candidates(session, prefix, candidates, hop, pcm=pcm)
        finally:
            session.close()

    def noise_plans(self, frames: np.ndarray, hop: int, s_begin: int = 0, s_end: Optional[int] = None) -> np.ndarray:
        """Diagnostics (tree solver): the noise-source plan records K5 computes for samples
        [s_begin, s_end) of frames[rows, F] -> uint64[rows, s_end - s_begin, AFS_PLAN_WORDS]."""
        if frames.dtype != FRAME_DTYPE or frames.ndim != 2:
            raise ValueError("frames must be a 2-D FRAME_DTYPE array [rows, F]")
        rows, F = frames.shape
        if s_end is None:
            s_end = (F - 1) * hop
        frames = np.ascontiguousarray(frames)
        out = np.zeros((rows, s_end - s_begin, _native.AFS_PLAN_WORDS), dtype=np.uint64)
        st = self._lib.afs_noise_plans(self._h, _vp(_addr(frames)), rows, F, hop, s_begin, s_end, _vp(_addr(out)))
        _native.check(st, self._h, "afs_noise_plans")
        return out

    def noise_plan_hops(self, frames: np.ndarray, hop: int, s_begin: int = 0, s_end: Optional[int] = None):
        """Diagnostics (tree solver, hop >= AFS_PLAN_HOP_MIN): K5's hop records of the hops samples
        [s_begin, s_end) span -> (uint8[rows, slots, AFS_PLAN_HOP_BYTES], the dense records of the
        mixed hops' samples uint64[rows, s_end - s_begin, AFS_PLAN_WORDS], zero elsewhere)."""
        if frames.dtype != FRAME_DTYPE or frames.ndim != 2:
            raise ValueError("frames must be a 2-D FRAME_DTYPE array [rows, F]")
        rows, F = frames.shape
        if s_end is None:
            s_end = (F - 1) * hop
        frames = np.ascontiguousarray(frames)
        slots = (s_end - 1) // hop - s_begin // hop + 1
        hops = np.zeros((rows, slots, _native.AFS_PLAN_HOP_BYTES), dtype=np.uint8)
        plans = np.zeros((rows, s_end - s_begin, _native.AFS_PLAN_WORDS), dtype=np.uint64)
        st = self._lib.afs_noise_plan_hops(self._h, _vp(_addr(frames)), rows, F, hop, s_begin, s_end,
                                           _vp(_addr(hops)), _vp(_addr(plans)))
        _native.check(st, self._h, "afs_noise_plan_hops")
        return hops, plans

    def plan_hop_words(self, hops: np.ndarray, ratio: np.ndarray) -> np.ndarray:
        """Diagnostics (tree solver): the plan words the synthesis kernel evaluates per sample from
        hop records hops[n, AFS_PLAN_HOP_BYTES] (uint8) at ratio[n] -> uint64[n, AFS_PLAN_WORDS]."""
        hops = np.ascontiguousarray(hops, dtype=np.uint8)
        ratio = np.ascontiguousarray(ratio, dtype=np.float64)
        n = ratio.shape[0]
        if hops.shape != (n, _native.AFS_PLAN_HOP_BYTES):
            raise ValueError("hops must be uint8[n, AFS_PLAN_HOP_BYTES]")
        out = np.zeros((n, _native.AFS_PLAN_WORDS), dtype=np.uint64)
        st = self._lib.afs_plan_hop_words(self._h, _vp(_addr(hops)), _vp(_addr(ratio)), n, _vp(_addr(out)))
        _native.check(st, self._h, "afs_plan_hop_words")
        return out

    def tube_interpolate(self, left: np.ndarray, right: np.ndarray, ratio: np.ndarray):
        """Diagnostics (tree solver): the synthesis kernel's interpolated pharynx/mouth areas and
        lengths for frames left[n], right[n] at ratio[n] -> (area[n, 40], length[n, 40])."""
        left = np.ascontiguousarray(left, dtype=FRAME_DTYPE)
        right = np.ascontiguousarray(right, dtype=FRAME_DTYPE)
        ratio = np.ascontiguousarray(ratio, dtype=np.float64)
        n = ratio.shape[0]
        if left.shape != (n,) or right.shape != (n,):
            raise ValueError("left, right and ratio must have n entries")
        area = np.zeros((n, 40))
        length = np.zeros((n, 40))
        st = self._lib.afs_tube_interpolate(self._h, _vp(_addr(left)), _vp(_addr(right)), _vp(_addr(ratio)), n,
                                            _vp(_addr(area)), _vp(_addr(length)))
        _native.check(st, self._h, "afs_tube_interpolate")
        return area, length

    def device_math(self, op, a: np.ndarray, b: Optional[np.ndarray] = None) -> np.ndarray:
        """Diagnostics (tree solver): out[k] = op(a[k], b[k]) with the synthesis kernel's device-only
        arithmetic (csrc/tree_core.h, compiled with the kernel's flags); op: a name or value of
        _native.MATH_OPS (afs_device_math.h), b: as many operands as a (zeros when the op takes one)."""
        op = _native.MATH_OPS[op] if isinstance(op, str) else int(op)
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.float64).ravel()
        if b.shape != a.shape:
            raise ValueError("a and b must have the same number of operands")
        out = np.zeros_like(a)
        st = self._lib.afs_device_math(self._h, op, _vp(_addr(a)), _vp(_addr(b)), a.shape[0], _vp(_addr(out)))
        _native.check(st, self._h, "afs_device_math")
        return out

    def kernel_times(self) -> dict:
        """(profile=True contexts) summed device time and count of the synthesis-kernel (K1),
        noise-source-plan (K5) and output-stage (K6) launches since the previous call (waits for
        the stream)."""
        t = _native.AfsKernelTiming()
        _native.check(self._lib.afs_kernel_times_ex(self._h, ctypes.byref(t)), self._h, "afs_kernel_times_ex")
        return {"synth_ms": t.synth_ms, "synth_launches": t.synth_launches, "plan_ms": t.plan_ms,
                "plan_launches": t.plan_launches, "output_ms": t.output_ms, "output_launches": t.output_launches}

    def rng_draws(self, batch: int) -> np.ndarray:
        """rand() calls per utterance of the last synthesize / play_target_sequences call
        (tree solver; the reference's count is what a wrapped rand() would count)."""
        d = np.zeros(int(batch), dtype=np.int64)
        _native.check(self._lib.afs_rng_draws(self._h, int(batch), _vp(_addr(d))), self._h, "afs_rng_draws")
        return d

    def af_to_frames(self, params, frames=None):
        """OneDimAreaFunction::calculateOneDimTubeFunction on the GPU.
        params[..., 16] -> frames[...] (tube fields filled; velum/glottis left as given)."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        shape = p.shape[:-1]
        n = int(np.prod(shape)) if shape else 1
        if frames is None:
            frames = np.zeros(shape, dtype=FRAME_DTYPE)
        st = self._lib.afs_af_to_frames(self._h, _vp(_addr(p)), n, _vp(_addr(frames)))
        _native.check(st, self._h, "afs_af_to_frames")
        return frames


    def target_sequence_samples(self, timing: Optional[dict] = None) -> int:
        """numSamples of playTargetSequence (``SAMPLING_RATE * totalTime_s``, truncated)."""
        ts = target_sequence(timing)
        return int(self._lib.afs_target_sequence_samples(ctypes.byref(ts), self.sampling_rate_hz))

    def play_target_sequences(self, shapes, targets, timing: Optional[dict] = None, seeds=None, out=None,
                              report: bool = False):
        """``playTargetSequence(targetShape, stationary_s, transition_s)`` for every row of
        ``targets[B, 4]`` (indices into ``shapes[S, 16]``) -> audio[B, T] float64.

        ``timing`` overrides fields of :func:`target_sequence` (``stationary_s``,
        ``transition_s``, ``f0_hz``, ``lung_pressure_dpa``, ``glottis``)."""
        shapes = np.ascontiguousarray(shapes, dtype=np.float64)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        if shapes.ndim != 2 or shapes.shape[1] != 16 or targets.ndim != 2 or targets.shape[1] != 4:
            raise ValueError("shapes must be [S, 16] and targets [B, 4]")
        ts = target_sequence(timing)
        B = targets.shape[0]
        T = int(self._lib.afs_target_sequence_samples(ctypes.byref(ts), self.sampling_rate_hz))
        if T < 0:
            raise ValueError("bad target-sequence timing")
        if seeds is None:
            seeds = np.arange(1, B + 1, dtype=np.uint32)
        if isinstance(seeds, np.ndarray):
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if out is None:
            out = np.zeros((B, T), dtype=np.float64)
        if _nbytes(out) != B * T * 8:
            raise ValueError("out must hold B*T doubles")
        nonfinite = np.zeros(B, dtype=np.uint8) if report else None
        rep = _native.AfsReport()
        st = self._lib.afs_play_target_sequences(self._h, _vp(_addr(shapes)), shapes.shape[0], _vp(_addr(targets)),
                                                 ctypes.byref(ts), _vp(_addr(seeds)), B, _vp(_addr(out)),
                                                 _vp(_addr(nonfinite)), ctypes.byref(rep))
        _native.check(st, self._h, "afs_play_target_sequences")
        if report:
            return out, {"device_ms": rep.device_ms, "samples": rep.samples,
                         "nonfinite_utterances": rep.nonfinite_utterances, "nonfinite": nonfinite}
        return out

    def to_int16(self, samples, out=None):
        """The reference's int16 audio ring format (Synthesizer.cpp:955-973) on the GPU:
        short(x * 32767) truncated, clipped outside [-1, 1], NaN -> 0."""
        if isinstance(samples, np.ndarray):
            samples = np.ascontiguousarray(samples, dtype=np.float64)
            n = samples.size
            if out is None:
                out = np.zeros(samples.shape, dtype=np.int16)
        else:
            n = int(samples.numel())
            if out is None:
                import torch
                out = torch.empty(tuple(samples.shape), dtype=torch.int16, device=samples.device)
        if _nbytes(out) != n * 2:
            raise ValueError("out must hold one int16 per sample")
        st = self._lib.afs_to_int16(self._h, _vp(_addr(samples)), n, _vp(_addr(out)))
        _native.check(st, self._h, "afs_to_int16")
        return out


# Names of the usual taps: (kind, index) in the reference's numbering.  Branch current c flows into
# section c for c < Tube::NUM_SECTIONS = 93 (TdsModel.cpp:93-98); the sections are Tube.h:53-79's.
TAPS = {
    # the flow through the glottis: the current into the upper glottis section 24 out of the lower
    # one, 23 (TdsModel.cpp:96-97, sourceSection = i - 1; Tube.h:66-67 the glottis sections)
    "glottal_flow": (_native.AFS_TAP_CURRENT, 24),
    # the two currents from the mouth opening into free space (TdsModel.cpp:115-121: NUM_SECTIONS,
    # NUM_SECTIONS + 1, source LAST_MOUTH_SECTION): through the radiation resistance and inductance
    "mouth_radiation_r": (_native.AFS_TAP_CURRENT, 93),
    "mouth_radiation_l": (_native.AFS_TAP_CURRENT, 94),
    # the two currents from the nostrils into free space (TdsModel.cpp:125-131: NUM_SECTIONS + 2, + 3)
    "nostril_radiation_r": (_native.AFS_TAP_CURRENT, 95),
    "nostril_radiation_l": (_native.AFS_TAP_CURRENT, 96),
    # the flow into the nose: FIRST_NOSE_SECTION's current, out of LAST_PHARYNX_SECTION (TdsModel.cpp:103)
    "nasal_flow": (_native.AFS_TAP_CURRENT, 65),
    # the subglottal pressure: LAST_TRACHEA_SECTION (Tube.h:74; section 22)
    "subglottal_pressure": (_native.AFS_TAP_PRESSURE, 22),
}
FIRST_PHARYNX_SECTION, FIRST_MOUTH_SECTION = 25, 41  # Tube.h:68-69
NUM_PHARYNX_MOUTH_SECTIONS = 40


def pharynx_mouth_pressure(i: int):
    """The pressure tap of pharynx/mouth section ``i`` (0 .. 39: the index of afs_frame's area_cm2;
    Tube section FIRST_PHARYNX_SECTION + i, Tube.h:68-69), e.g. the intra-oral
    pressure behind a constriction at section i + 1."""
    if not 0 <= int(i) < NUM_PHARYNX_MOUTH_SECTIONS:
        raise ValueError("pharynx/mouth sections are 0 .. 39")
    return (_native.AFS_TAP_PRESSURE, FIRST_PHARYNX_SECTION + int(i))


def tap(t):
    """(kind, index) of a tap given as a name of TAPS, ("pressure" | "current", index) or (kind, index)."""
    if isinstance(t, str):
        return TAPS[t]
    kind, index = t
    if isinstance(kind, str):
        kind = {"pressure": _native.AFS_TAP_PRESSURE, "current": _native.AFS_TAP_CURRENT}[kind]
    return int(kind), int(index)


def section_currents(section: int):
    """TdsModel's getCurrentIn / getCurrentOut topology: (in, (out0, out1)) of a section, -1: none."""
    cin, cout = ctypes.c_int32(), (ctypes.c_int32 * 2)()
    _native.check(_native.load().afs_section_currents(int(section), ctypes.byref(cin), cout), None,
                  "afs_section_currents")
    return cin.value, (cout[0], cout[1])


def shard_range(total: int, world: int, rank: int):
    """afs_shard_range: (first, count) of ``rank``'s contiguous block of ``total`` utterances."""
    f, n = ctypes.c_int64(), ctypes.c_int64()
    _native.load().afs_shard_range(int(total), int(world), int(rank), ctypes.byref(f), ctypes.byref(n))
    return f.value, n.value


def comm_unique_id() -> bytes:
    """afs_comm_unique_id (rank 0): the RCCL id every rank passes to :class:`Comm`."""
    buf = (ctypes.c_uint8 * _native.AFS_COMM_ID_BYTES)()
    _native.check(_native.load().afs_comm_unique_id(buf), None, "afs_comm_unique_id")
    return bytes(buf)


class Comm:
    """afs_comm: this process's rank of the audio gather (one process per GPU, RCCL)."""

    def __init__(self, ctx: Context, uid: bytes, rank: int, world: int):
        if len(uid) != _native.AFS_COMM_ID_BYTES:
            raise ValueError("the unique id holds AFS_COMM_ID_BYTES bytes")
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        buf = (ctypes.c_uint8 * _native.AFS_COMM_ID_BYTES).from_buffer_copy(uid)
        h = _vp()
        _native.check(ctx._lib.afs_comm_create(ctx.handle, buf, self.rank, self.world, ctypes.byref(h)), ctx.handle,
                      "afs_comm_create")
        self._h, self._lib = h, ctx._lib

    def gather_pcm(self, local, root_out=None, root_counts=None) -> None:
        """afs_gather_pcm: int16 device tensor ``local`` to rank 0's ``root_out`` (device)."""
        counts = None
        if root_counts is not None:
            counts = np.ascontiguousarray(root_counts, dtype=np.int64)
        n = int(local.numel()) if hasattr(local, "numel") else int(local.size)
        _native.check(self._lib.afs_gather_pcm(self._h, _vp(_addr(local)), n, _vp(_addr(root_out)),
                                               _vp(_addr(counts))), self.ctx.handle, "afs_gather_pcm")

    def fence(self) -> None:
        _native.check(self._lib.afs_comm_fence(self._h), self.ctx.handle, "afs_comm_fence")

    def synchronize(self) -> None:
        _native.check(self._lib.afs_comm_synchronize(self._h), self.ctx.handle, "afs_comm_synchronize")

    def gather_times(self) -> dict:
        """afs_comm_gather_times: device time and count of this rank's gathers since the last call
        (HIP events on the comm's stream; waits for it)."""
        ms, n = ctypes.c_double(), ctypes.c_int32()
        _native.check(self._lib.afs_comm_gather_times(self._h, ctypes.byref(ms), ctypes.byref(n)), self.ctx.handle,
                      "afs_comm_gather_times")
        return {"gather_ms": ms.value, "gathers": n.value}

    def close(self) -> None:
        if self._h:
            self._lib.afs_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Node:
    """Several GPUs driven from this one process (afs_comm_create_all + afs_multi_synthesize):
    ``synthesize`` shards the batch over the devices and returns the int16 audio of the whole
    batch, gathered to the first device over RCCL."""

    def __init__(self, sampling_rate_hz: float, devices: Sequence[int], solver: str = "tree", **options):
        self.ctxs = [Context(sampling_rate_hz, solver=solver, device=d, **options) for d in devices]
        n = len(self.ctxs)
        hs = (_vp * n)(*[c.handle for c in self.ctxs])
        self._comms = (_vp * n)()
        lib = self.ctxs[0]._lib
        _native.check(lib.afs_comm_create_all(hs, n, self._comms), self.ctxs[0].handle, "afs_comm_create_all")
        self._hs, self._lib = hs, lib

    def synthesize(self, frames: np.ndarray, hop: int, seeds=None, pcm_out=None, report: bool = False):
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        B, F = frames.shape
        T = (F - 1) * hop
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        if pcm_out is None:
            pcm_out = np.zeros((B, T), dtype=np.int16)
        nonfinite = np.zeros(B, dtype=np.uint8)
        rep = _native.AfsReport()
        st = self._lib.afs_multi_synthesize(self._hs, self._comms, len(self.ctxs), _vp(_addr(frames)),
                                            _vp(_addr(seeds)), B, F, hop, _vp(_addr(pcm_out)), _vp(_addr(nonfinite)),
                                            ctypes.byref(rep))
        _native.check(st, self.ctxs[0].handle, "afs_multi_synthesize")
        if report:
            return pcm_out, {"device_ms": rep.device_ms, "samples": rep.samples,
                             "nonfinite_utterances": rep.nonfinite_utterances, "nonfinite": nonfinite}
        return pcm_out

    def close(self) -> None:
        for i in range(len(self.ctxs)):
            if self._comms[i]:
                self._lib.afs_comm_destroy(self._comms[i])
                self._comms[i] = None
        for c in self.ctxs:
            c.close()


def target_sequence(overrides: Optional[dict] = None) -> "_native.AfsTargetSequence":
    """afs_target_sequence with the reference's constants (afs_target_sequence_default) and
    the given fields replaced."""
    ts = _native.AfsTargetSequence()
    _native.load().afs_target_sequence_default(ctypes.byref(ts))
    for k, v in (overrides or {}).items():
        if not hasattr(ts, k):
            raise TypeError(f"unknown target-sequence field {k}")
        cur = getattr(ts, k)
        if isinstance(cur, float):
            setattr(ts, k, float(v))
        else:
            vals = list(v)
            if len(vals) != len(cur):
                raise ValueError(f"{k} takes {len(cur)} values")
            for i, x in enumerate(vals):
                cur[i] = float(x)
    return ts


class Synthesizer:
    """Batch of ``B`` voices with the reference's incremental synthesis semantics.

    ``synthesize_signal_tds(frames, n)`` is ``Synthesizer::synthesizeSignalTds(newTube,
    newGlottisParams, n, newSignal)`` applied to every voice: the first call after
    construction / :meth:`reset` only latches the frames and returns an empty array.
    """

    def __init__(self, context: Context, batch: int = 1, seeds: Optional[Sequence[int]] = None):
        self.ctx = context
        self.batch = int(batch)
        lib = context._lib
        s = np.arange(1, self.batch + 1, dtype=np.uint32) if seeds is None else np.asarray(seeds, dtype=np.uint32)
        h = _vp()
        _native.check(lib.afs_session_create(context.handle, self.batch, _vp(_addr(s)), ctypes.byref(h)),
                      context.handle, "afs_session_create")
        self._h = h
        self._lib = lib

    def reset(self, seeds: Optional[Sequence[int]] = None) -> None:
        s = np.arange(1, self.batch + 1, dtype=np.uint32) if seeds is None else np.asarray(seeds, dtype=np.uint32)
        _native.check(self._lib.afs_session_reset(self._h, _vp(_addr(s))), self.ctx.handle, "afs_session_reset")

    def synthesize_signal_tds(self, frames: np.ndarray, num_samples: int, taps: bool = False, pcm: bool = False):
        """``taps=True``: returns (audio, taps[batch, n_taps, produced]) with the context's taps
        (:meth:`Context.set_taps`) after every sample.  ``pcm=True``: the audio as int16
        (afs_session_synthesize_pcm: what Synthesizer::synthesizeSegment stores of each call); no taps."""
        if pcm and taps:
            raise ValueError("the PCM calls have no taps")
        fr = np.ascontiguousarray(np.broadcast_to(frames, (self.batch,)), dtype=FRAME_DTYPE)
        n = max(int(num_samples), 1)
        if pcm:
            out = np.zeros((self.batch, n), dtype=np.int16)
            produced = ctypes.c_int32(0)
            st = self._lib.afs_session_synthesize_pcm(self._h, _vp(_addr(fr)), int(num_samples), _vp(_addr(out)), None,
                                                      ctypes.byref(produced), None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_pcm")
            return out[:, : produced.value]
        out = np.zeros((self.batch, n), dtype=np.float64)
        produced = ctypes.c_int32(0)
        if taps:
            tout = np.zeros((self.batch, getattr(self.ctx, "n_taps", 0), n), dtype=np.float64)
            st = self._lib.afs_session_synthesize_taps(self._h, _vp(_addr(fr)), int(num_samples), _vp(_addr(out)),
                                                       _vp(_addr(tout)), None, ctypes.byref(produced), None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_taps")
            return out[:, : produced.value], tout[:, :, : produced.value]
        st = self._lib.afs_session_synthesize(self._h, _vp(_addr(fr)), int(num_samples), _vp(_addr(out)), None,
                                              ctypes.byref(produced), None)
        _native.check(st, self.ctx.handle, "afs_session_synthesize")
        return out[:, : produced.value]

    def restart(self, voices, seeds=None) -> None:
        """afs_session_restart_voices: the listed voices (distinct indices) get fresh state -- what
        :meth:`reset` gives every voice -- and are unlatched; no other voice changes.  ``seeds``: one per
        listed voice (None: voice v is seeded v + 1)."""
        v = np.ascontiguousarray(voices, dtype=np.int32).reshape(-1)
        s = None
        if seeds is not None:
            s = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
            if s.shape != v.shape:
                raise ValueError("one seed per listed voice")
        _native.check(self._lib.afs_session_restart_voices(self._h, _vp(_addr(v)), _vp(_addr(s)), int(v.size)),
                      self.ctx.handle, "afs_session_restart_voices")

    @property
    def latched(self) -> np.ndarray:
        """uint8[batch]: 1 for the voices that hold a latched frame (the next frame plays a transition)."""
        f = np.zeros(self.batch, dtype=np.uint8)
        _native.check(self._lib.afs_session_latched(self._h, _vp(_addr(f))), self.ctx.handle, "afs_session_latched")
        return f

    def synthesize_frames(self, frames, num_frames, hop: int, out=None, taps: bool = False, taps_out=None,
                          pcm: bool = False, report: bool = False, f32: bool = False, packed: bool = False,
                          offsets=None, frame_start=None):
        """afs_session_synthesize_ragged: every voice plays its own number of frames in one call.
        ``frames``: a ``[batch, Fmax]`` FRAME_DTYPE array or uint8 GPU tensor ``[batch, Fmax, 1072]`` of
        which voice u plays the first ``num_frames[u]`` (the rest is never read), or a list of per-voice
        FRAME_DTYPE arrays (``num_frames=None``: their lengths; an empty array: the voice is idle).  A
        voice with count 0 is idle: nothing of it is read or written.  An unlatched voice latches its
        first frame and plays the others as transitions of ``hop`` samples, a latched one plays every
        frame.  Returns ``(audio[batch, out_stride], produced[batch])`` -- ``out_stride`` is the largest
        ``produced``, or the row length of a given ``out`` (numpy or GPU tensor; nothing is written at or
        past ``produced[u]`` in row u) -- then the taps ``[batch, n_taps, out_stride]`` and the report as
        :meth:`Context.synthesize_ragged` appends them.  ``pcm=True``: int16 audio
        (afs_session_synthesize_ragged_pcm; ``out``'s rows may be strided); no taps.
        ``packed=True`` with ``pcm=True`` or ``f32=True`` (afs_session_synthesize_ragged_packed): returns
        ``(flat, offsets, produced)`` (then the report) -- voice u's samples at ``flat[offsets[u]:offsets[u]
        + produced[u]]`` of a 1-D int16 or float32 array, tightly in voice order (``offsets`` int64
        ``[batch + 1]``), or at the caller's ``offsets[batch]`` (an idle voice's is not looked at); ``out``:
        a 1-D numpy array or GPU tensor to receive them.  ``f32`` needs ``packed``.
        ``frame_start``: int64 ``[batch]`` (afs_session_synthesize_indexed, _indexed_packed): ``frames`` is
        then one flat 1-D FRAME_DTYPE array, or a GPU tensor of whole frames, and voice u plays
        ``frames[frame_start[u]:frame_start[u] + num_frames[u]]`` -- read in place on the device; spans may
        overlap, an idle voice's start is not looked at.  Float64 (with taps) or packed int16 / float32."""
        fmt, dtype = _sample_format(pcm, f32, packed)
        if f32 and not packed:
            raise ValueError("a float32 pool call is packed: pass packed=True")
        if offsets is not None and not packed:
            raise ValueError("offsets belong to a packed call")
        pcm = fmt is not None
        if pcm and taps:
            raise ValueError("the PCM calls have no taps")
        B = self.batch
        if frame_start is not None:
            return self._synthesize_indexed(frames, frame_start, num_frames, int(hop), out, taps, taps_out, fmt, dtype,
                                            packed, offsets, report)
        if isinstance(frames, (list, tuple)):
            rows = [np.ascontiguousarray(f, dtype=FRAME_DTYPE).reshape(-1) for f in frames]
            if num_frames is None:
                num_frames = [len(r) for r in rows]
            padded = np.zeros((len(rows), max([len(r) for r in rows] + [1])), dtype=FRAME_DTYPE)
            for u, r in enumerate(rows):
                padded[u, : len(r)] = r
            frames = padded
        if isinstance(frames, np.ndarray):
            if frames.dtype != FRAME_DTYPE or frames.ndim != 2 or frames.shape[0] != B:
                raise ValueError("frames must be a 2-D FRAME_DTYPE array [batch, Fmax]")
            fstride = frames.shape[1]
            frames = np.ascontiguousarray(frames)
        else:
            fstride = int(frames.shape[1])
            if int(frames.shape[0]) != B or _nbytes(frames) != B * fstride * FRAME_DTYPE.itemsize:
                raise ValueError("device frames must hold batch*Fmax*1072 bytes")
        counts = None
        produced = np.zeros(B, dtype=np.int32)
        if num_frames is not None:  # (a host array: the library builds the launch layout from it)
            counts = np.ascontiguousarray(num_frames, dtype=np.int32)
            if counts.shape != (B,):
                raise ValueError("num_frames must hold batch counts")
        if packed:
            if counts is None:
                raise ValueError("num_frames must hold batch counts")
            lat = self.latched.astype(np.int64)
            lengths = [None if c == 0 else max(int(c) - 1 + int(l), 0) * int(hop) for c, l in zip(counts, lat)]
            out, addr, off, own = _packed_out(out, offsets, lengths, dtype)
            nonfinite = np.zeros(B, dtype=np.uint8) if report else None
            rep = _native.AfsReport()
            st = self._lib.afs_session_synthesize_ragged_packed(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                                int(hop), fmt, _vp(addr), _vp(_addr(own)),
                                                                _vp(_addr(nonfinite)), _vp(_addr(produced)),
                                                                ctypes.byref(rep) if report else None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_ragged_packed")
            if report:
                return out, off, produced, {"device_ms": rep.device_ms, "samples": rep.samples,
                                            "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                                            "nonfinite": nonfinite}
            return out, off, produced
        if out is None:
            width = 0
            if counts is not None:
                width = int(np.where(counts > 0, counts - 1 + self.latched.astype(np.int32), 0).max()) * hop
            out = np.zeros((B, max(width, 0)), dtype=np.int16 if pcm else np.float64)
        if len(out.shape) != 2 or int(out.shape[0]) != B:
            raise ValueError("out must be [batch, out_stride]")
        ostride = int(out.shape[1])
        if pcm:
            pcm_addr, pcm_stride = _pcm_rows(out, B)
        elif _nbytes(out) != B * ostride * 8:
            raise ValueError("out must be [batch, out_stride] doubles")
        nonfinite = np.zeros(B, dtype=np.uint8) if report else None
        if taps:
            nt = getattr(self.ctx, "n_taps", 0)
            if taps_out is None:
                taps_out = np.zeros((B, nt, ostride), dtype=np.float64)
            if nt and _nbytes(taps_out) != B * nt * ostride * 8:  # (no taps set: the library refuses the call)
                raise ValueError("taps_out must hold batch*n_taps*out_stride doubles")
        rep = _native.AfsReport()
        if pcm:
            st = self._lib.afs_session_synthesize_ragged_pcm(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                             int(hop), _vp(pcm_addr if ostride else 0), pcm_stride,
                                                             _vp(_addr(nonfinite)), _vp(_addr(produced)),
                                                             ctypes.byref(rep) if report else None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_ragged_pcm")
        else:
            st = self._lib.afs_session_synthesize_ragged(self._h, _vp(_addr(frames)), fstride, _vp(_addr(counts)),
                                                         int(hop), _vp(_addr(out) if ostride else 0), ostride,
                                                         _vp(_addr(taps_out) if taps else 0), _vp(_addr(nonfinite)),
                                                         _vp(_addr(produced)), ctypes.byref(rep) if report else None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_ragged")
        res = (out, produced) + ((taps_out,) if taps else ())
        if report:
            res += ({"device_ms": rep.device_ms, "samples": rep.samples,
                     "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                     "nonfinite": nonfinite},)
        return res

    def _synthesize_indexed(self, frames, frame_start, num_frames, hop, out, taps, taps_out, fmt, dtype, packed, offsets,
                            report):
        """:meth:`synthesize_frames` with ``frame_start``: the indexed calls.  Numpy over the voices
        throughout -- a step of a large pool costs no Python loop."""
        B = self.batch
        if isinstance(frames, np.ndarray):
            if frames.dtype != FRAME_DTYPE or frames.ndim != 1 or not frames.flags["C_CONTIGUOUS"]:
                raise ValueError("indexed frames must be a contiguous 1-D FRAME_DTYPE array")
            total = int(frames.shape[0])
        else:
            total, rest = divmod(_nbytes(frames), FRAME_DTYPE.itemsize)
            if rest or (hasattr(frames, "is_contiguous") and not frames.is_contiguous()):
                raise ValueError("device frames must be contiguous and hold whole frames of 1072 bytes")
        if num_frames is None:
            raise ValueError("num_frames must hold batch counts")
        counts = np.ascontiguousarray(num_frames, dtype=np.int32)
        starts = np.ascontiguousarray(frame_start, dtype=np.int64)
        if counts.shape != (B,) or starts.shape != (B,):
            raise ValueError("num_frames and frame_start must hold batch entries")
        produced = np.zeros(B, dtype=np.int32)
        nonfinite = np.zeros(B, dtype=np.uint8) if report else None
        rep = _native.AfsReport()
        lengths = np.where(counts > 0, counts.astype(np.int64) - 1 + self.latched, 0) * hop
        if fmt is not None:
            if not packed:
                raise ValueError("an indexed int16 or float32 call is packed: pass packed=True")
            own = None
            if offsets is None:
                off = np.zeros(B + 1, dtype=np.int64)
                np.cumsum(np.maximum(lengths, 0), out=off[1:])
                span = int(off[B])
            else:
                off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
                if off.size not in (B, B + 1):
                    raise ValueError("offsets must hold one row start per utterance")
                own = np.ascontiguousarray(off[:B])
                span = int(np.where(lengths > 0, own + lengths, 0).max(initial=0))
            if out is None:
                out = np.zeros(span, dtype=dtype)
            if len(out.shape) != 1:
                raise ValueError("a packed out is 1-D")
            if isinstance(out, np.ndarray):
                if out.dtype != dtype or not out.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"a packed out must be contiguous {np.dtype(dtype).name}")
            elif np.dtype(dtype).name not in str(out.dtype) or (out.shape[0] > 1 and int(out.stride(0)) != 1):
                raise ValueError(f"a packed out must be contiguous {np.dtype(dtype).name}")
            if int(out.shape[0]) < span:
                raise ValueError(f"a packed out must hold {span} samples")
            st = self._lib.afs_session_synthesize_indexed_packed(
                self._h, _vp(_addr(frames)), total, _vp(_addr(starts)), _vp(_addr(counts)), hop, fmt,
                _vp(_addr(out) if int(out.shape[0]) else 0), _vp(_addr(own)), _vp(_addr(nonfinite)), _vp(_addr(produced)),
                ctypes.byref(rep) if report else None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_indexed_packed")
            res = (out, off, produced)
        else:
            if out is None:
                out = np.zeros((B, max(int(lengths.max(initial=0)), 0)), dtype=np.float64)
            if len(out.shape) != 2 or int(out.shape[0]) != B or _nbytes(out) != B * int(out.shape[1]) * 8:
                raise ValueError("out must be [batch, out_stride] doubles")
            ostride = int(out.shape[1])
            if taps:
                nt = getattr(self.ctx, "n_taps", 0)
                if taps_out is None:
                    taps_out = np.zeros((B, nt, ostride), dtype=np.float64)
                if nt and _nbytes(taps_out) != B * nt * ostride * 8:
                    raise ValueError("taps_out must hold batch*n_taps*out_stride doubles")
            st = self._lib.afs_session_synthesize_indexed(
                self._h, _vp(_addr(frames)), total, _vp(_addr(starts)), _vp(_addr(counts)), hop,
                _vp(_addr(out) if ostride else 0), ostride, _vp(_addr(taps_out) if taps else 0), _vp(_addr(nonfinite)),
                _vp(_addr(produced)), ctypes.byref(rep) if report else None)
            _native.check(st, self.ctx.handle, "afs_session_synthesize_indexed")
            res = (out, produced) + ((taps_out,) if taps else ())
        if report:
            res += ({"device_ms": rep.device_ms, "samples": rep.samples,
                     "nonfinite_utterances": rep.nonfinite_utterances, "kernel": rep.kernel,
                     "nonfinite": nonfinite},)
        return res

    @property
    def voice_state_bytes(self) -> int:
        """afs_session_voice_state_bytes: the size of one voice's record (tree solver)."""
        n = int(self._lib.afs_session_voice_state_bytes(self._h))
        if n <= 0:
            raise _native.AfsError("afs_session_voice_state_bytes: " + _native.STATUS[5] + " (tree solver only)")
        return n

    def save_voices(self, voices, out=None):
        """afs_session_save_voices: the records of the listed voices (distinct indices), ``uint8[n,
        voice_state_bytes]`` -- a numpy array, or ``out``, which may be a uint8 GPU tensor of that shape
        (16-byte aligned).  The session does not change."""
        v = np.ascontiguousarray(voices, dtype=np.int32).reshape(-1)
        size = self.voice_state_bytes
        if out is None:
            out = np.zeros((v.size, size), dtype=np.uint8)
        if _nbytes(out) != v.size * size:
            raise ValueError("out must hold n records of voice_state_bytes")
        _native.check(self._lib.afs_session_save_voices(self._h, _vp(_addr(v)), int(v.size), _vp(_addr(out))),
                      self.ctx.handle, "afs_session_save_voices")
        return out

    def load_voices(self, voices, state) -> None:
        """afs_session_load_voices: voice ``voices[i]`` (distinct) continues as the voice saved in record
        ``state[i]`` would have -- whichever slot, session or context of the same sampling rate, options
        and lane width it was saved from.  ``state``: uint8 ``[n, voice_state_bytes]``, numpy or GPU
        tensor.  No other voice changes."""
        v = np.ascontiguousarray(voices, dtype=np.int32).reshape(-1)
        if isinstance(state, np.ndarray):
            state = np.ascontiguousarray(state, dtype=np.uint8)
        if _nbytes(state) != v.size * self.voice_state_bytes:
            raise ValueError("state must hold n records of voice_state_bytes")
        _native.check(self._lib.afs_session_load_voices(self._h, _vp(_addr(v)), int(v.size), _vp(_addr(state))),
                      self.ctx.handle, "afs_session_load_voices")

    def copy_voices(self, dst_voices, src_voices, src: Optional["Synthesizer"] = None) -> None:
        """afs_session_copy_voices: voice ``src_voices[i]`` of ``src`` (None: this session) becomes voice
        ``dst_voices[i]`` of this one.  ``dst_voices`` are distinct, ``src_voices`` may repeat; on one
        session the lists may overlap (every source is read first: ``copy_voices([0, 1], [1, 0])`` swaps)."""
        d = np.ascontiguousarray(dst_voices, dtype=np.int32).reshape(-1)
        s = np.ascontiguousarray(src_voices, dtype=np.int32).reshape(-1)
        if d.shape != s.shape:
            raise ValueError("one source per destination")
        src = self if src is None else src
        _native.check(self._lib.afs_session_copy_voices(self._h, _vp(_addr(d)), src._h, _vp(_addr(s)), int(d.size)),
                      self.ctx.handle, "afs_session_copy_voices")

    def fork(self, voice: int, into) -> None:
        """One voice copied into the voices ``into`` (distinct): each continues from the same instant."""
        into = np.ascontiguousarray(into, dtype=np.int32).reshape(-1)
        self.copy_voices(into, np.full(into.shape, int(voice), dtype=np.int32))

    def rng_draws(self) -> np.ndarray:
        """rand() calls of every voice since construction / the last reset (tree solver)."""
        d = np.zeros(self.batch, dtype=np.int64)
        _native.check(self._lib.afs_session_rng_draws(self._h, _vp(_addr(d))), self.ctx.handle,
                      "afs_session_rng_draws")
        return d

    # reference spelling
    synthesizeSignalTds = synthesize_signal_tds

    def close(self) -> None:
        if self._h:
            self._lib.afs_session_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_utterances(session, utterances, hop: int, chunk_frames: int, seeds=None, pcm: bool = True, finished=None):
    """The continuous-batching scheduler behind :meth:`Context.synthesize_stream`, written against
    what it needs of a session: ``batch``, ``restart(voices, seeds)`` and ``synthesize_frames(frames,
    num_frames, hop, out=, pcm=, report=True) -> (audio, produced, report)``.

    Every step, each empty voice takes the next utterance of the corpus (and is restarted with its
    seed), every live voice is given up to ``chunk_frames`` of its remaining frames, and a voice without
    an utterance -- the corpus is dry -- runs idle with count 0.  An utterance whose last frame has
    played is yielded as ``(index, audio)``; its voice starts the next utterance in the following step."""
    B, hop, chunk = int(session.batch), int(hop), int(chunk_frames)
    if chunk < 1 or hop < 1:
        raise ValueError("chunk_frames and hop must be at least 1")
    corpus = enumerate(utterances)
    index = [-1] * B            # the utterance a voice plays, -1: none
    frames = [None] * B         # its frames, the next one to supply, its audio and the samples it has
    pos, audio, have = [0] * B, [None] * B, [0] * B
    rows = np.zeros((B, chunk), dtype=FRAME_DTYPE)
    out = np.zeros((B, chunk * hop), dtype=np.int16 if pcm else np.float64)
    dry = False
    while True:
        started, start_seeds = [], []
        for u in range(B):
            if index[u] >= 0 or dry:
                continue
            nxt = next(corpus, None)
            if nxt is None:
                dry = True
                continue
            i, fr = nxt
            fr = np.ascontiguousarray(fr, dtype=FRAME_DTYPE).reshape(-1)
            if len(fr) < 2:
                raise ValueError(f"utterance {i} has {len(fr)} frames: at least 2 (one transition)")
            index[u], frames[u], pos[u], have[u] = i, fr, 0, 0
            audio[u] = np.zeros((len(fr) - 1) * hop, dtype=out.dtype)
            started.append(u)
            start_seeds.append(i + 1 if seeds is None else int(seeds[i]))
        if started:
            session.restart(started, start_seeds)
        if all(i < 0 for i in index):
            return
        counts = np.zeros(B, dtype=np.int32)
        for u in range(B):
            if index[u] >= 0:
                n = min(chunk, len(frames[u]) - pos[u])
                rows[u, :n] = frames[u][pos[u]:pos[u] + n]
                counts[u] = n
        res = session.synthesize_frames(rows, counts, hop, out=out, pcm=pcm, report=True)
        produced, rep = res[1], res[-1]
        for u in range(B):
            if index[u] < 0:
                continue
            n = int(produced[u])
            audio[u][have[u]:have[u] + n] = out[u, :n]
            have[u] += n
            pos[u] += int(counts[u])
            if pos[u] == len(frames[u]):
                if have[u] != len(audio[u]):
                    raise RuntimeError(f"utterance {index[u]}: {have[u]} of {len(audio[u])} samples produced")
                if finished is not None:
                    finished(index[u], u, session, int(rep["nonfinite"][u]))
                done = (index[u], audio[u])
                index[u], frames[u], audio[u] = -1, None, None
                yield done


def stream_corpus(session, frames, frame_offsets, hop: int, chunk_frames: int, seeds=None, pcm: bool = True,
                  f32: bool = False, out=None):
    """The scheduler behind :meth:`Context.synthesize_corpus`: a flat corpus streamed through the voices
    of a session with no frame moved on the host.  Written against ``batch``, ``restart(voices, seeds)``
    and ``synthesize_frames(frames, num_frames, hop, out=, pcm=, f32=, packed=True, offsets=,
    frame_start=, report=True) -> (out, offsets, produced, report)``.

    ``frames``: the corpus, one flat FRAME_DTYPE array or GPU tensor; utterance i is
    ``frames[frame_offsets[i]:frame_offsets[i + 1]]`` (``frame_offsets`` int64 ``[n + 1]``, at least 2
    frames each).  Voices take the utterances in order.  Every step gives each live voice up to
    ``chunk_frames`` of its remaining frames by index, and its audio goes to ``offsets[i]`` plus the samples
    it has played: the output stage writes every sample at its final place.  A voice whose utterance has
    ended is restarted with the next utterance's seed (``seeds[i]``; None: i + 1) before the next step.
    The bookkeeping of a step is numpy over the voices.  Returns ``(flat, offsets, nonfinite)``:
    ``offsets`` is :func:`ragged_offsets` of the corpus, utterance i's audio ``flat[offsets[i]:offsets[i +
    1]]`` -- int16 (``pcm``) or float32 (``f32``) -- and ``nonfinite`` uint8 ``[n]``.  ``out``: the caller's own
    1-D buffer of ``offsets[n]`` samples, numpy or a GPU tensor, returned as ``flat``; None: a numpy array
    made here (a host buffer is staged whole on every step: :meth:`Context.synthesize_corpus` passes a
    device buffer that lives for the whole run and copies it back once)."""
    fmt, dtype = _sample_format(pcm, f32, True)
    B, hop, chunk = int(session.batch), int(hop), int(chunk_frames)
    if chunk < 1 or hop < 1:
        raise ValueError("chunk_frames and hop must be at least 1")
    fo = np.ascontiguousarray(frame_offsets, dtype=np.int64).reshape(-1)
    if fo.size < 1 or fo[0] < 0:
        raise ValueError("frame_offsets must hold n + 1 non-negative frame indices")
    n = fo.size - 1
    lens = np.diff(fo)
    if n and int(lens.min()) < 2:
        i = int(np.argmin(lens))
        raise ValueError(f"utterance {i} has {int(lens[i])} frames: at least 2 (one transition)")
    seed_of = np.arange(1, n + 1, dtype=np.uint32) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint32)
    if seed_of.shape != (n,):
        raise ValueError("one seed per utterance")
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum((lens - 1) * hop, out=offsets[1:])
    total = int(offsets[n])
    flat = np.zeros(total, dtype=dtype) if out is None else out
    nonfinite = np.zeros(n, dtype=np.uint8)
    index = np.full(B, -1, dtype=np.int64)  # the utterance a voice plays, -1: none
    pos = np.zeros(B, dtype=np.int64)       # the frames of it the voice has been given
    played = np.zeros(B, dtype=np.int64)    # the samples of it the voice has produced
    handed = 0
    while True:
        free = np.flatnonzero(index < 0)[:n - handed]
        if free.size:
            ids = np.arange(handed, handed + free.size)
            index[free], pos[free], played[free] = ids, 0, 0
            session.restart(free.astype(np.int32), seed_of[ids])
            handed += int(free.size)
        live = index >= 0
        if not live.any():
            break
        i = np.where(live, index, 0)
        counts = np.where(live, np.minimum(lens[i] - pos, chunk), 0).astype(np.int32)
        starts = np.where(live, fo[i] + pos, 0)
        dest = np.where(live, offsets[i] + played, 0)
        res = session.synthesize_frames(frames, counts, hop, out=flat, pcm=pcm, f32=f32, packed=True, offsets=dest,
                                        frame_start=starts, report=True)
        played += res[2]
        pos += counts
        ended = live & (pos == lens[i])
        if (played[ended] != (lens[i[ended]] - 1) * hop).any():
            raise RuntimeError("an utterance ended with other than (F-1)*hop samples produced")
        nonfinite[index[ended]] = res[-1]["nonfinite"][ended]
        index[ended] = -1
    return flat, offsets, nonfinite


def branch_candidates(session, prefix, candidates, hop: int, pcm: bool = False):
    """The branching behind :meth:`Context.synthesize_candidates`, written against what it needs of a
    session of K voices: ``batch``, ``synthesize_frames(frames, num_frames, hop, pcm=)`` and ``fork(voice,
    into)``.  Three calls: the prefix on voice 0 beside K - 1 idle voices, one fork of voice 0 into the
    others, then every voice its candidate.  Returns the second call's audio ``[K, Fc*hop]``."""
    prefix = np.ascontiguousarray(prefix, dtype=FRAME_DTYPE).reshape(-1)
    candidates = np.ascontiguousarray(candidates, dtype=FRAME_DTYPE)
    K, hop = int(session.batch), int(hop)
    if candidates.ndim != 2 or candidates.shape[0] != K or candidates.shape[1] < 1:
        raise ValueError("candidates must hold one row of at least one frame per voice")
    if len(prefix) < 1 or hop < 1:
        raise ValueError("the prefix needs at least one frame (the one the candidates start from) and hop >= 1")
    Fp, Fc = len(prefix), candidates.shape[1]
    rows = np.zeros((K, Fp), dtype=FRAME_DTYPE)
    rows[0] = prefix
    counts = np.zeros(K, dtype=np.int32)
    counts[0] = Fp
    session.synthesize_frames(rows, counts, hop, pcm=pcm)
    if K > 1:
        session.fork(0, np.arange(1, K, dtype=np.int32))
    res = session.synthesize_frames(candidates, np.full(K, Fc, dtype=np.int32), hop, pcm=pcm)
    audio, produced = res[0], res[1]
    if not (np.asarray(produced) == Fc * hop).all():
        raise RuntimeError("a candidate produced other than Fc*hop samples")
    return audio[:, :Fc * hop]
