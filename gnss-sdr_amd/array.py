"""Python face of gsh_beam_* (include/gnss_sdr_hip.h): the antenna-array front end -- Beamformer_Filter / Array_Signal_Conditioner on the device,
several beams per block, each straight into its SampleStream, and the array covariance -- plus the numpy host helpers that turn a covariance into
weights.  Weights follow the block's convention y[n] = sum_a x_a[n] w_a (beamformer.cc:59): no conjugate."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import GSH_ARRAY_INTERLEAVED, GSH_ARRAY_MAX_ANTENNAS, GSH_ARRAY_MAX_BEAMS, GSH_ARRAY_PLANAR, check, fptr
from .sample_stream import _NP, ITEM_TYPES

LAYOUTS = {"planar": GSH_ARRAY_PLANAR, "interleaved": GSH_ARRAY_INTERLEAVED}


class ArrayFormat:
    """gsh_array_format: how the streams of an antenna array lie in memory.  layout "planar": one buffer per antenna (the beamformer block's
    input_items[a]; Multichannel_File_Signal_Source); "interleaved": one buffer of sample-major frames, antenna a of sample k is item k * A + a
    (the wire layout of Custom_UDP_Signal_Source).  first_is_q: the first value of every pair is Q (Custom_UDP's IQ_swap = false)."""

    def __init__(self, n_antennas: int, item_type: str = "gr_complex", layout: str = "planar", first_is_q: bool = False):
        self.n_antennas, self.item_type, self.layout, self.first_is_q = int(n_antennas), item_type, layout, bool(first_is_q)

    @property
    def n_buffers(self) -> int:
        return self.n_antennas if self.layout == "planar" else 1

    @property
    def item_bytes(self) -> int:
        return {0: 8, 1: 4, 2: 2}[ITEM_TYPES[self.item_type]]

    def struct(self) -> "_lib.ArrayFormat":
        return _lib.ArrayFormat(self.n_antennas, ITEM_TYPES[self.item_type], LAYOUTS[self.layout], int(self.first_is_q))

    def __repr__(self):
        return f"ArrayFormat(n_antennas={self.n_antennas}, item_type={self.item_type!r}, layout={self.layout!r}, first_is_q={self.first_is_q})"


def _pointers(ptrs):
    return (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs])


class Beamformer:
    """gsh_beam_*: n_beams weighted sums of the array's streams per block.  Rings are SampleStream objects."""

    def __init__(self, fmt: ArrayFormat, n_beams: int = 1, device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.fmt, self.n_beams, self.device = fmt, int(n_beams), device
        f = fmt.struct()
        check(self._lib.gsh_beam_create(device, C.byref(f), self.n_beams, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gsh_beam_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_weights(self, w) -> None:
        """w: complex [n_beams, n_antennas] (or [n_antennas] for one beam); a later call uses them from its first sample on"""
        a = np.ascontiguousarray(np.asarray(w, np.complex64).reshape(self.n_beams, self.fmt.n_antennas))
        check(self._lib.gsh_beam_set_weights(self._h, fptr(a)))

    @property
    def weights(self) -> np.ndarray:
        out = np.empty((self.n_beams, self.fmt.n_antennas), np.complex64)
        check(self._lib.gsh_beam_get_weights(self._h, fptr(out)))
        return out

    def set_adaptive(self, steering=None, reference=None, forgetting: float = 0.0, loading_rel: float = 0.0, loading_abs: float = 0.0) -> None:
        """gsh_adaptive_beam_set: from the next call on, every process_device / push / push_device forms the block's covariance, accumulates it
        (R_acc <- forgetting * R_acc + R_block), solves for every beam's weights and forms the beams with them, all on the device on the call's stream.
        steering: one vector [n_antennas] for every beam or one per beam [n_beams, n_antennas] (MVDR: w = conj(R^-1 s / (s^H R^-1 s)));
        reference: an element index, or one per beam (power inversion: that element's weight is held at 1).  The loading added to R_acc's diagonal is
        loading_rel * trace(R_acc) / n_antennas + loading_abs.  set_adaptive(None) turns the mode off: the weights of set_weights are in force again."""
        if steering is None and reference is None:
            check(self._lib.gsh_adaptive_beam_set(self._h, None))
            return
        if steering is not None and reference is not None:
            raise ValueError("an adaptive beam is constrained by a steering vector or by a reference element, not both")
        A = self.fmt.n_antennas
        c = np.zeros((GSH_ARRAY_MAX_BEAMS, GSH_ARRAY_MAX_ANTENNAS), np.complex128)
        if steering is not None:
            s = np.asarray(steering, np.complex128)
            if s.shape not in ((A,), (self.n_beams, A)):
                raise ValueError(f"steering of shape {s.shape} for {self.n_beams} beams of {A} antennas")
            c[:self.n_beams, :A] = s
        else:
            ref = np.broadcast_to(np.asarray(reference, np.int64), (self.n_beams,))
            if np.any(ref < 0) or np.any(ref >= A):
                raise ValueError(f"reference element {reference} of {A} antennas")
            c[np.arange(self.n_beams), ref] = 1.0
        conf = _lib.BeamAdapt(float(forgetting), float(loading_rel), float(loading_abs))
        C.memmove(conf.constraint_iq, np.ascontiguousarray(c).ctypes.data, c.nbytes)
        check(self._lib.gsh_adaptive_beam_set(self._h, C.byref(conf)))

    def adaptive_state(self) -> dict:
        """gsh_adaptive_beam_state (synchronous): blocks, failures, delta, r_acc (complex128 [A, A]) and the weights in force (complex64 [n_beams, A])"""
        st = _lib.BeamAdaptState()
        check(self._lib.gsh_adaptive_beam_state(self._h, C.byref(st)))
        A = self.fmt.n_antennas
        r = np.frombuffer(st.r_acc_iq, np.float64, 2 * A * A).copy().view(np.complex128).reshape(A, A)
        w = np.frombuffer(st.w_iq, np.float32, 2 * self.n_beams * A).copy().view(np.complex64).reshape(self.n_beams, A)
        return dict(blocks=int(st.blocks), failures=int(st.failures), delta=float(st.delta), r_acc=r, weights=w)

    def _host_buffers(self, items):
        """planar: a sequence of n_antennas arrays (or one array [n_antennas, ...]); interleaved: one array.  -> (arrays kept alive, pointers, n)"""
        dt = _NP[ITEM_TYPES[self.fmt.item_type]]

        def as_items(x):
            x = np.asarray(x)
            if dt is np.complex64 and not np.iscomplexobj(x):
                return np.ascontiguousarray(x, np.float32)   # interleaved float32 I,Q as read from a file
            return np.ascontiguousarray(x, dt)

        if self.fmt.layout == "planar":
            bufs = [as_items(x) for x in items]
            if len(bufs) != self.fmt.n_antennas:
                raise ValueError(f"{len(bufs)} buffers for {self.fmt.n_antennas} antennas")
        else:
            bufs = [as_items(items)]
        nbytes = {b.nbytes for b in bufs}
        per_sample = self.fmt.item_bytes * (1 if self.fmt.layout == "planar" else self.fmt.n_antennas)
        if len(nbytes) != 1 or bufs[0].nbytes % per_sample:
            raise ValueError("the buffers of an array block hold the same whole number of samples")
        return bufs, _pointers([b.ctypes.data for b in bufs]), bufs[0].nbytes // per_sample

    def process_device(self, src_ptrs, n: int, dst_ptrs, inverted_spectrum: bool = False, hip_stream: int = 0) -> None:
        """gsh_beam_process_device: n samples at the device pointers src_ptrs -> beam r at dst_ptrs[r] (complex64)"""
        if len(src_ptrs) != self.fmt.n_buffers or len(dst_ptrs) != self.n_beams:
            raise ValueError(f"{len(src_ptrs)} inputs / {len(dst_ptrs)} outputs for {self.fmt.n_buffers} buffers / {self.n_beams} beams")
        check(self._lib.gsh_beam_process_device(self._h, _pointers(src_ptrs), int(n), int(inverted_spectrum), _pointers(dst_ptrs),
                                                C.c_void_p(hip_stream) if hip_stream else None))

    def _rings(self, rings):
        if len(rings) != self.n_beams:
            raise ValueError(f"{len(rings)} rings for {self.n_beams} beams")
        return (C.c_void_p * len(rings))(*[r._h.value for r in rings]), (C.c_uint64 * len(rings))()

    def push(self, rings, items, inverted_spectrum: bool = False) -> list[int]:
        """gsh_beam_push: one array block held in host memory, beam r into rings[r]; synchronous.  Returns the absolute index of the first sample
        in every ring."""
        bufs, ptrs, n = self._host_buffers(items)
        h, first = self._rings(rings)
        check(self._lib.gsh_beam_push(self._h, h, ptrs, n, int(inverted_spectrum), first))
        return [int(v) for v in first]

    def push_device(self, rings, src_ptrs, n: int, inverted_spectrum: bool = False, hip_stream: int = 0) -> list[int]:
        if len(src_ptrs) != self.fmt.n_buffers:
            raise ValueError(f"{len(src_ptrs)} inputs for {self.fmt.n_buffers} buffers")
        h, first = self._rings(rings)
        check(self._lib.gsh_beam_push_device(self._h, h, _pointers(src_ptrs), int(n), int(inverted_spectrum),
                                             C.c_void_p(hip_stream) if hip_stream else None, first))
        return [int(v) for v in first]

    def covariance(self, items, inverted_spectrum: bool = False) -> np.ndarray:
        """gsh_beam_covariance: complex128 [A, A], R[i, j] = sum_n x_i[n] conj(x_j[n]) of a block held in host memory (a sum: divide by n yourself)"""
        bufs, ptrs, n = self._host_buffers(items)
        out = np.empty((self.fmt.n_antennas, self.fmt.n_antennas), np.complex128)
        check(self._lib.gsh_beam_covariance(self._h, ptrs, n, int(inverted_spectrum), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def covariance_device(self, src_ptrs, n: int, inverted_spectrum: bool = False) -> np.ndarray:
        if len(src_ptrs) != self.fmt.n_buffers:
            raise ValueError(f"{len(src_ptrs)} inputs for {self.fmt.n_buffers} buffers")
        out = np.empty((self.fmt.n_antennas, self.fmt.n_antennas), np.complex128)
        check(self._lib.gsh_beam_covariance_device(self._h, _pointers(src_ptrs), int(n), int(inverted_spectrum), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def time_process(self, n: int, reps: int = 20) -> float:
        """gsh_beam_time_process: average milliseconds of one beam pass over n samples (HIP events)"""
        ms = C.c_float(0.0)
        check(self._lib.gsh_beam_time_process(self._h, int(n), int(reps), C.byref(ms)))
        return float(ms.value)


def _loaded(R, loading: float) -> np.ndarray:
    R = np.asarray(R, np.complex128)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError(f"a covariance is square, not {R.shape}")
    return R + loading * np.eye(R.shape[0])


def power_inversion_weights(R, reference: int = 0, loading: float = 0.0) -> np.ndarray:
    """Power-inversion weights from the array covariance R (a sum or a mean: the scale cancels): minimise the output power with the reference
    element's weight held at 1.  With v = R^-1 e / (e^T R^-1 e), e the unit vector of `reference`, the weights in the block's convention
    y = sum_a x_a w_a are conj(v).  loading: added to R's diagonal first.  -> complex64 [A]"""
    Rl = _loaded(R, loading)
    e = np.zeros(Rl.shape[0], np.complex128)
    e[reference] = 1.0
    v = np.linalg.solve(Rl, e)
    return np.conj(v / v[reference]).astype(np.complex64)


def mvdr_weights(R, steering, loading: float = 0.0) -> np.ndarray:
    """Minimum-variance distortionless-response weights: v = R^-1 s / (s^H R^-1 s) for the steering vector s (x = s * signal + ...), so that v^H s = 1
    while v^H R v is least; in the block's convention y = sum_a x_a w_a the weights are conj(v).  -> complex64 [A]"""
    Rl = _loaded(R, loading)
    s = np.asarray(steering, np.complex128).reshape(-1)
    if s.size != Rl.shape[0]:
        raise ValueError(f"steering vector of {s.size} elements for {Rl.shape[0]} antennas")
    v = np.linalg.solve(Rl, s)
    return np.conj(v / (np.conj(s) @ v)).astype(np.complex64)
