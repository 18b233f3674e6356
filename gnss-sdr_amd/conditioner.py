"""Python face of gsh_cond_* (include/gnss_sdr_hip.h): the signal conditioner -- DataTypeAdapter, InputFilter and Resampler of a receiver's
Signal_Conditioner (signal_conditioner.cc:60-87) -- as one device pass per block straight into a SampleStream."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .sample_stream import ITEM_TYPES, PackedFormat, SampleStream, _flag, _packed_host

INPUT_ITEMS, INPUT_REAL, INPUT_PACKED = 0, 1, 2
REAL_KINDS = {"float": 1, "short": 2, "byte": 3}   # FirFilter.KINDS without gr_complex
_REAL_NP = {1: np.float32, 2: np.int16, 3: np.int8}
_ITEM_NP = {0: np.complex64, 1: np.int16, 2: np.int8}

# the reference's implementations of each stage that the one-pass kernel covers; everything else raises ValueError
ADAPTERS = {"Pass_Through": None, "Ibyte_To_Complex": "ibyte", "Ishort_To_Complex": "ishort"}
FILTERS = ("Pass_Through", "Fir_Filter", "Freq_Xlating_Fir_Filter")
RESAMPLERS = ("Pass_Through", "Direct_Resampler")
# input_item_type of the filter adapters (freq_xlating_fir_filter.cc:115-161, fir_filter.cc) -> the conditioner's input
_FILTER_INPUTS = ("gr_complex", "float", "short", "byte")


def _conf(input_kind, inverted_spectrum, taps, decimation, center_freq_hz, sampling_freq_hz, fs_in, fs_out):
    """-> (gsh_cond_conf, the taps array it points into)"""
    c = _lib.CondConf()
    if isinstance(input_kind, PackedFormat):
        c.input, c.packed = INPUT_PACKED, input_kind.struct()
    elif input_kind in REAL_KINDS:
        c.input, c.item_type = INPUT_REAL, REAL_KINDS[input_kind]
    elif input_kind in ITEM_TYPES:
        c.input, c.item_type = INPUT_ITEMS, ITEM_TYPES[input_kind]
    else:
        raise ValueError(f"unknown input kind {input_kind!r}")
    c.inverted_spectrum = int(bool(inverted_spectrum))
    t = np.ascontiguousarray(taps if taps is not None else [], np.float32).reshape(-1)
    c.n_taps = t.size
    c.taps = t.ctypes.data_as(C.POINTER(C.c_float)) if t.size else None
    c.decimation = int(decimation)
    c.center_freq_hz, c.sampling_freq_hz = float(center_freq_hz), float(sampling_freq_hz)
    c.fs_in, c.fs_out = float(fs_in), float(fs_out)
    return c, t


BLANKING_DEFAULTS = dict(pfa=0.04, length=32, segments_est=12500, segments_reset=5000000)   # pulse_blanking_filter.cc:43-50


def _blanking(blanking):
    """None or the property names of Pulse_Blanking_Filter (pfa, length, segments_est, segments_reset; defaults of the reference) -> gsh_cond_blanking"""
    if blanking is None:
        return None
    unknown = set(blanking) - set(BLANKING_DEFAULTS)
    if unknown:
        raise ValueError(f"blanking: unknown keys {sorted(unknown)} (known: {', '.join(BLANKING_DEFAULTS)})")
    b = dict(BLANKING_DEFAULTS, **blanking)
    return _lib.CondBlanking(float(b["pfa"]), int(b["length"]), int(b["segments_est"]), int(b["segments_reset"]))


# notch_filter.cc:41-51 / notch_filter_lite.cc:41-55; segments_coeff 0: Notch_Filter, >= 1: Notch_Filter_Lite with that n_segments_coeff
NOTCH_DEFAULTS = dict(pfa=0.001, p_c_factor=0.9, length=32, segments_est=12500, segments_reset=5000000, segments_coeff=0)


def _notch(notch):
    """None or the property names of Notch_Filter / Notch_Filter_Lite (pfa, p_c_factor, length, segments_est, segments_reset; segments_coeff >= 1
    for NotchLite; defaults of the reference) -> gsh_cond_notch"""
    if notch is None:
        return None
    unknown = set(notch) - set(NOTCH_DEFAULTS)
    if unknown:
        raise ValueError(f"notch: unknown keys {sorted(unknown)} (known: {', '.join(NOTCH_DEFAULTS)})")
    n = dict(NOTCH_DEFAULTS, **notch)
    return _lib.CondNotch(float(n["pfa"]), float(n["p_c_factor"]), int(n["length"]), int(n["segments_est"]), int(n["segments_reset"]), int(n["segments_coeff"]))


def outputs_after(n_in_total: int, input_kind="gr_complex", inverted_spectrum: bool = False, taps=None, decimation: int = 1, center_freq_hz: float = 0.0,
                  sampling_freq_hz: float = 1.0, fs_in: float = 0.0, fs_out: float = 0.0, blanking=None, notch=None) -> int:
    """gsh_cond_plan / gsh_cond_plan_blanked / gsh_cond_plan_notched: ring samples such a conditioner has produced once n_in_total input samples
    have arrived.  Host arithmetic, no GPU."""
    c, _t = _conf(input_kind, inverted_spectrum, taps, decimation, center_freq_hz, sampling_freq_hz, fs_in, fs_out)
    out = C.c_uint64(0)
    b, n = _blanking(blanking), _notch(notch)
    if b is not None and n is not None:
        raise ValueError("blanking and notch: one mitigation stage per conditioner")
    if n is not None:
        check(_lib.load().gsh_cond_plan_notched(C.byref(c), C.byref(n), int(n_in_total), C.byref(out)))
    elif b is None:
        check(_lib.load().gsh_cond_plan(C.byref(c), int(n_in_total), C.byref(out)))
    else:
        check(_lib.load().gsh_cond_plan_blanked(C.byref(c), C.byref(b), int(n_in_total), C.byref(out)))
    return int(out.value)


class SignalConditioner:
    """One handle for the whole chain.  input_kind: "gr_complex" / "ishort" / "ibyte" (complex items), "float" / "short" / "byte" (real items: they
    need a filter) or a PackedFormat.  taps None or empty: no filter.  fs_in = fs_out = 0: no resampler (fs_in is the rate after the filter).
    blanking: None, or dict(pfa=0.04, length=32, segments_est=12500, segments_reset=5000000) (any subset): pulse blanking (Pulse_Blanking_Filter)
    between the filter and the resampler; whole segments of `length` filter outputs are emitted, a partial one waits for the next push.
    notch: None, or dict(pfa=0.001, p_c_factor=0.9, length=32, segments_est=12500, segments_reset=5000000, segments_coeff=0) (any subset): the notch
    filter (Notch_Filter; segments_coeff >= 1: Notch_Filter_Lite) in that place instead; output k is the mitigated filter output k + 1, whole
    segments only.  One of blanking / notch per handle.
    Every push returns (first_out, n_out): the ring index of the block's first output and how many outputs it completed."""

    def __init__(self, ring: SampleStream | None = None, input_kind="gr_complex", inverted_spectrum: bool = False, taps=None, decimation: int = 1,
                 center_freq_hz: float = 0.0, sampling_freq_hz: float = 1.0, fs_in: float = 0.0, fs_out: float = 0.0, device: int = 0, blanking=None,
                 notch=None):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.input_kind = input_kind
        c, _t = _conf(input_kind, inverted_spectrum, taps, decimation, center_freq_hz, sampling_freq_hz, fs_in, fs_out)
        self._np = None if c.input == INPUT_PACKED else _REAL_NP[c.item_type] if c.input == INPUT_REAL else _ITEM_NP[c.item_type]
        self._per_sample = 1 if c.input != INPUT_ITEMS or c.item_type == 0 else 2   # array elements per input sample
        b, n = _blanking(blanking), _notch(notch)
        check(self._lib.gsh_cond_create(device, C.byref(c), C.byref(self._h)))
        self.ring = None
        try:
            if b is not None:
                check(self._lib.gsh_cond_set_blanking(self._h, C.byref(b)))
            if n is not None:
                check(self._lib.gsh_cond_set_notch(self._h, C.byref(n)))   # (with blanking as well: GSH_ERR_STATE, one mitigation stage per handle)
        except Exception:
            self.close()
            raise
        if ring is not None:
            self.bind(ring)

    @staticmethod
    def properties(role: dict) -> dict:
        """The constructor's keywords for a Signal_Conditioner configured with the reference's property names, given as
        {"DataTypeAdapter": {...}, "InputFilter": {...}, "Resampler": {...}} (each optional; `implementation` defaults to Pass_Through).
          DataTypeAdapter  Pass_Through | Ibyte_To_Complex | Ishort_To_Complex, inverted_spectrum (ibyte_to_complex.cc:34-51)
          InputFilter      Pass_Through | Fir_Filter | Freq_Xlating_Fir_Filter with input_item_type, decimation_factor, IF, sampling_frequency
                           (freq_xlating_fir_filter.cc:62-75) and `taps`: the caller's (firdes_low_pass, or a Remez design made on the host)
          Resampler        Pass_Through | Direct_Resampler with sample_freq_in, sample_freq_out (direct_resampler_conditioner.cc:36-43)
        ValueError for an implementation this mapping does not cover: Pulse_Blanking_Filter is mapped by properties_with_mitigation(), Notch_Filter
        and Notch_Filter_Lite by properties_with_notch()."""
        ada, fil, res = (dict(role.get(k, {})) for k in ("DataTypeAdapter", "InputFilter", "Resampler"))
        a_impl, f_impl, r_impl = (d.get("implementation", "Pass_Through") for d in (ada, fil, res))
        if a_impl not in ADAPTERS:
            raise ValueError(f"DataTypeAdapter.implementation {a_impl!r} is not covered ({', '.join(ADAPTERS)})")
        if f_impl not in FILTERS:
            raise ValueError(f"InputFilter.implementation {f_impl!r} is not covered ({', '.join(FILTERS)}); blanking and notch filters stay loose calls")
        if r_impl not in RESAMPLERS:
            raise ValueError(f"Resampler.implementation {r_impl!r} is not covered ({', '.join(RESAMPLERS)})")
        kw = dict(input_kind=ADAPTERS[a_impl] or ada.get("item_type", "gr_complex"), inverted_spectrum=bool(_flag(ada.get("inverted_spectrum", False))))
        if f_impl != "Pass_Through":
            if "taps" not in fil:
                raise ValueError("InputFilter.taps: the taps are the caller's (firdes_low_pass, or a Remez design made on the host)")
            item = fil.get("input_item_type", "gr_complex")
            if item not in _FILTER_INPUTS:
                raise ValueError(f"InputFilter.input_item_type {item!r} is not one of {', '.join(_FILTER_INPUTS)}")
            if fil.get("output_item_type", "gr_complex") != "gr_complex":
                raise ValueError("InputFilter.output_item_type: the ring holds gr_complex (the cshort / cbyte outputs of the xlating adapter are not covered)")
            if item != "gr_complex":
                if a_impl != "Pass_Through":
                    raise ValueError(f"a {a_impl} adapter yields gr_complex, the filter expects {item}")
                kw["input_kind"] = item
            xlating = f_impl == "Freq_Xlating_Fir_Filter"
            kw.update(taps=fil["taps"], decimation=int(fil.get("decimation_factor", 1)) if xlating else 1,
                      center_freq_hz=float(fil.get("IF", 0.0)) if xlating else 0.0, sampling_freq_hz=float(fil.get("sampling_frequency", 4000000.0)))
        if r_impl != "Pass_Through":
            if "sample_freq_out" not in res:
                raise ValueError("Resampler.sample_freq_out: the reference defaults it to GNSS-SDR.internal_fs_sps, which is not part of this role")
            kw.update(fs_in=float(res.get("sample_freq_in", 4000000.0)), fs_out=float(res["sample_freq_out"]))
        return kw

    @classmethod
    def from_properties(cls, ring: SampleStream | None, role: dict, device: int = 0) -> "SignalConditioner":
        return cls(ring, device=device, **cls.properties(role))

    @staticmethod
    def properties_with_mitigation(role: dict) -> dict:
        """properties() with InputFilter.implementation=Pulse_Blanking_Filter covered as well (pulse_blanking_filter.cc:43-53, :73-84):
          pfa, length, segments_est, segments_reset   the `blanking` keyword (defaults 0.04, 32, 12500, 5000000)
          IF (or `if`), sampling_frequency            |IF| > 1: a Freq_Xlating_Fir_Filter with decimation 1 in front of the blanker; its `taps` are
                                                      the caller's (the reference designs firdes::low_pass(1, sampling_frequency, bw, tw)).  |IF| <= 1: no filter
          item_type                                   gr_complex only
        Every other implementation is delegated to properties()."""
        fil = dict(role.get("InputFilter", {}))
        if fil.get("implementation", "Pass_Through") != "Pulse_Blanking_Filter":
            return SignalConditioner.properties(role)
        if fil.get("item_type", "gr_complex") != "gr_complex":
            raise ValueError(f"InputFilter.item_type {fil['item_type']!r}: Pulse_Blanking_Filter takes gr_complex only")
        kw = SignalConditioner.properties({k: v for k, v in role.items() if k != "InputFilter"})
        if kw["input_kind"] not in ("gr_complex", "ibyte", "ishort"):
            raise ValueError(f"Pulse_Blanking_Filter takes gr_complex, the adapter yields {kw['input_kind']!r}")
        if_hz = float(fil.get("IF", fil.get("if", 0.0)))
        if abs(if_hz) > 1.0:
            if "taps" not in fil:
                raise ValueError("InputFilter.taps: |IF| > 1 puts a Freq_Xlating_Fir_Filter in front of the blanker; its taps are the caller's "
                                 "(firdes_low_pass(1, sampling_frequency, bw, tw))")
            kw.update(taps=fil["taps"], decimation=1, center_freq_hz=if_hz, sampling_freq_hz=float(fil.get("sampling_frequency", 4000000.0)))
        kw["blanking"] = {k: type(d)(fil.get(k, d)) for k, d in BLANKING_DEFAULTS.items()}
        return kw

    @classmethod
    def from_properties_with_mitigation(cls, ring: SampleStream | None, role: dict, device: int = 0) -> "SignalConditioner":
        return cls(ring, device=device, **cls.properties_with_mitigation(role))

    @staticmethod
    def properties_with_notch(role: dict) -> dict:
        """properties_with_mitigation() with InputFilter.implementation = Notch_Filter | Notch_Filter_Lite covered as well (notch_filter.cc:41-56,
        notch_filter_lite.cc:41-61):
          pfa, p_c_factor, length, segments_est, segments_reset   the `notch` keyword (defaults 0.001, 0.9, 32, 12500, 5000000)
          coeff_rate, sampling_frequency                          Notch_Filter_Lite: n_segments_coeff = max(1, int((sampling_frequency / coeff_rate)
                                                                  / length)) in float32; coeff_rate defaults to 0.1 sampling_frequency, that (the
                                                                  reference reads SignalSource.sampling_frequency) to 4000000
          item_type                                               gr_complex only
        Neither adapter puts a filter in front of the block.  Every other implementation is delegated to properties_with_mitigation()."""
        fil = dict(role.get("InputFilter", {}))
        impl = fil.get("implementation", "Pass_Through")
        if impl not in ("Notch_Filter", "Notch_Filter_Lite"):
            return SignalConditioner.properties_with_mitigation(role)
        if fil.get("item_type", "gr_complex") != "gr_complex":
            raise ValueError(f"InputFilter.item_type {fil['item_type']!r}: {impl} takes gr_complex only")
        kw = SignalConditioner.properties({k: v for k, v in role.items() if k != "InputFilter"})
        if kw["input_kind"] not in ("gr_complex", "ibyte", "ishort"):
            raise ValueError(f"{impl} takes gr_complex, the adapter yields {kw['input_kind']!r}")
        notch = {k: type(d)(fil.get(k, d)) for k, d in NOTCH_DEFAULTS.items() if k != "segments_coeff"}
        notch["segments_coeff"] = 0
        if impl == "Notch_Filter_Lite":
            f32 = np.float32
            samp_freq = f32(fil.get("sampling_frequency", 4000000.0))
            coeff_rate = f32(fil.get("coeff_rate", f32(samp_freq * f32(0.1))))
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = f32(f32(samp_freq / coeff_rate) / f32(notch["length"]))
            if not np.isfinite(ratio):
                raise ValueError(f"InputFilter.coeff_rate {float(coeff_rate)!r} and length {notch['length']!r} give no coefficient count")
            notch["segments_coeff"] = max(1, int(ratio))
        kw["notch"] = notch
        return kw

    @classmethod
    def from_properties_with_notch(cls, ring: SampleStream | None, role: dict, device: int = 0) -> "SignalConditioner":
        return cls(ring, device=device, **cls.properties_with_notch(role))

    def set_notch(self, notch) -> None:
        """gsh_cond_set_notch: before the first push only, and not while blanking is on; None turns the stage off"""
        n = _notch(notch)
        check(self._lib.gsh_cond_set_notch(self._h, C.byref(n) if n is not None else None))

    def notch_state(self) -> dict:
        """gsh_cond_notch_state (waits for the queued pushes): thres, noise_pow_est, n_segments, filter_state, n_segments_coeff, z0 (NotchLite's
        coefficient; 0 for Notch) and the counters n_decided / n_filtered -- the duty cycle of the filter"""
        s = _lib.CondNotchState()
        check(self._lib.gsh_cond_notch_state(self._h, C.byref(s)))
        return dict(thres=np.float32(s.thres), noise_pow_est=np.float32(s.noise_pow_est), n_segments=int(s.n_segments), filter_state=bool(s.filter_state),
                    n_segments_coeff=int(s.n_segments_coeff), z0=np.complex64(complex(s.z0[0], s.z0[1])), n_decided=int(s.n_decided),
                    n_filtered=int(s.n_filtered))

    def set_blanking(self, blanking) -> None:
        """gsh_cond_set_blanking: before the first push only; None turns the stage off"""
        b = _blanking(blanking)
        check(self._lib.gsh_cond_set_blanking(self._h, C.byref(b) if b is not None else None))

    def blanking_state(self) -> dict:
        """gsh_cond_blanking_state (waits for the queued pushes): thres, noise_power_estimation, n_segments, last_filtered, and the counters
        n_decided / n_blanked -- the duty cycle of the blanker"""
        s = _lib.CondBlankingState()
        check(self._lib.gsh_cond_blanking_state(self._h, C.byref(s)))
        return dict(thres=np.float32(s.thres), noise_power_estimation=np.float32(s.noise_power_estimation), n_segments=int(s.n_segments),
                    last_filtered=bool(s.last_filtered), n_decided=int(s.n_decided), n_blanked=int(s.n_blanked))

    def close(self):
        if self._h:
            self._lib.gsh_cond_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, ring: SampleStream | None) -> None:
        """the conditioner's next output goes to the ring's next index as it stands now"""
        check(self._lib.gsh_cond_bind(self._h, ring._h if ring is not None else None))
        self.ring = ring

    def _host_block(self, items, n_in):
        if isinstance(self.input_kind, PackedFormat):
            return _packed_host(self.input_kind, items, n_in)
        a = np.ascontiguousarray(items, self._np).reshape(-1)
        return a, (a.size // self._per_sample if n_in is None else int(n_in))

    def push(self, items, n_in: int | None = None):
        """gsh_cond_push: a block in host memory (complex64 [n]; int16 / int8 [n, 2] interleaved I, Q; real items [n]; packed bytes), synchronous"""
        a, n = self._host_block(items, n_in)
        first, n_out = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.gsh_cond_push(self._h, C.c_void_p(a.ctypes.data) if a.size else None, n, C.byref(first), C.byref(n_out)))
        return int(first.value), int(n_out.value)

    def push_device(self, device_ptr: int, n_in: int, hip_stream: int = 0):
        first, n_out = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.gsh_cond_push_device(self._h, C.c_void_p(device_ptr), int(n_in), C.c_void_p(hip_stream) if hip_stream else None, C.byref(first),
                                             C.byref(n_out)))
        return int(first.value), int(n_out.value)

    def push_pinned_async(self, items: np.ndarray, n_in: int | None = None):
        """gsh_cond_push_pinned_async: `items` lies in page-locked memory (gsh_host_register) and must stay untouched until the ring's wait_copied() /
        wait_copied_upto(first_out + n_out) covers the push; nothing waits here."""
        a, n = self._host_block(items, n_in)
        self._keep_async = getattr(self, "_keep_async", [])[-3:] + [a]
        first, n_out = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.gsh_cond_push_pinned_async(self._h, C.c_void_p(a.ctypes.data) if a.size else None, n, C.byref(first), C.byref(n_out)))
        return int(first.value), int(n_out.value)

    def position(self):
        """(input samples taken, ring samples produced) since the handle was created"""
        n_in, n_out = C.c_uint64(0), C.c_uint64(0)
        check(self._lib.gsh_cond_position(self._h, C.byref(n_in), C.byref(n_out)))
        return int(n_in.value), int(n_out.value)

    def time_push(self, device_ptr: int, n_in: int, reps: int = 20) -> float:
        """gsh_cond_time_push: average milliseconds of the device work of one push of the block; position, history and ring stay as they are"""
        ms = C.c_float(0.0)
        check(self._lib.gsh_cond_time_push(self._h, C.c_void_p(device_ptr), int(n_in), int(reps), C.byref(ms)))
        return float(ms.value)
