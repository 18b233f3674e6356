"""Python face of gsh_gen_* (include/gnss_sdr_hip.h): the device signal generator -- the reference's Signal_Generator
(src/algorithms/signal_generator/gnuradio_blocks/signal_generator_c.cc = sg.cc) as a table-driven kernel that writes a caller's device buffer or a
SampleStream -- and the table builders that restate its generate_codes() (sg.cc:164-323) for GPS L1 C/A and Galileo E5a."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import check
from .codes import gps_l1_ca_code
from .sample_stream import SampleStream

MAX_SATS = 32
MAX_SIGNS = 1024
GPS_L1_CA_CODE_LENGTH = 1023
GPS_L1_CA_CODE_RATE = 1023000
GALILEO_E5A_CODE_LENGTH = 10230
GALILEO_E5A_CODE_RATE = 10230000


@dataclass
class Satellite:
    """What gsh_gen_set_satellite takes.  table_a / table_b: complex64 of one period (table_b None: absent); signs_*: +-1 per sign boundary."""
    table_a: np.ndarray
    table_b: np.ndarray | None
    delay_samples: int
    signs_a: np.ndarray = field(default_factory=lambda: np.ones(1, np.int8))
    signs_b: np.ndarray = field(default_factory=lambda: np.ones(1, np.int8))
    doppler_hz: float = 0.0
    start_phase_rad: float = 0.0
    carrier_offset_hz: float = 0.0

    @property
    def period(self) -> int:
        return int(np.asarray(self.table_a).size)


def cn0_scale(cn0_db: float, bw_bb_hz: float, two_components: bool = False) -> np.float32:
    """sqrt(10^(CN0/10) / BW_BB) in float32 as sg.cc:184 forms it (Pn = 1); two-component signals divide by two more (sg.cc:230).  bw_bb_hz is
    the block's BW_BB_ = BW_BB * fs / 2 (sg.cc:75)."""
    p = np.power(np.float32(10.0), np.float32(cn0_db) / np.float32(10.0), dtype=np.float32) / np.float32(bw_bb_hz)
    if two_components:
        p = p / np.float32(2.0)
    return np.sqrt(np.float32(p), dtype=np.float32)


def _sign_array(bits, repeat: int = 1) -> np.ndarray:
    s = np.repeat(np.asarray(bits, np.int8).reshape(-1), repeat)
    return s if s.size else np.ones(1, np.int8)


def gps_l1_ca_satellite(prn: int, fs: int, delay_chips: int = 0, doppler_hz: float = 0.0, cn0_db: float | None = None, bw_bb: float = 1.0,
                        data_bits=None, start_phase_rad: float = 0.0) -> Satellite:
    """GPS L1 C/A as generate_codes() builds it (sg.cc:173-194): the code shifted by code_length - delay_chips
    (gps_l1_ca_code_gen_int's chip_shift, gps_sdr_signal_replica.cc:80-99: chip lcv is chip lcv + shift of the unshifted code), sampled as
    gps_l1_ca_code_gen_complex_sampled does (chips in the imaginary part, float32 index, last sample pinned), one period of
    round(fs / 1000) samples.  cn0_db None: unscaled (the block with noise_flag false), else times cn0_scale(cn0_db, bw_bb * fs / 2).
    delay_samples as sg.cc:360.  data_bits: +-1 per 20 ms bit (one sign entry per code period, so at most 51 bits); None: +1."""
    L = GPS_L1_CA_CODE_LENGTH
    spc = int(round(np.float32(fs) / np.float32(GPS_L1_CA_CODE_RATE / L)))
    shift = (L - int(delay_chips)) % L
    code = np.roll(gps_l1_ca_code(prn), -shift)
    n = int(float(fs) / (GPS_L1_CA_CODE_RATE / L))
    if n != spc:
        raise ValueError(f"fs {fs}: the replica has {n} samples per code, the block expects {spc}")
    ts = np.float32(1.0) / np.float32(fs)
    tc = np.float32(1.0) / np.float32(GPS_L1_CA_CODE_RATE)
    idx = np.floor((ts * np.arange(n, dtype=np.float32)) / tc).astype(np.int64)
    idx[-1] = L - 1
    table = (1j * code[idx]).astype(np.complex64)
    if cn0_db is not None:
        table = _scaled(table, cn0_scale(cn0_db, np.float32(bw_bb) * np.float32(fs) / np.float32(2.0)))
    delay_samples = ((int(delay_chips) % L) * spc) // L
    signs = _sign_array(data_bits if data_bits is not None else [1], 20 if data_bits is not None else 1)
    return Satellite(table, None, delay_samples, signs, np.ones(1, np.int8), float(doppler_hz), float(start_phase_rad))


def _scaled(table: np.ndarray, scale: np.float32) -> np.ndarray:
    """complex<float> *= float: each part times the scale in float32"""
    out = np.empty(table.shape, np.complex64)
    out.real = table.real.astype(np.float32) * scale
    out.imag = table.imag.astype(np.float32) * scale
    return out


def galileo_e5a_satellite(primary_iq: np.ndarray, secondary_i, secondary_q, fs: int, delay_chips: int = 0, delay_sec: int = 1, doppler_hz: float = 0.0,
                          cn0_db: float | None = None, bw_bb: float = 1.0, data_bits=None, start_phase_rad: float = 0.0) -> Satellite:
    """Galileo E5a as generate_codes() builds it (sg.cc:219-233).  primary_iq: the 10 230 chips of galileo_e5_a_code_gen_complex_primary('5X')
    (I chips in the real part, Q chips in the imaginary one), secondary_i (20) and secondary_q (100): the +-1 secondary codes -- data, e.g. from
    tests/golden/siggen.npz; this module holds no Galileo tables.  The chips are resampled as `resampler` does (gnss_signal_replica.cc:272-287:
    float32 index, last sample pinned) and rotated by delay_samples = (delay_chips mod L) * samples_per_code / L (galileo_e5_signal_replica.cc:
    105-121, sg.cc:425).  A = (Re, 0) with sA = data bit x I secondary code, B = (0, Im) with sB = Q secondary code, an entry per code period
    (sg.cc:428-448): after boundary k >= 1 the block applies secondary chip (k - 1 + delay_sec) mod length, so delay_sec = 1 makes entry k chip
    k; entry 0 (before the first boundary) is the block's initial value, I chip 0 (sg.cc:110).  data_bits: +-1 per 20 ms symbol; None: +1."""
    L = GALILEO_E5A_CODE_LENGTH
    prim = np.asarray(primary_iq, np.complex64).reshape(-1)
    if prim.size != L:
        raise ValueError(f"the E5a primary code has {L} chips, not {prim.size}")
    spc = int(float(fs) / (GALILEO_E5A_CODE_RATE / L))
    if fs != GALILEO_E5A_CODE_RATE:
        t_out = np.float32(1.0) / np.float32(fs)
        idx = np.floor((t_out * np.arange(spc, dtype=np.float32)) * np.float32(GALILEO_E5A_CODE_RATE)).astype(np.int64)
        idx[-1] = L - 1
        prim = prim[idx]
    delay_samples = ((int(delay_chips) % L) * spc) // L
    table = np.roll(prim, delay_samples)
    if cn0_db is not None:
        table = _scaled(table, cn0_scale(cn0_db, np.float32(bw_bb) * np.float32(fs) / np.float32(2.0), two_components=True))
    a = np.zeros(spc, np.complex64)
    a.real = table.real
    b = np.zeros(spc, np.complex64)
    b.imag = table.imag
    sec_i = np.asarray(secondary_i, np.int8).reshape(-1)
    sec_q = np.asarray(secondary_q, np.int8).reshape(-1)
    k = np.arange(100)
    s_i = sec_i[(k - 1 + delay_sec) % sec_i.size]
    s_i[0] = sec_i[0]
    s_q = sec_q[(k - 1 + delay_sec) % sec_q.size].copy()
    if data_bits is not None:
        bits = np.repeat(np.asarray(data_bits, np.int8).reshape(-1), 20)
        if bits.size % 100:
            raise ValueError("data_bits: a whole number of 100-period secondary-code spans (5 symbols)")
        s_i = np.tile(s_i, bits.size // 100) * bits
    return Satellite(a, b, delay_samples, s_i.astype(np.int8), s_q.astype(np.int8), float(doppler_hz), float(start_phase_rad))


def philox_words(seed: int, sample_index: int) -> np.ndarray:
    """gsh_gen_philox_words: the four Philox4x32-10 words of a sample (the text the kernel runs, on the host)"""
    out = (C.c_uint32 * 4)()
    _lib.load().gsh_gen_philox_words(int(seed), int(sample_index), out)
    return np.array(out[:], np.uint32)


def _sat_args(sat: Satellite):
    """-> (ctypes arguments after fs / handle, the arrays they point into)"""
    a = np.ascontiguousarray(sat.table_a, np.complex64).reshape(-1)
    b = None if sat.table_b is None else np.ascontiguousarray(sat.table_b, np.complex64).reshape(-1)
    if b is not None and b.size != a.size:
        raise ValueError(f"table B has {b.size} samples, table A {a.size}")
    sa = np.ascontiguousarray(sat.signs_a, np.int8).reshape(-1)
    sb = np.ascontiguousarray(sat.signs_b, np.int8).reshape(-1)
    i8 = C.POINTER(C.c_int8)
    args = (_lib.fptr(a.view(np.float32)) if a.size else None, _lib.fptr(b.view(np.float32)) if b is not None else None, int(a.size),
            int(sat.delay_samples), sa.ctypes.data_as(i8) if sa.size else None, int(sa.size), sb.ctypes.data_as(i8) if sb.size else None, int(sb.size),
            float(sat.doppler_hz), float(sat.start_phase_rad), float(sat.carrier_offset_hz))
    return args, (a, b, sa, sb)


def check_satellite(fs: float, sat: Satellite) -> None:
    """gsh_gen_check_satellite: the checks of set_satellite alone (GshError), no GPU"""
    args, _keep = _sat_args(sat)
    check(_lib.load().gsh_gen_check_satellite(float(fs), *args))


class SignalGenerator:
    """n_sats satellites at fs samples per second.  Every satellite must be set before the first sample is made.  Sample n is the absolute index
    since the generator's start; seek() moves it, and what sample n holds never depends on how the stream is cut into calls."""

    def __init__(self, fs: float, n_sats: int, device: int = 0):
        self._lib = _lib.load()
        self._h = C.c_void_p()
        self.fs, self.n_sats, self.device = float(fs), int(n_sats), device
        check(self._lib.gsh_gen_create(device, self.fs, self.n_sats, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.gsh_gen_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_satellite(self, index: int, sat: Satellite) -> None:
        args, _keep = _sat_args(sat)
        check(self._lib.gsh_gen_set_satellite(self._h, int(index), *args))

    def set_noise(self, enabled: bool, seed: int = 0) -> None:
        check(self._lib.gsh_gen_set_noise(self._h, int(bool(enabled)), int(seed)))

    def seek(self, sample_index: int) -> None:
        check(self._lib.gsh_gen_seek(self._h, int(sample_index)))

    def position(self) -> int:
        n = C.c_uint64(0)
        check(self._lib.gsh_gen_position(self._h, C.byref(n)))
        return int(n.value)

    def generate_device(self, n: int, device_ptr: int) -> None:
        """the next n samples as complex64 at device_ptr (device memory, 8-byte aligned); synchronous"""
        check(self._lib.gsh_gen_generate_device(self._h, int(n), C.c_void_p(device_ptr)))

    def generate(self, n: int) -> np.ndarray:
        """the next n samples, read back (tests and small studies; a receiver takes them on the device)"""
        import torch
        buf = torch.empty((max(int(n), 1), 2), dtype=torch.float32, device=f"cuda:{self.device}")
        self.generate_device(n, buf.data_ptr())
        return buf.cpu().numpy().view(np.complex64).reshape(-1)[:int(n)].copy()

    def push(self, ring: SampleStream, n: int) -> int:
        """gsh_gen_push: the next n samples straight into the ring; -> the ring index of the first"""
        first = C.c_uint64(0)
        check(self._lib.gsh_gen_push(self._h, ring._h, int(n), C.byref(first)))
        return int(first.value)

    def time_generate(self, n: int, reps: int = 20) -> float:
        """gsh_gen_time_generate: average milliseconds of generating n samples from the present position; the position stays"""
        ms = C.c_float(0.0)
        check(self._lib.gsh_gen_time_generate(self._h, int(n), int(reps), C.byref(ms)))
        return float(ms.value)
