"""Host build of gnss-sdr_amd/csrc/cnav_stream.h (tests/host/cnav_stream_host.cc) for the tests: g++ -O2 -ffp-contract=off, as tests/tlm_host.py builds
viterbi_acs.h; and the golden file tests/golden/cnav.npz (minted from libswiftcnav by tests/golden/make_golden_cnav.py) as the tests read it."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from gnss_sdr_amd._lib import CnavChannelState, CnavJob, CnavMessage
from gnss_sdr_amd.telemetry import cnav_result_capacity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = (1, 63, 64, 65, 127, 128, 129, 599, 600, 601)
MESSAGE = np.dtype([("bits", "<u4", 10), ("symbol_index", "<u4"), ("delay", "<u4"), ("tow", "<u4"), ("prn", "u1"), ("msg_id", "u1"), ("alert", "u1"),
                    ("part", "u1"), ("invert", "u1"), ("invert_or", "u1"), ("reserved", "u1", 2)])
U8 = C.POINTER(C.c_uint8)


@functools.lru_cache(maxsize=1)
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="cnav_stream_host_"), "libcnav_stream_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "gnss-sdr_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "cnav_stream_host.cc"), "-o", out], check=True)
    so = C.CDLL(out)
    so.gsh_test_cnav_init.argtypes = [C.POINTER(CnavChannelState)]
    so.gsh_test_cnav_state_valid.argtypes = [C.POINTER(CnavChannelState)]
    so.gsh_test_cnav_push.argtypes = [C.POINTER(CnavChannelState), U8, C.c_uint32, C.POINTER(CnavMessage), C.c_uint32]
    so.gsh_test_cnav_push.restype = C.c_uint32
    so.gsh_test_cnav_quantise.argtypes = [C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_float, U8]
    so.gsh_test_cnav_acs.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)]
    so.gsh_test_cnav_acs.restype = C.c_uint32
    jb, mb, sb = C.c_int(), C.c_int(), C.c_int()
    assert so.gsh_test_cnav_sizes(C.byref(jb), C.byref(mb), C.byref(sb)) == 64
    assert (jb.value, mb.value, sb.value) == (C.sizeof(CnavJob), C.sizeof(CnavMessage), C.sizeof(CnavChannelState))
    return so


@functools.lru_cache(maxsize=1)
def golden():
    """-> {name: (symbols uint8, messages as MESSAGE records, final state as uint8[2480])}, plus raise_at / raise_by under "normalise" """
    z = np.load(os.path.join(ROOT, "tests", "golden", "cnav.npz"))
    cases = {}
    for name in z["names"]:
        name = str(name)
        cases[name] = (z["sym__" + name], np.ascontiguousarray(z["msg__" + name]).view(MESSAGE).reshape(-1), z["state__" + name])
        for a in cases[name]:
            a.setflags(write=False)
    return cases, int(z["raise_at"]), int(z["raise_by"])


def messages_array(table, count, base=0):
    """the first `count` gsh_cnav_message of a ctypes table -> MESSAGE records, symbol_index moved by base"""
    out = np.frombuffer(bytes(table), np.uint8)[:60 * count].view(MESSAGE).copy() if count else np.zeros(0, MESSAGE)
    out["symbol_index"] += base
    return out


def state_bytes(state):
    return np.frombuffer(bytes(state), np.uint8)


def state_from_bytes(raw):
    return CnavChannelState.from_buffer_copy(np.ascontiguousarray(raw, np.uint8).tobytes())


def raise_metrics(state, by):
    """what the minting driver does to a live decoder: adds `by` to all 128 metrics of both parts"""
    for p in state.part:
        for k in range(64):
            p.old_metrics[k] = (p.old_metrics[k] + by) & 0xFFFFFFFF
            p.new_metrics[k] = (p.new_metrics[k] + by) & 0xFFFFFFFF


def cuts(n, piece=None, rng=None):
    """where a stream of n symbols is cut: pieces of a fixed size, or random ones of 1..700"""
    at, out = 0, []
    while at < n:
        step = piece if piece else int(rng.integers(1, 701))
        out.append((at, min(n, at + step)))
        at = out[-1][1]
    return out


class HostCnavChannel:
    """one channel on the host build of the header"""

    def __init__(self, state=None):
        self.state = CnavChannelState()
        if state is None:
            lib().gsh_test_cnav_init(C.byref(self.state))
        else:
            C.memmove(C.byref(self.state), C.byref(state), C.sizeof(CnavChannelState))
        self.pushed = 0

    def push(self, symbols, capacity=None):
        """-> MESSAGE records, symbol_index counted from the channel's first symbol"""
        s = np.ascontiguousarray(symbols, np.uint8)
        cap = cnav_result_capacity(len(s)) if capacity is None else capacity
        table = (CnavMessage * max(1, cap))()
        n = lib().gsh_test_cnav_push(C.byref(self.state), s.ctypes.data_as(U8), len(s), table, cap)
        self.delivered = n   # may exceed the capacity: the rest was not written
        n = min(n, cap)
        out = messages_array(table, n, self.pushed)
        self.pushed += len(s)
        return out


def host_quantise(x, mode, scale=1.0):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(len(x), np.uint8)
    lib().gsh_test_cnav_quantise(x.ctypes.data_as(C.POINTER(C.c_float)), len(x), mode, scale, out.ctypes.data_as(U8))
    return out


ALIGNED = "hard_p0_up_s00"   # the reference delivers at symbols 703, 1279, 1919, 2495, 3135: 576 and 640 apart in turn
# (start, length) of a push that begins on a delivery symbol, and the deliveries the reference makes inside it; n / 600 + 1 is 1, 2 and 3 for these
ALIGNED_WINDOWS = ((703, 577, 2), (1279, 1153, 2), (703, 1153, 2), (703, 1793, 4), (1919, 577, 2))


def pending_delivery_state(cases):
    """A state that only set_state can make, with more than 299 decoded bits between two symbols: the channel after 1 600 symbols of ALIGNED (part 1
    locked, the second message delivered 320 symbols ago) with that second message put back in front of its decode buffer.  It delivers that message
    again on its next symbol and the third one, as the reference does, at symbol 1919: two messages within 320 symbols.  -> (state, symbols pushed)"""
    sym, want, _ = cases[ALIGNED]
    ch = HostCnavChannel()
    ch.push(sym[:1600])
    p = ch.state.part[0]
    assert p.flags & 4 and p.flags & 8 and not p.flags & 2 and p.n_decoded <= 180
    words = np.array(p.decoded[:], np.uint32)
    have = np.unpackbits(words.astype(">u4").view(np.uint8))[:p.n_decoded]
    again = np.unpackbits(want["bits"][1].astype(">u4").view(np.uint8))[:300]
    bits = np.concatenate([again, have, np.zeros(512 - 300 - len(have), np.uint8)])
    for k, w in enumerate(np.packbits(bits).view(">u4")):
        p.decoded[k] = int(w)
    p.n_decoded += 300
    return ch.state, 1600
