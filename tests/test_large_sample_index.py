"""Host arithmetic on absolute sample indices past 2^32 (no device): the pull-in hand-over (gsh_trk_pull_in, gsh_trk_pull_in_over) and the signal
conditioner's output bookkeeping (gsh_cond_plan behind conditioner.outputs_after).

Pull-in: only the difference between the read pointer and the acquisition's sample stamp may enter, so the answers at (nitems_read + B, stamp + B) must
equal those at (nitems_read, stamp) as bits, for every base the GPU tests of tests/test_large_sample_index_gpu.py use.  The straddling bases are used as
given (n = 4 000): 2^32 - 5 n - 3 puts the smaller of the two indices below 2^32 and, for the larger differences, the other one above it.

Bookkeeping: the bracketing of tests/test_conditioner_abi.py::test_host_bookkeeping_equals_a_walk_of_the_reference_accumulator, in Python integers, with
the input count beyond 2^32, 2^40 and 2^52."""
import ctypes as C
import struct

import numpy as np
import pytest

N = 4000
BASES = [2 ** 31 - 5 * N - 3, 2 ** 32 - 5 * N - 3, 2 ** 40 + 1, 2 ** 53 + 1]
BASE_IDS = ["2^31-5n-3", "2^32-5n-3", "2^40+1", "2^53+1"]
FS = 4e6
DIFFS = [0, 1, int(30 * FS)]          # 0, 1 and 30 s of samples between the read pointer and the stamp


def _pull_in(gsh, conf, nitems_read, delay, stamp, doppler):
    off, first, acc = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    assert gsh.gsh_trk_pull_in(C.byref(conf), nitems_read, delay, stamp, doppler, C.byref(off), C.byref(first), C.byref(acc)) == 0
    return off.value, first.value, struct.pack("<d", acc.value)


@pytest.mark.parametrize("base", BASES[1:], ids=BASE_IDS[1:])
@pytest.mark.parametrize("ahead", [False, True], ids=["stamp-behind", "stamp-ahead"])
def test_pull_in_takes_only_the_difference(gsh, base, ahead):
    from gnss_sdr_amd.tracking_loop import trk_conf
    crossed = 0
    for kw in (dict(fs_in=FS, vector_length=N, pull_in_time_s=5), dict(fs_in=FS, vector_length=N, pull_in_time_s=0),
               dict(fs_in=25e6, vector_length=25000, code_chip_rate=1.023e6, pull_in_time_s=29)):
        conf = trk_conf(**kw)
        for diff in DIFFS:
            # small indices: the stamp (or the read pointer) at 12 345, the other one `diff` samples on
            read0, stamp0 = (12345, 12345 + diff) if ahead else (12345 + diff, 12345)
            for delay, doppler in ((0.0, 0.0), (1234.56, -3456.5), (3999.49, 4999.0)):
                small = _pull_in(gsh, conf, read0, delay, stamp0, doppler)
                large = _pull_in(gsh, conf, read0 + base, delay, stamp0 + base, doppler)
                assert small == large, (kw, diff, delay, doppler, small, large)
            small = gsh.gsh_trk_pull_in_over(C.byref(conf), read0, stamp0)
            large = gsh.gsh_trk_pull_in_over(C.byref(conf), read0 + base, stamp0 + base)
            assert small == large, (kw, diff, small, large)
            # a stamp ahead of the read pointer wraps the unsigned difference: the transitory is over at once (trk.cc:1912), at any base
            if ahead and diff > 0:
                assert large == 1
            if not ahead:
                assert large == int(kw["pull_in_time_s"] < diff // int(kw["fs_in"]))
            crossed += min(read0, stamp0) + base < 2 ** 32 <= max(read0, stamp0) + base
    if base < 2 ** 32:
        assert crossed >= 3     # the straddling base: the two indices lie on either side of 2^32 for the 30 s differences


@pytest.mark.parametrize("n_in_total", [2 ** 32 + 17, 2 ** 40 + 1, 2 ** 52 + 1], ids=["2^32+17", "2^40+1", "2^52+1"])
@pytest.mark.parametrize("fs_in,fs_out", [(4e6, 2.5e6), (25e6, 4e6), (4e6, 4.092e6), (2e6, 6.5e6), (3e6, 3e6), (0.0, 0.0), (7e6, 1e6)])
@pytest.mark.parametrize("D", [1, 2, 8])
def test_conditioner_bookkeeping_far_into_a_stream(gsh, fs_in, fs_out, D, n_in_total):
    from gnss_sdr_amd.conditioner import outputs_after
    taps = [1.0, 2.0, 3.0] if D > 1 else None
    m = (n_in_total + D - 1) // D
    c = outputs_after(n_in_total, "gr_complex", taps=taps, decimation=D, sampling_freq_hz=1.0, fs_in=fs_in, fs_out=fs_out)
    if fs_in == fs_out:
        assert c == m
        return
    two_32 = 1 << 32
    if fs_in > fs_out:
        step = int(np.floor(two_32 * fs_out / fs_in))
        index = lambda j: -((-j * two_32) // step)      # noqa: E731
    else:
        step = int(np.floor(two_32 * fs_in / fs_out))
        index = lambda j: ((j + 1) * step) >> 32        # noqa: E731
    assert index(c - 1) < m <= index(c), (c, m, index(c - 1), index(c))
