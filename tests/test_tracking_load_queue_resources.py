"""Register / scratch budget of the half-chip E/P/L kernel with two trips of sample loads in flight (csrc/mcorr_device.h, GSH_MC_PAIR_QUEUE, round 10), read from
the built library's code-object metadata (no GPU needed; method of tests/test_kernel_resources.py).

The second set of sample registers costs the 128-thread half-chip flavour eight VGPRs.  It runs five waves per SIMD, which 512 / 5 = 102 registers allow in
allocation blocks of eight: 96 is the budget, VGPRs and AGPRs together, and a spill into scratch would cost more than the deeper queue can gain (a spilling flavour ran
45 % slower: profiles/r02/mcorr_bound_experiments.txt)."""
import os
import re

import pytest

import gnss_sdr_amd
from kernel_metadata import kernels

# mcorr_kernel_t128<3, 0, false, false, false, true, true>: E/P/L, standard mode, whole-code table, paired taps, half-chip shifts
HALF_CHIP_T128 = re.compile(r"mcorr_kernel_t128ILi3ELi0ELb0ELb0ELb0ELb1ELb1EE")


@pytest.fixture(scope="module")
def meta():
    lib = gnss_sdr_amd._lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("library not built")
    k = kernels(lib)
    assert len(k) > 50, "no gfx950 code objects found in the library"
    return k


def test_half_chip_128_thread_flavour_keeps_five_waves_per_simd(meta):
    found = {n: k for n, k in meta.items() if HALF_CHIP_T128.search(n)}
    assert len(found) == 1, sorted(found)
    for n, k in found.items():
        registers = k[".vgpr_count"] + k.get(".agpr_count", 0)
        print(n, "VGPRs", k[".vgpr_count"], "AGPRs", k.get(".agpr_count", 0), "scratch", k[".private_segment_fixed_size"])
        assert registers <= 96, (n, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert not k.get(".uses_dynamic_stack"), n
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k.get(".vgpr_spill_count"), k.get(".sgpr_spill_count"))
        assert k.get(".max_flat_workgroup_size", 128) == 128, (n, k.get(".max_flat_workgroup_size"))


def test_no_kernel_of_the_library_uses_scratch(meta):
    spilling = {n: k[".private_segment_fixed_size"] for n, k in meta.items() if k[".private_segment_fixed_size"] != 0}
    assert not spilling, spilling
    dynamic = [n for n, k in meta.items() if k.get(".uses_dynamic_stack")]
    assert not dynamic, dynamic
