"""Register / scratch / LDS budget of the E/P/L correlator's walk kernel (csrc/multicorrelator.hip, mcorr_walk_kernel_t128, round 11), read from the built library's
code-object metadata (no GPU needed; method of tests/test_kernel_resources.py).

The walk is the half-chip 128-thread flavour's body inside a loop over job slots.  It ships only inside that flavour's budget: at most 96 VGPRs and AGPRs together
(five waves per SIMD), no scratch and no spills, no static LDS (the dynamic array is the parent's, 13 696 bytes, and must start at address 0), work-groups of 128.
A loop around the body invites the compiler to keep loop invariants in registers across all of it; the kernel source says what it does against that."""
import os
import re

import pytest

import gnss_sdr_amd
from kernel_metadata import kernels

WALK = re.compile(r"mcorr_walk_kernel_t128")
# the regex of tests/test_tracking_load_queue_resources.py: mcorr_kernel_t128<3, 0, false, false, false, true, true>
HALF_CHIP_T128 = re.compile(r"mcorr_kernel_t128ILi3ELi0ELb0ELb0ELb0ELb1ELb1EE")


@pytest.fixture(scope="module")
def meta():
    lib = gnss_sdr_amd._lib.LIB_PATH
    if not os.path.exists(lib):
        pytest.skip("library not built")
    k = kernels(lib)
    assert len(k) > 50, "no gfx950 code objects found in the library"
    return k


def test_exactly_one_walk_kernel_inside_the_half_chip_flavours_budget(meta):
    found = {n: k for n, k in meta.items() if WALK.search(n)}
    assert len(found) == 1, sorted(found)
    for n, k in found.items():
        registers = k[".vgpr_count"] + k.get(".agpr_count", 0)
        print(n, "VGPRs", k[".vgpr_count"], "AGPRs", k.get(".agpr_count", 0), "SGPRs", k.get(".sgpr_count"), "scratch", k[".private_segment_fixed_size"],
              "static LDS", k[".group_segment_fixed_size"])
        assert registers <= 96, (n, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".private_segment_fixed_size"] == 0, (n, k[".private_segment_fixed_size"])
        assert not k.get(".uses_dynamic_stack"), n
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k.get(".vgpr_spill_count"), k.get(".sgpr_spill_count"))
        assert k[".group_segment_fixed_size"] == 0, (n, k[".group_segment_fixed_size"])  # dynamic LDS only, as the parent: the launcher passes the parent's size
        assert k.get(".max_flat_workgroup_size") == 128, (n, k.get(".max_flat_workgroup_size"))


def test_the_headline_kernel_is_still_found_by_its_name(meta):
    """The walk has a name of its own: the mangled name of the half-chip 128-thread flavour still matches exactly one kernel, with the resources it had."""
    found = {n: k for n, k in meta.items() if HALF_CHIP_T128.search(n)}
    assert len(found) == 1, sorted(found)
    assert not any(WALK.search(n) for n in found)
    for n, k in found.items():
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 96 and k[".private_segment_fixed_size"] == 0, (n, k[".vgpr_count"], k[".private_segment_fixed_size"])
