"""CPU: the compiled listing of pixel_desc_kernel, the pixel launch of a prepared sweep (and so of bench.py).

It must keep what pixel_kernel<2, double> is held to -- at most 256 VGPRs, no scratch, an LDS footprint that lets 8
workgroups share a CU: two wavefronts per SIMD -- and its pixel loop must be the one the roofline numerator of bench.py was
counted from: profiles/hbm_traffic.json holds the flops per pixel visit and the instruction mix of pixel_kernel<2, double>,
and both kernels run the same pixel_iter: the floating-point instructions and flops of pixel_desc_kernel<2>'s loop must equal
the committed ones, and its whole VALU count may not exceed the committed one."""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.fixture(scope="module")
def listing():
    import check_dpp_hazards as chk
    return "\n".join(chk.listing())


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_registers_scratch_and_lds(listing, mode):
    hits = re.findall(r"\.amdhsa_kernel (_Z17pixel_desc_kernelILi%dEE\S+)\n(.*?)\.end_amdhsa_kernel" % mode, listing, re.S)
    assert len(hits) == 1
    g = lambda k: int(re.search(r"\.amdhsa_%s (\S+)" % k, hits[0][1]).group(1))
    assert g("next_free_vgpr") <= 256 and g("private_segment_fixed_size") == 0
    assert 8 * g("group_segment_fixed_size") <= 160 * 1024


def test_the_pixel_loop_is_the_one_bench_counts(listing):
    import count_flops as cf
    committed = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
    flops, mix, _ = cf.analyse(listing, "_Z17pixel_desc_kernelILi2EEv", pixels_per_lane=cf.PIXELS_PER_LANE[""])
    assert flops == committed["flops_per_pixel_visit"], (flops, committed["flops_per_pixel_visit"])
    want = committed["instruction_mix"]
    for key in ("fp_instructions", "fma_class", "fp64_flops", "fp32_flops"):       # the arithmetic: instruction for instruction
        assert mix[key] == want[key], (key, mix[key], want[key])
    # the rest of the loop's VALU work is index and predicate arithmetic, which depends on where the patch's fields sit: the
    # figure bench.py prints must not understate it (2349 here against pixel_kernel's 2350)
    assert mix["valu_per_pixel_visit"] <= want["valu_per_pixel_visit"], (mix["valu_per_pixel_visit"], want["valu_per_pixel_visit"])
