"""The lens tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: vs_remap.hip's map reads, gathers and
stores go through VS_IDX, sites 591-601).  The three lens modules run in a child pytest with VS_AMD_LIB pointing at
variants/libvs_amd_bounds.so, set up the way tests/test_rolling_bounds_gpu.py sets up its children: every result must still be bit-identical
(the checks change no arithmetic) and after every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_remap_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3)\n"
            "pos = capi.lens_map(capi.lens_params(8, 5, k1=-0.3, zoom=0.8), 8, 5)\n"
            "capi.remap_batch(src, pos)\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


def test_the_lens_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- maps that hold the extremes of int32 are what an unchecked gather would go wrong on -- then the kernel-level
    and engine tests, without the allocation-failure walks and the tests that start children of their own; the CPU module rides along"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    mods = ["tests/test_lens_hostile_gpu.py", "tests/test_lens_gpu.py", "tests/test_lens_cpu.py"]
    expr = "not allocation_failure and not fresh_allocations and not long_routes"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
