"""The deflicker tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: vs_deflicker.hip's gathers, atomics
and stores go through VS_IDX, sites 545-553).  The three deflicker modules run in a child pytest with VS_AMD_LIB pointing at
variants/libvs_amd_bounds.so, set up the way tests/test_bounds_build_gpu.py sets up its children: every result must still be bit-identical (the
checks change no arithmetic) and after every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_deflicker_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = (np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3) % 200) + 20\n"
            "t = capi.Transform.of()\n"
            "st = capi.exposure_stats_batch(src, [[0, 1]], [[t, t]])\n"
            "g = capi.exposure_gains_batch(st, 8, 5)\n"
            "capi.bgr_gain_batch(src[:1], g)\n"
            "print('counted', int(st[0, 1, 0]), 'clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "counted 4 clean (0, '')" in out.stdout, out.stdout


def test_the_deflicker_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- NaN, singular and saturating maps are what an unchecked gather would go wrong on -- then the kernel-level and
    route tests, without the allocation-failure walks, the app test and the long chunked clips (whose kernels and indices the short clips run
    as well); the CPU module rides along (its library calls are argument checks)"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    mods = ["tests/test_deflicker_hostile_gpu.py", "tests/test_deflicker_gpu.py", "tests/test_deflicker_cpu.py"]
    expr = "not allocation_failure and not video_test and not chunked and not fresh_allocations and not quality_pin"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
