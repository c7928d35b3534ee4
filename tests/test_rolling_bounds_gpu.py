"""The rolling-shutter tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: vs_rolling.hip's gathers and
stores go through VS_IDX, sites 581-590).  The rolling-shutter modules run in a child pytest with VS_AMD_LIB pointing at
variants/libvs_amd_bounds.so, set up the way tests/test_bounds_build_gpu.py sets up its children: every result must still be bit-identical
(the checks change no arithmetic) and after every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean)."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_rolling_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = np.arange(2 * 5 * 8 * 3, dtype=np.uint8).reshape(2, 5, 8, 3)\n"
            "t = capi.Transform.of(0.01, 0.02, 3.0, -2.0)\n"
            "capi.rolling_batch(src, [[0, 1], [1, -1]], [[t, t], [t, t]])\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


def test_the_rolling_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib):
    """the hostile module first -- NaN, singular and saturating motions are what an unchecked gather would go wrong on -- then the kernel-level
    and engine tests, without the allocation-failure walks and the test that starts children of its own; the CPU module rides along"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    mods = ["tests/test_rolling_hostile_gpu.py", "tests/test_rolling_gpu.py", "tests/test_rolling_cpu.py"]
    expr = "not allocation_failure and not fresh_allocations"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1")
