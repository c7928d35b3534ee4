"""The resize tests against the debug build with bounds-checked indexing (tools/build_variant.sh bounds: vs_resize.hip's table, LDS, load and
store offsets go through VS_IDX, sites 637-648).  The resize modules run in a child pytest with VS_AMD_LIB pointing at
variants/libvs_amd_bounds.so, set up the way tests/test_ycbcr_bounds_gpu.py sets up its children: every result must still be bit-identical
(the checks change no arithmetic) and after every test the bounds record must be clean (tests/conftest.py::_bounds_record_stays_clean).  The
kernel-level modules run three times: with the form the library picks, and with each kernel form named through the test hooks."""
import pytest

from _bounds_child import bounds_lib, child_pytest, child_python

pytestmark = pytest.mark.gpu


def test_the_bounds_build_carries_the_resize_record(bounds_lib):
    code = ("from video_stabilizer_amd import capi\n"
            "import numpy as np\n"
            "src = np.arange(2 * 9 * 14 * 3, dtype=np.uint8).reshape(2, 9, 14, 3)\n"
            "capi.resize_batch(src, 5, 4, capi.RESIZE_AREA)\n"
            "capi.resize_batch(src, 20, 13, capi.RESIZE_LINEAR)\n"
            "print('clean', capi.debug_bounds_check())\n")
    out = child_python(code, bounds_lib)
    assert "clean (0, '')" in out.stdout


@pytest.mark.parametrize("form", [None, 0, 1], ids=["picked", "tiled", "direct"])
def test_the_resize_modules_pass_on_the_bounds_build_with_a_clean_record(bounds_lib, form):
    """the hostile module first, then the kernel-level grid, without the allocation-failure walks, the 65 537-frame case and the tests that
    start children of their own; with the library's own pick of the kernel form the stabilizer's module and the CPU module ride along"""
    # (every fresh device allocation of these runs starts filled with 0xA5: nothing compared against the restatement may depend on it)
    mods = ["tests/test_resize_hostile_gpu.py", "tests/test_resize_gpu.py"]
    if form is None:
        mods += ["tests/test_resize_stab_gpu.py", "tests/test_resize_cpu.py"]
    expr = "not allocation_failure and not fresh_allocations and not more_frames_than_a_grid and not scheduling_switch"
    child_pytest(mods, expr, bounds_lib, 1200, VS_TEST_POISON_ALLOC="165", VS_TEST_HOOKS="1",
                 VS_TEST_RESIZE_FORM=None if form is None else str(form))         # (None: the variable is taken out of the child's environment)
