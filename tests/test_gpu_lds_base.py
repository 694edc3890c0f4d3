"""The LDS base of the out-of-line device functions (SRBM_LDS_BASE, bilevel-gait-gen_amd/csrc/srbm_types.h) on the device, in both production builds,
through the hook srbm_debug_lds_base (csrc/srbm_dense_hooks.hiph): the address a kernel has for the dynamic LDS, the address an out-of-line
function makes from the constant, and the constant are one number -- 0 in a production build -- and a double the out-of-line function stores
through its address is the double the kernel reads through its own."""
import ctypes as C
import numpy as np
import pytest

from srbm_loader import host

pytestmark = pytest.mark.gpu
MARK = 0x5eed


@pytest.mark.parametrize('large', [False, True])
def test_out_of_line_lds_base_is_the_kernels(large):
    lib = host.lib(large)
    count = 3
    for slot in (0, 1, 63):
        out = np.full((count, 4), -1, np.int32)
        rc = lib.srbm_debug_lds_base(count, slot, out.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0, lib.srbm_last_error().decode()
        kernel, helper, const, seen = out.T
        print('slot %d: kernel %s helper %s constant %s' % (slot, kernel, helper, const))
        assert np.array_equal(kernel, helper) and np.array_equal(kernel, const)
        assert np.all(const == 0)                      # a production build has no static LDS in front of the dynamic LDS
        assert np.all(seen == MARK)
    out = np.zeros(4, np.int32)
    assert lib.srbm_debug_lds_base(1, 64, out.ctypes.data_as(C.POINTER(C.c_int))) != 0      # a slot beyond the hook's LDS is refused
