"""mccnn_debug_conv_impl: bits 0-1 choose the kernel family, bits 2-3 the backward edge kernel of one-input-feature layers.
The Python hook MCConvModule.debug_conv_impl owns bits 0-1 only: it must leave the library's bits 2-3 as it found them
(a suite run with the cooperative kernel forced through the environment keeps it forced after a test has used the hook)."""
import pytest


@pytest.fixture
def lib():
    from mccnn_amd import build, _lib
    build.build()
    return _lib.load()


def test_library_mask_keeps_four_bits_and_bit_4_preserves_the_upper_two(lib):
    prev = lib.mccnn_debug_conv_impl(0)
    try:
        assert lib.mccnn_debug_conv_impl(8 | 2) == 0
        assert lib.mccnn_debug_conv_impl(16 | 1) == 10       # bit 4: writes bits 0-1 only ...
        assert lib.mccnn_debug_conv_impl(4) == 9             # ... bit 3 was kept; without bit 4 all four bits are written
        assert lib.mccnn_debug_conv_impl(16) == 4
        assert lib.mccnn_debug_conv_impl(0x7fffffe0) == 4    # nothing above bit 3 is stored
        assert lib.mccnn_debug_conv_impl(0) == 0
    finally:
        lib.mccnn_debug_conv_impl(prev)


@pytest.mark.parametrize("upper", [4, 8])
def test_python_hook_leaves_the_edge_kernel_bits_alone(lib, upper):
    import mccnn_amd.MCConvModule as mc
    prev = lib.mccnn_debug_conv_impl(upper)
    try:
        for mask in (2, 4, 1, 0):   # (the hook's own bit 2 -- streaming kernels for depth-wise layers -- never reaches the library)
            before = mc.debug_conv_impl(mask)
            try:
                assert lib.mccnn_debug_conv_impl(16 | (mask & 3)) == (mask & 3) | upper
            finally:
                mc.debug_conv_impl(before)
        assert lib.mccnn_debug_conv_impl(16) & 12 == upper
    finally:
        lib.mccnn_debug_conv_impl(prev)
        mc.debug_conv_impl(0)
