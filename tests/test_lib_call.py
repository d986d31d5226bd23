"""CPU: the binding layer's call helpers (_lib.call, _lib.query) -- a failed call raises under the name of the symbol that was
called, with the library's own error string.  The size queries touch no device."""
import ctypes

import pytest


def test_failed_size_query_names_the_called_symbol_and_the_library_error():
    from cvpr2020_manet_amd import _lib
    lib = _lib.load()
    assert _lib.query("manet_local_volume_bytes_f16", 120, 214, 12) > 0
    with pytest.raises(RuntimeError) as err:
        _lib.query("manet_local_volume_bytes_f16", 120, 214, 13)  # the window radius is 0..12
    said = lib.manet_last_error_string().decode("utf-8", "replace")
    assert said and "manet_local_volume_bytes_f16 failed (code -1)" in str(err.value) and said in str(err.value)


def test_call_takes_a_name_or_the_bound_function():
    from cvpr2020_manet_amd import _lib, ops
    lib = _lib.load()
    n = ctypes.c_size_t(0)
    assert _lib.call(lib.manet_local_volume_bytes, 120, 214, 12, ctypes.byref(n)) is None and n.value == 240 * 107520 + 1024
    with pytest.raises(RuntimeError, match="manet_local_volume_bytes failed"):
        _lib.call(lib.manet_local_volume_bytes, 120, 214, -1, ctypes.byref(n))
    assert _lib.query("manet_correlation_out_dims", 8, 8, 4, 1, 4, 1, 1, out=(ctypes.c_int,) * 3) \
        == ops.correlation_out_dims(8, 8, 4, 1, 4, 1, 1)
    with pytest.raises(RuntimeError, match="manet_frame_workspace_bytes failed"):
        ops.frame_workspace_bytes(-1, 8, 8)
