"""The stand-alone forward entries refuse null pointers before they touch the handle (no device needed)."""
import ctypes

from ladi_vton_amd import _lib


def test_forward_refuses_null_pointers(lib):
    """ladi_unet_forward with a null handle, a null sample, a null output: non-zero and a message that names the entry.  The refusal of the
    buffers comes before the handle is dereferenced, so a block of zeros stands in for one"""
    handle = ctypes.cast(ctypes.create_string_buffer(4096), ctypes.c_void_p)
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    for h, sample, out in ((None, buf, buf), (handle, None, buf), (handle, buf, None)):
        lib.ladi_unet_set_freeu(None, 0, 1.0, 1.0, 1.0, 1.0)        # another entry's message is the last error now
        assert "ladi_unet_set_freeu" in _lib.last_error()
        rc = lib.ladi_unet_forward(h, sample, _lib.F32, 1, 1, 1, 1.0, out, _lib.F32, None)
        assert rc != 0 and "ladi_unet_forward:" in _lib.last_error() and "null" in _lib.last_error(), (rc, _lib.last_error())
    for name, args in (("ladi_unet_forward_pag", (0, 0)), ("ladi_unet_forward_cached_rows", (0, 0, 0))):
        rc = getattr(lib, name)(None, buf, _lib.F32, 1, 1, 1, 1.0, buf, _lib.F32, *args, None)
        assert rc != 0 and "null handle" in _lib.last_error(), (name, rc, _lib.last_error())
