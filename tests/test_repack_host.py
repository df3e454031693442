"""Host-side checks of the device re-pack's C boundary (no GPU): the two entry points exist and are bound, NULL arguments are refused
before anything is touched, and the ABI version did not move (the change is additive)."""
import ctypes as C

from eyoc_amd import _lib


def test_repack_symbols_are_exported_and_bound():
    lib = _lib.load()
    for name in ("eyoc_model_repack_workspace_bytes", "eyoc_model_repack_device"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert lib.eyoc_version() == 111


def test_repack_refuses_null_arguments():
    lib = _lib.load()
    assert lib.eyoc_model_repack_workspace_bytes(None) == 0
    layers = (_lib.LayerParams * 1)()
    fake = C.create_string_buffer(256)          # stands in for a handle: NULL checks come before any dereference
    p = C.c_void_p(C.addressof(fake))
    assert lib.eyoc_model_repack_device(None, p, layers, 1, p, 1 << 20, None) == _lib.ERR_INVALID
    assert b"eyoc_model_repack_device" in lib.eyoc_last_error()
    assert lib.eyoc_model_repack_device(p, None, layers, 1, p, 1 << 20, None) == _lib.ERR_INVALID
    assert b"NULL" in lib.eyoc_last_error()


def test_model_has_the_switch_and_it_is_off():
    import eyoc_amd
    m = eyoc_amd.load_model("ResUNetBN2C")(1, 32, bn_momentum=0.05, conv1_kernel_size=5, normalize_feature=True)
    assert m.device_repack is False and callable(m.repack_device)
    from eyoc_amd.train import ema_sync
    assert callable(ema_sync)
