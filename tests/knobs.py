"""The A/B switches of reazonspeech_amd/csrc/rs_knobs.h from a test or script: the library reads the environment once per process,
so a switch is changed in-process through rs_debug_set_knob, by its environment name (the second number of $RS_ATTN64 is RS_ATTN64_NW)."""
import contextlib
import ctypes


def _bind(lib):
    lib.rs_debug_set_knob.argtypes = [ctypes.c_char_p, ctypes.c_int]
    lib.rs_debug_set_knob.restype = ctypes.c_int
    lib.rs_debug_get_knob.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    lib.rs_debug_get_knob.restype = ctypes.c_int


def get_knob(lib, name):
    _bind(lib)
    v = ctypes.c_int(0)
    rc = lib.rs_debug_get_knob(name.encode(), ctypes.byref(v))
    if rc != 0:
        raise KeyError(f"{name} is not a switch of rs_knobs.h (rs_debug_get_knob returned {rc})")
    return v.value


def set_knob(lib, name, value):
    _bind(lib)
    rc = lib.rs_debug_set_knob(name.encode(), int(value))
    if rc != 0:
        raise KeyError(f"{name} is not a switch of rs_knobs.h (rs_debug_set_knob returned {rc})")


@contextlib.contextmanager
def knob(lib, name, value):
    """the switch `name` at `value` for the calls inside; the previous value is back afterwards"""
    previous = get_knob(lib, name)
    try:
        set_knob(lib, name, value)
        yield
    finally:
        set_knob(lib, name, previous)
