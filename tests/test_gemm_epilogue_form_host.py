"""The GEMM launcher's choice of epilogue form (k_gemm_bf16.hip pick_epi_form; host arithmetic inside librs_asr.so, callable
without a GPU): a compile-time form only when the launcher is certain, the run-time-flag form for everything else."""
import ctypes

import pytest

from reazonspeech_amd.runtime import capi
from knobs import get_knob, knob

RT, NONE, RELU, SILU, UNIT = 0, 1, 2, 3, 8
RES = capi.GEMM_RESIDUAL | capi.GEMM_OUT_F32 | capi.GEMM_BIAS


@pytest.fixture(scope="module")
def form():
    lib = capi.load()
    f = lib.rs_debug_gemm_epi_form
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int]
    f.restype = ctypes.c_int
    assert get_knob(lib, "RS_GEMM_EPI_GENERIC") == 0, "the compile-time forms are the default"
    return lambda bm, flags, alpha=1.0, ln_stats=0, out_bf16=0: f(bm, flags, alpha, ln_stats, out_bf16)


def test_forms_of_the_fastconformer_launches(form):
    assert form(256, capi.GEMM_BIAS | capi.GEMM_SILU) == SILU | UNIT                        # ffn_up
    assert form(256, capi.GEMM_BIAS) == NONE | UNIT                                         # qkv
    assert form(192, capi.GEMM_BIAS | capi.GEMM_GLU) == NONE | UNIT                         # pw1
    assert form(192, capi.GEMM_BIAS | capi.GEMM_RELU | capi.GEMM_ROWMASK) == RELU | UNIT    # subsampling
    # the other height of each has no compile-time form
    assert form(192, capi.GEMM_BIAS | capi.GEMM_SILU) == RT and form(192, capi.GEMM_BIAS) == RT
    assert form(256, capi.GEMM_BIAS | capi.GEMM_GLU) == RT and form(256, capi.GEMM_BIAS | capi.GEMM_RELU | capi.GEMM_ROWMASK) == RT
    for bm in (256, 192):
        # the f32 kinds measured no gain and have no compile-time form: att-out / pw2, ffn_down, joint_enc, sub_out
        assert form(bm, RES) == RT and form(bm, RES, ln_stats=1) == RT and form(bm, RES, 0.5) == RT
        assert form(bm, capi.GEMM_BIAS | capi.GEMM_OUT_F32) == RT and form(bm, capi.GEMM_BIAS | capi.GEMM_OUT_F32, 32.0) == RT


def test_run_time_form_when_not_certain(form):
    silu = capi.GEMM_BIAS | capi.GEMM_SILU
    assert form(192, capi.GEMM_BIAS | capi.GEMM_GLU, 0.99999994) == RT
    for bm in (256, 192):
        assert form(bm, silu, 0.99999994) == RT                   # the float32 below 1
        assert form(bm, capi.GEMM_BIAS, 0.99999994) == RT and form(bm, capi.GEMM_BIAS, 1.0000001) == RT and form(bm, silu, float("nan")) == RT
        assert form(bm, capi.GEMM_BIAS | capi.GEMM_RELU | capi.GEMM_SILU) == RT
        assert form(bm, capi.GEMM_SWOOSHL) == RT and form(bm, capi.GEMM_OUT_F32 | capi.GEMM_SWOOSHR) == RT
        assert form(bm, RES, out_bf16=1) == RT                    # the Zipformer's residual + bf16 copy
        assert form(bm, capi.GEMM_BIAS | capi.GEMM_RELU) == RT    # ReLU exists with the row mask only
        assert form(bm, capi.GEMM_ROWMASK) == RT
    for bm in (128, 64):
        assert form(bm, silu) == RT and form(bm, RES) == RT       # heights without compile-time forms


def test_knob_gives_the_run_time_form_to_every_launch(form):
    lib = capi.load()
    with knob(lib, "RS_GEMM_EPI_GENERIC", 1):
        for bm in (256, 192):
            for flags in (capi.GEMM_BIAS | capi.GEMM_SILU, capi.GEMM_BIAS, capi.GEMM_BIAS | capi.GEMM_GLU, RES,
                          capi.GEMM_BIAS | capi.GEMM_RELU | capi.GEMM_ROWMASK, capi.GEMM_OUT_F32):
                assert form(bm, flags) == RT
    assert form(256, capi.GEMM_BIAS | capi.GEMM_SILU) == SILU | UNIT
