"""not gpu: the one lookup of a registered tensor (reazonspeech_amd/csrc/rs_tensors.h) compiled on its own with g++.

Every rs_finalize turns names into kernel arguments through rs_tensor_lookup and its sticky reader: a tensor must be
registered (else RS_EMISSING), have exactly the wanted size and sit on a 16-byte boundary (else RS_EINVAL), and the text names
the tensor.  After a failure the reader does nothing more: later outputs stay as they were and the first text is kept.  Asking
whether a name is registered is no error."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_DIR = os.path.join(os.path.dirname(HERE), "reazonspeech_amd", "csrc")
RS_OK, RS_EINVAL, RS_EMISSING = 0, -1, -2

SOURCE = r"""
#include <string.h>
#include "rs_tensors.h"

static rs_tensor_table table;
static rs_tensor_reader* reader = nullptr;

extern "C" void reset() { table.clear(); delete reader; reader = new rs_tensor_reader(table); }
extern "C" void put(const char* name, uintptr_t ptr, size_t bytes) { table[name] = {(const void*)ptr, bytes}; }
static void copy(const std::string& s, char* text, size_t cap) { strncpy(text, s.c_str(), cap - 1); text[cap - 1] = 0; }
// one plain lookup: the code; *out is written only on success; the message
extern "C" int lookup(const char* name, size_t bytes, uintptr_t* out, char* text, size_t cap) {
    const void* p = (const void*)*out;
    std::string msg;
    const int rc = rs_tensor_lookup(table, name, bytes, p, msg);
    *out = (uintptr_t)p;
    copy(msg, text, cap);
    return rc;
}
// the sticky reader: the reader's code after this get, its text
extern "C" int reader_get(const char* name, size_t bytes, uintptr_t* out, char* text, size_t cap) {
    const void* p = (const void*)*out;
    reader->get_bytes(name, bytes, p);
    *out = (uintptr_t)p;
    copy(reader->msg, text, cap);
    return reader->rc;
}
extern "C" int reader_has(const char* name) { return reader->has(name) ? 1 : 0; }
extern "C" int reader_ok() { return reader->ok() ? 1 : 0; }
extern "C" int codes(int i) { return i == 0 ? RS_OK : i == 1 ? RS_EINVAL : RS_EMISSING; }
"""

BASE = 0x7f0000001000      # a 16-byte aligned address; nothing is read through it
ELEM = 4                   # float32
N = 24


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("tensors")
    src, so = d / "tensors_lookup.cpp", d / "libtensors_lookup.so"
    src.write_text(SOURCE)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", HEADER_DIR, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.put.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t]
    for f in (lib.lookup, lib.reader_get):
        f.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t), ctypes.c_char_p, ctypes.c_size_t]
    lib.reader_has.argtypes = [ctypes.c_char_p]
    assert [lib.codes(i) for i in range(3)] == [RS_OK, RS_EINVAL, RS_EMISSING]
    return lib


def call(f, name, nbytes, before=0xdead0):
    out = ctypes.c_size_t(before)
    text = ctypes.create_string_buffer(512)
    rc = f(name.encode(), nbytes, ctypes.byref(out), text, 512)
    return rc, out.value, text.value.decode()


@pytest.fixture
def table(lib):
    lib.reset()
    lib.put(b"enc.w", BASE, N * ELEM)
    lib.put(b"enc.b", BASE + 4096, N * ELEM)
    lib.put(b"enc.odd", BASE + 8192 + 8, N * ELEM)
    return lib


def test_found(table):
    rc, ptr, text = call(table.lookup, "enc.w", N * ELEM)
    assert rc == RS_OK and ptr == BASE and text == ""


def test_missing_names_the_tensor(table):
    rc, ptr, text = call(table.lookup, "enc.g", N * ELEM)
    assert rc == RS_EMISSING and ptr == 0xdead0
    assert text == "weight tensor 'enc.g' was not registered"


def test_size_off_by_one_element(table):
    for want in ((N - 1) * ELEM, (N + 1) * ELEM):
        rc, ptr, text = call(table.lookup, "enc.w", want)
        assert rc == RS_EINVAL and ptr == 0xdead0
        assert text == f"tensor 'enc.w': expected {want} bytes, got {N * ELEM}"


def test_pointer_eight_bytes_in(table):
    rc, ptr, text = call(table.lookup, "enc.odd", N * ELEM)
    assert rc == RS_EINVAL and ptr == 0xdead0
    assert text == "tensor 'enc.odd' is not 16-byte aligned"


def test_first_failure_sticks(table):
    rc, ptr, text = call(table.reader_get, "enc.w", N * ELEM)
    assert rc == RS_OK and ptr == BASE and text == "" and table.reader_ok()
    rc, ptr, first = call(table.reader_get, "enc.g", N * ELEM)
    assert rc == RS_EMISSING and ptr == 0xdead0 and "'enc.g'" in first and not table.reader_ok()
    # a lookup that would succeed, and one that would fail differently: neither runs
    rc, ptr, text = call(table.reader_get, "enc.b", N * ELEM)
    assert rc == RS_EMISSING and ptr == 0xdead0 and text == first
    rc, ptr, text = call(table.reader_get, "enc.odd", N * ELEM)
    assert rc == RS_EMISSING and ptr == 0xdead0 and text == first


def test_presence_query_is_no_error(table):
    assert table.reader_has(b"enc.w") == 1
    assert table.reader_has(b"enc.w.f32") == 0
    assert table.reader_ok()
    rc, ptr, text = call(table.reader_get, "enc.b", N * ELEM)
    assert rc == RS_OK and ptr == BASE + 4096 and text == ""
