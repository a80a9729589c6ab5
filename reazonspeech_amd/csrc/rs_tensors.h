// rs_tensors.h — the one lookup of a registered tensor (host only, plain C++: no HIP include).
//
// rs_set_tensor files (pointer, bytes) under a name; every rs_finalize of every family turns names into kernel arguments through
// rs_tensor_lookup: registered, exactly the wanted size, 16-byte aligned (the kernels read weights in 16-byte pieces).
// rs_tensor_reader is the form the finalize functions use: the first failure sticks and every later lookup does nothing, so a
// finalize reads as a plain list of names and checks once where it needs the pointers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <unordered_map>
#include <utility>

#include "../../include/rs_asr.h"

typedef std::unordered_map<std::string, std::pair<const void*, size_t>> rs_tensor_table;   // name -> (pointer, bytes)

static inline bool rs_tensor_present(const rs_tensor_table& t, const std::string& name) { return t.count(name) != 0; }

// RS_OK: `out` is the tensor.  RS_EMISSING / RS_EINVAL: `out` is untouched and `msg` says what is wrong with which tensor.
static inline int rs_tensor_lookup(const rs_tensor_table& t, const std::string& name, size_t bytes, const void*& out, std::string& msg) {
    char buf[512];
    const auto it = t.find(name);
    if (it == t.end()) {
        snprintf(buf, sizeof buf, "weight tensor '%s' was not registered", name.c_str());
        msg = buf;
        return RS_EMISSING;
    }
    if (it->second.second != bytes) {
        snprintf(buf, sizeof buf, "tensor '%s': expected %zu bytes, got %zu", name.c_str(), bytes, it->second.second);
        msg = buf;
        return RS_EINVAL;
    }
    if ((uintptr_t)it->second.first & 15) {
        snprintf(buf, sizeof buf, "tensor '%s' is not 16-byte aligned", name.c_str());
        msg = buf;
        return RS_EINVAL;
    }
    out = it->second.first;
    return RS_OK;
}

struct rs_tensor_reader {
    const rs_tensor_table& table;
    int rc = RS_OK;          // the first failure's code ...
    std::string msg;         // ... and text
    explicit rs_tensor_reader(const rs_tensor_table& t) : table(t) {}
    bool ok() const { return rc == RS_OK; }
    bool has(const std::string& name) const { return rs_tensor_present(table, name); }   // for the optional groups: absence is no error
    void get_bytes(const std::string& name, size_t bytes, const void*& out) {
        if (rc == RS_OK) rc = rs_tensor_lookup(table, name, bytes, out, msg);
    }
};
