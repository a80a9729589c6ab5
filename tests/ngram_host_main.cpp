// Stand-alone driver of reazonspeech_amd/csrc/rs_ngram_check.h for tests/test_ngram_lm_host.py (built with g++, once plain and once
// under the host sanitizers).  Reads tables from the file named by argv[1], one per block:
//   n_nodes n_children n_logits order start unk_logp
//   then the eight arrays of rs_ngram in its order, one line each: "<count> v v v ..."   (count -1 = a null pointer)
// Every array lives in a heap block of exactly its size, so a validator that reads past a table is caught by AddressSanitizer.
// Prints one line per table: "<code> <message>"; the same call without a message buffer must give the same code, and a message
// buffer of 8 bytes must stay terminated.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../reazonspeech_amd/csrc/rs_ngram_check.h"

template <class T>
static bool read_array(FILE* f, std::vector<T>& v, bool& null, const char* fmt) {
    int n = 0;
    if (fscanf(f, "%d", &n) != 1) return false;
    null = n < 0;
    v.assign(n > 0 ? n : 0, T());
    for (int i = 0; i < n; ++i)
        if (fscanf(f, fmt, &v[i]) != 1) return false;
    v.shrink_to_fit();
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    for (;;) {
        rs_ngram_host t;
        memset(&t, 0, sizeof t);
        if (fscanf(f, "%d %d %d %d %d %f", &t.n_nodes, &t.n_children, &t.n_logits, &t.order, &t.start, &t.unk_logp) != 6) break;
        std::vector<int32_t> ia[6];
        std::vector<float> fa[2];
        bool in[6], fn[2];
        // child_begin child_tok child_node root_child | logp backoff | suffix level
        for (int k = 0; k < 4; ++k) if (!read_array(f, ia[k], in[k], "%d")) return 2;
        for (int k = 0; k < 2; ++k) if (!read_array(f, fa[k], fn[k], "%f")) return 2;
        for (int k = 4; k < 6; ++k) if (!read_array(f, ia[k], in[k], "%d")) return 2;
        auto ip = [&](int k) -> const int32_t* { return in[k] ? nullptr : ia[k].data(); };
        t.child_begin = ip(0); t.child_tok = ip(1); t.child_node = ip(2); t.root_child = ip(3);
        t.logp = fn[0] ? nullptr : fa[0].data(); t.backoff = fn[1] ? nullptr : fa[1].data();
        t.suffix = ip(4); t.level = ip(5);
        char msg[256];
        memset(msg, '#', sizeof msg);
        const int rc = rs_ngram_check_table(&t, msg, sizeof msg);
        if (memchr(msg, 0, sizeof msg) == nullptr) return 3;
        if (rs_ngram_check_table(&t, nullptr, 0) != rc) return 4;
        char tiny[8];
        memset(tiny, '#', sizeof tiny);
        if (rs_ngram_check_table(&t, tiny, sizeof tiny) != rc || memchr(tiny, 0, sizeof tiny) == nullptr) return 5;
        printf("%d %s\n", rc, msg);
    }
    fclose(f);
    if (rs_ngram_check_table(nullptr, nullptr, 0) != RS_EINVAL) return 6;
    return 0;
}
