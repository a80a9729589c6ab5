// Stand-alone driver of reazonspeech_amd/csrc/rs_knobs.h for tests/test_knobs_host.py (built with g++ and the host sanitizers;
// one process per case, because the table reads the environment once per process).
//   dump     one line per row: "<environment name> <value> <given>"
//   setget   a set followed by a get, and setenv calls after the first read that must change nothing
//   unknown  return codes for a name that is not a row
//   threads  eight readers against one writer (the ThreadSanitizer build)
#include <stdio.h>

#include <string>
#include <thread>
#include <vector>

#include "../reazonspeech_amd/csrc/rs_knobs.h"

static int get(const char* name) {
    int v = -12345;
    const int rc = rs_knob_get_named(name, &v);
    return rc == RS_OK ? v : -12345;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "dump") {
        for (int i = 0; i < RS_KNOB_COUNT; ++i)
            printf("%s %d %d\n", rs_knob_rows[i].env, rs_knob((rs_knob_id)i), (int)rs_knob_given((rs_knob_id)i));
        return 0;
    }
    if (mode == "setget") {
        printf("first %d\n", get("RS_GEMM_TILE"));                       // the first read: the environment is consulted here
        setenv("RS_GEMM_TILE", "64", 1);
        setenv("RS_SUB_IM2COL", "1", 1);
        setenv("RS_ATTN64", "2,2", 1);
        printf("after_setenv %d %d %d %d\n", get("RS_GEMM_TILE"), get("RS_SUB_IM2COL"), get("RS_ATTN64"), get("RS_ATTN64_NW"));
        printf("set_rc %d %d\n", rs_knob_set_named("RS_GEMM_TILE", 128), rs_knob_set_named("RS_ATTN64_NW", 3));
        printf("after_set %d %d %d\n", get("RS_GEMM_TILE"), rs_knob(RS_KNOB_GEMM_TILE), get("RS_ATTN64_NW"));
        printf("given %d\n", (int)rs_knob_given(RS_KNOB_GEMM_TILE));     // a set is not the environment
        return 0;
    }
    if (mode == "unknown") {
        int v = 7;
        printf("%d %d %d %d %d\n", rs_knob_set_named("RS_NO_SUCH_SWITCH", 1), rs_knob_get_named("RS_NO_SUCH_SWITCH", &v), v,
               rs_knob_set_named(nullptr, 1), RS_EINVAL);
        return 0;
    }
    if (mode == "threads") {
        const int iters = 4000;
        long long sums[8] = {};
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&sums, t] {
                for (int i = 0; i < iters; ++i)
                    for (int k = 0; k < RS_KNOB_COUNT; ++k) sums[t] += rs_knob((rs_knob_id)k) + (int)rs_knob_given((rs_knob_id)k);
            });
        th.emplace_back([] {
            for (int i = 0; i < iters; ++i) rs_knob_set((rs_knob_id)(i % RS_KNOB_COUNT), i & 3);
        });
        for (auto& x : th) x.join();
        long long total = 0;
        for (long long s : sums) total += s;
        printf("done %d\n", total >= 0);
        return 0;
    }
    fprintf(stderr, "usage: %s dump | setget | unknown | threads\n", argv[0]);
    return 2;
}
