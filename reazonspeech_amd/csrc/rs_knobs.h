// rs_knobs.h — the one table of the A/B switches (host only, plain C++: no HIP include).
//
// Every $RS_* variable that selects a kernel form is a row of RS_KNOBS below; nothing else in csrc/ reads the environment.
// The environment is read ONCE per process, under one call_once, by whichever comes first of a read (rs_knob) or a write
// (rs_knob_set); afterwards a row changes only through rs_knob_set (rs_debug_set_knob from outside).  Rows are atomics: launch
// paths on any thread read them while a test or script writes them.  The defaults are the measured winners (DESIGN.md has
// the table with the profile that decided each); a row selects a code path, not state, which is why it is not per context —
// the rows a context copies at its first rs_finalize (rs_knob_given) are the exception, and rs_set_option wins there.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "../../include/rs_asr.h"

// X(identifier, environment name, kind, default, meaning).  Kinds: PRESENT = the variable being set at all means 1, whatever its
// text ("0" too); INT = atoi of its text.  $RS_ATTN64 = "kbc,nw" fills two rows; the second is addressed as RS_ATTN64_NW and is not
// a variable of its own (a missing second number leaves it at its default).
#define RS_KNOBS(X)                                                                                                                   \
    X(GEMM_TILE, "RS_GEMM_TILE", INT, 0, "forced GEMM tile height (256 / 192 / 128 / 64); 0 = by shape")                              \
    X(GEMM_GROUP_M, "RS_GEMM_GROUP_M", INT, 0, "row panels per XCD tile group; 0 = by shape")                                         \
    X(GEMM_PAIRS, "RS_GEMM_PAIRS", INT, 2, "2 = two tiles per workgroup, LDS ring carried over; 1 = ring restarted; 0 = one tile")    \
    X(GEMM_BREG, "RS_GEMM_BREG", INT, 0, "1 = 256- / 192-row launches keep the weight operand out of LDS (global -> VGPR)")           \
    X(GEMM_EPI_GENERIC, "RS_GEMM_EPI_GENERIC", INT, 0, "1 = every GEMM launch takes the epilogue that tests ReLU / SiLU and multiplies by alpha at run time") \
    X(ATTN_PERSIST,"RS_ATTN_PERSIST", INT, 0, "1 = full attention on resident workgroups that walk the items (n >= 2: on n)")        \
    X(ATTN_STREAM, "RS_ATTN_STREAM", INT, 0, "1 = the streaming attention form (+ 16 x mask: phases left out, for timing)")           \
    X(ATTN64, "RS_ATTN64", INT, 4, "head_dim 64: key blocks per chunk; 0 = the one-workgroup-per-CU geometry")                        \
    X(ATTN64_NW, "RS_ATTN64_NW", INT, 4, "head_dim 64: waves per workgroup (the second number of $RS_ATTN64)")                        \
    X(ATTN_F32_OLD, "RS_ATTN_F32_OLD", PRESENT, 0, "float32 attention: the first form (one wave per key sum)")                        \
    X(ATTN_F32_KEYS, "RS_ATTN_F32_KEYS", PRESENT, 0, "float32 attention: the second form (keys over lanes, no MFMA)")                 \
    X(GLU_GENERIC, "RS_GLU_GENERIC", INT, 0, "GLU + depthwise conv: 1 = the any-kernel-size path, 2 = the f32-tile kernel on the gated layout") \
    X(SUB_IM2COL, "RS_SUB_IM2COL", PRESENT, 0, "ESPnet subsampling: gather the 3 x 3 patches into a matrix first (sizes the workspace too)") \
    X(FUSE_GLU, "RS_FUSE_GLU", INT, 1, "context default: 0 = GLU in the depthwise kernel, not the pw1 GEMM epilogue")                 \
    X(DEFER_OUT_NORM, "RS_DEFER_OUT_NORM", INT, 1, "context default: 0 = every output norm stores its f32 rows")                      \
    X(DECODE_SCREEN, "RS_DECODE_SCREEN", INT, 1, "context default: 0 = exact evaluation of every joint column")                       \
    X(DECODE_NARROW, "RS_DECODE_NARROW", INT, 1, "context default: 0 = the wide-tile LSTM / projection kernels")                      \
    X(DECODE_NO_XCD, "RS_DECODE_NO_XCD", PRESENT, 0, "greedy decode: joint grids not padded to a multiple of 8 column tiles")         \
    X(DECODE_NO_LOOKAHEAD, "RS_DECODE_NO_LOOKAHEAD", PRESENT, 0, "greedy decode: one frame per utterance and step at every batch size") \
    X(VERIFY_WIDE, "RS_VERIFY_WIDE", INT, 0, "screened joint: 1 = a workgroup per row for V <= 3072 too")                             \
    X(DECODE_TRACE, "RS_DECODE_TRACE", PRESENT, 0, "greedy decode: print the step count of every call to stderr")                     \
    X(BEAM_SPEC, "RS_BEAM_SPEC", INT, 3, "beam search: evaluations asked for per iteration (1 .. 8; sizes the workspace too)")         \
    X(BEAM_TRACE, "RS_BEAM_TRACE", PRESENT, 0, "beam search: phase timing of the step kernel")                                        \
    X(BEAM_RECORD_LDS, "RS_BEAM_RECORD_LDS", PRESENT, 0, "beam search: the any-vocabulary record kernel on a small vocabulary")       \
    X(LOGMEL_OLD, "RS_LOGMEL_OLD", PRESENT, 0, "log-mel: the first form (16 frames per workgroup, filterbank read from global memory)") \
    X(SUB_CONV0_OLD, "RS_SUB_CONV0_OLD", PRESENT, 0, "conv0 + dw1: the first form (a workgroup per output row, every odd conv0 row twice)") \
    X(SUB_DW_OLD, "RS_SUB_DW_OLD", PRESENT, 0, "bf16 depthwise stage: the first form (a thread per output bin, every input row read by two rows)") \
    X(AVSR_POSCONV_OLD, "RS_AVSR_POSCONV_OLD", PRESENT, 0, "AV-HuBERT positional convolution: the VALU form")                         \
    X(K2_CONV1_OLD, "RS_K2_CONV1_OLD", PRESENT, 0, "Zipformer conv1: the VALU form (the one other channel counts run)")               \
    X(K2_ATTW_SWEEPS, "RS_K2_ATTW_SWEEPS", INT, 1, "Zipformer attention weights: 3 = the three-sweep kernel")                         \
    X(K2_CONV2_FUSED, "RS_K2_CONV2_FUSED", INT, 1, "default of option k2_conv2_fused: 0 = patch matrix + GEMM launch")                \
    X(K2_CNX_FUSED, "RS_K2_CNX_FUSED", INT, 1, "default of option k2_cnx_fused: 0 = the ConvNeXt pointwise pair as two GEMM launches")

enum rs_knob_id {
#define RS_KNOB_ENUM(id, env, kind, def, what) RS_KNOB_##id,
    RS_KNOBS(RS_KNOB_ENUM)
#undef RS_KNOB_ENUM
    RS_KNOB_COUNT
};
enum rs_knob_kind { RS_KNOB_PRESENT, RS_KNOB_INT };
struct rs_knob_row { const char* env; rs_knob_kind kind; int def; };
static const rs_knob_row rs_knob_rows[RS_KNOB_COUNT] = {
#define RS_KNOB_ROW(id, env, kind, def, what) {env, RS_KNOB_##kind, def},
    RS_KNOBS(RS_KNOB_ROW)
#undef RS_KNOB_ROW
};

struct rs_knob_table {
    std::atomic<int> value[RS_KNOB_COUNT];
    std::atomic<bool> given[RS_KNOB_COUNT];   // the environment gave the row a value
    std::once_flag once;
};
inline rs_knob_table rs_knob_state;           // (an inline variable: one table for all translation units of the library)

inline void rs_knobs_read_env() {
    std::call_once(rs_knob_state.once, [] {
        rs_knob_table& t = rs_knob_state;
        for (int i = 0; i < RS_KNOB_COUNT; ++i) { t.value[i] = rs_knob_rows[i].def; t.given[i] = false; }
        for (int i = 0; i < RS_KNOB_COUNT; ++i) {
            const char* e = i == RS_KNOB_ATTN64_NW ? nullptr : getenv(rs_knob_rows[i].env);
            if (!e) continue;
            t.given[i] = true;
            t.value[i] = rs_knob_rows[i].kind == RS_KNOB_PRESENT ? 1 : atoi(e);
            if (i == RS_KNOB_ATTN64) {
                t.given[RS_KNOB_ATTN64_NW] = true;
                if (const char* c = strchr(e, ',')) t.value[RS_KNOB_ATTN64_NW] = atoi(c + 1);
            }
        }
    });
}

inline int rs_knob(rs_knob_id id) { rs_knobs_read_env(); return rs_knob_state.value[id].load(std::memory_order_relaxed); }
inline bool rs_knob_given(rs_knob_id id) { rs_knobs_read_env(); return rs_knob_state.given[id].load(std::memory_order_relaxed); }
inline void rs_knob_set(rs_knob_id id, int v) { rs_knobs_read_env(); rs_knob_state.value[id].store(v, std::memory_order_relaxed); }

// by environment name (rs_debug_set_knob / rs_debug_get_knob): RS_EINVAL for a name that is not a row
inline int rs_knob_find(const char* env_name) {
    for (int i = 0; env_name && i < RS_KNOB_COUNT; ++i)
        if (!strcmp(env_name, rs_knob_rows[i].env)) return i;
    return -1;
}
inline int rs_knob_set_named(const char* env_name, int v) {
    const int i = rs_knob_find(env_name);
    if (i < 0) return RS_EINVAL;
    rs_knob_set((rs_knob_id)i, v);
    return RS_OK;
}
inline int rs_knob_get_named(const char* env_name, int* v) {
    const int i = rs_knob_find(env_name);
    if (i < 0 || !v) return RS_EINVAL;
    *v = rs_knob((rs_knob_id)i);
    return RS_OK;
}
